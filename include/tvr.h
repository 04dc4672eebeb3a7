/* tvr.h — C-ABI of the MI355X-native TensoRF volume renderer (libtvr.so, gfx950).
 *
 * The reference (FREDZEL2020/jittor-MYC-NeRFs, tensorf-myc) has NO FFI on this path: the hot path is
 * Python calling Jittor ops.  The boundary kept is therefore the Python call surface of the model and
 * renderer; this header is the C-ABI underneath it.  Each entry point cites the
 * reference interface (paths relative to /root/reference/) whose work it performs.
 *
 * Conventions
 *   - every function returns 0 on success, a negative tvr_status otherwise; tvr_last_error() gives a
 *     thread-local message.  Nothing throws, nothing calls hipDeviceSynchronize.
 *   - ALL device memory is caller-owned (torch allocations): fp32, contiguous, 16-byte aligned.
 *     The library never allocates device memory; sizes come from the *_bytes() queries.
 *   - all work is enqueued on the caller-supplied stream (a hipStream_t passed as void*).
 *   - every OUTPUT matrix whose row width is the kernels' own (not a shape the reference shows) is passed with its size in bytes
 *     (`*_bytes`) and checked on the host before anything is launched: a buffer that is too small is refused with TVR_ERR_SCRATCH
 *     instead of being overrun on the device.  (Round 2: a caller that allocated tvr_app_h_forward's h as [m, sum(app_n_comp)]
 *     instead of the kernels' [m,144] had 144 - sum columns written past its end — a device fault at the next sync.)
 *     tvr_render's rgb_out [n,3] / depth_out [n] and the tvr_vm_grads tensors have the reference's own shapes and carry no count.
 *   - a tvr_scene may be used from one stream at a time; distinct scenes are independent.
 */
#ifndef TVR_H
#define TVR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TVR_VERSION 141   /* (still 141: tvr_cp_scene_packed_bytes / tvr_cp_scene_create are ADDITIVE exports — no existing entry point, struct or layout changed)
                           * 141 (round 6): tvr_train_forward / _backward take TensorVMSplit scenes with up to six encoding frequencies; tvr_train_work_describe.
                           * 140 (round 6): tvr_mlpnet_forward / _train_forward take packed_bytes and a caller-owned work buffer (tvr_mlpnet_work_bytes);
                           * tvr_mlpnet_packed_bytes no longer counts a ticket word; no entry point writes through a const pointer */

typedef enum {
    TVR_OK = 0,
    TVR_ERR_INVALID = -1,      /* bad argument / unsupported configuration */
    TVR_ERR_HIP = -2,          /* a HIP runtime call failed */
    TVR_ERR_SCRATCH = -3,      /* scratch / packed buffer too small or misaligned */
    TVR_ERR_UNSUPPORTED = -4   /* configuration outside what the kernels are built for */
} tvr_status;

typedef struct tvr_scene tvr_scene;
typedef struct tvr_profile tvr_profile;

/* Hyper-parameters of one field: TensorBase.__init__ (tensorf-myc/models/tensorBase.py:141-176),
 * update_stepSize (:197-209) and TensorVMSplit.init_svd_volume (tensorf-myc/models/tensoRF.py:146-164). */
typedef struct {
    float aabb[6];                 /* lo[3], hi[3] */
    int32_t grid[3];               /* gridSize (x, y, z) */
    int32_t density_n_comp[3];     /* 1..16 per plane (the kernels are built for 16; fewer are packed with zero channels, exact) */
    int32_t app_n_comp[3];         /* 1..48 per plane (built for 48; zero-padded likewise) */
    int32_t app_dim;               /* 27 */
    int32_t featureC;              /* 1..128 (built for 128; hidden units that do not exist are zero weights) */
    int32_t view_pe, fea_pe;       /* 0..6 each (shadingMode MLP_Fea).  0..2: the fused kernels (built for 2, 2; every shipped config).  3..6 — TensorBase's own constructor
                                    * defaults are 6, 6 (tensorBase.py:141-145) — render through the lockstep layer-1 form (+213 KB of packed weights, ~1.6 x the frame time)
                                    * and TRAIN through the eager chain (tvr_train_forward / tvr_mlp_train_forward refuse them).  variant 1 (REFTensoRF): 2, 2 only.
                                    * Anything larger: TVR_ERR_UNSUPPORTED from tvr_scene_packed_bytes / tvr_scene_create */
    float near_, far_;             /* near_far */
    float step_size;               /* stepSize = mean(units)*step_ratio, computed by the host in fp32 */
    float inv_aabb_size[3];        /* invaabbSize = 2/(hi-lo), computed by the host in fp32 (:201) */
    float density_shift;           /* -10 */
    float distance_scale;          /* 25 */
    float weight_thres;            /* rayMarch_weight_thres 1e-4 */
    int32_t fea2dense_act;         /* 0 softplus, 1 relu (:444-448) */
    int32_t variant;               /* 0 TensorVMSplit (models/tensoRF.py:141), 1 REFTensoRF (models/REFTensoRF.py:64) */
} tvr_scene_desc;

/* Device pointers to the parameters in the REFERENCE layout (tensoRF.py:154-164, tensorBase.py:69-71):
 * planes (1,C,H,W) channel-first, lines (1,C,L,1), Linear weights [out,in] row-major. */
typedef struct {
    const float *density_plane[3], *density_line[3];
    const float *app_plane[3], *app_line[3];
    const float *basis_mat;              /* [app_dim, sum(app_n_comp)]  (144 columns at the built-for shape) */
    const float *W1, *b1, *W2, *b2, *W3, *b3;   /* W1 [featureC, 30 + 54 fea_pe + 6 view_pe] = [128,150]; variant 1: [128,151] (MLPRender_Fea_Ref, REFTensoRF.py:9-16);
                                                 * W2 [featureC,featureC], W3 [3,featureC] */
    /* variant 1 only (REFTensoRF.init_svd_volume, REFTensoRF.py:86-96): normal_linear [3,144], diffuse_linear [3,144],
     * specular_linear [1,144], rho_linear [1,144] and their biases, in that order */
    const float *ref_W[4], *ref_b[4];
} tvr_scene_params;

/* Optional per-sample outputs (additional_output=True of TensorBase.execute, tensorBase.py:533-534,
 * plus the intermediates the parity tests compare bit for bit).  Any pointer may be NULL. */
typedef struct {
    float *z;            /* [n,S]   z_vals */
    uint8_t *valid;      /* [n,S]   ray_valid after the alpha mask */
    uint8_t *bbox_valid; /* [n,S]   in-box test only */
    int32_t *cell;       /* [n,S,3] floor of the un-normalised grid coordinate per axis */
    float *sigma_feature;/* [n,S] */
    float *sigma;        /* [n,S] */
    float *alpha;        /* [n,S] */
    float *weight;       /* [n,S] */
    float *rgb;          /* [n,S,3] (zero where weight <= thres) */
    float *bg_weight;    /* [n]     T after the last sample */
    float *acc;          /* [n]     sum of weights */
    float *t_min;        /* [n] */
} tvr_dense_out;

/* Counters added to by tvr_render when `stats` is non-NULL (device memory, 8 x uint64, caller zeroes). */
enum { TVR_STAT_SAMPLES_EVAL = 0,   /* density samples actually gathered (valid, before termination) */
       TVR_STAT_SAMPLES_BBOX = 1,   /* in-box samples visited (alpha-mask lookups when a mask is set) */
       TVR_STAT_APP = 2,            /* appearance samples (weight > thres) */
       TVR_STAT_RAYS_TERMINATED = 3,/* rays stopped early by eps_T */
       /* clock probes, summed over the workgroups of a launch: shader-clock ticks (s_memtime) and 100 MHz reference ticks (s_memrealtime) between
        * a workgroup's first and last instruction -> the clock the kernel really ran at = 0.1 GHz * CLK / REF (bench.py's roofline peaks) */
       TVR_STAT_MARCH_CLK = 4, TVR_STAT_MARCH_REF = 5, TVR_STAT_SHADE_CLK = 6, TVR_STAT_SHADE_REF = 7,
       TVR_STAT_COUNT = 8 };

int tvr_version(void);
const char *tvr_last_error(void);

/* Packed (channels-last, zero-padded) copy of the parameters: size query, create, refresh, destroy.
 * Replaces nothing in the reference — it is the HBM layout behind TensorVMSplit's ParameterLists. */
size_t tvr_scene_packed_bytes(const tvr_scene_desc *desc);
int tvr_scene_create(const tvr_scene_desc *desc, void *packed_dev, size_t packed_bytes, tvr_scene **out);
int tvr_scene_update(tvr_scene *scene, const tvr_scene_params *params, void *stream);
/* A CP-decomposed field (TensorCP, tensorf-myc/models/tensoRF.py:317-447): three LINES per factor and no planes,
 *   sigma_feature(p) = sum_r L0[r](p_z) L1[r](p_y) L2[r](p_x),   features(p) = basis_mat (A0[r](p_z) A1[r](p_y) A2[r](p_x))_r      (vecMode = [2, 1, 0])
 * behind TensorBase's march, MLPRender_Fea and compositing.  Both calls read the same tvr_scene_desc: density_n_comp[0] = R_sigma in 1..96 and app_n_comp[0] = R_app in
 * 1..288 (entries [1], [2] are ignored), variant 0, everything else as for TensorVMSplit; more than that is TVR_ERR_UNSUPPORTED with the field named in tvr_last_error().
 * The result is an ordinary tvr_scene.  tvr_scene_update on it reads density_line[3] / app_line[3] ([1, R, L_i, 1], line i along axis 2 - i), basis_mat [27, R_app] and
 * W1 .. b3; the plane pointers are ignored and may be NULL.
 * ACCEPT a CP scene: tvr_scene_update / _touch / _destroy, tvr_scene_set_alpha, tvr_scene_set_range_check, tvr_scene_set / get_render_pieces, tvr_render_scratch_bytes(_min)
 * (a CP render stages features, direction and colour per queue entry: 132 B more per entry than a VM scene, and that is what the two queries report), tvr_render (dense,
 * stats, jitter, eps_T, prof and pieces as ever; no host read), tvr_density_feature, tvr_density_gradient, tvr_app_feature, tvr_mlp_render, tvr_filter_rays.
 * REFUSE it with TVR_ERR_UNSUPPORTED before any launch (the message says "CP"): tvr_render_z and every *_ref call, tvr_march_forward(_z) / _backward(_z), tvr_app_h_forward /
 * _backward, tvr_grad_scratch_bytes and tvr_train_work_bytes (they return 0), tvr_mlp_train_forward, tvr_train_forward / _backward, tvr_train_work_describe,
 * tvr_scene_set_arith with a mode other than TVR_ARITH_F32, tvr_scene_validate_arith: through THESE entry points CP scenes are inference-only, and they compute in the
 * default arithmetic.  CP scenes train through the tvr_cp_* calls below (CP TRAINING), which are entry points of their own.
 * Arithmetic: the lines, their products and the basis product are plain fp32 (FMAs); the network behind them is tvr_mlp_render's (fp16 hi / lo split, range rule below). */
size_t tvr_cp_scene_packed_bytes(const tvr_scene_desc *desc);
int tvr_cp_scene_create(const tvr_scene_desc *desc, void *packed_dev, size_t packed_bytes, tvr_scene **out);
/* CP TRAINING (csrc/tvr_cp_train.hip): the gradients of the CP march and of the CP features, through entry points of their OWN — the refusals listed above stand as
 * they are, and these calls refuse a scene that is not a CP scene with TVR_ERR_UNSUPPORTED.  ADDITIVE exports: TVR_VERSION is unchanged.
 *   tvr_cp_grad_scratch_bytes   the packed gradient images: three density lines [L_i + 1][rd], three appearance lines [L_i + 1][ra], basis_mat [27][ra] (rd / ra: the
 *                               components rounded up to 16 / 4), each block 256-B aligned.  0 for a NULL or non-CP scene.
 *   tvr_cp_march_forward        tvr_march_forward's contract on a CP scene: the plain tvr_scratch_describe layout, the same argument checks, header words and fault flag,
 *                               the ray-ordered queue for n_rays <= 65536.  Queue positions, weights, acc and depth are the bits tvr_render computes on the same rays.
 *   tvr_cp_march_backward       tvr_march_backward's contract: grad_w [queue length] in queue order, grad_acc [n_rays]; writes out->density_line[0..2] ([1, R_sigma, L_i, 1]).
 *                               The kernel recomputes the forward march bit for bit (same rays, jitter and eps_T as the forward call; fwd_scratch intact).
 *   tvr_cp_app_backward         entries xyz_norm [m,3] and grad_features [m,27] (the gradient of tvr_app_feature's output, which is the forward of this call and accepts
 *                               a CP scene); writes out->app_line[0..2] ([1, R_app, L_i, 1]) and out->basis_mat ([27, R_app]).  m == 0: TVR_OK, zeroed gradients.
 * Each backward call zeroes the images it owns, accumulates, and OVERWRITES the tensors it names in `out` (reference layouts: no pad texel, no pad channel — nothing
 * of the padding reaches them); the other members of `out` are not read.  NULL, short or misaligned buffers are refused before any launch.
 * Sums across rays / entries are float atomics (one per lane and retired line tap, 64 consecutive floats per wave-instruction; the basis columns once per 256 entries):
 * results are reproducible to ROUNDING, not bit for bit — two runs on the same inputs differ in the last bits of sums whose terms arrive in another order.
 * Not offered for CP: explicit depths, lam6, the fused step (tvr_train_*), the MFMA network kernels (tvr_mlp_train_*), the reduced arithmetics. */
typedef struct { float *density_line[3], *app_line[3], *basis_mat; } tvr_cp_grads;
size_t tvr_cp_grad_scratch_bytes(const tvr_scene *scene);
int tvr_cp_march_forward(tvr_scene *scene, const float *rays, int64_t n_rays, int32_t n_samples, const float *jitter, float eps_T, float *depth_out, void *scratch,
                         size_t scratch_bytes, void *stream);
int tvr_cp_march_backward(tvr_scene *scene, const float *rays, int64_t n_rays, int32_t n_samples, const float *jitter, float eps_T, const void *fwd_scratch,
                          size_t fwd_scratch_bytes, const float *grad_w, const float *grad_acc, void *grad_scratch, size_t grad_scratch_bytes, const tvr_cp_grads *out,
                          void *stream);
int tvr_cp_app_backward(tvr_scene *scene, const float *xyz_norm, int64_t m, const float *grad_features, size_t grad_features_bytes, void *grad_scratch,
                        size_t grad_scratch_bytes, const tvr_cp_grads *out, void *stream);
/* CONCURRENCY: a scene's packed images are shared by every call that names the scene.  Any number of tvr_render(_z) calls may be in flight on different streams at once as
 * long as each has its own scratch and output buffers (they only READ the scene; render.py::FrameStream keeps two frames in flight this way).  Whatever WRITES the scene's
 * device state — tvr_scene_update, tvr_scene_set_alpha, tvr_scene_validate_arith, the first TVR_ARITH_F16 render after an update (it converts the fp16 copies), the first
 * render after an update of a scene with a density volume (it bakes the volume), tvr_scene_set_density_volume — must be
 * ordered by the caller against every call still reading it (stream waits or events); the library inserts no cross-stream synchronisation. */
/* tvr_scene_update captured into a hipGraph (a whole training step, tvr_train_forward's host does that): every REPLAY re-packs the fp32 images on the device and runs no
 * host code, so whatever the host derived from "the parameters as last packed" is stale afterwards — (a) a range proof that switched the fp16-range check off
 * (tvr_scene_set_range_check(scene, 0)): switch it back on, or prove again, before rendering; (b) the fp16 copies of the appearance factors that TVR_ARITH_F16 gathers
 * (converted by an un-captured update or by the first render in that mode): call tvr_scene_touch() before the next render, which then converts first.
 * tvr_scene_touch: "the packed fp32 images were rewritten behind the host's back" — marks every derived copy (the fp16 copies, the density volume) stale.  Host-only, no launch. */
int tvr_scene_touch(tvr_scene *scene);
/* AlphaGridMask (tensorBase.py:39-59): volume (gz,gy,gx) fp32 (non-negative) in device memory, kept by reference; NULL clears.
 * bits (optional, tvr_alpha_bits_bytes() of device memory, kept by reference): the march then tests `sample_alpha(p) > 0` (:491-496) on a
 * bit volume built here from the float one — same result, 1/32 of the footprint; NULL keeps the 8-tap float lookup. */
size_t tvr_alpha_bits_bytes(const int32_t agrid_xyz[3]);
int tvr_scene_set_alpha(tvr_scene *scene, const float *alpha_volume_dev, const int32_t agrid_xyz[3],
                        const float alpha_aabb[6], const float alpha_inv_size[3], void *bits, size_t bits_bytes, void *stream);
/* BAKED DENSITY VOLUME (inference).  The density feature  sum_i sum_c bilinear(plane_ic)(u,v) * linear(line_ic)(w)  is, inside a grid cell, exactly the trilinear
 * interpolation of the eight corner values  D[z][y][x] = sum_i sum_c plane_ic * line_ic  (a bilinear function times a linear one of the third coordinate is trilinear;
 * the march already uses one cell index and one weight per axis for all planes and lines).  D depends on the parameters alone, so a scene may carry it:
 *   tvr_density_volume_bytes(desc)   (gx+1)(gy+1)(gz+1) fp32, x fastest; the +1 layer is padding (it only ever meets weight 0 and holds 0); 0 for a bad descriptor;
 *   tvr_scene_set_density_volume(scene, buf, bytes, stream)   attaches `buf` (device memory, the CALLER's, kept by reference like tvr_scene_set_alpha's bits;
 *                                    256-byte aligned); buf == NULL detaches.  TVR_ERR_INVALID for a NULL scene, TVR_ERR_SCRATCH for a buffer that is too small or
 *                                    misaligned, TVR_ERR_UNSUPPORTED for a CP scene (tvr_last_error() says which).  If tvr_scene_update has run, the volume is baked
 *                                    here on `stream`; otherwise by the first render.
 * ONE EVALUATOR PER SCENE: while a volume is attached EVERY call that runs the render march — tvr_render (with and without `dense`), tvr_render_z,
 * tvr_render_normals, tvr_scene_validate_arith's probes, the pieces of a call rendered piecewise — takes the density feature from the volume (four loads of two adjacent
 * floats and seven lerps per sample instead of twelve 64-B texels, six line texels and a 48-term contraction), so whatever was bit-identical between those calls still is.
 * With no volume attached the factored kernels run, unchanged.  The training forwards (tvr_march_forward(_z), tvr_train_forward), tvr_density_feature,
 * tvr_density_gradient and tvr_alpha_* always evaluate the factored form.  The two forms differ by fp32 rounding only (against fp64 on a 128^3 scene, |feature| <= 41:
 * factored 4.2e-6, volume 6.4e-6 max abs); a sample whose weight sits within that of weight_thres may enter or leave the appearance queue (about 1e-4 on its pixel).
 * BAKE: one kernel, every value the fp64 sum of the 48 exact products in a fixed order, rounded once; it reads the packed images, i.e. what the factored march reads.
 * STALENESS: tvr_scene_update and tvr_scene_touch only mark the volume stale (a training step that never renders pays nothing); the next call that runs the render
 * march bakes first, on ITS stream (in a call rendered piecewise: before the fork), and records an event; a later call on a DIFFERENT stream waits on that event, so
 * a second stream never reads a half-baked volume.  The bake WRITES the scene's device state: like the fp16 conversion below it must be ordered by the caller against
 * calls on other streams still reading the volume (see CONCURRENCY).
 * STREAM CAPTURE (as for the fp16 copies, tvr_scene_set_arith): a hipGraph that captured a render bakes in whether a volume was attached and whether a bake was due.
 * A render captured while the volume is stale captures the bake in front of its march — every replay bakes again — and the volume STAYS marked stale (a capture runs
 * nothing), so the next un-captured render bakes too.  Under capture no event is recorded or waited on: bring the volume up to date (one un-captured render, or the
 * attach itself) and synchronise before capturing on another stream.  Capture again after attaching or detaching.  ADDITIVE exports: TVR_VERSION is unchanged. */
size_t tvr_density_volume_bytes(const tvr_scene_desc *desc);
int tvr_scene_set_density_volume(tvr_scene *scene, void *volume_dev, size_t volume_bytes, void *stream);
/* BAKED APPEARANCE VOLUME (inference).  The same identity for the appearance features: inside a grid cell  plane_ic(u,v) * line_ic(w)  is trilinear, basis_mat is linear
 * and has no bias, so the 27 features  F = basis_mat . cat_i(P_i * L_i)  are exactly the trilinear interpolation of the cell's eight corner values of F.  A TensorVMSplit
 * scene with at most two encoding frequencies may carry them:
 *   tvr_appearance_volume_bytes(desc)   (gx+1)(gy+1)(gz+1) records of 128 B, x fastest, the +1 layer padding as in the density volume (3.49 GB at 300^3); 0 for a bad
 *                                    descriptor and for descriptors whose scenes take no volume (REFTensoRF, more than two encoding frequencies);
 *   tvr_scene_set_appearance_volume(scene, buf, bytes, stream)   attaches `buf` (device memory, the CALLER's, kept by reference, 256-byte aligned); buf == NULL detaches.
 *                                    TVR_ERR_INVALID for a NULL scene; TVR_ERR_SCRATCH for a buffer that is too small or misaligned; TVR_ERR_UNSUPPORTED for a CP scene, a
 *                                    REFTensoRF scene (its four heads read the 144 products), a scene with more than two encoding frequencies, and any grid whose volume
 *                                    reaches 4 GiB (the gather keeps 32-bit byte offsets; tvr_appearance_volume_bytes reports the size, the caller keeps the factored form).
 *                                    If tvr_scene_update has run, the volume is baked here on `stream`; otherwise by the first render.
 * RECORD: 32 fp32 = one cache line.  Slot 8 g + j (g = 0..3) holds feature 4 g + j for j < 4 and feature 16 + 4 g + (j - 4) for j >= 4 — the eight base values lane
 * group g of the render kernel owns, as one 32-B segment; the slots of rows 27..31 (view direction, constant) hold 0.
 * ONE EVALUATOR PER SCENE: while a volume is attached EVERY call that runs the render path's shade in the default arithmetic — tvr_render (with and without `dense`),
 * tvr_render_z, tvr_scene_validate_arith's TVR_ARITH_F32 probes, the pieces of a call rendered piecewise — reads eight corner records per sample and interpolates 27
 * channels (seven lerps each) instead of gathering 144 channels over six taps and contracting them with basis_mat; with none attached the factored kernel runs, unchanged.
 * tvr_app_feature, tvr_mlp_render, the training forwards and the reduced arithmetics always evaluate the factored form.  The fp16-range check of the volume form covers
 * what it splits (features, layer-2 inputs); it never sees the 144 products: attach a volume only to parameters whose range is PROVEN (the Python host's rule).
 * BAKE: one kernel; every value the sum over k = 48 plane + channel, in that order, of fp64 FMAs  basis[row][k] * (plane_k * line_k)  (the inner product is exact in
 * fp64), rounded once.  It reads what the factored kernel reads: the packed planes and lines, and basis_mat as the kernel's matrix operands hold it — the sum of the
 * fp16 hi and lo parts, i.e. basis_mat truncated to 22 bits.
 * STALENESS, STREAMS, CAPTURE: exactly as the density volume — tvr_scene_update / tvr_scene_touch mark it stale, the next call that launches the render shade in the
 * default arithmetic bakes on ITS stream before any fork and records an event, calls on other streams wait on it; under capture the bake is captured in front and the
 * volume stays marked stale.  ADDITIVE exports: TVR_VERSION is unchanged. */
size_t tvr_appearance_volume_bytes(const tvr_scene_desc *desc);
int tvr_scene_set_appearance_volume(tvr_scene *scene, void *volume_dev, size_t volume_bytes, void *stream);
/* fp16-range check of the inference entry points (tvr_render(_z), tvr_app_feature(_ref), tvr_mlp_render(_ref)); ON when a scene is created.
 * ON: every value that enters a matrix product through the fp16 hi / lo split is held against fp16's largest finite value on the way (one v_max3 per two
 * values, ~1.5 % of the shade kernel's time); an appearance sample with an operand at or beyond 65 504 gets NaN as its colour / features, so its pixel is NaN,
 * never a silently clipped product.  OFF: no check — for hosts that have PROVEN the range from the parameters (the Python host does, by interval bounds, at
 * pack time: field.py::TensorVMSplit._fp16_range_proven) and want the last 1.5 %.  Weights are the host's to check (a bound on max|W| needs no kernel). */
int tvr_scene_set_range_check(tvr_scene *scene, int32_t on);
/* Arithmetic of the appearance network's matrix products (basis 144->27 and REFTensoRF's heads, layers 1 and 2) in tvr_render(_z) and tvr_mlp_render(_ref) of a scene
 * with at most two encoding frequencies.  The reference computes them in fp32 (tensorBase.py:76-86, tensoRF.py:243); fp32 accumulation in every mode:
 *   TVR_ARITH_F32    (default) three fp16 products per fp32 product — weights AND activations as fp16 hi + lo: ~2^-22 per product, fp32-class;
 *   TVR_ARITH_F16ACT layers 1 and 2 take two products — weights keep hi + lo (22 bits), their inputs (features, encoded values, relu outputs) are rounded to
 *                    fp16 (nearest even, 2^-12 relative); the basis product and REFTensoRF's heads keep three (their outputs feed sin / cos, where an error is amplified): 0.70 of the matrix work;
 *   TVR_ARITH_F16    one product — activations as fp16 (nearest even), weights as the HI image of the default mode, i.e. truncated toward zero to fp16 (a one-sided
 *                    2^-11 per weight instead of an unbiased 2^-12: the measured errors below include it): 1/3 of the matrix work; and the gather of tvr_render(_z) reads fp16 COPIES of the appearance
 *                    planes / lines (kept in the packed buffer, converted from the fp32 images with round-to-nearest-even by the first TVR_ARITH_F16 render behind an
 *                    update — tvr_scene_update itself converts nothing): half the bytes through the L1 return path, interpolation still in fp32.
 *                    (A hipGraph that captured a render bakes in the mode and whether a conversion was due: capture again after switching modes.)
 * fp16 rounding is RELATIVE: the reduced modes' absolute error grows with the scale of the features and hidden activations (|feature| <= 23: picture within 6.4e-5 / 3.5e-4
 * of the fp32 path in F16ACT / F16; |feature| ~ 230: 6.5e-4 / 1.5e-3) — a scene with unusually large features keeps the default.
 * The reduced modes are OPT-IN trades inside north_star's parity bar (RGB L-inf 1e-3 against the fp32 path): measured against TVR_ARITH_F32 on the 800x800 bench frame
 * and against the oracle on the fixtures, see DESIGN.md 4.7 and tests/test_gpu_arith.py for the numbers and the bars the tests hold.  Layer 3, encoding, interpolation,
 * density, compositing: fp32 in every mode.  (NerfPlusPlus's background network has the same switch in its descriptor: tvr_mlpnet_desc.arith.)  Every other entry point (tvr_app_feature(_ref), the training forwards, scenes with more than two encoding
 * frequencies) computes with three products whatever the mode says.  Range: as for the default (|x| < 65 504); a rounded activation beyond it becomes inf, and
 * the range check marks its sample NaN as in the default mode.
 * GATE (round 5): a reduced mode never runs on parameters it has not been MEASURED on.  fp16 rounding is relative, so no bound from the parameters alone is useful
 * (interval bounds on |W| |x| overestimate the error a thousandfold and would refuse every scene); instead tvr_scene_validate_arith renders a caller-chosen probe batch
 * of rays in TVR_ARITH_F32 and in the requested mode and compares the pictures:
 *   tvr_scene_set_arith(scene, mode)   records the REQUEST; the kernels keep computing in TVR_ARITH_F32 (tvr_last_error() says so, the call returns TVR_OK) unless
 *                                      the mode is already validated for the parameters as packed;
 *   tvr_scene_validate_arith(...)      max |rgb_mode - rgb_f32| over the probe rays <= tol: the mode is IN EFFECT from here on; otherwise the scene stays in
 *                                      TVR_ARITH_F32 and tvr_last_error() carries the measured difference (TVR_OK either way: *max_diff_out and tvr_scene_get_arith tell).
 *                                      One host synchronisation.  work: (8 n_rays) floats + 256 B of device memory, 16-byte aligned.  The Python host calls it with up to 8192 rays of the
 *                                      first inference batch after every parameter change and a tolerance of 2.5e-4 (a quarter of the parity bar);
 *   tvr_scene_update / tvr_scene_touch void the validation (new parameters): TVR_ARITH_F32 until validated again;
 *   tvr_scene_get_arith                the mode IN EFFECT (what the next render computes in); tvr_scene_get_arith_requested the request.
 * So tvr_render(_z) / tvr_mlp_render(_ref) cannot leave the parity bar silently through a reduced mode: either the mode was measured on this scene's own rays, or it does not run.
 * (tvr_mlpnet_desc.arith, NerfPlusPlus's background network, is a field of a stateless descriptor: the library cannot gate it — the Python host measures it the same way,
 *  variants.py::NerfPlusPlus._settle_bg_arith, and a C host must do likewise.)
 *   A probe that shades fewer than min(TVR_ARITH_MIN_PROBE_SAMPLES, 2 n_rays) appearance samples (rays that miss the box, empty space: both pictures are background, the difference is 0)
 *   has measured nothing: it neither validates nor refuses — the mode stays out of effect, *probe_app_samples_out (optional) tells, and the caller probes again with
 *   rays that hit the scene (round 6; before, such a probe opened the gate for free). */
enum { TVR_ARITH_F32 = 0, TVR_ARITH_F16ACT = 1, TVR_ARITH_F16 = 2 };
#define TVR_ARITH_MIN_PROBE_SAMPLES 2048
int tvr_scene_set_arith(tvr_scene *scene, int32_t mode);
int tvr_scene_get_arith(const tvr_scene *scene);
int tvr_scene_get_arith_requested(const tvr_scene *scene);
int tvr_scene_validate_arith(tvr_scene *scene, const float *rays, int64_t n_rays, int32_t n_samples, int32_t white_bg, float eps_T, float tol,
                             void *scratch, size_t scratch_bytes, float *work, size_t work_bytes, float *max_diff_out, int64_t *probe_app_samples_out, void *stream);
int tvr_scene_destroy(tvr_scene *scene);

/* TensorBase.execute over a ray batch (tensorBase.py:476-536, ndc_ray=False; variant 1: REFTensoRF.execute,
 * models/REFTensoRF.py:174-256, without the training-only normal penalty) as called by
 * OctreeRender_trilinear_fast (tensorf-myc/renderer.py:12-27).
 *   rays [n,6] (o,d); jitter [n] or NULL (is_train: one u per ray, tensorBase.py:351-353);
 *   eps_T: stop a ray once transmittance < eps_T (0 = exact, never stop); must be <= weight_thres;
 *   rgb_out [n,3], depth_out [n]; scratch of tvr_render_scratch_bytes(); dense/stats/prof may be NULL.
 * Arithmetic and its range: everything is fp32 except the matrix products of the appearance network (basis 144->27, layers 1 and 2), which
 * run on the matrix cores as THREE fp16 products per fp32 product (each operand = fp16 hi + fp16 lo, hi*hi + hi*lo + lo*hi, fp32
 * accumulation): ~2^-22 relative error per product, i.e. fp32-class results, but operands pass through fp16's exponent range —
 * |weight|, |appearance feature|, |activation| must stay below 65 504 (the conversion saturates there) and parts below 6e-8 are
 * flushed.  Leaving the range is REPORTED, not silent: with the scene's range check on (the default, tvr_scene_set_range_check) a sample
 * whose operands reach 65 504 renders as NaN.  Layer 3, the positional encoding, interpolation, density and compositing are plain fp32.  The shipped scenes and the reference's
 * 0.1 * randn initialisation are far inside this range (tests: |feature| up to ~1100, weights at 1e-4 scale).
 * PIECES (round 6): a call of at least 6 x piece_rays rays (tvr_scene_set_render_pieces; default 30 720, so every call of 184 320 rays or more — smaller calls gain
 * nothing from two or three pieces, measured) is rendered as
 * K = round(n / piece_rays) pieces of consecutive rays (equal sizes, multiples of 512 rays, the last one shorter), piece k on library-owned stream k & 1 in that stream's half of `scratch`; the two streams fork from the caller's
 * stream by an event and are joined back into it by two more before the call returns, so for the caller everything is still ordered on ITS stream (and a capture of
 * the caller's stream captures the fork and join).  Why: the kernels of one piece take the CUs the other piece's kernels leave as they drain, and a march beside a shade
 * kernel uses the chip's power budget better than either alone — the 800x800 bench frame takes 2 - 4 % less time (profiles/r06_split_frame.txt), pixels unchanged BIT
 * FOR BIT (a ray's result does not depend on the batch it arrives in).  What a caller can notice: (a) the march's fault flag NaNs the pixels of the PIECE that raised
 * it, not of the whole call; (b) tvr_profile records one launch set per piece and the kernels of two pieces overlap, so its sums are per-launch durations as a
 * profiler would list them, not a partition of the call's wall time; (c) calls with `dense` are never cut; (d) one tvr_render(_z) at a time per scene from ONE host
 * thread (the scene owns the two streams; calls from different caller streams queue their pieces on the same two).  tvr_scene_set_render_pieces(scene, 0) switches it off. */
int tvr_scene_set_render_pieces(tvr_scene *scene, int32_t piece_rays);   /* 0: off; < 0: the library's default; else >= 16 (pieces are rounded up to multiples of 512 rays, of 16 below 512) */
int tvr_scene_get_render_pieces(const tvr_scene *scene);
size_t tvr_render_scratch_bytes(const tvr_scene *scene, int64_t n_rays, int32_t n_samples);
/* enough for a call WITHOUT `dense`: two pieces' worth when the call is rendered in pieces (1.3 GB instead of 13 GB for an 800x800 x 512 frame), else the same as above */
size_t tvr_render_scratch_bytes_min(const tvr_scene *scene, int64_t n_rays, int32_t n_samples);
int tvr_render(tvr_scene *scene, const float *rays, int64_t n_rays, int32_t n_samples, int32_t white_bg,
               const float *jitter, float eps_T, float *rgb_out, float *depth_out,
               void *scratch, size_t scratch_bytes, const tvr_dense_out *dense, uint64_t *stats,
               tvr_profile *prof, void *stream);

/* The same with EXPLICIT sample depths z_vals [n,S] (ascending per ray) instead of uniform steps from the box entry: the foreground of
 * NerfPlusPlus.execute (tensorf-myc/models/nerfplusplus.py:272-276), whose sample_ray (:239-269) spaces the samples between `near`
 * and the bounding sphere and perturbs every one.  dists[j] = z[j+1]-z[j], 0 for the last (tensorBase.py:488).
 * t_last_tiny_out [n] or NULL: prod_j (1 - alpha_j + 1e-6), the `bg_lambda` of nerfplusplus.py:277-278. */
int tvr_render_z(tvr_scene *scene, const float *rays, int64_t n_rays, int32_t n_samples, int32_t white_bg,
                 const float *z_vals, float eps_T, float *rgb_out, float *depth_out, float *t_last_tiny_out,
                 void *scratch, size_t scratch_bytes, const tvr_dense_out *dense, uint64_t *stats, void *stream);

/* TensorVMSplit.compute_densityfeature (tensoRF.py:209-225): xyz_norm [m,3] -> out [m]. */
int tvr_density_feature(tvr_scene *scene, const float *xyz_norm, int64_t m, float *out, size_t out_bytes, void *stream);
/* The spatial gradient of tvr_density_feature's value f as a symmetric difference (the reference has no counterpart; a surface normal is -grad / |grad|):
 *   grad[i][k] = (f(p_i + h_k e_k) - f(p_i - h_k e_k)) * (0.5 / h_k),   k = x, y, z in the order of xyz_norm, h_k = half_width[k] in normalised-coordinate units.
 * f is exactly tvr_density_feature's: arbitrary coordinates, align_corners = True, zeros padding.  The shifted coordinate p +- h, the difference and the product with
 * 0.5 / h_k are separately rounded fp32, and every f is evaluated by tvr_density_feature's own expressions in its order: sigma_feature [m] (or NULL) receives f(p_i)
 * bit-equal to tvr_density_feature, and grad is bit-equal to the same quotient of tvr_density_feature at the shifted points — from ONE kernel that evaluates each
 * factor only where the shift moves it (VM: a term's plane at 5 positions and its line at 3 instead of 7 + 7; CP: each line at 3 instead of 7).
 * Not the analytic derivative of the interpolant: that one is one-sided and jumps across grid lines, which is where marching-cubes vertices lie; the symmetric
 * difference is defined and continuous everywhere.  VM scenes of every variant and CP scenes are accepted.
 * Errors, all before any launch: TVR_ERR_SCRATCH for grad_bytes < m * 12 or (sigma_feature given) sigma_bytes < m * 4; TVR_ERR_INVALID for a NULL scene / xyz_norm /
 * half_width / grad, m < 0, or a half width that is not finite and > 0.  m == 0 succeeds and launches nothing. */
int tvr_density_gradient(tvr_scene *scene, const float *xyz_norm, int64_t m, const float half_width[3], float *sigma_feature /* [m] or NULL */, size_t sigma_bytes,
                         float *grad /* [m,3] */, size_t grad_bytes, void *stream);
/* The normal map of a ray batch: tvr_render's march (same rays, jitter, eps_T, alpha mask; uniform steps only) followed by ONE kernel that turns the march's queue of
 * appearance samples e = {x_e = normalize_coord(o + d z), w_e > weight_thres} into
 *   N_i = sum_e w_e n_e,   n_e = v_e / sqrt(max(|v_e|^2, 1e-30)),   v_e = -(g_e * inv_aabb_size),   g_e = tvr_density_gradient's value at x_e for half_width
 * (a zero gradient gives a zero vector, never NaN).  N is world-space fp32 and is NOT renormalised: |N_i| <= acc_i up to rounding, a ray without an entry gives 0, and
 * 0.5 N + 0.5 acc + (1 - acc) bg is the picture a viewer expects, edges blending into the background as the colour does.  The sum over e runs in an order that depends
 * on the ray's own entries only: the result is bit-reproducible and independent of the batch, of chunking and of which wave took the ray.
 *   normal_out [n,3]; acc_out [n] or NULL: the march's acc (the sum of ALL weights of the ray); depth_out [n] or NULL: tvr_render's depth.
 * Header clear, march, normal kernel on the caller's stream: no allocation, no synchronisation, no shade, nothing per entry written to memory besides the march's queue.
 * The scratch (tvr_render_normals_scratch_bytes; 256-byte aligned) holds the header, the per-ray arrays and the queue's positions and ray indices: 20 B per sample of
 * capacity, n * S of them.  TensorVMSplit, REFTensoRF (the same VM density field) and CP scenes are accepted; explicit depths (tvr_render_z) are not offered.
 * If the march raises its fault flag, every output of the call is NaN, as tvr_render's pixels are.
 * Errors, all before any launch: TVR_ERR_INVALID for a NULL scene / rays / normal_out / half_width, n_rays < 0, n_samples or eps_T outside tvr_render's ranges,
 * n_rays * n_samples >= 2^32, or a half width that is not finite and > 0 (the message names half_width); TVR_ERR_SCRATCH for an undersized normal_out / acc_out /
 * depth_out / scratch (the message names the buffer) or a misaligned scratch.  n_rays == 0 succeeds and launches nothing.  ADDITIVE exports: TVR_VERSION is unchanged. */
size_t tvr_render_normals_scratch_bytes(const tvr_scene *scene, int64_t n_rays, int32_t n_samples);
int tvr_render_normals(tvr_scene *scene, const float *rays, int64_t n_rays, int32_t n_samples, const float *jitter /* [n] or NULL */, float eps_T,
                       const float half_width[3], float *normal_out /* [n,3] */, size_t normal_bytes, float *acc_out /* [n] or NULL */, size_t acc_bytes,
                       float *depth_out /* [n] or NULL */, size_t depth_bytes, void *scratch, size_t scratch_bytes, void *stream);
/* TensorVMSplit.compute_appfeature (tensoRF.py:228-244): xyz_norm [m,3] -> out [m,app_dim]. */
int tvr_app_feature(tvr_scene *scene, const float *xyz_norm, int64_t m, float *out, size_t out_bytes, void *stream);
/* MLPRender_Fea.execute (tensorBase.py:76-86): viewdirs [m,3], features [m,app_dim] -> rgb [m,3]. */
int tvr_mlp_render(tvr_scene *scene, const float *viewdirs, const float *features, int64_t m, float *rgb, size_t rgb_bytes, void *stream);
/* REFTensoRF.compute_appfeature (models/REFTensoRF.py:107-133), variant-1 scenes: xyz_norm [m,3] -> features [m,app_dim] and
 * extra [m,8] = {normal_vector 3 (not normalised), rgb_d 3, relu(specular_tint), relu(rho)}. */
int tvr_app_feature_ref(tvr_scene *scene, const float *xyz_norm, int64_t m, float *features, size_t features_bytes, float *extra, size_t extra_bytes,
                        void *stream);
/* MLPRender_Fea_Ref.execute (models/REFTensoRF.py:18-28), variant-1 scenes: viewdirs [m,3] (the reflection directions),
 * features [m,app_dim], dot_product [m] -> sigmoid rgb [m,3]. */
int tvr_mlp_render_ref(tvr_scene *scene, const float *viewdirs, const float *features, const float *dot_product, int64_t m,
                       float *rgb, size_t rgb_bytes, void *stream);
/* AlphaGridMask.sample_alpha (tensorBase.py:50-56): xyz [m,3] (world) -> out [m].  Stand-alone (the reference's
 * AlphaGridMask is its own module): volume (gz,gy,gx) fp32, grid (gx,gy,gz), aabb, invgridSize = 1/size*2 (:46). */
int tvr_alpha_sample(const float *alpha_volume_dev, const int32_t agrid_xyz[3], const float alpha_aabb[6],
                     const float alpha_inv_size[3], const float *xyz, int64_t m, float *out, size_t out_bytes, void *stream);

/* ---- training step (caller: tensorf-myc/train.py:225-261) ------------------------------------------------
 * The TensoRF-specific halves of forward and backward are HIP kernels; the 144->27 basis, the positional encoding and the
 * three Linears run as library GEMMs under the host's autograd between them. */

/* Byte offsets of the regions of a tvr_render / tvr_march_forward scratch buffer, for hosts that consume the queue:
 * counter u32[4] = {queue length, the march's tile counter, FAULT flag, training-workspace OVERFLOW flag (tvr_train_forward)}: the flag is non-zero if a wave of the march kernel gave up waiting for its
 * tile number (1: overtaken in the 64-slot ring, 2: spin limit; tvr_march.hip) — tvr_render then writes NaN to every pixel and depth of the call,
 * hosts that consume the queue read it with the queue length; ray_off/ray_cnt u32[n]; acc f32[n]; q_pos float4[cap] {xyz_norm, weight}; q_out float4[cap] {rgb, weight};
 * q_ray u32[cap]; q_j u32[cap]; cap = n_rays * n_samples.  Each ray's entries are contiguous and in sample order.
 * The `counter` region is a 256-byte header the library zeroes at the start of every call; beyond the four words above it holds the kernels' own work counters (word 16: the
 * shade kernels' tile tickets, word 32: the march's ray counter) — hosts must not write it between a call's launches. */
typedef struct { size_t counter, ray_off, ray_cnt, acc, q_pos, q_out, q_ray, q_j, total; } tvr_scratch_layout;
int tvr_scratch_describe(int64_t n_rays, int32_t n_samples, tvr_scratch_layout *out);

/* The march alone (sample_ray .. raw2alpha, tensorBase.py:487-513): fills the queue (q_pos, q_ray, ray_off, ray_cnt, counter),
 * acc [n] and depth_out [n].  Same arithmetic as tvr_render.
 * RAY ORDER: for n_rays <= 65 536 (TVR_RAY_ORDER_MAX_RAYS: every training batch of the reference) the queue is put into ray order behind the march — ray_off
 * ascends with the ray index — so that every reduction over the appearance samples (the weight-gradient products) runs in the same order run to run: the network's
 * gradients of tvr_train_backward are bit-identical run to run for such batches, the VM factors' (fp32 atomic scatter) reproducible to rounding.  The pass uses the
 * scratch's q_out and q_j regions as temporaries: their contents are undefined afterwards.  Larger batches keep the order the march kernel's waves finished in
 * (every gradient reproducible to rounding only).  A march that raised its fault flag leaves the queue as it lies (the pass returns at once). */
int tvr_march_forward(tvr_scene *scene, const float *rays, int64_t n_rays, int32_t n_samples, const float *jitter, float eps_T,
                      float *depth_out, void *scratch, size_t scratch_bytes, void *stream);

/* Explicit-depth variant (NerfPlusPlus foreground under autograd); t_last_tiny_out [n] or NULL as in tvr_render_z. */
int tvr_march_forward_z(tvr_scene *scene, const float *rays, int64_t n_rays, int32_t n_samples, const float *z_vals, float eps_T,
                        float *depth_out, float *t_last_tiny_out, void *scratch, size_t scratch_bytes, void *stream);

/* TensorBase.filtering_rays (tensorBase.py:411-441; train.py:196-199, 296) in one pass: mask[i] = 1 if ray i is kept.  bbox_only: the slab test against the
 * scene's aabb (t_max > t_min, zero direction components replaced by 1e-6).  Otherwise: any of the N_samples evaluation-mode samples of sample_ray
 * (entry distance clamped to [near, far], j * stepSize) has alpha > 0 in the scene's alpha mask — all samples are looked up, as the reference does. */
int tvr_filter_rays(tvr_scene *scene, const float *rays, int64_t n_rays, int32_t N_samples, int32_t bbox_only, uint8_t *mask, size_t mask_bytes,
                    void *stream);

/* Gradient outputs in the REFERENCE parameter layout ((1,C,H,W) planes, (1,C,L,1) lines); each call overwrites its six. */
typedef struct { float *density_plane[3], *density_line[3], *app_plane[3], *app_line[3]; } tvr_vm_grads;
size_t tvr_grad_scratch_bytes(const tvr_scene *scene);      /* packed gradient images used internally by the two backward calls */

/* d loss / d density factors from grad_w [queue length] (d loss / d weight of each appearance sample, queue order) and
 * grad_acc [n] (d loss / d acc_map).  fwd_scratch is the untouched scratch of the matching tvr_march_forward call. */
int tvr_march_backward(tvr_scene *scene, const float *rays, int64_t n_rays, int32_t n_samples, const float *jitter, float eps_T,
                       const void *fwd_scratch, size_t fwd_scratch_bytes, const float *grad_w, const float *grad_acc,
                       void *grad_scratch, size_t grad_scratch_bytes, const tvr_vm_grads *out, void *stream);

/* Explicit-depth variant; t_last_tiny [n] (forward values) with grad_t_last_tiny [n] = d loss / d t_last_tiny, or both NULL. */
int tvr_march_backward_z(tvr_scene *scene, const float *rays, int64_t n_rays, int32_t n_samples, const float *z_vals, float eps_T,
                         const void *fwd_scratch, size_t fwd_scratch_bytes, const float *grad_w, const float *grad_acc,
                         const float *t_last_tiny, const float *grad_t_last_tiny, void *grad_scratch, size_t grad_scratch_bytes,
                         const tvr_vm_grads *out, void *stream);

/* h [m,144] = bilinear(app_plane) * linear(app_line), plane-major (tensoRF.py:235-241, before basis_mat), and its backward.
 * h is ALWAYS 144 columns wide — the kernels' layout, 3 planes x 48 channels: column 48 p + c is component c of plane p, and the columns
 * behind a plane's own app_n_comp[p] components are written as zeros — whatever the scene's component counts (a zero-padded scene's
 * basis_mat is [27, sum(app_n_comp)]; the host gathers the columns it owns).  h_bytes / dh_bytes >= m * 144 * 4. */
int tvr_app_h_forward(tvr_scene *scene, const float *xyz_norm, int64_t m, float *h_out, size_t h_bytes, void *stream);
int tvr_app_h_backward(tvr_scene *scene, const float *xyz_norm, int64_t m, const float *dh, size_t dh_bytes, void *grad_scratch,
                       size_t grad_scratch_bytes, const tvr_vm_grads *out, void *stream);

/* The appearance network of a TRAINING step (TensorVMSplit; train.py:225-261 through tensoRF.py:244 `basis_mat` and tensorBase.py:76-86
 * `MLPRender_Fea.execute`) on the m appearance samples of a batch, forward and backward, as register-resident MFMA chains.
 *   forward : h [m,144] (tvr_app_h_forward), viewdirs [m,3] -> rgb [m,3]; the inference kernel's own instructions, so a training forward and
 *             an evaluation render agree bit for bit.  Saved for the backward: feats32 [m,32] (27 features + 5 zeros), h1 / h2 [m,128] = the
 *             outputs of layers 1 / 2 after their ReLU.  Uses the scene's packed weights (tvr_scene_update first).
 *   backward: grad_rgb [m,3] (w.r.t. the sigmoid output) -> dh [m,144] (feed tvr_app_h_backward), plus the matrices whose products with
 *             the saved activations are the weight gradients (tvr_gemm_tn): d_out4 [m,4] = {grad of layer 3's output, 0}, dh2 / dh1 [m,128] =
 *             gradients of the pre-ReLU outputs of layers 2 / 1, dfeats32 [m,32] = gradient of the 27 features (+ 5 zeros):
 *               dW3 = d_out^T h2, db3 = colsum(d_out); dW2 = dh2^T h1, db2 = colsum(dh2); dW1 = dh1^T X with X = tvr_pe_concat(feats, viewdirs),
 *               db1 = colsum(dh1); d basis_mat = dfeats^T h.
 *             W1 [128,150], W2 [128,128], W3 [3,128], basis [27,144]: the CURRENT parameters in the reference layout; they are packed into
 *             `image` (tvr_mlp_train_image_bytes() of 256-byte aligned device memory, caller-owned) by the call itself.
 *             gscale_dev: device scalar, a power of two.  The MFMA operands pass through fp16 (see tvr_render), and MSE gradients of a
 *             4096-ray batch are O(1e-5): gradients are multiplied by gscale on entry and by 1 / gscale on exit; choose it so that
 *             max |grad_rgb| * gscale is O(100) (results do not depend on it beyond rounding).
 *             sat_flag_dev (optional device uint32, caller zeroes): set to 1 by the backward kernel if a scaled gradient reached fp16's largest
 *             finite value on its way into a matrix product (the split saturates there silently) — the step's gradients are then clipped and
 *             the caller should lower gscale.
 * All matrices row-major, contiguous, 16-byte aligned; m * 576 < 2^32 per call (both directions).  Every output is passed with its size in
 * bytes: rgb m*3*4, feats32 / dfeats32 m*32*4, h1 / h2 / dh1 / dh2 m*128*4, d_out4 m*4*4, dh m*144*4. */
size_t tvr_mlp_train_image_bytes(void);
int tvr_mlp_train_forward(tvr_scene *scene, const float *h, const float *viewdirs, int64_t m, float *rgb, size_t rgb_bytes, float *feats32,
                          size_t feats32_bytes, float *h1, size_t h1_bytes, float *h2, size_t h2_bytes, void *stream);
int tvr_mlp_train_backward(const float *W1, const float *W2, const float *W3, const float *basis, const float *grad_rgb, const float *rgb, const float *feats32,
                           const float *h1, const float *h2, int64_t m, const float *gscale_dev, float *d_out4, size_t d_out4_bytes, float *dh2,
                           size_t dh2_bytes, float *dh1, size_t dh1_bytes, float *dfeats32, size_t dfeats32_bytes, float *dh, size_t dh_bytes,
                           uint32_t *sat_flag_dev, void *image, size_t image_bytes, void *stream);

/* The same for a REFTensoRF scene (what configs/Scar.txt:28 trains; models/REFTensoRF.py:107-133, 174-256): h -> basis_mat and the four heads
 * {normal, specular tint, diffuse, rho} -> normalised normal, d = -view, dot = d.n, reflection = 2 dot n - d -> MLPRender_Fea_Ref([-dot, features, reflection,
 * PE(features), PE(reflection)]) = rgb_s -> rgb = relu(tint) * rgb_s + rgb_d, in one kernel (the inference kernel's instructions).
 *   forward : additionally saves g8 [m,8] = the raw head outputs {normal 3 (not normalised), tint, rgb_d 3, rho} and rgb_s [m,3] (the network's sigmoid output);
 *             feats32 [m,32] = {27 features, reflection 3, -dot, 0}: the 31 base values of layer 1.  -dot (column 30) is a differentiable output of the host's
 *             autograd function: REFTensoRF's normal penalty sum_i w_i relu(-dot_i)^2 (REFTensoRF.py:236-239) is formed from it.
 *   backward: grad_rgb [m,3] w.r.t. the final colour, grad_in0 [m] or NULL = d loss / d(-dot) arriving through that output -> dh [m,144] (through basis_mat AND the
 *             heads), d_out4 / dh2 / dh1 as above, dfeats32 [m,32] = gradients of {features 27, reflection 3, -dot, 0}, dg8 [m,8] = gradients of the raw head
 *             outputs.  Weight gradients: as above with X = tvr_pe_concat(features, reflection, -dot) [m,151] for dW1, d basis_mat = dfeats32[:, :27]^T h, and
 *             d heads = dg8^T h (rows {normal 3, specular, diffuse 3, rho}), bias gradients = column sums.
 *             W1 [128,151]; heads_W = {normal_linear [3,144], diffuse_linear [3,144], specular_linear [1,144], rho_linear [1,144]} weights (the order of
 *             tvr_scene_params.ref_W). */
int tvr_mlp_train_forward_ref(tvr_scene *scene, const float *h, const float *viewdirs, int64_t m, float *rgb, size_t rgb_bytes, float *feats32, size_t feats32_bytes,
                              float *h1, size_t h1_bytes, float *h2, size_t h2_bytes, float *g8, size_t g8_bytes, float *rgb_s, size_t rgb_s_bytes, void *stream);
int tvr_mlp_train_backward_ref(const float *W1, const float *W2, const float *W3, const float *basis, const float *const heads_W[4], const float *grad_rgb,
                               const float *grad_in0, const float *rgb_s, const float *feats32, const float *h1, const float *h2, const float *g8, const float *viewdirs,
                               int64_t m, const float *gscale_dev, float *d_out4, size_t d_out4_bytes, float *dh2, size_t dh2_bytes, float *dh1, size_t dh1_bytes,
                               float *dfeats32, size_t dfeats32_bytes, float *dg8, size_t dg8_bytes, float *dh, size_t dh_bytes, uint32_t *sat_flag_dev, void *image,
                               size_t image_bytes, void *stream);

/* ---- the training step as two calls with NO host read in between (round 3) -------------------------------------------------------------------
 * tvr_train_forward  = tvr_march_forward -> tvr_app_h_forward -> tvr_mlp_train_forward(_ref) -> the compositing tail (tensorBase.py:520-527);
 * tvr_train_backward = its gradient -> tvr_mlp_train_backward(_ref) -> the weight / bias gradients (tvr_gemm_tn, column sums) -> tvr_app_h_backward ->
 *                      tvr_march_backward.
 * Every kernel behind the march takes the number of appearance samples from the device (the queue counter in the forward scratch) and works in `work`,
 * a caller-owned buffer of tvr_train_work_bytes(app_cap) sized for app_cap appearance samples — so the sequence of launches is fixed and the step can be
 * captured in a hipGraph.  If a step's queue is longer than app_cap, word 3 of the scratch header (tvr_scratch_layout.counter) is set and the step's
 * results are void: the caller reads that word where it reads the loss and repeats with a larger capacity.  The compositing sums run in a fixed order:
 * the step is bit-reproducible (torch's index_add is not).
 *   forward : rgb_map [n,3], depth [n]; pen_ray [n] (variant 1 only, else NULL) = per-ray sum_e w_e relu(-dot_e)^2, whose sum over rays is REFTensoRF's
 *             normal penalty (REFTensoRF.py:236-239).
 *   backward: grad_rgb_map [n,3], grad_pen_ray [n] or NULL -> gradients of every parameter: the VM factors through `vm_out` (all twelve), the network
 *             through `mlp_out` (reference layouts; heads: variant 1 only).  `weights`: the CURRENT parameters (reference layout), packed by the call.
 *             grad_scale_target: see tvr_mlp_train_backward's gscale (64 is the tested default); sat_flag_dev as there.
 * SHAPES (round 6): REFTensoRF scenes: featureC 128, view_pe = fea_pe = 2, 48 appearance components per plane.  TensorVMSplit scenes: EVERY shape the scene accepts —
 * 1 .. 16 density and 1 .. 48 appearance components per plane (zero channels in the packed scene; basis_mat's [27, sum n] columns mapped on the way in and out), featureC
 * 1 .. 128 (units that do not exist are zero rows / columns of the packed weights, their gradients are cropped out of the 128-wide products), view_pe / fea_pe 0 .. 6.
 * TensorBase's own defaults — 8 / 24 components, 6 / 6 frequencies, tensorBase.py:141-145 — are among them.  With more than two frequencies the forward is the lockstep
 * layer-1 kernel of tvr_render and the backward takes dX slot by slot over a streamed W1^T image; for every shape but 2 / 2 at width 128 dW1 is reduced in column blocks
 * of 152 columns (csrc/tvr_mlp_train.hip, tvr_train.hip pe_concat_gen_kernel). */
typedef struct { const float *W1, *W2, *W3, *basis; const float *heads_W[4]; } tvr_train_weights;   /* heads_W: normal, diffuse, specular, rho (variant 1) */
typedef struct { float *W1, *b1, *W2, *b2, *W3, *b3, *basis; float *heads_W[4], *heads_b[4]; } tvr_train_mlp_grads;
size_t tvr_train_work_bytes(const tvr_scene *scene, int64_t n_rays, int32_t n_samples, int64_t app_cap);
/* Byte offsets inside `work` of what a step leaves there (version 141), for hosts that inspect a step — the parity tests check every stage of the backward against
 * fp64 arithmetic on these very tensors.  Saved by the forward: h [cap,144], feats32 [cap,32], h1 / h2 [cap,128] (relu outputs), rgb [cap,3]; written by the backward:
 * grgb [cap,3] (gradient of the per-sample colours), d_out4 [cap,4], dh2 / dh1 [cap,128], dfeats32 [cap,32], dh [cap,144], X (the MLP input: [cap,150] / [cap,151], or for
 * scenes with more than two encoding frequencies x_blocks column blocks of x_block_cols columns, block b a contiguous [cap, w_b] matrix at X + b * cap * x_block_cols
 * floats, w_b = the block's columns rounded up to 4).  Rows beyond the step's queue length (scratch header word 0) are undefined. */
typedef struct { size_t h, feats32, h1, h2, rgb, grgb, d_out4, dh2, dh1, dfeats32, dh, X, total; int32_t x_blocks, x_block_cols; } tvr_train_work_layout;
int tvr_train_work_describe(const tvr_scene *scene, int64_t n_rays, int32_t n_samples, int64_t app_cap, tvr_train_work_layout *out);
int tvr_train_forward(tvr_scene *scene, const float *rays, int64_t n_rays, int32_t n_samples, const float *jitter, float eps_T, int32_t white_bg,
                      void *fwd_scratch, size_t fwd_scratch_bytes, void *work, size_t work_bytes, int64_t app_cap,
                      float *rgb_map, float *depth, float *pen_ray, void *stream);
int tvr_train_backward(tvr_scene *scene, const float *rays, int64_t n_rays, int32_t n_samples, const float *jitter, float eps_T, int32_t white_bg,
                       const void *fwd_scratch, size_t fwd_scratch_bytes, void *work, size_t work_bytes, int64_t app_cap, const tvr_train_weights *weights,
                       const float *grad_rgb_map, const float *grad_pen_ray, float grad_scale_target, void *grad_scratch, size_t grad_scratch_bytes,
                       const tvr_vm_grads *vm_out, const tvr_train_mlp_grads *mlp_out, uint32_t *sat_flag_dev, void *stream);

/* C [Ka,Kb] = A^T B for tall-skinny fp32 operands A [M,Ka] (row stride lda), B [M,Kb] (row stride ldb): the weight gradients dW = dY^T X of
 * the training step's Linears (MLPRender_Fea's three layers tensorBase.py:69-71, basis_mat tensoRF.py:150) over the M appearance samples of
 * a batch.  fp32 semantics (fp32-input MFMA), fixed summation order (bit-reproducible); C is overwritten;
 * (Ka/32 rounded up) * (Kb/32 rounded up) <= 20.  scratch: tvr_gemm_tn_scratch_bytes() of device memory (per-workgroup partial sums). */
size_t tvr_gemm_tn_scratch_bytes(int32_t Ka, int32_t Kb, int64_t M);
int tvr_gemm_tn(const float *A, int32_t lda, int32_t Ka, const float *B, int32_t ldb, int32_t Kb, int64_t M, float *C,
                void *scratch, size_t scratch_bytes, void *stream);
/* The same product plus colsum_A [Ka] = A^T 1 in the same pass (a virtual ones column of B): the weight and the bias gradient of a Linear from one read of dY.
 * Ka x (Kb + 1) must fit the 20 tiles, Ka + Kb <= 320; scratch: tvr_gemm_tn_scratch_bytes(Ka, Kb + 1, M). */
int tvr_gemm_tn_bias(const float *A, int32_t lda, int32_t Ka, const float *B, int32_t ldb, int32_t Kb, int64_t M, float *C, float *colsum_A,
                     void *scratch, size_t scratch_bytes, void *stream);
/* The same on the fp16-split MFMAs with A * s (s = *scale_dev, a power of two; the result is divided by s again): for operands whose range is known to fit fp16
 * at that scale (a caller-chosen gradient scale).  colsum_A optional.  Ka <= 128, Ka + Kb <= 320. */
int tvr_gemm_tn_scaled(const float *A, int32_t lda, int32_t Ka, const float *B, int32_t ldb, int32_t Kb, int64_t M, float *C, float *colsum_A,
                       const float *scale_dev, void *scratch, size_t scratch_bytes, void *stream);

/* The MLP input of the training step in one pass: X [m,150] = [features 27, viewdirs 3, PE(features), PE(viewdirs)] (MLPRender_Fea.execute,
 * tensorBase.py:76-82; positional_encoding :9-15), or X [m,151] with dot_product [m] in front (MLPRender_Fea_Ref, REFTensoRF.py:19-24) when
 * dot_product is non-NULL; and its backward (grad_viewdirs / grad_dot may be NULL). */
int tvr_pe_concat(const float *features, const float *viewdirs, const float *dot_product, int64_t m, float *X, size_t X_bytes, void *stream);
int tvr_pe_concat_backward(const float *features, const float *viewdirs, const float *grad_X, int64_t m, int32_t with_dot,
                           float *grad_features, size_t grad_features_bytes, float *grad_viewdirs, float *grad_dot, void *stream);

/* TVLoss.forward (tensorf-myc/utils.py:123-142) of one plane x (C,H,W), batch 1: value [1] = weight * 2 (h_tv/count_h + w_tv/count_w) and
 * grad (C,H,W) = d value / d x in the same pass; fixed summation order.  scratch: 2048 bytes. */
int tvr_tv_loss(const float *x, int32_t C, int32_t H, int32_t W, float weight, float *value, float *grad, void *scratch, size_t scratch_bytes,
                void *stream);

/* The two parameter-only regularisers of train.py:237-244 that are not TV, each ONE launch forward and ONE backward, fixed summation order; the
 * backward reads the upstream gradient grad_value[0] from the device.  Up to 8 tensors per call (host arrays of device pointers / sizes).
 *   tvr_l1_mean:    value[0] = sum_t mean |xs[t]|                         TensorVMSplit.density_L1, tensoRF.py:190-194 (3 planes + 3 lines)
 *   tvr_line_ortho: value[0] = sum_t mean |offdiag(V_t V_t^T)|, V_t = vs[t] as (n_comp[t], n_size[t]), 2..48 components
 *                                                                          TensorVMSplit.vector_comp_diffs / vectorDiffs, tensoRF.py:178-188
 * scratch: tvr_l1_mean_scratch_bytes(counts, n) / TVR_LINE_ORTHO_SCRATCH_BYTES (256 since version 141: eight workgroups per line factor, one partial sum each; 32 before). */
#define TVR_LINE_ORTHO_SCRATCH_BYTES 256
size_t tvr_l1_mean_scratch_bytes(const int64_t *counts, int32_t n);
int tvr_l1_mean(const float *const *xs, const int64_t *counts, int32_t n, float *value, void *scratch, size_t scratch_bytes, void *stream);
int tvr_l1_mean_backward(const float *const *xs, float *const *grads, const int64_t *counts, int32_t n, const float *grad_value, void *stream);
int tvr_line_ortho(const float *const *vs, const int32_t *n_comp, const int32_t *n_size, int32_t n, float *value, void *scratch, size_t scratch_bytes,
                   void *stream);
int tvr_line_ortho_backward(const float *const *vs, float *const *grads, const int32_t *n_comp, const int32_t *n_size, int32_t n,
                            const float *grad_value, void *stream);

/* Per-kernel HIP-event timing of tvr_render calls (march / shade / composite), for bench.py's roofline.  max_calls bounds the CALLS recorded; a call rendered in
 * pieces records one set of events per piece (created on first use). */
int tvr_profile_create(int32_t max_calls, tvr_profile **out);
int tvr_profile_reset(tvr_profile *prof);
/* After the stream is synchronised: sums over recorded calls, ms[0..2] = march, shade, composite; returns #calls. */
int tvr_profile_read(tvr_profile *prof, float ms[3]);
int tvr_profile_destroy(tvr_profile *prof);

/* ---- NerfPlusPlus background network: `Embedder` + `MLPNet.forward`, models/nerfplusplus.py:7-56, 66-140, as
 * evaluated by `NerfPlusPlus.execute` on the background samples (:280-302).  W = 128, D base layers with one skip, sigma = |Linear|,
 * rgb = sigmoid(Linear(relu(Linear([base_remap, view embedding])))).  `base_remap` (Linear 128->256) has no activation behind it:
 * the caller folds it into the first rgb layer (rgbh_W_base = W_rgb0[:, :256] @ W_remap, rgbh_b = W_rgb0[:, :256] @ b_remap + b_rgb0). */
typedef struct tvr_mlpnet_desc {
    int32_t D;                  /* base layers (bg_D; 2..4) */
    int32_t W;                  /* 128 (nerfplusplus.py:159) */
    int32_t skip;               /* `skips=[int(bg_D/2)]`: after base layer `skip` the point embedding is concatenated in front */
    int32_t pos_freqs;          /* bg_freq: the 4-vector point gets 4 + 8*pos_freqs inputs */
    int32_t view_freqs;         /* bg_view_freq (2): 3 + 6*view_freqs inputs */
    int32_t samples_per_ray;    /* sample s uses viewdirs[s / samples_per_ray] */
    int32_t arith;              /* TVR_ARITH_* (above) of tvr_mlpnet_forward: 0 = three fp16 products per fp32 product (fp32-class, the default); F16ACT = every layer's inputs
                                 * rounded to fp16, weights hi + lo; F16 = plain fp16 operands.  tvr_mlpnet_train_forward computes fp32-class whatever this says */
} tvr_mlpnet_desc;

typedef struct tvr_mlpnet_params {   /* fp32 device pointers, row-major [out,in] as torch / Jittor Linear */
    const void *base_W[4], *base_b[4];
    const void *sigma_W, *sigma_b;   /* [1,128], [1] */
    const void *rgbh_W_base;         /* [64,128]  (folded, see above) */
    const void *rgbh_W_view;         /* [64,15] = W_rgb0[:, 256:] */
    const void *rgbh_b;              /* [64] */
    const void *rgbo_W, *rgbo_b;     /* [3,64], [3] */
} tvr_mlpnet_params;

size_t tvr_mlpnet_packed_bytes(const tvr_mlpnet_desc *desc);
/* Byte offsets of the regions of a packed network: MFMA fragment blocks, the biases, and the block table tvr_mlpnet_pack writes ONCE and tvr_mlpnet_repack walks on the
 * device every training step (pointers to the parameter tensors + the slice each fragment block takes).  Nothing but pack / repack writes any of it. */
typedef struct { size_t fragments, biases, block_table, block_table_bytes, total; } tvr_mlpnet_layout;
int tvr_mlpnet_describe(const tvr_mlpnet_desc *desc, tvr_mlpnet_layout *out);
/* builds the MFMA fragment image (synchronises the stream once: packing is an explicit, rare call) */
int tvr_mlpnet_pack(const tvr_mlpnet_desc *desc, const tvr_mlpnet_params *params, void *packed, size_t packed_bytes, void *stream);
/* pts [n,4] (inverted-sphere points, depth2pts_outside), viewdirs [ceil(n / samples_per_ray), 3] -> rgb [n,3] (sigmoid applied), sigma [n] (abs applied).
 * `packed` (packed_bytes >= tvr_mlpnet_packed_bytes(), checked) is READ-ONLY to every forward: any number of forwards may share it on different streams.
 * `work`: tvr_mlpnet_work_bytes() of caller-owned device memory, 16-byte aligned — the kernel's per-launch ticket word (dynamic hand-out of the sample tiles), zeroed and
 * advanced by the call: one launch per work buffer at a time.  (Round 5 kept that word in 256 extra bytes of `packed` and wrote it through the const pointer without
 * knowing the buffer's size: version 130.  DESIGN.md 11 has the abort that preceded it.) */
size_t tvr_mlpnet_work_bytes(void);
int tvr_mlpnet_forward(const tvr_mlpnet_desc *desc, const void *packed, size_t packed_bytes, const void *pts, const void *viewdirs, int64_t n_samples, void *rgb,
                       void *sigma, void *work, size_t work_bytes, void *stream);
/* Training (`optimizer.backward(loss)` through MLPNet, train.py:258): the same kernel also saves what the backward needs, all fp32,
 * caller-owned, 16-B aligned, with byte counts that are checked before the launch:
 *   act[l] [n,128] = relu output of base layer l; rgb_hidden [n,64] = relu output of rgb_layers[0]; sigma_pre [n] = the sigma head before `abs`;
 *   embed_pos [n, 4 + 8 pos_freqs] and embed_view [n,16] (15 values + a zero) = the two Embedder outputs as matrices (operands of dW = dY^T E).
 * tvr_mlpnet_repack: the fragment image again from the tensors the table inside `packed` already points at (tvr_mlpnet_pack ran once with the same
 * pointers; their values change every optimizer step) — no host synchronisation. */
typedef struct tvr_mlpnet_saved {
    void *act[4];
    size_t act_bytes;                /* of EACH act[l] */
    void *rgb_hidden;
    size_t rgb_hidden_bytes;
    void *sigma_pre;
    size_t sigma_pre_bytes;
    void *embed_pos;
    size_t embed_pos_bytes;
    void *embed_view;
    size_t embed_view_bytes;
    /* optional (mask_bytes = 0: not written): the ReLU masks of act[l] / rgb_hidden as BITS, [n][2] 64-bit words each — word h of sample s holds at bit
     * 16 b + 4 q + i whether unit 32 b + 8 q + 4 h + i is positive, the order tvr_linear_dx's `mask_bits` takes (16 B per sample instead of 512) */
    void *act_mask[4];
    void *rgb_hidden_mask;
    size_t mask_bytes;               /* of EACH mask buffer: >= n x 16 */
} tvr_mlpnet_saved;
int tvr_mlpnet_train_forward(const tvr_mlpnet_desc *desc, const void *packed, size_t packed_bytes, const void *pts, const void *viewdirs, int64_t n_samples, void *rgb,
                             void *sigma, const tvr_mlpnet_saved *saved, void *work, size_t work_bytes, void *stream);
int tvr_mlpnet_repack(const tvr_mlpnet_desc *desc, const tvr_mlpnet_params *params, void *packed, size_t packed_bytes, void *stream);
/* The input gradient of a Linear over a tall batch with the ReLU mask in front of it fused in (fp32-input MFMAs, W staged in LDS):
 *   dX[m, k] = (sum_{n < N} dY[m, n] W[n, k]) * (mask[m, k] > 0 ? 1 : 0)     (mask NULL: no mask)
 * dY [M, ldy] with N a multiple of 8 in [8,128] (columns n_valid..N-1 of dY must be finite, rows n_valid.. of W are taken as zero), W row-major
 * [n_valid, ldw] = a torch / Jittor Linear weight [out, in] (the reduction runs over its rows), K in {32, 64, 96, 128} columns of W / dX / mask;
 * ldy, ldx, ldm multiples of 4 and all pointers 16-B aligned.  What autograd computes for `relu(Linear(x))` chains (MLPNet.forward, nerfplusplus.py:119-140).
 * scale_dev (optional; N then a multiple of 16): a device scalar s, a power of two — the products run on the fp16-split MFMAs with dY * s (three products,
 * fp32-grade) for callers that know dY's range at that scale, ~3x the rate of the fp32 form; a non-finite result raises *sat_flag_dev (optional).
 * mask_bits (optional, instead of mask): the same mask as bits, [M][2] 64-bit words in the layout tvr_mlpnet_train_forward writes (above). */
int tvr_linear_dx(const float *dY, int32_t ldy, int32_t N, const float *W, int32_t ldw, int32_t n_valid, int32_t K, const float *mask, int32_t ldm,
                  const uint64_t *mask_bits, float *dX, int32_t ldx, size_t dX_bytes, int64_t M, const float *scale_dev, uint32_t *sat_flag_dev, void *stream);
/* out[k] = sum_m A[m, k], k < K <= 128, fixed summation order (the bias gradients of the same Linears).  scratch: tvr_colsum_scratch_bytes(). */
size_t tvr_colsum_scratch_bytes(void);
int tvr_colsum(const float *A, int32_t lda, int32_t K, int64_t M, float *out, void *scratch, size_t scratch_bytes, void *stream);

/* The background of NerfPlusPlus.execute around that network (nerfplusplus.py:280-308).
 * tvr_npp_bg_points: z_lin [n_samples] (the `linspace(0, radii, N)` depths), t_rand [n_rays,n_samples] (the `rand_like` draw of
 *   `perturb_samples`, :196-205) -> pts [n_rays,n_samples,4] = `depth2pts_outside` (:207-237) of the perturbed depths and z
 *   [n_rays,n_samples] = those depths, both already FLIPPED along the sample axis (:296-297).
 * tvr_npp_bg_composite: rgb [n_rays,n_samples,3], sigma, z (flipped order) -> rgb_out [n_rays,3] = sum_k alpha_k T_k rgb_k with
 *   alpha = 1 - exp(-sigma * (z_k - z_{k+1})), last distance 1e10, T = cumprod(1 - alpha + 1e-6) shifted by one (:298-308). */
int tvr_npp_bg_points(const void *rays_o, const void *rays_d, int64_t n_rays, const void *z_lin, int32_t n_samples, const void *t_rand, float radii,
                      void *pts, void *z, void *stream);
int tvr_npp_bg_composite(const void *rgb, const void *sigma, const void *z, int64_t n_rays, int32_t n_samples, void *rgb_out, void *stream);

/* Iso-surface of a dense fp32 volume as an indexed triangle mesh: marching cubes (train.py:41-59 `export_mesh` -> utils.py:146-207, where the reference calls
 * skimage.measure.marching_cubes on the CPU).  ADDITIVE exports: TVR_VERSION is unchanged.
 *   volume [dims[0]][dims[1]][dims[2]] fp32, z fastest (TensorBase.getDenseAlpha's layout); a grid point is INSIDE iff value >= level.
 *   Grid point p = (i * dims[1] + j) * dims[2] + k owns the edges that leave it along +x, +y, +z.  Vertices: one per grid edge whose ends straddle the level, ordered by
 *   (owner point, axis x < y < z) — the mesh is indexed and welded by construction; for end values a (owner) and b: t = (level - a) / (b - a), voxel coordinate = index + t,
 *   world = origin + coordinate * spacing (fp32, each operation rounded on its own).  Triangles: ordered by cell (the point at the cell's minimum corner), then by the case
 *   table's order (csrc/tvr_mc_table.h, generated by scripts/gen_mc_table.py); normals (right-hand rule) point from inside to outside, flip != 0 reverses each triangle.
 *   The output is a function of the arguments alone: bit-identical from run to run.
 * Two steps, because the sizes of the outputs are results:
 *   tvr_mesh_count fills `scratch` (tvr_mesh_scratch_bytes(dims), 256-byte aligned) and leaves {n_vertices, n_triangles} in counts_dev[2]; the caller reads them once,
 *   allocates verts [n_vertices,3] fp32 and faces [n_triangles,3] int32, and calls
 *   tvr_mesh_emit with the SAME volume, dims, level and scratch.  n_vertices / n_triangles are the capacities of the two outputs: no store happens at or beyond them whatever
 *   volume and scratch hold, and if they are not the counted totals *fault_flag_dev becomes 1 and nothing is written (the flag is only ever set; the caller zeroes it).
 *   Zero vertices / triangles is a valid result (verts / faces may then be NULL).
 * Errors, all before any launch: TVR_ERR_INVALID for a NULL pointer, a dimension below 2, a scratch / output buffer smaller than stated above or a misaligned scratch, counts
 *   outside 0 .. 3 points / 5 points; TVR_ERR_UNSUPPORTED for 3 * points >= 2^31 (indices are int32).  tvr_mesh_scratch_bytes returns 0 for such dims.
 * The scan is reduce / scan / add over tiles of TVR_MESH_TILE points; one workgroup walks the tile sums TVR_MESH_SCAN_CHUNK at a time (no workgroup waits for another). */
#define TVR_MESH_TILE 1024
#define TVR_MESH_SCAN_CHUNK 256
size_t tvr_mesh_scratch_bytes(const int32_t dims[3]);
int tvr_mesh_count(const float *volume, const int32_t dims[3], float level, void *scratch, size_t scratch_bytes, int64_t *counts_dev, void *stream);
int tvr_mesh_emit(const float *volume, const int32_t dims[3], float level, const float origin[3], const float spacing[3], const void *scratch, size_t scratch_bytes,
                  float *verts, size_t verts_bytes, int64_t n_vertices, int32_t *faces, size_t faces_bytes, int64_t n_triangles, int32_t flip,
                  uint32_t *fault_flag_dev, void *stream);

/* Connected components of an indexed triangle mesh and a filter that keeps whole components (csrc/tvr_mesh_cc.hip; the reference writes whatever skimage returns,
 * utils.py:146-207, so an exported field carries its floaters).  ADDITIVE exports: TVR_VERSION is unchanged.  faces [n_triangles][3] int32 indexes n_vertices vertices.
 *   Component: two vertices are connected iff a chain of triangles links them (a triangle connects its three vertices); a vertex no triangle uses is a component of
 *   its own with zero triangles.  Label of a component = its SMALLEST vertex index (a function of the mesh alone).  Size = the triangles whose FIRST vertex carries the label.
 * tvr_mesh_components: vertex_label [n_vertices] int32 = the label of each vertex's component; component_faces [n_vertices] int32 = at a label (vertex_label[v] == v) the
 *   component's triangle count, 0 elsewhere; *n_components_dev (int64) = the number of labels.  Union-find over the vertices driven by the triangles: a root is only ever
 *   hooked under a smaller index, so the root of a finished tree is the component's minimum whatever the order the atomics land in; a flatten pass then writes every
 *   vertex's root.  scratch: tvr_mesh_components_scratch_bytes (256-byte aligned); its second uint32 holds, after the call, the most steps any one walk took (diagnostic).
 *   A triangle index outside 0 .. n_vertices-1 sets *fault_flag_dev = 1 and NOTHING else is written (a pass over the triangles precedes every other store); no load or
 *   store leaves the caller's buffers whatever `faces` holds.  Every walk is bounded (2 n_vertices + 64 steps; indices strictly decrease along a walk, so the bound is
 *   out of reach unless vertex_label is overwritten during the call) and gives up by setting the flag.  The flag is only ever set; the caller zeroes it.
 * Filter, in the two steps of tvr_mesh_count / tvr_mesh_emit because the output sizes are results.  keep_root [n_vertices] uint8 is read at labels only: a vertex
 *   survives iff keep_root[vertex_label[v]] != 0, a triangle iff its first vertex does.
 *   tvr_mesh_filter_count fills `scratch` (tvr_mesh_filter_scratch_bytes, 256-byte aligned: 9 B per element of max(n_vertices, n_triangles) rounded up to TVR_MESH_TILE)
 *   with the keep flags and their exclusive scans (the reduce / scan / add scheme above) and leaves {surviving vertices, surviving triangles} in counts_dev[2].
 *   A triangle index or a label outside 0 .. n_vertices-1 sets the flag, is neither followed nor kept, and makes the following emit write nothing.
 *   tvr_mesh_filter_emit with the SAME faces, counts and scratch: verts_out [n_vertices_out][3] fp32 = the surviving rows of verts, bit for bit and in their order (verts
 *   and verts_out may both be NULL: indices only); faces_out [n_triangles_out][3] int32 = the surviving triangles in their order, re-indexed; kept_vertex [n_vertices_out]
 *   int32 = the old index of each new vertex (ascending).  The declared counts are the capacities: no store happens at or beyond them, and if they are not the counted
 *   totals the flag is set and nothing is written.  A surviving triangle whose corner did not survive (labels that do not belong to these faces) sets the flag.
 * n_triangles == 0 or n_vertices == 0 is valid (the arrays of that length may be NULL).  Errors, all before any launch: TVR_ERR_INVALID for a NULL pointer, a negative
 *   count, an undersized buffer, a misaligned scratch, declared output counts above n_vertices / n_triangles; TVR_ERR_UNSUPPORTED for a count above 2^31 - 1 (int32
 *   indices).  The two *_scratch_bytes functions return 0 for such counts. */
size_t tvr_mesh_components_scratch_bytes(int64_t n_vertices, int64_t n_triangles);
int tvr_mesh_components(const int32_t *faces, int64_t n_triangles, int64_t n_vertices, int32_t *vertex_label, size_t vertex_label_bytes, int32_t *component_faces,
                        size_t component_faces_bytes, int64_t *n_components_dev, void *scratch, size_t scratch_bytes, uint32_t *fault_flag_dev, void *stream);
size_t tvr_mesh_filter_scratch_bytes(int64_t n_vertices, int64_t n_triangles);
int tvr_mesh_filter_count(const int32_t *faces, int64_t n_triangles, int64_t n_vertices, const int32_t *vertex_label, const uint8_t *keep_root, void *scratch,
                          size_t scratch_bytes, int64_t *counts_dev, uint32_t *fault_flag_dev, void *stream);
int tvr_mesh_filter_emit(const float *verts, const int32_t *faces, int64_t n_triangles, int64_t n_vertices, const void *scratch, size_t scratch_bytes, float *verts_out,
                         size_t verts_out_bytes, int64_t n_vertices_out, int32_t *faces_out, size_t faces_out_bytes, int64_t n_triangles_out, int32_t *kept_vertex,
                         size_t kept_vertex_bytes, uint32_t *fault_flag_dev, void *stream);

/* Mesh simplification by vertex clustering (Rossignac-Borrel; csrc/tvr_mesh_simplify.hip): vertices are snapped to a regular lattice of cells, each cell's vertices
 * merge into their mean, triangles are re-indexed, collapsed ones and exact duplicates go.  ADDITIVE exports: TVR_VERSION is unchanged.
 *   verts [n_vertices][3] fp32, faces [n_triangles][3] int32; origin / cell / inv_cell: three HOST floats each, inv_cell = 1 / cell computed by the caller (the kernels
 *   never divide by cell).  All arithmetic below is fp32 with every operation rounded on its own, except where stated.
 * Cell of a vertex, per axis: g = (v - origin) * inv_cell, c = floorf(g).  A coordinate exactly on a cell boundary belongs to the UPPER cell.  (Marching-cubes vertices
 *   lie on grid edges: with cell a whole number of voxels and origin the volume's, most vertices have two coordinates exactly on a boundary — the common case.)  A vertex
 *   with !(0 <= c && c < 2^21) on any axis (NaN, infinity, anything outside the lattice) sets *fault_flag_dev and no output is written.  key = cx | cy << 21 | cz << 42.
 * Cluster = the vertices with the same key.  Its representative is its SMALLEST old vertex index; new vertices are numbered in ascending order of representative, so
 *   vertex_map [n_vertices] (old -> new) and the vertex order are functions of the mesh alone.
 * Position of a new vertex, per axis: f = g - (float)c (exact), q = (uint32_t)(f * 1048576.0f) (truncates; q < 2^20); sum = the 64-bit INTEGER sum of q over the
 *   cluster, n = its member count; frac = (float)((double)sum / ((double)n * 1048576.0)); pos = (origin + (float)c * cell) + frac * cell, with c the cell of the
 *   cluster.  Integer sums make the mean independent of the order the atomics land in; no float is added atomically anywhere.
 * Triangles: corners are mapped through vertex_map.  A triangle with two equal new corners is dropped.  Of the triangles whose new corner triples are equal up to
 *   ROTATION (the same orientation) only the one with the smallest old index survives; the reverse orientation is a different triangle and stays.  Survivors keep their
 *   relative order and their own corner order.
 * NOT promised: manifoldness, closedness.  Unused vertices DO occur: every cluster gets a vertex whether or not a surviving triangle uses it (an input vertex no
 *   triangle uses is clustered like any other).
 * Two steps, because the output sizes are results (as tvr_mesh_count / tvr_mesh_emit):
 *   tvr_mesh_simplify_count fills `scratch` (tvr_mesh_simplify_scratch_bytes, 256-byte aligned) and leaves {n_vertices', n_triangles'} in counts_dev[2];
 *   tvr_mesh_simplify_emit with the SAME inputs and scratch writes verts_out [n_vertices_out][3], faces_out [n_triangles_out][3] and vertex_map [n_vertices].  The
 *   declared counts are the capacities: no store happens at or beyond them, and if they are not the counted totals the flag is set and nothing is written.
 * Mechanism: two insert-only open-addressing hash tables in scratch (linear probing, capacity a power of two >= max(256, 2 x elements)).  Cells: 64-bit atomicCAS on the
 *   key, 32-bit atomicMin on the representative.  Triangles: a slot holds a triangle index, claimed by atomicCAS from empty; an occupant whose mapped triple equals one's
 *   own is joined by atomicMin, another is probed past; nothing is deleted, so equal keys meet in one slot.  Every probe sequence is bounded by the capacity and gives up
 *   by setting the flag (which is only ever set; the caller zeroes it).  No loop waits for another workgroup.  The survivor flags are scanned by the reduce / scan / add
 *   scheme above.  After the count the scratch's second uint32 holds the longest probe sequence seen, in slots (diagnostic: it
 *   depends on the order insertions land in; no output does).
 * Scratch, linear in the counts: 256 B + 9 B per element of max(n_vertices, n_triangles) rounded up to TVR_MESH_TILE (flags and scans, + 8 B per tile) + per vertex 4 B
 *   (representative) + 32 B (member count and three sums) + 12 B per cell slot (2 to 4 slots a vertex) + per triangle 4 B (slot) + 4 B per triangle slot (2 to 4 a
 *   triangle): at most 84 B per vertex + 20 B per triangle + the 9 B per element, each array rounded up to 256 B.
 * A face index outside 0 .. n_vertices-1 sets the flag and nothing else is written; no load or store leaves the caller's buffers whatever faces and verts hold.
 * n_vertices == 0 or n_triangles == 0 is valid input and a valid result (arrays of that length may be NULL).  Errors, all before any launch: TVR_ERR_INVALID for a NULL
 *   pointer, a negative count, an undersized buffer, a misaligned scratch, a non-positive or non-finite cell / inv_cell, declared output counts above the inputs';
 *   TVR_ERR_UNSUPPORTED for a count above 2^31 - 1; tvr_mesh_simplify_scratch_bytes then returns 0. */
size_t tvr_mesh_simplify_scratch_bytes(int64_t n_vertices, int64_t n_triangles);
int tvr_mesh_simplify_count(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const float origin[3], const float cell[3],
                            const float inv_cell[3], void *scratch, size_t scratch_bytes, int64_t *counts_dev, uint32_t *fault_flag_dev, void *stream);
int tvr_mesh_simplify_emit(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const float origin[3], const float cell[3],
                           const float inv_cell[3], void *scratch, size_t scratch_bytes, float *verts_out, size_t verts_out_bytes, int64_t n_vertices_out,
                           int32_t *faces_out, size_t faces_out_bytes, int64_t n_triangles_out, int32_t *vertex_map, size_t vertex_map_bytes,
                           uint32_t *fault_flag_dev, void *stream);

/* Vertex adjacency of an indexed triangle mesh, with the number of face sides on every edge (csrc/tvr_mesh_smooth.hip): the structure that says whether a mesh is closed
 * and the one smoothing gathers over.  ADDITIVE exports: TVR_VERSION is unchanged.  faces [n_triangles][3] int32 indexes n_vertices vertices.
 *   Sides: a face (a, b, c) has the three sides {a,b}, {b,c}, {c,a}; a side with two equal ends is ignored (a face (a, a, b) still gives the side {a,b}, twice;
 *   a face (a, a, a) gives none).  Orientation is ignored: {a,b} and {b,a} are the same side.
 *   Neighbours: u is a neighbour of v iff some side is {u, v}.  The row of v holds its DISTINCT neighbours in ASCENDING order; a vertex no side uses has an empty row.
 *   offsets [n_vertices + 1] int32: offsets[0] = 0, row v = neighbours[offsets[v] .. offsets[v+1] - 1], offsets[n_vertices] = H, the number of half-edges (every
 *   undirected edge appears twice, once in each end's row).  neighbours [H] int32.
 *   edge_faces [H] int32, parallel to neighbours: the number of sides equal to that edge, counted over all faces — a face listed twice counts twice, a reversed face
 *   counts like any other.  1 = a boundary edge, 2 = the edge of a closed 2-manifold, above 2 = a non-manifold edge.
 *   A mesh is closed iff no edge_faces is 1.  The output is a function of (faces, n_vertices) alone: the same on every run.
 * Two steps, because H is a result (as tvr_mesh_count / tvr_mesh_emit):
 *   tvr_mesh_adjacency_count fills `scratch` (tvr_mesh_adjacency_scratch_bytes, 256-byte aligned) and leaves counts_dev[4] int64 = {H, boundary_edges, nonmanifold_edges,
 *   max_degree}: boundary_edges = UNDIRECTED edges with edge_faces == 1, nonmanifold_edges = those with edge_faces > 2, max_degree = the longest row.
 *   tvr_mesh_adjacency_emit with the SAME faces, counts and scratch writes offsets, neighbours and edge_faces.  n_half_edges is the capacity of the two arrays AND must
 *   be the counted H: no store happens at or beyond it, and if it is not the counted H *fault_flag_dev becomes 1 and NOTHING is written (offsets included).
 *   A face index outside 0 .. n_vertices-1 sets the flag at count time (the four counts are then 0) and makes the following emit set it again and write nothing; no load
 *   or store leaves the caller's buffers whatever `faces` holds.  The flag is only ever set; the caller zeroes it.
 * Mechanism: every side adds 1 to the RAW degree of both ends (32-bit atomicAdd); a 32-bit reduce / scan / add over tiles of TVR_MESH_TILE entries gives the raw row
 *   starts; every side writes each end into the other's raw row through a per-row cursor (atomicAdd; the order inside a raw row is the only thing that depends on the order
 *   atomics land in); every raw row is sorted and run-length encoded, which yields the distinct neighbours, edge_faces and the degree: a raw row of at most
 *   TVR_MESH_ADJ_SHORT_ROW entries by ONE THREAD (insertion sort), a longer one by ONE WORKGROUP (a bitonic network for any length, log2(n)(log2(n)+1)/2 passes of n/2
 *   comparators over 256 lanes, then two block scans); a scan of the degrees gives offsets; the emit copies row fronts.  No float is involved, no loop waits for another
 *   workgroup, every loop is bounded by a count below 2^31.
 * Scratch, linear in the counts: 256 B + per vertex 16 B (degree, long-row slot, raw row start, offset) + 4 B per TVR_MESH_TILE vertices + per triangle 48 B (6 raw
 *   entries and their 6 counts), each array rounded up to 256 B.
 * n_vertices == 0 or n_triangles == 0 is valid (offsets always has its n_vertices + 1 entries; arrays of length 0 may be NULL).  Errors, all before any launch:
 *   TVR_ERR_INVALID for a NULL pointer, a negative count, an undersized buffer, a misaligned scratch; TVR_ERR_UNSUPPORTED for n_vertices or 6 * n_triangles above
 *   2^31 - 1 (H <= 6 * n_triangles and indices are int32); tvr_mesh_adjacency_scratch_bytes then returns 0. */
#define TVR_MESH_ADJ_SHORT_ROW 64
size_t tvr_mesh_adjacency_scratch_bytes(int64_t n_vertices, int64_t n_triangles);
int tvr_mesh_adjacency_count(const int32_t *faces, int64_t n_triangles, int64_t n_vertices, void *scratch, size_t scratch_bytes, int64_t *counts_dev,
                             uint32_t *fault_flag_dev, void *stream);
int tvr_mesh_adjacency_emit(const int32_t *faces, int64_t n_triangles, int64_t n_vertices, const void *scratch, size_t scratch_bytes, int32_t *offsets,
                            size_t offsets_bytes, int32_t *neighbours, size_t neighbours_bytes, int32_t *edge_faces, size_t edge_faces_bytes, int64_t n_half_edges,
                            uint32_t *fault_flag_dev, void *stream);

/* Taubin lambda|mu smoothing of vertex positions over that adjacency (csrc/tvr_mesh_smooth.hip).  ADDITIVE export.  verts / verts_out [n_vertices][3] fp32; offsets,
 * neighbours, edge_faces as above (any CSR with offsets non-decreasing from 0 to n_half_edges and neighbours in 0 .. n_vertices-1 is taken; the sums follow ITS order).
 *   All arithmetic is fp32 and every operation is rounded on its own (no fused multiply-add); the division is IEEE correctly rounded.
 *   One iteration = two half steps, the first with weight w = lambda, the second with w = mu.  In a half step every vertex v, per axis, with deg = its row's length:
 *     deg == 0, or v pinned:  p'[v] = p[v]
 *     else  s = p[n_0]; s = s + p[n_k] for k = 1 .. deg-1 in the row's stored order (the sum STARTS from the first neighbour, not from zero: -0.0 survives);
 *           m = s / (float)deg;  d = m - p[v];  t = w * d;  p'[v] = p[v] + t
 *   Every vertex of a half step reads the positions the previous half step left (Jacobi, not Gauss-Seidel): one launch per half step over two buffers of the scratch,
 *   the last one into verts_out; no atomics, no grid-wide barrier, so the result is a function of the arguments alone: bit-identical from run to run.
 *   pin_boundary != 0: v is pinned iff one of its edges has edge_faces == 1.  pin_boundary == 0: nothing is pinned and edge_faces may be NULL.
 *   iterations == 0 copies verts to verts_out bit for bit.  Non-finite coordinates are not an error: they spread to neighbours as the arithmetic dictates.
 * A first kernel checks the adjacency: offsets[0] == 0, offsets non-decreasing, offsets[n_vertices] == n_half_edges, every neighbour in 0 .. n_vertices-1.  A violation
 *   sets *fault_flag_dev (only ever set; the caller zeroes it), every later kernel returns at once and verts_out stays unwritten.  The gather re-checks every index it
 *   uses, so no load leaves the caller's buffers whatever they hold.
 * scratch: tvr_mesh_smooth_scratch_bytes, 256-byte aligned: 256 B + 2 x 16 B per vertex (positions are kept as 16-byte rows {x, y, z, pinned}).
 * Errors, all before any launch: TVR_ERR_INVALID for a NULL pointer where data is due, a negative count, iterations outside 0 .. TVR_MESH_SMOOTH_MAX_ITERATIONS, a
 *   non-finite lambda or mu, verts_out_bytes != 12 * n_vertices, too little or misaligned scratch; TVR_ERR_UNSUPPORTED for a count above 2^31 - 1;
 *   tvr_mesh_smooth_scratch_bytes then returns 0.
 * NOT promised: that vertices stay on the iso-surface (they leave it), that self-intersections go, that the volume is kept (Taubin keeps it approximately). */
#define TVR_MESH_SMOOTH_MAX_ITERATIONS 1000
size_t tvr_mesh_smooth_scratch_bytes(int64_t n_vertices, int64_t n_half_edges);
int tvr_mesh_smooth(const float *verts, int64_t n_vertices, const int32_t *offsets, const int32_t *neighbours, const int32_t *edge_faces, int64_t n_half_edges,
                    int32_t iterations, float lambda, float mu, int32_t pin_boundary, void *scratch, size_t scratch_bytes, float *verts_out, size_t verts_out_bytes,
                    uint32_t *fault_flag_dev, void *stream);

/* Newton projection of mesh vertices onto the iso-surface of the density field (csrc/tvr_mesh_project.hip).  ADDITIVE export: TVR_VERSION is unchanged.
 * THE SURFACE.  alpha(p) = 1 - exp(-feature2density(f(p)) * length) = level is the set f(p) = f*, where f is tvr_density_feature's value at normalize_coord(p) and
 *   f* = feature2density^-1(sigma*), sigma* = -log1p(-level) / length;  softplus: f* = log(expm1(sigma*)) - density_shift;  relu: f* = sigma* (> 0).
 *   `length` is what getDenseAlpha passes to compute_alpha, the scene's step_size.  The HOST computes f* in fp64 and passes it rounded to one float, target_feature.
 *   LIMITATION: the alpha mask is NOT consulted.  Where a mask cuts alpha to zero inside the f >= f* region, the exported surface follows the mask's boundary while this
 *   call pulls vertices towards f = f*, up to max_move away.
 * INPUTS.  verts [n_vertices][3] fp32: WORLD positions where the field was sampled.  pinned [n_vertices] uint8 or NULL: non-zero = copy the vertex through.
 *   iterations N in 0 .. TVR_MESH_PROJECT_MAX_ITERATIONS.  half_width[3]: tvr_density_gradient's, normalised units.  max_move[3]: world units, the half edges of the
 *   trust box about the input vertex.  tol >= 0: feature units.
 * PER VERTEX, with p_0 the input, lo / hi / inv the scene's aabb[0], aabb[1] and inv_aabb_size; every operation below is fp32 and rounded on its own (no fused
 *   multiply-add), in exactly this order; the division is IEEE correctly rounded:
 *     n_k = (p_k - lo) * inv - 1                                       (normalize_coord's three operations, per axis)
 *     (f_k, g_k) = tvr_density_gradient's (sigma_feature, grad) at n_k for half_width, bit for bit (the same per-point code, csrc/tvr_gradient.h)
 *     r_k = f_k - f*
 *   step (k < N):
 *     gw = g_k * inv                                                   (the world-space gradient, per axis)
 *     s  = r_k / max((gw.x * gw.x + gw.y * gw.y) + gw.z * gw.z, 1e-30)
 *     q  = p_k - s * gw                                                (per axis: one product, one difference)
 *     p_{k+1} = min(max(min(max(q, p_0 - max_move), p_0 + max_move), lo), hi)      (the trust box first, then the aabb; p_0 -+ max_move are rounded fp32 sums)
 *   result: the first p_k, k = 0 .. N, with |r_k| <= tol — the vertex is CONVERGED and iterates no further; otherwise the p_k with the smallest |r_k|, the smaller k on
 *     a tie.  Hence |residual_out| <= |r_0| always, with equality only where the result is p_0.
 *   exceptions: a pinned vertex, and every vertex when N = 0, is copied through bit for bit (r_0 is still evaluated; it is converged iff |r_0| <= tol).  A non-finite
 *     p_0, a non-finite r_k or a non-finite q (before the clamps) at any k FREEZES the vertex at its best iterate so far (p_0 if there is none) and counts it as
 *     non-finite; no load leaves the scene's buffers whatever the coordinates are.  A zero gradient gives s * gw = 0: q = p_k, which only the clamps can move.
 *     A vertex outside the aabb is clamped INTO it by its first step, even beyond max_move.
 * OUTPUTS.  verts_out [n_vertices][3] (may alias verts).  residual_in [n_vertices] or NULL = r_0.  residual_out [n_vertices] = r at the result, bit-equal to
 *   tvr_density_feature(normalize_coord(result)) - f* (for a vertex frozen with no finite residual: r_0 as evaluated).  counts_dev [4] int64 on the device, ZEROED BY THE
 *   CALL on `stream`: {converged, moved (result != p_0 in some bit), clamped (a clamp changed q at least once), non-finite}.
 *   No position depends on an atomic or on another vertex: the outputs are the same bit for bit on every run, for every batch split and vertex order.
 * Mechanism: VM scenes a quad of lanes per vertex, CP scenes a lane per vertex (tvr_density_gradient's mappings); N + 1 gradient evaluations in registers, a finished
 *   vertex is held, not retired (wave-uniform trip count); no scratch, no LDS; the counters are one ballot + one 64-bit atomic add per wave and counter.
 * VM scenes of every variant and CP scenes are taken; an attached density volume is not used (the factored form, as tvr_density_gradient).
 * Errors, all before any launch: TVR_ERR_INVALID for a NULL scene / counts_dev / half_width / max_move, a scene without parameters, n_vertices < 0, NULL verts /
 *   verts_out / residual_out with n_vertices > 0, iterations outside the range, a non-finite or non-positive half_width or max_move, a non-finite target_feature, tol < 0
 *   or NaN; TVR_ERR_UNSUPPORTED for n_vertices above 2^31 - 1; TVR_ERR_SCRATCH for an output buffer that is too short (tvr_last_error() names it).
 *   n_vertices == 0 succeeds and launches no kernel.  No host read happens inside the call.
 * NOT promised: that triangles keep their orientation or do not fold over (the only guard is the trust box); anything about surfaces an alpha mask cut. */
#define TVR_MESH_PROJECT_MAX_ITERATIONS 64
int tvr_mesh_project(tvr_scene *scene, const float *verts, int64_t n_vertices, const uint8_t *pinned /* or NULL */, float target_feature, int32_t iterations,
                     const float half_width[3], const float max_move[3], float tol, float *verts_out, size_t verts_out_bytes, float *residual_in /* or NULL */,
                     size_t residual_in_bytes, float *residual_out, size_t residual_out_bytes, int64_t *counts_dev /* [4], zeroed by the call */, void *stream);

/* Depth-buffer rasteriser for indexed triangle meshes in the camera conventions of rays.py (csrc/tvr_mesh_raster.hip): what puts an exported mesh into the image space
 * of tvr_render / tvr_render_normals.  ADDITIVE exports: TVR_VERSION is unchanged.  verts [n_vertices][3] fp32 WORLD positions, faces [n_triangles][3] int32.
 * All arithmetic is fp32 with every operation rounded on its own (no fused multiply-add), in exactly the order written; divisions and the square root are IEEE correctly
 * rounded.  A dot product a . b is (a.x * b.x + a.y * b.y) + a.z * b.z; a cross product a x b is (a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x).
 * CAMERA (tvr_mesh_camera).  c2w[12]: 3 x 4 row-major, the matrix rays.get_rays takes (after the BLENDER2OPENCV product); R = its 3 x 3 part, o = its last column.
 *   Pixel p = j * W + i has the camera-space direction dir = (-(((i + .5) - cx) / fx), ((j + .5) - cy) / fy, -1): rays.get_ray_directions, so pixel p's ray is row p of
 *   rays.frame_rays.  A vertex goes to camera space as q = R^T (v - o): d = v - o, q_k = (d_0 * R[0][k] + d_1 * R[1][k]) + d_2 * R[2][k]; the point o + s * R * dir of
 *   the pixel's ray is q = s * dir.  The camera looks along -z: a corner's camera depth is -q.z.
 * COVERAGE: homogeneous edge functions, no clipping (a triangle that crosses the camera plane is handled by the same test).  For triangle t with camera-space corners
 *   q0, q1, q2 (vertex indices v0, v1, v2):  n_0 = q1 x q2, n_1 = q2 x q0, n_2 = q0 x q1;  det = q0 . n_0;  sg = +1 if det > 0, -1 if det < 0.  A triangle with det == 0
 *   (or NaN) or a non-finite camera-space coordinate is SKIPPED and counted.  E_k = sg * (dir . n_k).  Edge k runs from corner (k+1)%3 to corner (k+2)%3; the pixel is
 *   covered iff for every k: E_k > 0, or E_k == 0 and owner_k, with owner_k = (vertex index at the edge's start < vertex index at its end) XOR (sg < 0).
 *   a x b and b x a are exact negations of each other, so two triangles that share an edge evaluate it to exactly opposite values: a ray through the shared edge of two
 *   equally facing triangles is claimed by exactly one of them — no pinholes, no double claims, whatever the rounding of the values.  ACCEPTED: a ray exactly through a
 *   vertex (two E_k == 0) may be claimed by none of the fan around it.
 *   cull != 0 drops the triangles with det > 0: for a proper rotation R those are the ones whose outward side (right-hand rule, the orientation of tvr_mesh_emit with
 *   flip == 0) faces away from the camera; det < 0 faces it.
 * DEPTH, from the triangle's plane (det / sum of E loses four digits to cancellation at a camera distance of 4; the plane form does not):
 *   pn = (q1 - q0) x (q2 - q0);  s = (pn . q0) / (dir . pn);  depth = s * sqrt(dir . dir)  — the Euclidean distance from o, what tvr_render's depth_map measures along the
 *   loader's unit directions.  A covered pixel counts only if depth is finite and > near.
 * BOX.  A triangle is offered the pixels of its screen box only.  With z_k = -q_k.z:  all three z_k <= 0: no pixel (wholly behind).  Some z_k <= 0: the whole image (the
 *   price of not clipping).  Else u_k = cx - fx * (q_k.x / z_k), w_k = cy + fy * (q_k.y / z_k), and the box is  i in max(ceil(min u - 1.5), 0) .. min(floor(max u + .5), W-1),
 *   j likewise from w and H: the pixels whose centres lie within one pixel of the corners' extent.  The pad is three orders of magnitude above the rounding of the
 *   edge functions for any triangle that is not a sliver of a 10^-4 of a pixel, so the box changes no result; it is part of the definition so that it is one.
 * RESULT per pixel: the covered triangle with the smallest depth; ties in depth go to the smallest triangle index.
 *   depth [H*W] fp32, +inf where nothing is hit;  tri [H*W] int32, -1 where nothing is hit;  bary [H*W][3]: b_k = E_k / ((E_0 + E_1) + E_2) of the winner, zeros where
 *   nothing is hit;  attr_out [H*W][n_attr] (attr [n_vertices][n_attr], n_attr <= TVR_MESH_RASTER_MAX_ATTR) = (b_0 * a[v0] + b_1 * a[v1]) + b_2 * a[v2], zeros where
 *   nothing is hit;  counts_dev int32[4], zeroed by the call on `stream` (unless the fault flag is raised) = {pixels hit, triangles skipped, triangles that covered no pixel (culled, behind, off screen
 *   or between pixel centres; whether another triangle won the pixel does not matter), triangles that took the large path}.
 *   depth, tri, bary, attr_out and the first three counts are functions of (mesh, camera) alone: they do not depend on launch geometry, on the order atomics land in,
 *   or on large_bbox.
 * Mechanism, one fixed launch sequence without a host read: check the face indices; clear H*W 64-bit keys to all ones; one lane per triangle sets it up and walks a box
 *   of at most large_bbox pixels (0 = TVR_MESH_RASTER_LARGE_BBOX) itself, a larger one goes to a queue (one atomic add per wave); a fixed grid of workgroups then draws the queue's
 *   entries, 256 lanes striding over one box, a box shared by grid / entries workgroups when there are fewer entries than workgroups; a last kernel unpacks every pixel's key and recomputes E_k, b_k and the attributes by the same expressions.  A claim is
 *   one 64-bit atomicMin of (depth bits << 32) | t (depth > 0: the bit pattern orders as the value), skipped when a relaxed agent-scope load shows a key that is not
 *   larger (keys only decrease: a stale read can cost a redundant atomic, never a wrong skip).  No workgroup waits for another.
 *   A face index outside 0 .. n_vertices-1 sets *fault_flag_dev = 1 and NOTHING else is written (the flag is only ever set; the caller zeroes it).  No load or store
 *   leaves the caller's buffers whatever faces, verts and scratch hold.
 * scratch: tvr_mesh_raster_scratch_bytes (256-byte aligned): 256 B + 8 B per pixel + 4 B per triangle, each array rounded up to 256 B; 0 for counts out of range.
 * n_triangles == 0 is valid and yields an empty image (verts / faces may then be NULL).  Errors, all before any launch: TVR_ERR_INVALID for a NULL cam / depth / tri /
 *   bary / scratch / counts_dev / fault_flag_dev, NULL faces or verts where there are triangles, a negative count, H or W < 1, a non-finite camera entry, fx or fy <= 0,
 *   near < 0 or non-finite, cull outside 0 / 1, large_bbox < 0, n_attr outside 0 .. TVR_MESH_RASTER_MAX_ATTR, attr or attr_out NULL with n_attr > 0, a misaligned scratch;
 *   TVR_ERR_UNSUPPORTED for H * W, n_triangles or n_vertices >= 2^31 and for H or W above TVR_MESH_RASTER_MAX_SIDE = 2^24 (beyond it a pixel centre i + .5
 *   and the box's clamp (float)(W - 1) are no longer exact fp32 numbers, and "inside the image by construction" would not hold); TVR_ERR_SCRATCH for an undersized depth / tri / bary / attr_out / scratch (tvr_last_error()
 *   names the buffer).
 * NOT promised: anti-aliasing (one sample at the pixel centre), anything about rays exactly through a vertex, a facing rule for an improper R. */
#define TVR_MESH_RASTER_LARGE_BBOX 64
#define TVR_MESH_RASTER_MAX_ATTR 8
#define TVR_MESH_RASTER_MAX_SIDE 16777216          /* 2^24: the largest H or W */
typedef struct {
    float c2w[12];
    int32_t H, W;
    float fx, fy, cx, cy;
    float near_;                   /* >= 0 */
    int32_t cull;                  /* 0 / 1 */
    int32_t large_bbox;            /* pixels; 0 = TVR_MESH_RASTER_LARGE_BBOX */
} tvr_mesh_camera;
size_t tvr_mesh_raster_scratch_bytes(int64_t n_triangles, int32_t H, int32_t W);
int tvr_mesh_raster(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const tvr_mesh_camera *cam, const float *attr /* or NULL */,
                    int32_t n_attr, float *depth, size_t depth_bytes, int32_t *tri, size_t tri_bytes, float *bary, size_t bary_bytes, float *attr_out /* or NULL */,
                    size_t attr_out_bytes, void *scratch, size_t scratch_bytes, int32_t *counts_dev /* [4] */, uint32_t *fault_flag_dev, void *stream);

/* Per-triangle texture atlas of an indexed triangle mesh (csrc/tvr_mesh_texture.hip): colour resolution that does not depend on the triangle count.  ADDITIVE exports:
 * TVR_VERSION is unchanged.  No UV unwrapping: every triangle gets its own right-angled patch, two triangles share a square, the layout is closed-form, and the atlas is
 * a function of (mesh, field, patch size) alone.  All device arithmetic is fp32 with every operation rounded on its own (no fused multiply-add), in exactly the order
 * written; divisions are IEEE correctly rounded.
 * PARAMETERS.  P = patch side in texels, TVR_MESH_ATLAS_MIN_P = 5 <= P <= TVR_MESH_ATLAS_MAX_P = 64;  L = P - 4 = texel steps along a patch edge (an edge carries L + 1
 *   samples);  F = n_triangles, S = ceil(F / 2) squares;  C >= 1 squares per atlas row.  The atlas is Wa = C * P texels wide and Ha = max(ceil(S / C), 1) * P high (so
 *   Ha >= P even for F = 0), row-major: the linear index of texel (X, Y) is Y * Wa + X.  Ha * Wa < 2^31.
 * PLACEMENT.  Triangle t lives in square s = t >> 1, half h = t & 1; the square's corner texel is (X0, Y0) = ((s % C) * P, (s / C) * P).  Texel (a, b) of a square,
 *   0 <= a, b < P, belongs to half 0 if a + b <= P - 1, with local coordinates (x, y) = (a, b); else to half 1 with (x, y) = (P - 1 - a, P - 1 - b).  Every texel has
 *   exactly one owner or none: none when its square is >= S, or when it lies in half 1 of the last square and F is odd.  Those report triangle -1.
 * TEXEL TO POINT.  Local (x, y) of triangle t with corners v0, v1, v2 (faces[t][0..2]):  b1 = x / L, b2 = y / L, b0 = (1 - b1) - b2 (x, y, L converted to fp32, exact);
 *   p = (b0 * v0 + b1 * v1) + b2 * v2 per coordinate.  The corner texels (0,0), (L,0), (0,L) reproduce v0, v1, v2 exactly for finite vertices (a coordinate -0 comes out
 *   +0).  Texels with x + y > L are the GUTTER: extrapolated in the triangle's plane, not clamped, so the texture samples one continuous function across the hypotenuse.
 * SAMPLING a hit (t, b0, b1, b2) (tvr_mesh_raster's tri and bary):  x = min(max(b1 * L, 0), L), y = min(max(b2 * L, 0), L) (a NaN becomes 0);  i = floor(x),
 *   j = floor(y), fx = x - i, fy = y - j;  the taps T00 = T(i, j), T10 = T(i+1, j), T01 = T(i, j+1), T11 = T(i+1, j+1) are texels in the half's LOCAL coordinates, mapped
 *   to the atlas by the half's rule;  top = T00 + fx * (T10 - T00), bot = T01 + fx * (T11 - T01), out = top + fy * (bot - top), per channel.  uint8 texels are converted
 *   to fp32 as they are (0 .. 255, no scaling).
 * WHY L = P - 4.  With exact barycentrics the four taps have x + y <= L + 1; with the rasteriser's rounded ones (b1 + b2 may exceed 1 by an ulp) x + y <= L + 2 = P - 2.
 *   Both halves own their texels up to exactly that sum (half 0: a + b <= P - 1; half 1: x + y <= P - 2), so no tap of a hit reads the other triangle's texels or leaves
 *   the square; one more ring is left for an external viewer's filtering.
 * tvr_mesh_atlas_points: the n texels with linear indices texel0 .. texel0 + n - 1 (a range, so that a bake is chunked and its memory bounded):  pos_out [n][3] fp32 the
 *   point, tri_out [n] int32 the owner; unowned texels get -1 and a zero point.  One lane per texel.  A face index outside 0 .. n_vertices-1 in a triangle of the square
 *   rows the range touches (every triangle a texel of the range can belong to; the whole mesh when the range is the whole atlas) sets *fault_flag_dev = 1 and NOTHING
 *   else is written; the flag is only ever set, the caller zeroes it, and a flag that is already up on entry likewise keeps the call from writing.
 * tvr_mesh_texture_sample: per pixel p of a tvr_mesh_raster result (tri [n_pix], bary [n_pix][3]) the sampling rule on `atlas` [Ha][Wa][3], fmt 0 = uint8, 1 = fp32;
 *   out [n_pix][3] fp32, zeros where tri < 0 or tri >= n_triangles.  Every tri is compared with n_triangles and every tap's index with Ha * Wa before a load (a tap
 *   outside reads as 0; none is for a consistent atlas).  bary values that are no barycentrics (b1 + b2 far above 1) stay inside the square but may read the other half.
 * Both are memory-bound gathers without atomics, LDS or scratch: 16 B written per texel (the 36 + 12 B of a triangle are shared by its ~P^2 / 2 texels);
 *   16 B read + 4 taps x 3 B (uint8) or x 12 B (fp32) gathered + 12 B written per pixel.  No load or store leaves the caller's buffers whatever faces, tri and bary hold.
 * n_triangles == 0, n == 0 and n_pix == 0 are valid (the arrays of that length may be NULL).  Errors, all before any launch, tvr_last_error() names the argument:
 *   TVR_ERR_INVALID for a NULL pointer where data is due, a negative count, P outside 5 .. 64, C < 1, a range that leaves the atlas, fmt outside 0 / 1, Ha or Wa that
 *   are not the ones F, P, C make;  TVR_ERR_UNSUPPORTED for Ha * Wa, n_triangles, n_vertices or n_pix >= 2^31;  TVR_ERR_SCRATCH for an undersized pos_out / tri_out / out.
 * TEXTURE COORDINATES of a file (host side, float64; mesh.atlas_uv): corner k of triangle t sits at the atlas texel (X, Y) of its local corner (0,0), (L,0), (0,L);
 *   u = (X + .5) / Wa, v = 1 - (Y + .5) / Ha, image row 0 = Y = 0.
 * NOT promised: seams under mip-mapping beyond one ring, view-dependent colour, any packing of patches by triangle size (a sliver gets the patch of a large triangle). */
#define TVR_MESH_ATLAS_MIN_P 5
#define TVR_MESH_ATLAS_MAX_P 64
int tvr_mesh_atlas_points(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, int32_t P, int32_t C, int64_t texel0, int64_t n,
                          float *pos_out, size_t pos_bytes, int32_t *tri_out, size_t tri_bytes, uint32_t *fault_flag_dev, void *stream);
int tvr_mesh_texture_sample(const int32_t *tri, const float *bary, int64_t n_pix, const void *atlas, int32_t fmt, int32_t Ha, int32_t Wa, int32_t P, int32_t C,
                            int64_t n_triangles, float *out, size_t out_bytes, void *stream);

/* Ray queries against an indexed triangle mesh (csrc/tvr_mesh_bvh.hip): a linear bounding-volume hierarchy over the triangles, closest-hit and any-hit casts of
 * arbitrary rays, and the cosine-weighted openness (ambient occlusion) of points on the mesh.  ADDITIVE exports: TVR_VERSION is unchanged.  DESIGN.md §4.17.
 * verts [n_vertices][3] fp32, faces [n_triangles][3] int32.  All arithmetic is fp32 with every operation rounded on its own (no fused multiply-add), in exactly the order
 * written; divisions are IEEE correctly rounded; dot and cross products are tvr_mesh_raster's.
 * RAY: an origin o and a direction d, fp32; d need not be unit length; t is parametric, the hit point is o + t * d.
 * (RAY, TRIANGLE): tvr_mesh_raster's own expressions with the camera rotation taken as the identity, the camera centre at o and dir = d.  q_k = v_k - o;
 *   n_0 = q1 x q2, n_1 = q2 x q0, n_2 = q0 x q1;  det = q0 . n_0;  sg = +1 if det > 0, -1 if det < 0;  det == 0, NaN or a non-finite q: no hit.  E_k = sg * (d . n_k);
 *   inside iff for every k: E_k > 0, or E_k == 0 and owner_k = (vertex index at the start of edge k < index at its end) XOR (sg < 0), edge k running from corner (k+1)%3
 *   to corner (k+2)%3.  t = (pn . q0) / (d . pn) with pn = (q1 - q0) x (q2 - q0).  A hit needs t finite and t_min < t <= t_max.  cull != 0 drops det > 0.
 *   As in the rasteriser, the two evaluations of a shared edge are exact negations of each other: a ray that passes between two equally facing triangles across their
 *   shared edge belongs to exactly one of them.  NOT promised: anything for a ray exactly through a vertex (it may miss the whole fan).
 * CLOSEST HIT (mode TVR_MESH_BVH_CLOSEST): the hit with the smallest t, ties going to the smaller triangle index.  t [n_rays] (+inf on a miss), tri [n_rays] (-1),
 *   bary [n_rays][3]: b_k = E_k / ((E_0 + E_1) + E_2) (zeros).  ANY HIT (mode TVR_MESH_BVH_ANY): hit [n_rays] uint8 only, 1 iff some triangle is hit; which one was found
 *   is not defined.  The buffers of the other mode may be NULL.  A ray with a non-finite component or d == 0 never hits and is counted (refused).  A triangle with a
 *   non-finite vertex is never hit and is counted by the build.  Results do not depend on the order or the batching of the rays.
 * THE HIERARCHY is a linear BVH (Karras 2012) over 64-bit keys, one per triangle: (30-bit Morton code of the centroid ((v0 + v1) + v2) * (1/3) in the bounding box of
 *   the triangles whose vertices are all finite, 10 bits per axis, x highest) << 32 | triangle index; a triangle with a non-finite vertex or an index outside
 *   0 .. n_vertices-1 gets the largest code 2^30 - 1.
 *   tvr_mesh_bvh_keys writes keys_out [n_triangles]; THE CALLER SORTS THEM ascending (they are unique, so every correct sort gives the same order; the Python side uses
 *   torch.sort on the device); tvr_mesh_bvh_build takes the sorted keys and writes the blob.  build checks that the keys ascend strictly, carry codes below 2^30 and name
 *   every triangle exactly once; if not, or if a face index is outside 0 .. n_vertices-1, *fault_flag_dev = 1, the header's `bad` word is set and no tree is written.
 *   Node numbering: 2F-1 nodes; 0 .. F-2 are internal (0 is the root), node F-1+i is the leaf of the i-th sorted key; F == 1: node 0 is the one leaf; F == 0: no node.
 *   Boxes are exact min / max of the corners; the leaf of a skipped triangle has the empty box lo = +inf, hi = -inf.  Topology: every internal node finds its key range
 *   and its split from the sorted keys alone.  Refit: 62 launches; launch p computes the internal nodes whose two children were finished by an EARLIER launch (a pass
 *   number per node says which), so no workgroup hands data to another inside a launch and the kernel boundary is the only ordering.  The height is at most 62 (the keys
 *   have 62 significant bits, every level splits on one); a root left unfinished raises the fault flag.  No host read anywhere.
 *   The blob is a function of (verts, faces) alone: the same bytes on every run (build zeroes the padding).  60 B per triangle + 256 B.
 *   counts_dev of build (int32[4], may be NULL): {triangles skipped, height, internal nodes, the header's bad word}.
 *   tvr_mesh_bvh_describe gives the blob's layout (byte offsets from its start, strides in bytes): header {uint32 magic, F, bad, height, skipped, 3 reserved; float lo[3],
 *   hi[3] = the root's box}, boxes [2F-1][lo xyz, hi xyz], children [F-1][2] int32 node numbers, leaf_order [F] int32 triangle indices.
 * TRAVERSAL (tvr_mesh_bvh_cast): one lane per ray; a 64-entry stack per lane in LDS; the nearer child is visited first and the farther one pushed, so the stack never
 *   holds more than one entry per level; a push beyond 64 entries is dropped and raises the fault flag.  A node is skipped only if the ray's PADDED slab test misses its
 *   box or enters it at a t strictly greater than the best hit so far (strictly: an equal t may still win the tie on the index).  Padding: every face of the box is moved
 *   outwards by 2^-15 x the largest per-axis distance from o to the box; a stated margin for the rounding of E_k, not a proof.
 *   counts_dev of cast / occlusion (int64[4], may be NULL; zeroed by the call): {rays hit, rays refused, node tests, triangle tests}, summed per wave, one atomic per
 *   wave and counter.  Every index read from the blob and the faces is checked against its bound before use; an inconsistent blob (wrong magic, F, or bad != 0) or an
 *   index outside its range raises the fault flag, and no load or store leaves the caller's buffers.
 * AMBIENT OCCLUSION (tvr_mesh_bvh_occlusion): points [n_points][3], normals [n_points][3], a direction table dirs [n_dirs][3] (finite), bias, t_max; out [n_points].
 *   Per point, for k = 0 .. n_dirs-1 in order: c = dirs_k . n;  d'_k = dirs_k if c >= 0, else -dirs_k;  w_k = d'_k . n (= |c|);  the ray runs from
 *   (p.x + bias * n.x, p.y + bias * n.y, p.z + bias * n.z) along d'_k in any-hit mode over (0, t_max], cull off;  out = (sum w_k * visible_k) / (sum w_k), both sums in k
 *   order.  out = 1 where the normal is zero or non-finite or sum w_k is not > 0.  One lane per point.  counts_dev as for cast, per ray.
 * Errors, all before any launch, tvr_last_error() names the argument: TVR_ERR_INVALID for a NULL pointer where data is due, a negative count, a misaligned blob or
 *   scratch (256 B) or keys (8 B), mode or cull outside 0 / 1, a NaN t_min / t_max, a non-finite bias, n_dirs above TVR_MESH_BVH_MAX_DIRS; TVR_ERR_UNSUPPORTED for
 *   n_triangles above TVR_MESH_BVH_MAX_TRIANGLES (the *_bytes queries then return 0) and for n_vertices, n_rays or n_points >= 2^31; TVR_ERR_SCRATCH for an undersized
 *   blob, scratch, keys or output.  n_triangles == 0 is valid (an empty tree: every ray misses), so are n_rays == 0 and n_points == 0. */
#define TVR_MESH_BVH_MAX_TRIANGLES 1073741824      /* 2^30: the 2F - 1 node numbers fit int32 */
#define TVR_MESH_BVH_MAX_DIRS 65536
#define TVR_MESH_BVH_CLOSEST 0
#define TVR_MESH_BVH_ANY 1
typedef struct {
    size_t header, boxes, children, leaf_order, total;     /* byte offsets from the blob's start; total == tvr_mesh_bvh_bytes */
    size_t box_stride, child_stride, leaf_stride;          /* bytes per node / per internal node / per leaf */
    size_t n_nodes, n_internal;
} tvr_mesh_bvh_layout;
size_t tvr_mesh_bvh_bytes(int64_t n_triangles);
size_t tvr_mesh_bvh_scratch_bytes(int64_t n_triangles);
int tvr_mesh_bvh_describe(int64_t n_triangles, tvr_mesh_bvh_layout *out);
int tvr_mesh_bvh_keys(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, uint64_t *keys_out, size_t keys_bytes, void *scratch,
                      size_t scratch_bytes, uint32_t *fault_flag_dev, void *stream);
int tvr_mesh_bvh_build(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const uint64_t *sorted_keys, void *bvh, size_t bvh_bytes,
                       void *scratch, size_t scratch_bytes, int32_t *counts_dev /* [4] or NULL */, uint32_t *fault_flag_dev, void *stream);
int tvr_mesh_bvh_cast(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, const float *origins,
                      const float *dirs, int64_t n_rays, float t_min, float t_max, int32_t mode, int32_t cull, float *t, size_t t_bytes, int32_t *tri, size_t tri_bytes,
                      float *bary, size_t bary_bytes, uint8_t *hit, size_t hit_bytes, int64_t *counts_dev /* [4] or NULL */, uint32_t *fault_flag_dev, void *stream);
int tvr_mesh_bvh_occlusion(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, const float *points,
                           const float *normals, int64_t n_points, const float *dirs, int32_t n_dirs, float bias, float t_max, float *out, size_t out_bytes,
                           int64_t *counts_dev /* [4] or NULL */, uint32_t *fault_flag_dev, void *stream);

/* The closest point of a mesh to arbitrary points, on the hierarchy above (csrc/tvr_mesh_bvh.hip; mesh.closest_points / mesh_distance).  An ADDITIVE export: TVR_VERSION
 * is unchanged.  DESIGN.md §4.18.  points [n_points][3] fp32; dist [n_points], tri [n_points], bary [n_points][3].  All arithmetic is fp32, every operation rounded on
 * its own (no fused multiply-add), in exactly the order written; divisions and the square root are IEEE correctly rounded; u . v = (u.x * v.x + u.y * v.y) + u.z * v.z.
 * (POINT p, TRIANGLE): translate first, a = v0 - p, b = v1 - p, c = v2 - p (every error is then relative to the distance, not to the coordinates); a pair with a
 *   non-finite component of a, b or c is no candidate.  The point of the triangle closest to the origin by the Voronoi regions (Ericson, Real-Time Collision Detection
 *   §5.1.5):  ab = b - a, ac = c - a, bc = c - b;  d1 = -(ab . a), d2 = -(ac . a), d3 = -(ab . b), d4 = -(ac . b), d5 = -(ab . c), d6 = -(ac . c);
 *   n = ab x ac;  va = (b x bc) . n, vb = (ac x a) . n, vc = (a x ab) . n, with u x v = (u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x).
 *   (In exact arithmetic these are Ericson's d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2; as triple products their error grows with a triangle's aspect
 *   ratio, not with its square — marching cubes makes slivers.)  The regions in this FIXED order, the first that holds gives the closest point x (per axis) and the
 *   weights (w0, w1, w2):
 *     1 vertex A  d1 <= 0 and d2 <= 0                          x = a                          (1, 0, 0)
 *     2 vertex B  d3 >= 0 and d4 <= d3                         x = b                          (0, 1, 0)
 *     3 edge AB   vc <= 0 and d1 >= 0 and d3 <= 0              v = d1 / (d1 - d3)             x = a + v * ab                 (1 - v, v, 0)
 *     4 vertex C  d6 >= 0 and d5 <= d6                         x = c                          (0, 0, 1)
 *     5 edge AC   vb <= 0 and d2 >= 0 and d6 <= 0              w = d2 / (d2 - d6)             x = a + w * ac                 (1 - w, 0, w)
 *     6 edge BC   va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0    w = (d4 - d3) / ((d4 - d3) + (d5 - d6))    x = b + w * bc         (0, 1 - w, w)
 *     7 face      otherwise    den = (va + vb) + vc, v = vb / den, w = vc / den                x = (a + v * ab) + w * ac      ((1 - v) - w, v, w)
 *   D = x . x.  A pair whose D is not finite (NaN: a zero-area triangle that reaches region 7; +inf: an overflow) is no candidate.
 * RESULT: the candidate with the smallest D, ties going to the smaller triangle index, provided D <= max_dist * max_dist (one fp32 product; max_dist = +inf is allowed):
 *   dist = sqrt(D), tri, bary = (w0, w1, w2).  Otherwise, and for an empty tree: dist = +inf, tri = -1, bary = 0.  A point with a non-finite component is refused: the
 *   same outputs, and it is counted.  A point that IS a vertex of the mesh gets dist == 0.0 exactly and the smallest triangle index of that vertex's fan (regions 1, 2, 4
 *   return the translated vertex, which is 0; at corner C, vc is a sum of squares and region 3 does not hold).  A triangle with a non-finite vertex is never named (the build keeps it out of every box).  Results do not depend on the
 *   order or the batching of the points; two runs are bit-equal.
 * TRAVERSAL: the cast's — one lane per point, the 64-entry stack per lane in LDS, 128-lane workgroups, the child with the smaller lower bound first and the other pushed,
 *   a guarded push, a step budget of 2F - 1, a popped node tested again.  A node is skipped only if the lower bound of its box is STRICTLY greater than the best D so far
 *   (max_dist * max_dist before any candidate; strictly: an equal D may still win on the index).  The lower bound: l = lo - p, h = hi - p per axis; m = the largest of
 *   |l|, |h| over the axes; pad = m * 2^-15; g = max(max(l - pad, -(h + pad)), 0) per axis; bound = g . g — the squared distance to the box with every face moved outwards
 *   by pad.  As for the casts, a stated margin for the rounding of D, not a proof; what is tested is bit-equality with a brute-force restatement of the definition.
 *   counts_dev (int64[4], may be NULL; zeroed by the call): {points answered, points refused, node tests, triangle tests}.  Index and blob checks as for the casts.
 * Errors, all before any launch: TVR_ERR_INVALID for a NULL pointer where data is due, a negative count, a misaligned blob, a NaN or negative max_dist;
 *   TVR_ERR_UNSUPPORTED for n_vertices or n_points >= 2^31 and n_triangles above TVR_MESH_BVH_MAX_TRIANGLES; TVR_ERR_SCRATCH for an undersized blob or output.
 *   n_points == 0 and n_triangles == 0 are valid.
 * The sign is tvr_mesh_bvh_signed's, below.  NOT built: k nearest, refitting a tree after its vertices moved. */
int tvr_mesh_bvh_nearest(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, const float *points,
                         int64_t n_points, float max_dist, float *dist, size_t dist_bytes, int32_t *tri, size_t tri_bytes, float *bary, size_t bary_bytes,
                         int64_t *counts_dev /* [4] or NULL */, uint32_t *fault_flag_dev, void *stream);

/* The signed distance to a closed mesh: a table of pseudo-normals (csrc/tvr_mesh_pseudo.hip) and the closest-point query above with a sign (csrc/tvr_mesh_bvh.hip;
 * mesh.build_pseudonormals / signed_distance / contains / signed_distance_grid).  ADDITIVE exports: TVR_VERSION is unchanged.  DESIGN.md §4.19.  Arithmetic as above:
 * fp32, every operation rounded on its own, in the order written, divisions and square roots IEEE correctly rounded, the dot and cross products of tvr_mesh_bvh_nearest.
 * THE TABLE (Baerentzen & Aanaes, "Signed distance computation using the angle weighted pseudonormal", 2005) over (verts, faces):
 *   face_n [F][3]     n_f = (ab x ac) / len per component, ab = v1 - v0, ac = v2 - v0, len = sqrt((ab x ac) . (ab x ac)).  A face with a non-finite vertex coordinate, or
 *                     whose len is not a finite number > 0 (zero area, underflow, overflow), gets (0, 0, 0) and is counted: degenerate_faces.
 *   edge_n [F][3][3]  edge k of face f runs from corner (k+1)%3 to corner (k+2)%3 (tvr_mesh_raster's convention); a half-edge is h = 3 f + k.  The entry of (f, k) is
 *                     the sum, starting from (0, 0, 0), of n_g over ALL half-edges (g, j) on the same undirected edge {smaller vertex index, larger vertex index}, in
 *                     ascending h: both sides of an edge hold the same bits.  Per undirected edge, by the number m of half-edges on it: m == 1 open_edges, m > 2
 *                     nonmanifold_edges, m == 2 and both half-edges leave the same vertex inconsistent_edges (two faces that run the edge in the same direction).
 *                     Half-edges of degenerate faces count like any other (they add zeros); a face (a, b, a) puts two half-edges on {a, b} and one on {a, a}.
 *   vert_n [V][3]     the sum, starting from (0, 0, 0), over the corners (f, k) that hold the vertex, in ascending 3 f + k, degenerate faces left out, of
 *                     angle * n_f per component (one product, one sum), angle = atan2f(|e1 x e2|, e1 . e2) with e1 = v_(k+1)%3 - v_k, e2 = v_(k+2)%3 - v_k and
 *                     |u| = sqrt(u . u).  NOT normalised: only its direction is used.  atan2f is the device library's, not correctly rounded: vert_n is the same
 *                     bits on every run, but is specified as a direction (tests compare it with fp64 as an angle).  A vertex no face uses holds (0, 0, 0).
 *   The mesh is CLOSED (as far as the table can tell) when all four counters are 0; only then do the signs below mean inside / outside.
 *   No float atomics: every sum is formed by one thread in the stated order, so the blob is a function of (verts, faces) alone — the same bytes on every run (build
 *   zeroes the padding).  The counters are integer sums.  256 B + 48 B per triangle + 12 B per vertex, each array rounded up to 256 B.
 *   tvr_mesh_pseudonormals_keys writes two arrays of 3 F uint64 (keys_bytes is the size of EACH): corner_keys_out[c] = vertex << 32 | c for corner c = 3 f + k (unique),
 *   edge_keys_out[h] = smaller vertex << 32 | larger vertex for half-edge h (the two sides of an edge share it); a vertex index outside 0 .. n_vertices-1 gives 2^31 - 1
 *   in its place and raises the fault flag.  THE CALLER SORTS both ascending: the corner keys by any correct sort, the edge keys STABLY and with the permutation
 *   (edge_order[i] = the half-edge whose key is sorted_edge_keys[i], int64, as torch.sort(stable=True) returns it).  tvr_mesh_pseudonormals_build checks: corner keys
 *   strictly ascending, each naming a corner below 3 F exactly once and the vertex the faces hold there; edge keys ascending, equal keys in ascending edge_order, every
 *   half-edge below 3 F exactly once under the key the faces give it; face indices inside 0 .. n_vertices-1.  If not: *fault_flag_dev = 1, the header's `bad` word is set,
 *   the counters read 0 and no normal is to be trusted (the signed query refuses such a table).  The sums run over the sorted runs: the first entry of a run of equal
 *   vertices / equal edge keys walks its run, so a vertex or an edge with k faces costs one thread k steps.  No host read anywhere.
 *   counts_dev of build (int32[4], may be NULL): {degenerate_faces, open_edges, nonmanifold_edges, inconsistent_edges}.
 *   tvr_mesh_pseudonormals_describe gives the blob's layout (byte offsets from its start, strides in bytes): header {uint32 magic, F, V, bad, degenerate_faces,
 *   open_edges, nonmanifold_edges, inconsistent_edges}, face_n [F] x 12 B, edge_n [F] x 36 B (edge k at + 12 k), vert_n [V] x 12 B.
 * THE SIGNED QUERY (tvr_mesh_bvh_signed): traversal, pair arithmetic, tie rule, pruning bound, max_dist and refusals are tvr_mesh_bvh_nearest's, unchanged; tri and bary
 *   are bit-equal to its outputs and |sdist| to its dist.  For the winning triangle the pair is evaluated once more (the same expressions, the same bits), giving the
 *   region r = 1 .. 7 that held and the closest point x in the frame translated to the query point p, so p - closest = -x.  The normal N by region: vert_n of corner A,
 *   B, C for r = 1, 2, 4; edge_n[tri][2], [tri][1], [tri][0] for r = 3 (AB), 5 (AC), 6 (BC); face_n[tri] for r = 7.  s = -(N . x).
 *   sdist = -dist if s < 0, else +dist; +0.0 where dist == 0; +inf where nearest gives +inf.  feature [n_points] int8 = r - 1 (0 .. 6: A, B, AB, C, AC, BC, face),
 *   -1 without an answer.  A point with dist > 0 whose s is 0 or NaN, or whose N is zero or non-finite, is UNDECIDED: it is reported as +dist and counted.
 *   tri, bary and feature may each be NULL and are then not written.
 *   WHY A MISJUDGED REGION IS HARMLESS: rounding can assign a point that lies at the boundary between two regions of a triangle (or of two triangles that tie) to
 *   either.  At the boundary between the face region and an edge or vertex region the closest point lies on that edge or vertex AND p - closest is perpendicular to the
 *   face, i.e. parallel to n_f.  The edge's and the vertex's pseudo-normals are sums of normals of faces that all contain the closest point, n_f among them, and for a
 *   closed mesh the angle-weighted theorem gives N . (p - closest) the sign of inside / outside for EVERY feature whose Voronoi cell contains p, the cells' common
 *   boundary included: both choices of N agree in sign there.  The same holds between an edge's and a vertex's region.  Only |s| near 0 is at risk, which for a point
 *   off the surface means p - closest nearly tangent to the pseudo-normal's plane; DESIGN.md §4.19 measures that margin.
 *   LATTICE MODE: points == NULL and lattice != NULL.  n_points is then dims[0] * dims[1] * dims[2] (the argument is ignored; at most 2^31 - 1), point
 *   i = (ix * dims[1] + iy) * dims[2] + iz has p.x = origin[0] + (float)ix * spacing[0] (one product, one sum), likewise y and z: the outputs are laid out as
 *   tvr_mesh_count reads its volume, and marching cubes with the same origin and spacing puts the zero level set back where the mesh is.  No point array exists.
 *   counts_dev (int64[5], may be NULL; zeroed by the call): {points answered, points refused, node tests, triangle tests, points undecided}; the second evaluation of
 *   the winner is not counted as a test.  Index and blob checks as for the casts; a table whose header does not carry this mesh's F and V, or is marked bad, raises the
 *   fault flag and nothing is answered.
 * Errors, all before any launch: as for tvr_mesh_bvh_nearest, and TVR_ERR_INVALID for both or neither of points / lattice with points to answer, a negative lattice
 *   dimension, a non-finite lattice origin or spacing, misaligned keys (8 B) or table (256 B); TVR_ERR_SCRATCH for undersized keys, scratch or outputs and for a table
 *   whose size is not exactly tvr_mesh_pseudonormals_bytes(n_vertices, n_triangles) — a table of another mesh's size.  n_points == 0 and n_triangles == 0 are valid. */
typedef struct {
    size_t header, face_n, edge_n, vert_n, total;          /* byte offsets from the blob's start; total == tvr_mesh_pseudonormals_bytes */
    size_t face_stride, edge_stride, vert_stride;          /* bytes per face / per face (three edges) / per vertex */
} tvr_mesh_pseudonormals_layout;
typedef struct {
    float origin[3], spacing[3];
    int32_t dims[3];
} tvr_mesh_lattice;
size_t tvr_mesh_pseudonormals_bytes(int64_t n_vertices, int64_t n_triangles);
size_t tvr_mesh_pseudonormals_scratch_bytes(int64_t n_triangles);
int tvr_mesh_pseudonormals_describe(int64_t n_vertices, int64_t n_triangles, tvr_mesh_pseudonormals_layout *out);
int tvr_mesh_pseudonormals_keys(const int32_t *faces, int64_t n_vertices, int64_t n_triangles, uint64_t *corner_keys_out, uint64_t *edge_keys_out, size_t keys_bytes,
                                uint32_t *fault_flag_dev, void *stream);
int tvr_mesh_pseudonormals_build(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const uint64_t *sorted_corner_keys,
                                 const uint64_t *sorted_edge_keys, const int64_t *edge_order, void *table, size_t table_bytes, void *scratch, size_t scratch_bytes,
                                 int32_t *counts_dev /* [4] or NULL */, uint32_t *fault_flag_dev, void *stream);
int tvr_mesh_bvh_signed(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, const void *table,
                        size_t table_bytes, const float *points, int64_t n_points, const tvr_mesh_lattice *lattice, float max_dist, float *sdist, size_t sdist_bytes,
                        int32_t *tri, size_t tri_bytes, float *bary, size_t bary_bytes, int8_t *feature, size_t feature_bytes, int64_t *counts_dev /* [5] or NULL */,
                        uint32_t *fault_flag_dev, void *stream);

/* Inside / outside for ANY triangle soup: the generalized winding number (Jacobson, Kavan & Sorkine-Hornung 2013) by its hierarchical evaluation (Barill, Dickson,
 * Schmidt, Levin & Jacobson 2018; dipole order only) on the hierarchy above (csrc/tvr_mesh_winding.hip; mesh.build_winding / winding_number / winding_contains /
 * winding_number_grid / signed_distance_winding / remesh_watertight).  ADDITIVE exports: TVR_VERSION is unchanged.  DESIGN.md §4.20.  Arithmetic as above: fp32, every
 * operation rounded on its own, in the order written, divisions and square roots IEEE correctly rounded, u . v = (u.x * v.x + u.y * v.y) + u.z * v.z and
 * u x v = (u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x).
 * w(q) = (1 / 4 pi) * sum over the triangles of the signed solid angle they subtend at q: 1 inside a closed outward-oriented shell, 0 outside, k inside k nested or
 *   overlapping shells, and a smooth function in between for a soup with holes, doubled walls or unwelded corners.  Inside means w > 0.5.
 * THE TABLE (tvr_mesh_winding_build) over a hierarchy's blob: one row of 8 fp32 per INTERNAL node i = 0 .. F-2, {A.x, A.y, A.z, c.x, c.y, c.z, r, a}.
 *   Moments of a leaf, from its triangle (v0, v1, v2):  ab = v1 - v0, ac = v2 - v0;  A_t = 0.5f * (ab x ac) per component;  a_t = sqrt(A_t . A_t);
 *   g_k = ((v0_k + v1_k) + v2_k) / 3.0f;  m_t,k = a_t * g_k.  A triangle the hierarchy skipped (a non-finite coordinate) has A_t = m_t = 0, a_t = 0.
 *   Moments of an internal node: A = A(left child) + A(right child), m = m(left) + m(right), a = a(left) + a(right), per component, left = children[i][0].
 *   Row: ok = a > 0 and a finite;  c_k = m_k / a if ok, else 0;  e_k = max(c_k - lo_k, hi_k - c_k) with (lo, hi) the node's box AS IT STANDS IN THE BLOB;
 *   r = sqrt(e . e), the distance from c to the farthest corner of the box;  r = +inf if not ok or if r is not finite (such a node is never approximated).
 *   The sums are formed bottom-up in the refit's discipline: 62 launches, launch p computes the nodes whose two children were finished by an EARLIER launch (a pass
 *   number per node in scratch), so the kernel boundary is the only ordering and the order of every sum is the tree's; no float atomics.  m lives in scratch.  A root
 *   left unfinished, or a blob that is not this mesh's hierarchy, sets the header's bad word and *fault_flag_dev = 1.  The table is a function of (verts, faces) alone:
 *   the same bytes on every run (build zeroes the padding).  256 B + 32 B per internal node, rounded up to 256 B.  F <= 1: the header alone.
 *   tvr_mesh_winding_describe: header {uint32 magic, F, bad, 5 reserved} at `header`, rows [n_rows] x row_stride (32) B at `rows`.
 * THE QUERY (tvr_mesh_winding_query): one lane per point, the cast's 64-entry stack per lane in LDS, 128-lane workgroups, a guarded push, a step budget of 2F - 1.
 *   Start at the root.  An INTERNAL node with row (A, c, r, a):  d = c - q per component;  d2 = d . d;  the node is ACCEPTED iff d2 > (beta * r) * (beta * r) (two fp32
 *   products; false for a NaN).  Accepted: the term (d . A) / (d2 * sqrt(d2)) — the dipole A . d / |d|^3 — and the subtree is left.  Otherwise the LEFT child is visited
 *   next and the right one pushed.  A LEAF with triangle (v0, v1, v2):  a = v0 - q, b = v1 - q, c = v2 - q;  la = sqrt(a . a), lb, lc likewise;
 *   num = a . (b x c);  den = (((la * lb) * lc + (a . b) * lc) + (b . c) * la) + (c . a) * lb;  the term 2.0f * atan2f(num, den) (Van Oosterom & Strackee 1983; atan2f
 *   is the device library's).  A skipped triangle adds nothing.  Every term is fp32; the terms are summed in visiting order in an fp64 accumulator, and
 *   w = (float)(sum / 12.566370614359172).  beta in [1, +inf]: beta >= 1 keeps q outside the box of every accepted node (the ball of radius r about c holds the box);
 *   beta = +inf accepts nothing and gives the exact sum.  First- and second-order terms are NOT built.
 *   A point with a non-finite component is refused: w = NaN, and it is counted.  F == 0: w = 0.  A point ON the surface gets a finite value, not further specified.
 *   Points come from `points` [n_points][3] or from `lattice` exactly as in tvr_mesh_bvh_signed (the grid point is formed in the kernel).  Results do not depend on the
 *   order or batching of the points; two runs are bit-equal.
 *   counts_dev (int64[5], may be NULL; zeroed by the call): {points answered, points refused, node visits (internal nodes whose row was tested), dipole terms,
 *   triangle terms}.  Index and blob checks as for the casts; a table whose header does not carry this mesh's F, or is marked bad, raises the fault flag and every
 *   point gets NaN.
 * Errors, all before any launch: TVR_ERR_INVALID for a NULL pointer where data is due, a negative count, a misaligned blob, table or scratch (256 B), beta below 1 or NaN,
 *   both or neither of points / lattice with points to answer, a negative lattice dimension, a non-finite lattice origin or spacing; TVR_ERR_UNSUPPORTED for counts beyond
 *   the hierarchy's; TVR_ERR_SCRATCH for an undersized blob, scratch or output and for a table whose size is not exactly tvr_mesh_winding_bytes(n_triangles). */
typedef struct {
    size_t header, rows, total;                            /* byte offsets from the table's start; total == tvr_mesh_winding_bytes */
    size_t row_stride, n_rows;                             /* 32 bytes per internal node; n_rows = max(n_triangles - 1, 0) */
} tvr_mesh_winding_layout;
size_t tvr_mesh_winding_bytes(int64_t n_triangles);
size_t tvr_mesh_winding_scratch_bytes(int64_t n_triangles);
int tvr_mesh_winding_describe(int64_t n_triangles, tvr_mesh_winding_layout *out);
int tvr_mesh_winding_build(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, void *table,
                           size_t table_bytes, void *scratch, size_t scratch_bytes, uint32_t *fault_flag_dev, void *stream);
int tvr_mesh_winding_query(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, const void *table,
                           size_t table_bytes, const float *points, int64_t n_points, const tvr_mesh_lattice *lattice, float beta, float *w, size_t w_bytes,
                           int64_t *counts_dev /* [5] or NULL */, uint32_t *fault_flag_dev, void *stream);

/* Which triangles cut through which: the triangle-pair query on the hierarchy above (csrc/tvr_mesh_crossings.hip; mesh.self_intersections / mesh_intersections /
 * mesh_check).  ADDITIVE exports: TVR_VERSION is unchanged.  DESIGN.md §4.21.  Arithmetic as above: fp32, every operation rounded on its own (no fused multiply-add), in
 * the order written, divisions IEEE correctly rounded, the dot and cross products of tvr_mesh_bvh_cast.
 * SEGMENT: side k of a triangle runs between corner (k+1)%3 and corner (k+2)%3, oriented from the smaller vertex index u to the larger v:  o = verts[u],
 *   d = verts[v] - verts[u] per axis.  (The orientation depends on the indices alone, so the two triangles on an edge test the same segment.)
 * (SEGMENT, TRIANGLE) PIERCING: the (RAY, TRIANGLE) pair of tvr_mesh_bvh_cast applied to (o, d) with t_min = 0, t_max = 1, cull off — so 0 < t <= 1 — the ownership rule
 *   and everything else as they stand there.  The piercing point is (o.x + t * d.x, o.y + t * d.y, o.z + t * d.z).  LIMIT: a segment that lies in the triangle's plane
 *   has det == 0 and never pierces, so COPLANAR OVERLAP IS NOT DETECTED; nothing is promised for a segment exactly through a vertex of the triangle.
 * SHARING: a segment is never tested against a triangle one of whose corners has the same POSITION as one of the segment's end points (all three coordinates compare
 *   equal).  By position, not by index: neighbours in a welded mesh, in an unwelded soup and across duplicated vertices are treated alike.  Consequence: pairs that share
 *   an edge, and duplicate faces, are never reported; a pair that shares one vertex is tested with the sides that do not touch it.
 * PAIR: triangles a and b CROSS iff at least one of six tests pierces, in this fixed order: sides 0, 1, 2 of a against b, then sides 0, 1, 2 of b against a.  n_pierce
 *   is how many of the six pierce; points[0], points[1] are the first two piercing points in test order, points[1] = points[0] when n_pierce == 1.  In general position
 *   n_pierce == 2 and the two points are the ends of the intersection segment.  A triangle with a non-finite corner, or with an index out of range, crosses nothing.
 * SELF QUERY (mode TVR_MESH_CROSSINGS_SELF): all unordered pairs i < j of the hierarchy's mesh, a = i, b = j; verts_q / faces_q are not read and the n_*_q ignored.
 * TWO-MESH QUERY (mode TVR_MESH_CROSSINGS_MESH): all pairs (q, a), q a triangle of the query mesh (verts_q, faces_q), a a triangle of the hierarchy's mesh; in the test
 *   order above a = q's triangle and b = the tree's.  Sharing applies by position all the same.  Below, Nq is the number of query triangles (n_triangles in a self query).
 * TRAVERSAL: one lane per query triangle, the cast's 64-entry stack per lane in LDS, 128-lane workgroups, a guarded push, a step budget of 2F - 1.  A node is entered iff
 *   its box overlaps the query triangle's box (exact min / max of its corners), both widened: g_k = qlo_k - hi_k, h_k = lo_k - qhi_k per axis; m = the largest of |g|, |h|
 *   over the axes; pad = m * 2^-15; overlap iff every g_k <= pad and h_k <= pad (and the node's box is not empty).  Both children overlapping: the left one first, the
 *   right one pushed.  In a self query the lane of triangle i evaluates a leaf j only when j > i.  The padding is a stated margin for pairs the fp32 test reports although
 *   the exact triangles miss each other by a rounding error, not a proof; what is tested is set-equality with a brute-force restatement of the definition.
 * TWO PASSES, because the output's size is not known in advance (as tvr_mesh_count / _emit):
 *   tvr_mesh_crossings_count writes count_out [Nq] int32 (how many triangles query triangle i crosses) and total_dev [1] int64 (their sum), and zeroes and fills
 *   counts_dev (int64[4], may be NULL): {pairs, query triangles refused (a non-finite corner or an index out of range), node tests, triangle-pair tests}.  THE CALLER reads
 *   the total and forms offsets [Nq+1] int64, the exclusive scan of count_out with the total at the end.
 *   tvr_mesh_crossings_emit repeats the walk and writes row offsets[i] + k for the k-th pair query triangle i finds: pairs [n_pairs][2] int32 = (i, j), n_pierce [n_pairs]
 *   int32, and points [n_pairs][2][3] fp32 unless points is NULL.  Within one query triangle the rows are in walk order, which is the same on every run; THE CALLER SORTS
 *   the rows by the 64-bit key i << 32 | j (unique, so every correct sort gives the same order): pairs ascend by (first index, second index) and the output is the same
 *   bytes on every run.  A lane whose walk does not find exactly offsets[i+1] - offsets[i] pairs, or whose offsets do not lie in 0 .. n_pairs in ascending order, raises
 *   the fault flag and writes nothing outside its rows.  No float atomics; no atomics on the output order (the counters are integer sums, one atomic per wave).
 *   Index and blob checks as for the casts: an inconsistent blob (wrong magic, F, or bad != 0) raises the fault flag and nothing is reported; no load or store leaves
 *   the caller's buffers whatever the blob, the offsets and the faces hold.
 * Errors, all before any launch, tvr_last_error() names the argument: TVR_ERR_INVALID for a NULL pointer where data is due, a negative count, a mode outside 0 / 1, a
 *   misaligned blob (256 B) or offsets (8 B); TVR_ERR_UNSUPPORTED for n_vertices(_q) >= 2^31, n_triangles(_q) above TVR_MESH_BVH_MAX_TRIANGLES or n_pairs >= 2^31;
 *   TVR_ERR_SCRATCH for an undersized blob, count_out, offsets or output.  n_triangles == 0 and n_triangles_q == 0 are valid (no pair), so is n_pairs == 0.
 * NOT built: coplanar overlap, the intersection curve as connected polylines, repairing what is found. */
#define TVR_MESH_CROSSINGS_SELF 0
#define TVR_MESH_CROSSINGS_MESH 1
int tvr_mesh_crossings_count(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, int32_t mode,
                             const float *verts_q, int64_t n_vertices_q, const int32_t *faces_q, int64_t n_triangles_q, int32_t *count_out, size_t count_bytes,
                             int64_t *total_dev, int64_t *counts_dev /* [4] or NULL */, uint32_t *fault_flag_dev, void *stream);
int tvr_mesh_crossings_emit(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, int32_t mode,
                            const float *verts_q, int64_t n_vertices_q, const int32_t *faces_q, int64_t n_triangles_q, const int64_t *offsets, size_t offsets_bytes,
                            int64_t n_pairs, int32_t *pairs, size_t pairs_bytes, int32_t *n_pierce, size_t n_pierce_bytes, float *points /* or NULL */,
                            size_t points_bytes, uint32_t *fault_flag_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TVR_H */
