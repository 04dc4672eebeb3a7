/* tvr_ngp.h — C-ABI of the alt path (BASELINE configs[4]) in libtvr.so: JNeRF Instant-NGP inference
 * (occupancy-bitfield ray march -> multiresolution hash grid + SH-16 -> density / colour networks -> compositing) on MI355X,
 * and the occupancy grid built and refreshed from the network (the tvr_ngp_grid_* calls at the end).
 *
 * The reference reaches these steps through Jittor's inline-op API (`jt.code(..., cuda_src=...)`, SURVEY.md §8b "Config-5
 * boundary"); the entry points below are what a binding for that path would call instead.  Conventions are tvr.h's: plain
 * pointers and sizes, `int` return (0 ok, negative tvr_status, text via tvr_last_error()), caller-owned DEVICE buffers
 * (fp32 / int32 / uint8, contiguous, 16-byte aligned), all work enqueued on the caller's hipStream_t (passed as void*),
 * no allocation and no synchronisation inside.  File:line references are under jnerf-myc/python/jnerf/.
 */
#ifndef TVR_NGP_H
#define TVR_NGP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TVR_NGP_GRIDSIZE 128      /* density_grid_sampler.py:34 NERF_GRIDSIZE */
#define TVR_NGP_CASCADES 5        /* :33 NERF_CASCADES */
#define TVR_NGP_STEPS 1024        /* :37 MAX_STEP */
#define TVR_NGP_LEVELS 16         /* hash_encoder.py:18-19: n_levels 16, 2 features per level */
#define TVR_NGP_BITFIELD_BYTES (TVR_NGP_GRIDSIZE * TVR_NGP_GRIDSIZE * TVR_NGP_GRIDSIZE * TVR_NGP_CASCADES / 8)

/* Sampling configuration = what RaySampler / DensityGridSampler bake into their kernel source
 * (ray_sampler.py:55-58, density_grid_sampler.py:94-113). */
typedef struct tvr_ngp_march_cfg {
    float aabb_lo[3], aabb_hi[3];   /* dataset.py:214-215: 0.5 -+ aabb_scale/2 */
    float near_distance;            /* cfg near_distance */
    float cone_angle;               /* cfg cone_angle_constant */
    int32_t const_dt;               /* cfg const_dt: 1 = dt is MIN_CONE_STEPSIZE/2 everywhere */
    uint64_t rng_state, rng_inc;    /* the process-global pcg32 (`global_vars.py:16`) AS OF THIS CALL; the caller advances it by 2^32
                                       per slab afterwards (`ray_sampler.py:61`) */
    uint32_t slab_rays;             /* 0: one slab (the reference's call: ray i draws from state advanced by 8*i).  k > 0: the call covers
                                       several of the reference's k-ray slabs (`runner.py:209-222`, k = n_rays_per_batch): ray i draws what
                                       it would in slab i/k, i.e. from state advanced by (i/k)*2^32 + 8*(i%k) */
} tvr_ngp_march_cfg;

/* Hash-grid level table (grid_encode.py:24-39; kernel_grid's scale, HashEncode.h:142), evaluated by the host. */
typedef struct tvr_ngp_grid_cfg {
    uint32_t offsets[TVR_NGP_LEVELS + 1];   /* first ENTRY (2 floats) of each level; offsets[16] = total entries */
    float scale[TVR_NGP_LEVELS];            /* exp2(level*log2(per_level_scale))*base_resolution - 1 */
} tvr_ngp_grid_cfg;

/* NGPNetworks, plain-Linear branch (ngp_network.py:60-68): bias-free, row-major [out,in] fp32 device pointers. */
typedef struct tvr_ngp_net_params {
    const void *density0;   /* [64,32] */
    const void *density1;   /* [16,64] */
    const void *rgb0;       /* [64,32]  input = [density_mlp output (16), SH (16)] */
    const void *rgb1;       /* [64,64] */
    const void *rgb2;       /* [3,64]  */
} tvr_ngp_net_params;

/* update_bitfield (update_bitfield.py:14-31, op_header/update_bitfield.h:23-70): density_grid [5*128^3] fp32 (Morton order per
 * cascade) -> bitfield [TVR_NGP_BITFIELD_BYTES] and mean_out[1] = mean(max(cascade-0 density, 0)).  scratch: 4 KiB. */
int tvr_ngp_update_bitfield(const void *density_grid, void *bitfield, void *mean_out, void *scratch, size_t scratch_bytes, void *stream);

/* rays_sampler (ray_sampler.py:20-72, op_header/ray_sampler.h:4-114).  rays_o / rays_d [n_rays,3].
 * Outputs: coords [max_samples,7] = (warped pos, warped dt, warped dir) — rows [0,total) are written, the rest untouched;
 * numsteps [n_rays,2] int32 = (steps, base); ray_index [n_rays] int32 (rank among rays that received a slab, -1 without steps);
 * counter [2] uint32 = (rays with a slab, total steps).  Bases are the exclusive prefix sum of the step counts IN RAY ORDER
 * (the reference draws them from an atomicAdd in arrival order; per-ray contents are identical, the layout here is
 * deterministic).  A ray whose slab would cross max_samples gets (0, base) as in the reference.
 * scratch: tvr_ngp_sample_scratch_bytes(n_rays). */
size_t tvr_ngp_sample_scratch_bytes(int64_t n_rays);
int tvr_ngp_sample(const tvr_ngp_march_cfg *cfg, const void *rays_o, const void *rays_d, int64_t n_rays, const void *bitfield,
                   void *coords, int64_t max_samples, void *numsteps, void *ray_index, void *counter,
                   void *scratch, size_t scratch_bytes, void *stream);

/* HashEncoder.execute (hash_encoder.py:26-30; extract_position + kernel_grid + transpose, HashEncode.h:36-50,117-199,254-268):
 * positions [n, pos_stride floats] (first 3 used) in [0,1] -> out [n,32]. */
int tvr_ngp_hash_encode(const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *positions, int32_t pos_stride, int64_t n,
                        void *out, void *stream);

/* SHEncoder.execute (sh_encoder.py:26-53, SphericalEncode.h:44-100): directions warped to [0,1], [n, dir_stride floats]
 * -> out [n,16]. */
int tvr_ngp_sh_encode(const void *dirs, int32_t dir_stride, int64_t n, void *out, void *stream);

/* Packed MFMA image of the five weight matrices (refresh after the weights change). */
size_t tvr_ngp_net_packed_bytes(void);
int tvr_ngp_net_pack(const tvr_ngp_net_params *params, void *packed, size_t packed_bytes, void *stream);

/* NGPNetworks.execute_ (ngp_network.py:78-85) fused: positions [n, pos_stride floats] in [0,1], directions warped to [0,1]
 * [n, dir_stride floats] (the sampler's rows: coords, stride 7 and coords+4, stride 7) -> out [n,4] = (rgb raw, density raw).
 * n is read from n_dev[0] (uint32, device; e.g. counter+1 of tvr_ngp_sample) when n_dev != NULL, clamped to n_max;
 * otherwise n = n_max.  Rows of `out` from n on are left as they were.
 * Valid range: the default build hands the hash features, every hidden activation, the 16 density outputs and the SH values from one
 * layer to the next as TWO fp16 halves (hi = the value rounded toward zero, lo = the remainder), which sum to the value exactly only
 * while |value| <= 65504, the largest finite fp16.  Above that the hi half saturates: the outputs stay finite but are WRONG, and
 * nothing reports it.  Outputs are held to 2e-4 * max(1, |out|) against fp64 up to half that range (3e4).  The same holds for
 * tvr_ngp_render, which runs the same network code. */
int tvr_ngp_network(const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *net_packed, const void *positions, int32_t pos_stride,
                    const void *dirs, int32_t dir_stride, int64_t n_max, const void *n_dev, void *out, void *stream);

/* CalcRgb.inference (calc_rgb.py:118-150 -> compute_rgbs_inference_fp32, declared calc_rgb.h:45-60; rgb logistic, density exp):
 * net_out [n,4], coords [n,7], numsteps [n_rays,2] -> rgb [n_rays,3]. */
int tvr_ngp_composite(const void *net_out, const void *coords, const void *numsteps, int64_t n_rays, const float background[3],
                      void *rgb, void *stream);

/* One frame = what Runner.render_img (runner.py:195-228) returns for these rays, without rows, network outputs or slabs in between:
 * the march records each step's t, then one kernel walks every ray's steps 32 at a time through the encoders and networks and
 * composites them in order, stopping at the sample where compute_rgbs_inference breaks (T < 1e-4) — the samples behind it
 * contribute nothing, so their gathers and networks are skipped.  cfg->slab_rays = n_rays_per_batch reproduces the slab loop's
 * jitter.  rgb [n_rays,3]; stats (optional, device) uint64[2] = (samples evaluated, samples marched).
 * "Evaluated" counts WHOLE TILES of 32 steps (the last tile of a ray counts its real steps only), up to and including the tile that
 * holds the break: a ray of n steps adds n if it never breaks, and min(n, 32 * (b / 32 + 1)) if it breaks at sample b (the first
 * sample that sees T < 1e-4 in front of it) — the samples of that tile behind b went through the networks although they are not
 * composited.  A ray without steps adds nothing and receives the background itself; stats are zeroed even when n_rays == 0.
 * scratch: tvr_ngp_render_scratch_bytes(n_rays). */
size_t tvr_ngp_render_scratch_bytes(int64_t n_rays);
int tvr_ngp_render(const tvr_ngp_march_cfg *cfg, const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *net_packed, const void *rays_o,
                   const void *rays_d, int64_t n_rays, const void *bitfield, const float background[3], void *rgb, void *stats,
                   void *scratch, size_t scratch_bytes, void *stream);

/* tvr_ngp_render with HIP events around its two kernels, recorded on `stream`; WAITS for completion (a measurement entry point, unlike
 * everything else here) and returns ms_out = (march ms, render-kernel ms). */
int tvr_ngp_render_profiled(const tvr_ngp_march_cfg *cfg, const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *net_packed, const void *rays_o,
                            const void *rays_d, int64_t n_rays, const void *bitfield, const float background[3], void *rgb, void *stats,
                            void *scratch, size_t scratch_bytes, void *stream, float ms_out[2]);

/* ---- the occupancy grid from the network: DensityGridSampler.update_density_grid / update_density_grid_nerf (density_grid_sampler.py:200-259) ----
 * G = TVR_NGP_GRIDSIZE, cells = G^3, MIN_CONE_STEPSIZE = 1.73205080757f / 1024; density_grid and density_grid_tmp are [5 * cells] fp32 in Morton order per
 * cascade, as tvr_ngp_update_bitfield reads them.  ALL arithmetic below is fp32, every operation rounded on its own in the order written (no contraction;
 * divisions correctly rounded); 2^level is exact.  The pcg32 is pcg32.h's (ngp.Pcg32): next_float = bits((next_uint >> 9) | 0x3f800000) - 1.
 * xyz(c) = (morton3D_invert(c >> 0), morton3D_invert(c >> 1), morton3D_invert(c >> 2)).  Every call checks its arguments on the host before any launch. */

/* mark_untrained_density_grid (op_header/mark_untrained_density_grid.h): cell i, level = i / cells, pos = ((xyz(i % cells) + 0.5f) / G - 0.5f) * 2^level + 0.5f,
 * r = 0.5f * 1.73205080757f * 2^level / G.  focal_lengths [n,2]; xforms [n,3,4] row-major in the NGP convention (matrix_nerf2ngp): columns 0..2 are the camera
 * axes c0, c1, c2, column 3 the origin.  Camera j SEES the cell iff, with p = pos - column 3 and (x, y, z) = ((p0*c[0] + p1*c[1]) + p2*c[2]) for c = c0, c1, c2:
 * z > 0, |x| - r < z / fx * (0.5f * res_w) and |y| - r < z / fy * (0.5f * res_h).  If (grid[i] < 0) != (no camera sees it): grid[i] = seen ? 0 : -1; other
 * cells keep their value.  n_images == 0 marks every cell unseen. */
int tvr_ngp_grid_mark_untrained(void *density_grid, int32_t n_images, const void *focal_lengths, const void *xforms, int32_t res_w, int32_t res_h, void *stream);

/* generate_grid_samples_nerf_nonuniform (op_header/generate_grid_samples_nerf_nonuniform.h) on its own.  Sample i of n (0 <= n < 2^30) copies the generator
 * (rng_state, rng_inc), advances the copy by 4 * i and draws: level = (uint32)(next_float * n_cascades) % n_cascades; for j = 0..9:
 * idx = ((i + ema_step * n) * 56924617u + j * 19349663u + 96925573u) % cells + level * cells (uint32 wrap-around), stopping at the first j with
 * density_grid[idx] > thresh — when none does, THE TENTH INDEX IS KEPT; then with three more floats u (x, y, z in this order):
 * pos = ((xyz(idx % cells) + u) / G - 0.5f) * 2^level + 0.5f and positions_out[i] = (pos - aabb_lo) / (aabb_hi - aabb_lo), indices_out[i] = idx.
 * positions_out [n,3] fp32, indices_out [n] uint32.  n_cascades in 1..5. */
int tvr_ngp_grid_samples(int64_t n, uint32_t ema_step, int32_t n_cascades, float thresh, uint64_t rng_state, uint64_t rng_inc, const float aabb_lo[3],
                         const float aabb_hi[3], const void *density_grid, void *positions_out, void *indices_out, void *stream);

/* NGPNetworks.density (ngp_network.py:87-90) without the colour half: positions [n, pos_stride floats] in [0,1] -> out [n] = the raw density.  Hash gather and
 * density_mlp only (a third of tvr_ngp_network's MFMAs, no SH); the SAME gathers and MFMAs in the same order, so out[i] is BIT-EQUAL to column 3 of
 * tvr_ngp_network on the same positions, in whichever arithmetic the library was built with.  n / n_dev as for tvr_ngp_network; its valid range applies. */
int tvr_ngp_density(const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *net_packed, const void *positions, int32_t pos_stride, int64_t n_max,
                    const void *n_dev, void *out, void *stream);

/* splat_grid_samples_nerf_max_nearest_neighbor: for i < n, atomicMax on the uint32 view of grid_tmp[indices[i]] with the bits of
 * __expf(raw[i]) * MIN_CONE_STEPSIZE (v_exp_f32 of raw * log2(e); cascade level 0's step for every cascade, as in the reference; non-negative floats are
 * ordered like their bits).  Indices >= 5 * cells are ignored.  grid_tmp is NOT zeroed here. */
int tvr_ngp_grid_splat(const void *indices, const void *raw, int64_t n, void *grid_tmp, void *stream);

/* ema_grid_samples_nerf over all 5 * cells: prev = density_grid[i]; density_grid[i] = prev < 0 ? prev : fmaxf(prev * decay, grid_tmp[i]). */
int tvr_ngp_grid_ema(const void *grid_tmp, void *density_grid, float decay, void *stream);

/* One update_density_grid_nerf, in one call without a host read: density_grid_tmp (caller's scratch, tmp_bytes >= 5 * cells * 4, else TVR_ERR_SCRATCH) is
 * zeroed; ONE kernel draws both sample populations in registers — population 0: n_uniform samples with thresh -0.01 from (rng_state, rng_inc); population 1:
 * n_nonuniform samples with thresh 0.01 from that generator advanced by 2^32 (done here, on the host); each population with its own i and n in the index
 * hash — runs each sample through the hash gather and density_mlp and splats it; then the ema sweep, then tvr_ngp_update_bitfield.  Neither population reads
 * what the splat writes, so density_grid, density_grid_tmp, bitfield and mean_out are BIT-EQUAL to tvr_ngp_grid_samples (twice) -> tvr_ngp_density ->
 * tvr_ngp_grid_splat -> tvr_ngp_grid_ema -> tvr_ngp_update_bitfield.  Nothing is written per sample except the one atomic.  The kernel evaluates the
 * samples in an order of its own (by the Morton cell of their first candidate, for the gathers' locality): the splat is a maximum, no bit depends on it.
 * The caller advances its generator afterwards (the reference: by 2^32 after each of the two generate calls). */
int tvr_ngp_grid_update(const float aabb_lo[3], const float aabb_hi[3], const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *net_packed,
                        void *density_grid, void *density_grid_tmp, size_t tmp_bytes, void *bitfield, void *mean_out, int64_t n_uniform, int64_t n_nonuniform,
                        uint32_t ema_step, int32_t n_cascades, float decay, uint64_t rng_state, uint64_t rng_inc, void *stream);

/* ---- training the field: Runner.train (runner/runner.py:62-86) at row level ----
 * The sampler is the same call in training and inference (density_grid_sampler.py:138-140): tvr_ngp_sample supplies the rows.  The reference's compaction
 * (op_header/compacted_coord.h; its `T < EPSILON` break is commented out, :40-43) keeps every step of every ray until the row capacity is reached; with bases
 * handed out as the prefix sum in ray order that is the slice coords[0 : min(total, n_rows)] and, per ray, nc = min(n_rows - min(n_rows, base), n) rows.  The
 * reference's arrival-order atomics give another layout with the same per-ray content.  The five Linears train through tvr_linear_dx and tvr_gemm_tn (tvr.h). */

/* CalcRgb.execute, forward (calc_rgb.py:35-78; compute_rgbs_fp32 ships only as an object file, so the loop is modelled on compute_rgbs_inference as
 * oracle/ngp_oracle.c restates it, and on the comment at calc_rgb.h:2-4).  net_out [n_rows,4], coords [n_rows,7], numsteps [n_rays,2] = (n, base),
 * bg [n_rays,3] DEVICE, rgb_out [n_rays,3].  Ray i, T = 1, for j = 0 .. nc-1: stop if T < 1e-4; row base + j: c = logistic(out[0:3]), sigma = exp(out[3]),
 * dt = column 3 unwarped, alpha = 1 - exp(-sigma dt); rgb += alpha * T * c; T *= 1 - alpha.  Afterwards, if the loop walked all n UNCOMPACTED steps
 * (j == n: no break, not cut by the capacity), rgb += T * bg[i].  A ray with n == 0 receives bg[i]; a ray with n > 0 and nc == 0 receives 0.
 * The per-sample arithmetic is tvr_ngp_composite's own: with one background for all rays and n_rows >= the total, rgb_out is BIT-EQUAL to it.
 * PARITY-UNPINNED: the reference also passes density_grid_mean into that binary, whose source is absent; no regularisation term is added here and the mean is
 * not consumed. */
int tvr_ngp_composite_train(const void *net_out, const void *coords, const void *numsteps, int64_t n_rays, int64_t n_rows, const void *bg, void *rgb_out,
                            void *stream);

/* The derivative of tvr_ngp_composite_train with the set of composited samples held fixed (the stop index is not differentiated).  rgb_out is the forward's
 * output, grad_rgb [n_rays,3], grad_net_out [n_rows,4].  With g = grad_rgb[i], T_j the transmittance in front of sample j and
 * suffix_j = rgb_out[i] - sum_{k<=j} alpha_k T_k c_k (everything behind j, the background term included where it was added):
 *   d / d out[0:3] = g * alpha_j T_j * c (1 - c)          d / d out[3] = sigma_j dt_j * dot(g, T_j (1 - alpha_j) c_j - suffix_j).
 * suffix_j is summed from the last composited sample backwards (the subtraction above cancels where little is left behind j while sigma_j dt_j is large), so
 * rgb_out is kept in the signature only: it is not read and may be NULL.  EVERY row of grad_net_out[0:n_rows] is written: rows behind a break, behind the capacity cut, and rows no ray owns are exactly 0 (the buffer is zeroed on
 * the stream first).  One owner per row, no atomics: the same bytes on every run.  PARITY-UNPINNED like the forward (no density_grid_mean term). */
int tvr_ngp_composite_backward(const void *net_out, const void *coords, const void *numsteps, int64_t n_rays, int64_t n_rows, const void *bg, const void *rgb_out,
                               const void *grad_rgb, void *grad_net_out, void *stream);

/* kernel_grid_backward (HashEncode.h:300-396): for sample i, level l, corner k, feature f: grad_grid[2 * (offsets[l] + e) + f] += w * grad_enc[i, 2l + f], with
 * e and w EXACTLY the forward's (the same fma, floor, dense wrap and clamp as tvr_ngp_hash_encode; w formed in the forward's factor order, then one product).
 * grad_enc [n,32]; grad_grid [2 * offsets[16]] is ACCUMULATED into — the caller zeroes it.  positions [n, pos_stride floats] are read in place (the sampler's
 * rows: stride 7); there is no gradient with respect to them (the reference detaches them).  The adds are float atomics (one global_atomic_add_f32 each, and
 * LDS float atomics in front of them for the levels small enough to be pre-summed per workgroup): the result depends on arrival order in its last bits, so two
 * runs need not be byte-identical.  Per entry: |got - exact| <= (count + 8) * 2^-23 * sum |w g| over that entry's `count` contributions. */
int tvr_ngp_hash_encode_backward(const tvr_ngp_grid_cfg *grid_cfg, const void *positions, int32_t pos_stride, int64_t n, const void *grad_enc, void *grad_grid,
                                 void *stream);

/* ---- geometry: the density's spatial gradient, and the density on a lattice (csrc/tvr_ngp_geom.hip) ----
 *
 * tvr_ngp_density_gradient: positions [n, pos_stride floats] in [0,1] -> raw_out [n] (may be NULL) and grad_out [n,3] = d raw / d position, the position being the
 * unit-cube position the kernels take.  n / n_dev / row stride as for tvr_ngp_density; rows from n on are left as they were; every check on the host before any launch.
 * raw_out is BIT-EQUAL to tvr_ngp_density (the same gathers, fma chains and MFMAs in the same order; the tangent work sits between them).
 * DEFINITION.  Level l, with encode_level's own x = fmaf(p, scale_l, 0.5), cell floor(x) and fp32 fractions f = x - floor(x), corner values v (feature c = 0, 1):
 *   d enc[2l+c] / d p_k = scale_l * sum over the 8 corners of (d w / d f_k) * v_c,   d w / d f_k = the corner's weight with its factor k replaced by +1 (far corner
 *   along k) or -1 (near corner) — the dy_dx block of kernel_grid (HashEncode.h:206-249), which the reference carries and never calls.
 *   h = W0 enc (density_mlp.0), raw = W1[0,:] relu(h) (density_mlp.2);  grad raw = sum_k (W0^T (W1[0,:] * [h > 0]))_k * d enc_k / d p.
 * The gradient is piecewise: inside one cell of every level and one ReLU pattern it is a constant times a bilinear function of the fractions, and THAT is the
 * definition — no smoothing across cells, no finite difference.  [h > 0] is decided by an fp32-class evaluation of h (error about 2^-22 of sum_k |W0_jk| |enc_k|): at
 * a point where some |h_j| is within that of 0 an exact evaluation may pick the other branch.
 * EVALUATION (forward mode).  The corner sum is taken edge by edge, (product of the two other factors) * (far value - near value) over the four edges along k; the
 * three tangent encodings go through density_mlp.0 as three more operand columns against the same packed weight image (four times tvr_ngp_density's layer-0 products,
 * no memory traffic beyond its own), are masked by [h > 0], and row 0 of density_mlp.2 is applied in fp32 (read from the packed fp32 image).  In the default build the
 * mask's h is evaluated separately from the value's: the value path resolves hash features below 2^-14 to multiples of 2^-24 only (its fp16 halves), which leaves a
 * hidden unit of a small encoding at exactly 0; for the mask the encoding column is divided by a power of two of its own first, through the same weights.
 * RANGE.  scale_l reaches 2048 * aabb_scale - 1 (32 767 at aabb_scale 16) and multiplies differences of the table's values, so a tangent can pass the 65504 up to which
 * the default build's fp16 hi/lo split is exact.  Each tangent column (one sample, one axis) is therefore divided by a power of two of its own — chosen from its largest
 * magnitude so that this lies in [2^14, 2^15) — before the split (both halves rounded to nearest, which that range allows), and the hidden tangents are multiplied back
 * afterwards.  Powers of two are exact and the layer is linear in the column, so nothing is assumed about scale_l, the table's values or the weights beyond
 * tvr_ngp_network's own valid range for the VALUE path. */
int tvr_ngp_density_gradient(const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *net_packed, const void *positions, int32_t pos_stride, int64_t n_max,
                             const void *n_dev, void *raw_out, void *grad_out, void *stream);

/* tvr_ngp_density_grid: the RAW density on a lattice.  volume_out [dims[0], dims[1], dims[2]] fp32, the last axis fastest (as tvr_mesh_count / tvr_mesh_emit read a
 * volume).  Lattice point (i, j, k) is the unit-cube position p = (fmaf(i, spacing[0], origin[0]), fmaf(j, spacing[1], origin[1]), fmaf(k, spacing[2], origin[2])),
 * formed in the kernel: no point tensor exists.  The level set sigma = s of the density is raw = log s.
 *   - a point with a coordinate outside [0, 1] receives empty_value;
 *   - with bitfield != NULL (TVR_NGP_BITFIELD_BYTES, as tvr_ngp_update_bitfield writes it): x = p * (aabb_hi - aabb_lo) + aabb_lo (fp32: one subtraction on the host,
 *     then a product and a sum, each rounded), mip = min(4, max(0, frexp exponent of max_k |x_k - 0.5|, + 1)), cell c_k = clamp((int)(((x_k - 0.5) * 2^-mip + 0.5)
 *     * 128), 0, 127) — the march's lookup (cascaded_grid_idx_at) — and a point whose bit morton(c) of cascade mip is clear receives empty_value WITHOUT being
 *     evaluated; aabb_lo / aabb_hi are read only in this case;
 *   - every other point holds exactly what tvr_ngp_density returns for p (the same tile code: bit-equal).
 * Work is handed out in bricks of 2 x 4 x 4 lattice points (one 32-sample tile), neighbouring bricks to neighbouring waves; a brick without a point to evaluate
 * does no gather and no MFMA.  dims: each > 0 (else TVR_ERR_INVALID) and the product at most 2^31 (else TVR_ERR_UNSUPPORTED).  No atomics: the same bytes on every run. */
int tvr_ngp_density_grid(const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *net_packed, const void *bitfield, const float aabb_lo[3],
                         const float aabb_hi[3], const int32_t dims[3], const float origin[3], const float spacing[3], float empty_value, void *volume_out,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif
