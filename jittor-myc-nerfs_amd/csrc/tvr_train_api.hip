// tvr_train_api.hip — the training entry points of libtvr.so (include/tvr.h): the march and appearance backward, the fused network kernels (tvr_mlp_train_*), CP
// training (tvr_cp_*), the training step without a host read (tvr_train_*), the encoding, the regularisers and the dense linear algebra.  tvr_march_forward(_z) is
// in tvr_api.hip.  Host code only and no kernel: argument checks, scratch carving and launches on the caller's stream.  A call's checks run in a fixed order: the
// first one that fails decides the status and the text of tvr_last_error().  Checks precede the first launch; tvr_train_backward's grad_scratch / vm_out come with step 4.
#include "tvr_scene.h"

#include <cstring>
#include <initializer_list>

// ---- the checks that recur ------------------------------------------------------------------------------------------------------------------------------------------
// the packed gradient images of a backward call (tvr_grad_scratch_bytes / tvr_cp_grad_scratch_bytes: the packed layout up to the network images)
static int grad_scratch_ok(const tvr_scene *s, const void *grad_scratch, size_t have)
{
    if (have < s->lay.mlp_image || (uintptr_t)grad_scratch % 256) return fail(TVR_ERR_SCRATCH, "gradient scratch too small or misaligned");
    return TVR_OK;
}

// m rows of the fused network kernels: a row's widest record is 576 B and the kernels index with 32 bits
static int rows_fit(int64_t m)
{
    if ((uint64_t)m * 576u >= (1ull << 32)) return fail(TVR_ERR_INVALID, "m = %lld: 32-bit row offsets inside the kernels allow 7.4 M entries per call", (long long)m);
    return TVR_OK;
}

static bool aligned16(std::initializer_list<const void *> ptrs)
{
    uintptr_t bits = 0;
    for (const void *p : ptrs) bits |= (uintptr_t)p;
    return bits % 16 == 0;
}

// One factor family — density or appearance, of a VM scene (planes and lines, n_comp[i] components) or a CP scene (`plane` NULL: lines only, n_comp[0] components) —
// as packed gradient blocks of `width` channels: cleared before a backward kernel accumulates into them, unpacked into the caller's tensors behind it
static int zero_grad_blocks(const tvr_scene *s, float *const *plane, float *const *line, int width, hipStream_t stream)
{
    const tvr_scene_desc &d = s->desc;
    for (int i = 0; i < 3; ++i) {
        const size_t W = d.grid[kMatH[i][0]], H = d.grid[kMatH[i][1]], Ln = d.grid[kVecH[i]];
        if (plane) HIP_TRY(launch_zero_f32(plane[i], (long long)((H + 1) * (W + 1) * width), stream));       // (channel counts are multiples of 4, blocks 256-B aligned)
        HIP_TRY(launch_zero_f32(line[i], (long long)((Ln + 1) * width), stream));
    }
    return TVR_OK;
}

static int unpack_grad_blocks(const tvr_scene *s, float *const *plane, float *const *line, float *const *out_plane, float *const *out_line, const int32_t *n_comp, int width,
                              hipStream_t stream)
{
    const tvr_scene_desc &d = s->desc;
    for (int i = 0; i < 3; ++i) {
        const int W = d.grid[kMatH[i][0]], H = d.grid[kMatH[i][1]], Ln = d.grid[kVecH[i]], nc = n_comp[plane ? i : 0];
        if (plane) HIP_TRY(launch_unpack_grad(plane[i], out_plane[i], nc, width, H, W, stream));
        HIP_TRY(launch_unpack_grad(line[i], out_line[i], nc, width, Ln, 1, stream));
    }
    return TVR_OK;
}

// (a CP scene has no planes: its layout's plane offsets are 0, so dplane / aplane are just `g` there and mean nothing — tvr_cp_* read dline / aline only)
static TrainGrads carve_grads(const tvr_scene *s, char *g)
{
    TrainGrads tg;
    for (int i = 0; i < 3; ++i) {
        tg.dplane[i] = (float *)(g + s->lay.dplane[i]);
        tg.dline[i] = (float *)(g + s->lay.dline[i]);
        tg.aplane[i] = (float *)(g + s->lay.aplane[i]);
        tg.aline[i] = (float *)(g + s->lay.aline[i]);
    }
    return tg;
}

// ---- the march and appearance backward of VM scenes ------------------------------------------------------------------------------------------------------------------
static int march_backward_impl(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, const MarchSampling &sm, float eps_T, const void *fwd_scratch,
                               size_t fwd_scratch_bytes, const float *grad_w, const float *grad_acc, const float *lam6, const float *grad_lam6,
                               void *grad_scratch, size_t grad_scratch_bytes, const tvr_vm_grads *out, void *stream_, long long gw_cap = -1)
{
    NOT_CP(s);
    TRY(scene_ready(s));
    if (!rays || !fwd_scratch || !grad_w || !grad_acc || !grad_scratch || !out || n_rays <= 0) return fail(TVR_ERR_INVALID, "NULL argument");
    TRY(fwd_scratch_ok(fwd_scratch, fwd_scratch_bytes, n_rays, S, false, "forward scratch %zu B < %zu B"));
    TRY(grad_scratch_ok(s, grad_scratch, grad_scratch_bytes));
    for (int i = 0; i < 3; ++i)
        if (!out->density_plane[i] || !out->density_line[i]) return fail(TVR_ERR_INVALID, "density gradient pointer %d is NULL", i);
    hipStream_t stream = (hipStream_t)stream_;
    TrainGrads tg = carve_grads(s, (char *)grad_scratch);
    TRY(zero_grad_blocks(s, tg.dplane, tg.dline, TVR_CD, stream));
    MarchOut mo = carve_scratch((char *)fwd_scratch, scratch_layout(n_rays, S), nullptr);
    HIP_TRY(launch_march_backward(s->dev, rays, (int)n_rays, S, sm, eps_T, mo, grad_w, grad_acc, lam6, grad_lam6, tg, stream, gw_cap));
    return unpack_grad_blocks(s, tg.dplane, tg.dline, out->density_plane, out->density_line, s->desc.density_n_comp, TVR_CD, stream);
}

static int app_h_backward_impl(tvr_scene *s, const float *xyz, int xyz_stride, int64_t m, const unsigned *m_dev, const float *dh, void *grad_scratch,
                               size_t grad_scratch_bytes, const tvr_vm_grads *out, void *stream_)
{
    NOT_CP(s);
    TRY(scene_ready(s));
    if (!grad_scratch || !out || m < 0 || (m > 0 && (!xyz || !dh))) return fail(TVR_ERR_INVALID, "NULL argument");
    TRY(grad_scratch_ok(s, grad_scratch, grad_scratch_bytes));
    for (int i = 0; i < 3; ++i)
        if (!out->app_plane[i] || !out->app_line[i]) return fail(TVR_ERR_INVALID, "appearance gradient pointer %d is NULL", i);
    hipStream_t stream = (hipStream_t)stream_;
    TrainGrads tg = carve_grads(s, (char *)grad_scratch);
    TRY(zero_grad_blocks(s, tg.aplane, tg.aline, TVR_CA, stream));
    if (m > 0) HIP_TRY(launch_app_h_backward(s->dev, xyz, m, dh, tg, stream, xyz_stride, m_dev));
    return unpack_grad_blocks(s, tg.aplane, tg.aline, out->app_plane, out->app_line, s->desc.app_n_comp, TVR_CA, stream);
}

extern "C" {

size_t tvr_grad_scratch_bytes(const tvr_scene *s)
{
    if (!s) return 0;
    if (cp_refused(s, __func__) != TVR_OK) return 0;
    return s->lay.mlp_image;      // the VM blocks come first in the packed layout; the gradient images mirror them
}

int tvr_march_backward(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, const float *jitter, float eps_T, const void *fwd_scratch,
                       size_t fwd_scratch_bytes, const float *grad_w, const float *grad_acc, void *grad_scratch, size_t grad_scratch_bytes,
                       const tvr_vm_grads *out, void *stream)
{
    const MarchSampling sm = {jitter, nullptr};
    return march_backward_impl(s, rays, n_rays, S, sm, eps_T, fwd_scratch, fwd_scratch_bytes, grad_w, grad_acc, nullptr, nullptr, grad_scratch,
                               grad_scratch_bytes, out, stream);
}

int tvr_march_backward_z(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, const float *z_vals, float eps_T, const void *fwd_scratch,
                         size_t fwd_scratch_bytes, const float *grad_w, const float *grad_acc, const float *t_last_tiny,
                         const float *grad_t_last_tiny, void *grad_scratch, size_t grad_scratch_bytes, const tvr_vm_grads *out, void *stream)
{
    if (!z_vals) return fail(TVR_ERR_INVALID, "z_vals is NULL");
    if ((t_last_tiny == nullptr) != (grad_t_last_tiny == nullptr)) return fail(TVR_ERR_INVALID, "t_last_tiny and its gradient go together");
    const MarchSampling sm = {nullptr, z_vals};
    return march_backward_impl(s, rays, n_rays, S, sm, eps_T, fwd_scratch, fwd_scratch_bytes, grad_w, grad_acc, t_last_tiny, grad_t_last_tiny,
                               grad_scratch, grad_scratch_bytes, out, stream);
}

int tvr_app_h_forward(tvr_scene *s, const float *xyz, int64_t m, float *h_out, size_t h_bytes, void *stream)
{
    NOT_CP(s);
    if (m > 0) NEED("h_out [m,144]", h_bytes, m, TVR_KAPP);
    TRY(scene_ready(s));
    if (m == 0) return TVR_OK;
    if (!xyz || !h_out || m < 0) return fail(TVR_ERR_INVALID, "xyz/h_out NULL or m < 0");
    HIP_TRY(launch_app_h_forward(s->dev, xyz, m, h_out, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_app_h_backward(tvr_scene *s, const float *xyz, int64_t m, const float *dh, size_t dh_bytes, void *grad_scratch, size_t grad_scratch_bytes,
                       const tvr_vm_grads *out, void *stream_)
{
    NOT_CP(s);
    if (m > 0) NEED("dh [m,144]", dh_bytes, m, TVR_KAPP);
    return app_h_backward_impl(s, xyz, 3, m, nullptr, dh, grad_scratch, grad_scratch_bytes, out, stream_);
}

// ---- the fused network kernels (csrc/tvr_mlp_train.hip) ----------------------------------------------------------------------------------------------------------------
size_t tvr_mlp_train_image_bytes(void) { return mlp_train_image_bytes(); }

static int mlp_train_forward_impl(tvr_scene *s, int variant, const float *h, const float *viewdirs, int64_t m, float *rgb, size_t rgb_bytes, float *feats32,
                                  size_t feats32_bytes, float *h1, size_t h1_bytes, float *h2, size_t h2_bytes, float *g8, size_t g8_bytes, float *rgb_s, size_t rgb_s_bytes,
                                  void *stream)
{
    const char *fn = variant ? "tvr_mlp_train_forward_ref" : "tvr_mlp_train_forward";
    TRY(cp_refused(s, fn));
    if (m > 0) {
        NEED_FN(fn, "rgb [m,3]", rgb_bytes, m, 3);
        NEED_FN(fn, "feats32 [m,32]", feats32_bytes, m, 32);
        NEED_FN(fn, "h1 [m,128]", h1_bytes, m, TVR_FEATC);
        NEED_FN(fn, "h2 [m,128]", h2_bytes, m, TVR_FEATC);
        if (variant) {
            NEED_FN(fn, "g8 [m,8]", g8_bytes, m, 8);
            NEED_FN(fn, "rgb_s [m,3]", rgb_s_bytes, m, 3);
        }
        TRY(rows_fit(m));
    }
    TRY(scene_ready(s));
    if (s->desc.variant != variant)
        return fail(TVR_ERR_UNSUPPORTED, "%s: the scene is %s", fn, s->desc.variant ? "a REFTensoRF scene (tvr_mlp_train_forward_ref)" : "a TensorVMSplit scene (tvr_mlp_train_forward)");
    {
        const tvr_scene_desc &d = s->desc;
        bool std_shape = d.featureC == TVR_FEATC && d.view_pe == 2 && d.fea_pe == 2;
        for (int i = 0; i < 3; ++i) std_shape = std_shape && d.app_n_comp[i] == TVR_CA;
        if (!std_shape) return fail(TVR_ERR_UNSUPPORTED, "%s: the fused training kernels take 48 appearance components, featureC 128, view_pe = fea_pe = 2 "
                                                         "(zero-padded shapes train through the library-GEMM path)", fn);
    }
    if (m == 0) return TVR_OK;
    if (!h || !viewdirs || !rgb || !feats32 || !h1 || !h2 || m < 0 || (variant && (!g8 || !rgb_s))) return fail(TVR_ERR_INVALID, "NULL argument or m < 0");
    if (!aligned16({h, feats32, h1, h2, g8})) return fail(TVR_ERR_INVALID, "h / feats32 / h1 / h2 / g8 must be 16-byte aligned");
    ShadeArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.n = m; sa.h_in = h; sa.viewdirs = viewdirs; sa.out = rgb; sa.t_feats = feats32; sa.t_h1 = h1; sa.t_h2 = h2; sa.t_g8 = g8; sa.t_rgbs = rgb_s;
    HIP_TRY(launch_shade(s->dev, SH_SRC_H, SH_DST_TRAIN, sa, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_mlp_train_forward(tvr_scene *s, const float *h, const float *viewdirs, int64_t m, float *rgb, size_t rgb_bytes, float *feats32, size_t feats32_bytes,
                          float *h1, size_t h1_bytes, float *h2, size_t h2_bytes, void *stream)
{
    return mlp_train_forward_impl(s, 0, h, viewdirs, m, rgb, rgb_bytes, feats32, feats32_bytes, h1, h1_bytes, h2, h2_bytes, nullptr, 0, nullptr, 0, stream);
}

int tvr_mlp_train_forward_ref(tvr_scene *s, const float *h, const float *viewdirs, int64_t m, float *rgb, size_t rgb_bytes, float *feats32, size_t feats32_bytes,
                              float *h1, size_t h1_bytes, float *h2, size_t h2_bytes, float *g8, size_t g8_bytes, float *rgb_s, size_t rgb_s_bytes, void *stream)
{
    return mlp_train_forward_impl(s, 1, h, viewdirs, m, rgb, rgb_bytes, feats32, feats32_bytes, h1, h1_bytes, h2, h2_bytes, g8, g8_bytes, rgb_s, rgb_s_bytes, stream);
}

// tvr_mlp_train_backward and _ref: `heads_W`, `dg8_bytes` and `rb` (g8, viewdirs, grad_in0, dg8) are the latter's, whose `rgb` is rgb_s; grad_in0 may be NULL
static int mlp_train_backward_impl(const char *fn, const float *W1, const float *W2, const float *W3, const float *basis, const float *const *heads_W, const float *grad_rgb,
                                   const float *rgb, const float *feats32, const float *h1, const float *h2, int64_t m, const float *gscale_dev, float *d_out4,
                                   size_t d_out4_bytes, float *dh2, size_t dh2_bytes, float *dh1, size_t dh1_bytes, float *dfeats32, size_t dfeats32_bytes, size_t dg8_bytes,
                                   float *dh, size_t dh_bytes, uint32_t *sat_flag_dev, void *image, size_t image_bytes, const MlpRefBwd *rb, void *stream)
{
    if (m == 0) return TVR_OK;
    if (m > 0) {
        NEED_FN(fn, "d_out4 [m,4]", d_out4_bytes, m, 4);
        NEED_FN(fn, "dh2 [m,128]", dh2_bytes, m, TVR_FEATC);
        NEED_FN(fn, "dh1 [m,128]", dh1_bytes, m, TVR_FEATC);
        NEED_FN(fn, "dfeats32 [m,32]", dfeats32_bytes, m, 32);
        if (rb) NEED_FN(fn, "dg8 [m,8]", dg8_bytes, m, 8);
        NEED_FN(fn, "dh [m,144]", dh_bytes, m, TVR_KAPP);
    }
    const bool ref_null = rb && (!heads_W || !heads_W[0] || !heads_W[1] || !heads_W[2] || !heads_W[3] || !rb->g8 || !rb->viewdirs || !rb->dg8);
    if (!W1 || !W2 || !W3 || !basis || !grad_rgb || !rgb || !feats32 || !h1 || !h2 || !gscale_dev || !d_out4 || !dh2 || !dh1 || !dfeats32 || !dh || !image || m < 0 || ref_null)
        return fail(TVR_ERR_INVALID, "NULL argument or m < 0");
    if (image_bytes < mlp_train_image_bytes() || (uintptr_t)image % 256) return fail(TVR_ERR_SCRATCH, "training image buffer too small or misaligned");
    TRY(rows_fit(m));
    if (!aligned16({feats32, h1, h2, d_out4, dh2, dh1, dfeats32, dh, rb ? rb->g8 : nullptr, rb ? rb->dg8 : nullptr}))
        return fail(TVR_ERR_INVALID, "activation / gradient matrices must be 16-byte aligned");
    HIP_TRY(launch_pack_train_image(W1, W2, W3, basis, heads_W, image, (hipStream_t)stream));
    HIP_TRY(launch_mlp_train_backward(grad_rgb, rgb, feats32, h1, h2, m, gscale_dev, d_out4, dh2, dh1, dfeats32, dh, sat_flag_dev, image, rb, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_mlp_train_backward(const float *W1, const float *W2, const float *W3, const float *basis, const float *grad_rgb, const float *rgb, const float *feats32,
                           const float *h1, const float *h2, int64_t m, const float *gscale_dev, float *d_out4, size_t d_out4_bytes, float *dh2, size_t dh2_bytes,
                           float *dh1, size_t dh1_bytes, float *dfeats32, size_t dfeats32_bytes, float *dh, size_t dh_bytes, uint32_t *sat_flag_dev,
                           void *image, size_t image_bytes, void *stream)
{
    return mlp_train_backward_impl(__func__, W1, W2, W3, basis, nullptr, grad_rgb, rgb, feats32, h1, h2, m, gscale_dev, d_out4, d_out4_bytes, dh2, dh2_bytes, dh1, dh1_bytes,
                                   dfeats32, dfeats32_bytes, 0, dh, dh_bytes, sat_flag_dev, image, image_bytes, nullptr, stream);
}

int tvr_mlp_train_backward_ref(const float *W1, const float *W2, const float *W3, const float *basis, const float *const heads_W[4], const float *grad_rgb,
                               const float *grad_in0, const float *rgb_s, const float *feats32, const float *h1, const float *h2, const float *g8, const float *viewdirs,
                               int64_t m, const float *gscale_dev, float *d_out4, size_t d_out4_bytes, float *dh2, size_t dh2_bytes, float *dh1, size_t dh1_bytes,
                               float *dfeats32, size_t dfeats32_bytes, float *dg8, size_t dg8_bytes, float *dh, size_t dh_bytes, uint32_t *sat_flag_dev, void *image,
                               size_t image_bytes, void *stream)
{
    MlpRefBwd rb;
    rb.g8 = g8; rb.viewdirs = viewdirs; rb.grad_in0 = grad_in0; rb.dg8 = dg8; rb.rays = nullptr; rb.q_ray = nullptr;
    return mlp_train_backward_impl(__func__, W1, W2, W3, basis, heads_W, grad_rgb, rgb_s, feats32, h1, h2, m, gscale_dev, d_out4, d_out4_bytes, dh2, dh2_bytes, dh1, dh1_bytes,
                                   dfeats32, dfeats32_bytes, dg8_bytes, dh, dh_bytes, sat_flag_dev, image, image_bytes, &rb, stream);
}

// ---- CP training (include/tvr.h, CP TRAINING; csrc/tvr_cp_train.hip): entry points of their own beside the refusals above ----
// the gradient images mirror the packed CP layout: carve_grads' dline[i] / aline[i] blocks (a CP scene has no planes), then the basis block ([27][ra] here, at
// lay.cp_basis), which ends where the network images begin
size_t tvr_cp_grad_scratch_bytes(const tvr_scene *s)
{
    if (cp_required(s, __func__) != TVR_OK) return 0;
    return s->lay.mlp_image;
}

int tvr_cp_march_forward(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, const float *jitter, float eps_T, float *depth_out, void *scratch,
                         size_t scratch_bytes, void *stream_)
{
    TRY(cp_required(s, __func__));
    TRY(scene_ready(s));
    if (!rays || !depth_out || n_rays <= 0) return fail(TVR_ERR_INVALID, "rays/depth_out NULL or n_rays <= 0");
    TRY(march_args_ok(s, n_rays, S, eps_T, scratch, scratch_bytes, "scratch too small (%zu < %zu) or misaligned"));
    ScratchLayout L = scratch_layout(n_rays, S);
    hipStream_t stream = (hipStream_t)stream_;
    MarchOut mo = carve_scratch((char *)scratch, L, depth_out);
    const MarchSampling sm = {jitter, nullptr};
    HIP_TRY(launch_zero_header(mo.counter, stream));                   // [0] queue length, [1] the march's tile counter, [2] its fault flag
    HIP_TRY(launch_cp_march(s->dev, s->cpd, rays, (int)n_rays, S, sm, eps_T, mo, nullptr, stream));
    if (n_rays <= TVR_RAY_ORDER_MAX_RAYS)                              // a training queue in ray order, as march_forward_impl leaves it
        HIP_TRY(launch_queue_ray_order(mo, (unsigned *)((char *)scratch + L.ray_new), mo.q_out, (unsigned *)((char *)scratch + L.q_j), (int)n_rays, stream));
    return TVR_OK;
}

int tvr_cp_march_backward(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, const float *jitter, float eps_T, const void *fwd_scratch, size_t fwd_scratch_bytes,
                          const float *grad_w, const float *grad_acc, void *grad_scratch, size_t grad_scratch_bytes, const tvr_cp_grads *out, void *stream_)
{
    TRY(cp_required(s, __func__));
    TRY(scene_ready(s));
    if (!rays || !fwd_scratch || !grad_w || !grad_acc || !grad_scratch || !out || n_rays <= 0) return fail(TVR_ERR_INVALID, "NULL argument or n_rays <= 0");
    for (int i = 0; i < 3; ++i)
        if (!out->density_line[i]) return fail(TVR_ERR_INVALID, "density gradient pointer %d is NULL", i);
    TRY(march_args_ok(s, n_rays, S, eps_T, fwd_scratch, fwd_scratch_bytes, "forward scratch %zu B < %zu B or misaligned"));
    TRY(grad_scratch_ok(s, grad_scratch, grad_scratch_bytes));
    hipStream_t stream = (hipStream_t)stream_;
    TrainGrads G = carve_grads(s, (char *)grad_scratch);
    TRY(zero_grad_blocks(s, nullptr, G.dline, s->cpd.rd, stream));                                    // (rd is a multiple of 16, blocks 256-B aligned)
    MarchOut mo = carve_scratch((char *)fwd_scratch, scratch_layout(n_rays, S), nullptr);
    HIP_TRY(launch_cp_march_backward(s->dev, s->cpd, rays, (int)n_rays, S, jitter, eps_T, mo, grad_w, grad_acc, G.dline, stream));
    return unpack_grad_blocks(s, nullptr, G.dline, nullptr, out->density_line, s->desc.density_n_comp, s->cpd.rd, stream);
}

int tvr_cp_app_backward(tvr_scene *s, const float *xyz, int64_t m, const float *grad_features, size_t grad_features_bytes, void *grad_scratch, size_t grad_scratch_bytes,
                        const tvr_cp_grads *out, void *stream_)
{
    TRY(cp_required(s, __func__));
    TRY(scene_ready(s));
    if (!grad_scratch || !out || m < 0 || (m > 0 && (!xyz || !grad_features))) return fail(TVR_ERR_INVALID, "NULL argument or m < 0");
    for (int i = 0; i < 3; ++i)
        if (!out->app_line[i]) return fail(TVR_ERR_INVALID, "appearance gradient pointer %d is NULL", i);
    if (!out->basis_mat) return fail(TVR_ERR_INVALID, "basis_mat gradient pointer is NULL");
    if (m > 0) NEED("grad_features [m,27]", grad_features_bytes, m, TVR_APPDIM);
    if ((uint64_t)m >= (1ull << 32)) return fail(TVR_ERR_INVALID, "m = %lld: at most 2^32 - 1 entries per call", (long long)m);
    TRY(grad_scratch_ok(s, grad_scratch, grad_scratch_bytes));
    hipStream_t stream = (hipStream_t)stream_;
    const tvr_scene_desc &d = s->desc;
    TrainGrads G = carve_grads(s, (char *)grad_scratch);
    float *g_basis = (float *)((char *)grad_scratch + s->lay.cp_basis);
    TRY(zero_grad_blocks(s, nullptr, G.aline, s->cpd.ra, stream));                                    // (ra is a multiple of 4)
    HIP_TRY(launch_zero_f32(g_basis, (long long)TVR_APPDIM * s->cpd.ra, stream));
    if (m > 0) HIP_TRY(launch_cp_app_backward(s->dev, s->cpd, xyz, m, grad_features, G.aline, g_basis, stream));
    TRY(unpack_grad_blocks(s, nullptr, G.aline, nullptr, out->app_line, d.app_n_comp, s->cpd.ra, stream));
    HIP_TRY(launch_copy_cols(out->basis_mat, d.app_n_comp[0], 0, g_basis, s->cpd.ra, d.app_n_comp[0], TVR_APPDIM, stream));
    return TVR_OK;
}

// ---- the training step without a host read (include/tvr.h: tvr_train_forward / tvr_train_backward) ----
struct WorkLayout {
    size_t h, feats32, h1, h2, rgb, g8, rgb_s, pre, grgb, gin0, grad_w, grad_acc, d_out4, dh2, dh1, dfeats32, dg8, dh, X, tmp, gemm, colsum, image, scalars, total;
};
static WorkLayout work_layout(int64_t n_rays, int32_t S, int64_t cap, bool gen = false)
{
    WorkLayout L;
    size_t off = 0;
    auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * sizeof(float), 256); return o; };
    const size_t c = (size_t)cap, n = (size_t)n_rays;
    L.h = take(c * TVR_KAPP); L.feats32 = take(c * 32); L.h1 = take(c * TVR_FEATC); L.h2 = take(c * TVR_FEATC); L.rgb = take(c * 3);
    L.g8 = take(c * 8); L.rgb_s = take(c * 3); L.pre = take(n * 3);
    L.grgb = take(c * 3); L.gin0 = take(c); L.grad_w = take(n * (size_t)S); L.grad_acc = take(n);
    L.d_out4 = take(c * 4); L.dh2 = take(c * TVR_FEATC); L.dh1 = take(c * TVR_FEATC); L.dfeats32 = take(c * 32); L.dg8 = take(c * 8); L.dh = take(c * TVR_KAPP);
    L.X = take(c * (gen ? (size_t)TVR_GENX_FLOATS : (size_t)TVR_GENX_W));    // (more than two encoding frequencies: three column blocks of 152, tvr_train.hip pe_concat_gen_kernel; otherwise one block or [cap,150 / 151])
    L.tmp = take((size_t)TVR_FEATC * TVR_GENX_W + 256);       // gemm_tn results that are wider than the gradient they feed ([4,128], [32,144], [8,144]; a [128,152] block of dW1, dW2 of a narrow network) and bias sums
    size_t g = gemm_tn_scratch_bytes(TVR_FEATC, TVR_GENX_W + 1, cap);        // (+ 1: the ones column that carries the bias gradient)
    L.gemm = take(g / sizeof(float) + 64);
    L.colsum = take(colsum_scratch_bytes() / sizeof(float));
    L.image = take(mlp_train_image_bytes() / sizeof(float) + 64);
    L.scalars = take(64);                                     // [0] max |gradient| bits, [1] gscale
    L.total = off;
    return L;
}

// dW1 in column blocks (tvr_train.hip pe_concat_gen_kernel) for every shape but the kernels' own 2 / 2 at width 128: more than two frequencies (three blocks), fewer (one
// block of 30 .. 144 columns), a narrower network (its gradients are cropped out of the 128-wide products).  What tvr_train_work_describe tells the caller about X and
// what tvr_train_backward multiplies are this one answer
struct W1Blocks { bool blocks; int n_in, nb; };
static W1Blocks w1_blocks(const tvr_scene *s)
{
    const tvr_scene_desc &d = s->desc;
    W1Blocks B;
    B.n_in = TVR_APPDIM + 3 + 2 * TVR_APPDIM * d.fea_pe + 6 * d.view_pe;
    B.blocks = d.variant == 0 && (s->dev.gen != 0 || d.fea_pe != 2 || d.view_pe != 2 || d.featureC < TVR_FEATC);
    B.nb = B.blocks ? (B.n_in + TVR_GENX_W - 1) / TVR_GENX_W : 1;
    return B;
}

static int train_args_ok(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, const void *fwd_scratch, size_t fwd_bytes, const void *work, size_t work_bytes,
                         int64_t app_cap)
{
    NOT_CP(s);
    TRY(scene_ready(s));
    const tvr_scene_desc &d = s->desc;
    // round 6: view_pe / fea_pe up to 6 (TensorVMSplit scenes: the lockstep layer 1 forward, the streamed W1^T backward); REFTensoRF keeps 2 / 2
    // and (TensorVMSplit) any component counts the kernels hold, <= 16 / 48 per plane — TensorBase's own defaults are 8 / 24: the packed scene carries zero channels, basis_mat's
    // columns are mapped in pack_train_image_kernel and its gradient is copied back plane by plane
    // — and any hidden width up to 128 and any frequencies 0 .. 6: every TensorVMSplit shape the scene itself accepts (check_desc) trains through the fused step
    bool std_shape = d.variant == 0 ? (d.featureC >= 1 && d.featureC <= TVR_FEATC && d.view_pe >= 0 && d.view_pe <= TVR_GEN_PE && d.fea_pe >= 0 && d.fea_pe <= TVR_GEN_PE)
                                    : (d.featureC == TVR_FEATC && d.view_pe == 2 && d.fea_pe == 2);
    for (int i = 0; i < 3; ++i) std_shape = std_shape && (d.app_n_comp[i] == TVR_CA || (d.variant == 0 && d.app_n_comp[i] >= 1 && d.app_n_comp[i] <= TVR_CA));
    if (!std_shape) return fail(TVR_ERR_UNSUPPORTED, "the fused training step takes REFTensoRF scenes at featureC 128, view_pe = fea_pe = 2, 48 appearance components per plane (TensorVMSplit: any shape the scene accepts)");
    if (!rays || n_rays <= 0 || S <= 0 || S > 4096 || app_cap <= 0) return fail(TVR_ERR_INVALID, "rays NULL, or n_rays / n_samples / app_cap out of range");
    if ((size_t)n_rays * (size_t)S >= (1ull << 32) || (uint64_t)app_cap * 576u >= (1ull << 32)) return fail(TVR_ERR_INVALID, "n_rays * n_samples and app_cap * 576 must be < 2^32");
    TRY(fwd_scratch_ok(fwd_scratch, fwd_bytes, n_rays, S, true, "forward scratch too small or misaligned"));
    if (!work || work_bytes < work_layout(n_rays, S, app_cap, s->dev.gen != 0).total || (uintptr_t)work % 256) return fail(TVR_ERR_SCRATCH, "training workspace too small (tvr_train_work_bytes) or misaligned");
    return TVR_OK;
}

size_t tvr_train_work_bytes(const tvr_scene *s, int64_t n_rays, int32_t n_samples, int64_t app_cap)
{
    if (n_rays <= 0 || n_samples <= 0 || app_cap <= 0) return 0;
    if (cp_refused(s, __func__) != TVR_OK) return 0;
    return work_layout(n_rays, n_samples, app_cap, s && s->dev.gen).total;           // (a scene with more than two encoding frequencies has the wider X)
}

int tvr_train_work_describe(const tvr_scene *s, int64_t n_rays, int32_t n_samples, int64_t app_cap, tvr_train_work_layout *out)
{
    NOT_CP(s);
    if (!s || !out || n_rays <= 0 || n_samples <= 0 || app_cap <= 0) return fail(TVR_ERR_INVALID, "tvr_train_work_describe: NULL argument or a count <= 0");
    const WorkLayout W = work_layout(n_rays, n_samples, app_cap, s->dev.gen != 0);
    out->h = W.h; out->feats32 = W.feats32; out->h1 = W.h1; out->h2 = W.h2; out->rgb = W.rgb; out->grgb = W.grgb; out->d_out4 = W.d_out4; out->dh2 = W.dh2; out->dh1 = W.dh1;
    out->dfeats32 = W.dfeats32; out->dh = W.dh; out->X = W.X; out->total = W.total;
    const W1Blocks B = w1_blocks(s);
    out->x_blocks = B.nb;
    out->x_block_cols = B.blocks ? TVR_GENX_W : (s->desc.variant == 1 ? TVR_NIN_REF : TVR_NIN);
    return TVR_OK;
}

int tvr_train_forward(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, const float *jitter, float eps_T, int32_t white_bg, void *fwd_scratch,
                      size_t fwd_bytes, void *work, size_t work_bytes, int64_t app_cap, float *rgb_map, float *depth, float *pen_ray, void *stream_)
{
    TRY(train_args_ok(s, rays, n_rays, S, fwd_scratch, fwd_bytes, work, work_bytes, app_cap));
    const bool ref = s->desc.variant == 1;
    if (!rgb_map || !depth || (ref && !pen_ray)) return fail(TVR_ERR_INVALID, "rgb_map / depth (/ pen_ray for a REFTensoRF scene) is NULL");
    hipStream_t stream = (hipStream_t)stream_;
    const MarchSampling sm = {jitter, nullptr};
    TRY(march_forward_impl(s, rays, n_rays, S, sm, eps_T, depth, nullptr, fwd_scratch, fwd_bytes, stream_));
    const ScratchLayout SL = scratch_layout(n_rays, S);
    const MarchOut mo = carve_scratch((char *)fwd_scratch, SL, depth);
    const WorkLayout W = work_layout(n_rays, S, app_cap, s->dev.gen != 0);
    char *w = (char *)work;
    HIP_TRY(launch_app_h_forward(s->dev, (const float *)mo.q_pos, app_cap, (float *)(w + W.h), stream, 4, mo.counter));
    ShadeArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.n = app_cap; sa.counter = mo.counter; sa.h_in = (const float *)(w + W.h); sa.q_ray = mo.q_ray; sa.rays = rays;
    sa.out = (float *)(w + W.rgb); sa.t_feats = (float *)(w + W.feats32); sa.t_h1 = (float *)(w + W.h1); sa.t_h2 = (float *)(w + W.h2);
    sa.t_g8 = (float *)(w + W.g8); sa.t_rgbs = (float *)(w + W.rgb_s);
    HIP_TRY(launch_shade(s->dev, SH_SRC_H, SH_DST_TRAIN, sa, stream));
    HIP_TRY(launch_composite_train_forward(mo, (int)n_rays, app_cap, white_bg, (const float *)(w + W.rgb), (const float *)(w + W.feats32), ref ? 1 : 0, rgb_map,
                                           (float *)(w + W.pre), pen_ray, stream));
    return TVR_OK;
}

int tvr_train_backward(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, const float *jitter, float eps_T, int32_t white_bg, const void *fwd_scratch,
                       size_t fwd_bytes, void *work, size_t work_bytes, int64_t app_cap, const tvr_train_weights *wt, const float *grad_rgb_map,
                       const float *grad_pen_ray, float grad_scale_target, void *grad_scratch, size_t grad_scratch_bytes, const tvr_vm_grads *vm_out,
                       const tvr_train_mlp_grads *mo_, uint32_t *sat_flag_dev, void *stream_)
{
    TRY(train_args_ok(s, rays, n_rays, S, fwd_scratch, fwd_bytes, work, work_bytes, app_cap));
    const bool ref = s->desc.variant == 1;
    if (!wt || !wt->W1 || !wt->W2 || !wt->W3 || !wt->basis || !grad_rgb_map || !vm_out || !mo_ || !(grad_scale_target > 0.0f)) return fail(TVR_ERR_INVALID, "NULL argument or grad_scale_target <= 0");
    if (!mo_->W1 || !mo_->b1 || !mo_->W2 || !mo_->b2 || !mo_->W3 || !mo_->b3 || !mo_->basis) return fail(TVR_ERR_INVALID, "a network gradient pointer is NULL");
    if (ref)
        for (int i = 0; i < 4; ++i)
            if (!wt->heads_W[i] || !mo_->heads_W[i] || !mo_->heads_b[i]) return fail(TVR_ERR_INVALID, "REFTensoRF head %d (normal, diffuse, specular, rho): weight or gradient pointer is NULL", i);
    hipStream_t stream = (hipStream_t)stream_;
    const ScratchLayout SL = scratch_layout(n_rays, S);
    const MarchOut mo = carve_scratch((char *)fwd_scratch, SL, nullptr);
    const bool gen = s->dev.gen != 0;
    const WorkLayout W = work_layout(n_rays, S, app_cap, gen);
    char *w = (char *)work;
    auto F = [&](size_t off) { return (float *)(w + off); };
    unsigned *amax = (unsigned *)(w + W.scalars);
    float *gscale = (float *)(w + W.scalars) + 1;
    const unsigned *mdev = mo.counter;
    const int nin = ref ? TVR_NIN_REF : TVR_NIN;
    // 1. compositing backward: gradients of the per-sample colours, of the weights and of acc; the scale of the fused backward
    HIP_TRY(launch_composite_train_backward(mo, (int)n_rays, app_cap, white_bg, F(W.rgb), F(W.feats32), ref ? F(W.g8) : nullptr, F(W.pre), grad_rgb_map, ref ? grad_pen_ray : nullptr,
                                            F(W.grgb), F(W.gin0), F(W.grad_w), F(W.grad_acc), amax, grad_scale_target, gscale, stream));
    // 2. the network backward (register-resident MFMA chains), dh through basis_mat (and the heads)
    const int fc = s->desc.featureC;
    const W1Blocks B1 = w1_blocks(s);
    const bool blocks = B1.blocks;
    HIP_TRY(launch_pack_train_image(wt->W1, wt->W2, wt->W3, wt->basis, ref ? wt->heads_W : nullptr, w + W.image, stream, s->desc.fea_pe, s->desc.view_pe, s->desc.app_n_comp, fc));
    MlpRefBwd rb;
    rb.g8 = F(W.g8); rb.viewdirs = nullptr; rb.grad_in0 = F(W.gin0); rb.dg8 = F(W.dg8); rb.rays = rays; rb.q_ray = mo.q_ray;
    HIP_TRY(launch_mlp_train_backward(F(W.grgb), ref ? F(W.rgb_s) : F(W.rgb), F(W.feats32), F(W.h1), F(W.h2), app_cap, gscale, F(W.d_out4), F(W.dh2), F(W.dh1), F(W.dfeats32),
                                      F(W.dh), sat_flag_dev, w + W.image, ref ? &rb : nullptr, stream, mdev, gen ? 1 : 0));
    // 3. weight gradients: dW = dY^T X over the step's appearance samples (tall-skinny reductions, fixed order), bias gradients = column sums
    if (blocks) HIP_TRY(launch_pe_concat_gen(F(W.feats32), 32, rays, mo.q_ray, s->desc.fea_pe, s->desc.view_pe, app_cap, mdev, F(W.X), stream));
    else if (ref) HIP_TRY(launch_pe_concat_strided(F(W.feats32), 32, F(W.feats32) + 27, 32, nullptr, nullptr, F(W.feats32) + 30, 32, app_cap, mdev, F(W.X), stream));
    else HIP_TRY(launch_pe_concat_strided(F(W.feats32), 32, nullptr, 0, rays, mo.q_ray, nullptr, 0, app_cap, mdev, F(W.X), stream));
    float *tmp = F(W.tmp), *gsc = F(W.gemm), *csc = F(W.colsum);
    // (the bias gradients ride along as a virtual ones column of the second operand: no second pass over d_out / dh2 / dh1)
    float *bs3 = tmp + 32 * TVR_KAPP + 16, *btmp = tmp + TVR_FEATC * TVR_GENX_W + 64;          // (btmp: a 128-entry bias sum of a product whose rows are cropped afterwards)
    // The products run on the fp16-split MFMAs at the backward's own gradient scale (the same values went through fp16 at that scale inside
    // mlp_train_backward / basis_backward, which raise the saturation flag if they do not fit): the kernel then runs at its staging rate.
    HIP_TRY(launch_gemm_tn(F(W.d_out4), 4, 4, F(W.h2), TVR_FEATC, TVR_FEATC, app_cap, tmp, gsc, stream, mdev, bs3, gscale));
    if (fc == TVR_FEATC) HIP_TRY(launch_copy_f32(mo_->W3, tmp, 3 * TVR_FEATC, stream));
    else HIP_TRY(launch_copy_cols(mo_->W3, fc, 0, tmp, TVR_FEATC, fc, 3, stream));             // W3's gradient is [3, fc]: the first fc columns of the [4,128] product
    HIP_TRY(launch_copy_f32(mo_->b3, bs3, 3, stream));
    if (fc == TVR_FEATC) HIP_TRY(launch_gemm_tn(F(W.dh2), TVR_FEATC, TVR_FEATC, F(W.h1), TVR_FEATC, TVR_FEATC, app_cap, mo_->W2, gsc, stream, mdev, mo_->b2, gscale));
    else {                                                                                      // [fc, fc] and [fc] out of the 128-wide product (units that do not exist: exact zeros)
        HIP_TRY(launch_gemm_tn(F(W.dh2), TVR_FEATC, TVR_FEATC, F(W.h1), TVR_FEATC, TVR_FEATC, app_cap, tmp, gsc, stream, mdev, btmp, gscale));
        HIP_TRY(launch_copy_cols(mo_->W2, fc, 0, tmp, TVR_FEATC, fc, fc, stream));
        HIP_TRY(launch_copy_f32(mo_->b2, btmp, fc, stream));
    }
    if (blocks) {
        // dW1 [fc, n_in] block by block (tvr_train.hip pe_concat_gen_kernel): each block's product lands in `tmp` and is copied to its columns; the bias rides with block 0
        const int n_in = B1.n_in, nb = B1.nb;
        for (int b = 0; b < nb; ++b) {
            const int cols = b == nb - 1 ? n_in - b * TVR_GENX_W : TVR_GENX_W, wb = (cols + 3) & ~3;
            HIP_TRY(launch_gemm_tn(F(W.dh1), TVR_FEATC, TVR_FEATC, F(W.X) + (size_t)b * (size_t)app_cap * TVR_GENX_W, wb, wb, app_cap, tmp, gsc, stream, mdev,
                                   b == 0 ? (fc == TVR_FEATC ? mo_->b1 : btmp) : nullptr, gscale));
            HIP_TRY(launch_copy_cols(mo_->W1, n_in, b * TVR_GENX_W, tmp, wb, cols, fc, stream));
            if (b == 0 && fc < TVR_FEATC) HIP_TRY(launch_copy_f32(mo_->b1, btmp, fc, stream));
        }
    } else
    HIP_TRY(launch_gemm_tn(F(W.dh1), TVR_FEATC, TVR_FEATC, F(W.X), nin, nin, app_cap, mo_->W1, gsc, stream, mdev, mo_->b1, gscale));
    HIP_TRY(launch_gemm_tn(F(W.dfeats32), 32, 32, F(W.h), TVR_KAPP, TVR_KAPP, app_cap, tmp, gsc, stream, mdev, nullptr, gscale));
    {
        int k_app = 0;
        for (int i = 0; i < 3; ++i) k_app += s->desc.app_n_comp[i];
        if (k_app == TVR_KAPP) HIP_TRY(launch_copy_f32(mo_->basis, tmp, TVR_APPDIM * TVR_KAPP, stream));
        else                                     // fewer components: the gradient's [27, k_app] takes plane p's columns 48 p .. 48 p + n_p of the [32,144] product
            for (int i = 0, off = 0; i < 3; off += s->desc.app_n_comp[i], ++i)
                HIP_TRY(launch_copy_cols(mo_->basis, k_app, off, tmp + i * TVR_CA, TVR_KAPP, s->desc.app_n_comp[i], TVR_APPDIM, stream));
    }
    if (ref) {
        HIP_TRY(launch_gemm_tn(F(W.dg8), 8, 8, F(W.h), TVR_KAPP, TVR_KAPP, app_cap, tmp, gsc, stream, mdev));      // rows: normal 0..2, specular 3, diffuse 4..6, rho 7
        HIP_TRY(launch_copy_f32(mo_->heads_W[0], tmp, 3 * TVR_KAPP, stream));
        HIP_TRY(launch_copy_f32(mo_->heads_W[2], tmp + 3 * TVR_KAPP, TVR_KAPP, stream));
        HIP_TRY(launch_copy_f32(mo_->heads_W[1], tmp + 4 * TVR_KAPP, 3 * TVR_KAPP, stream));
        HIP_TRY(launch_copy_f32(mo_->heads_W[3], tmp + 7 * TVR_KAPP, TVR_KAPP, stream));
        float *bs = tmp + 32 * TVR_KAPP;
        HIP_TRY(launch_colsum(F(W.dg8), 8, 8, app_cap, mdev, bs, csc, stream));
        HIP_TRY(launch_copy_f32(mo_->heads_b[0], bs, 3, stream));
        HIP_TRY(launch_copy_f32(mo_->heads_b[2], bs + 3, 1, stream));
        HIP_TRY(launch_copy_f32(mo_->heads_b[1], bs + 4, 3, stream));
        HIP_TRY(launch_copy_f32(mo_->heads_b[3], bs + 7, 1, stream));
    }
    // 4. scatter dh into the appearance planes / lines, then the march backward for the density factors
    TRY(app_h_backward_impl(s, (const float *)mo.q_pos, 4, app_cap, mdev, F(W.dh), grad_scratch, grad_scratch_bytes, vm_out, stream_));
    const MarchSampling sm = {jitter, nullptr};
    return march_backward_impl(s, rays, n_rays, S, sm, eps_T, fwd_scratch, fwd_bytes, F(W.grad_w), F(W.grad_acc), nullptr, nullptr, grad_scratch, grad_scratch_bytes, vm_out,
                               stream_, app_cap);
}

// ---- the encoding and the regularisers (csrc/tvr_train.hip, tvr_reg.hip) -----------------------------------------------------------------------------------------------
int tvr_pe_concat(const float *features, const float *viewdirs, const float *dot_product, int64_t m, float *X, size_t X_bytes, void *stream)
{
    if (m == 0) return TVR_OK;
    if (m > 0) NEED(dot_product ? "X [m,151]" : "X [m,150]", X_bytes, m, dot_product ? TVR_NIN_REF : TVR_NIN);
    if (!features || !viewdirs || !X || m < 0) return fail(TVR_ERR_INVALID, "features/viewdirs/X NULL or m < 0");
    HIP_TRY(launch_pe_concat(features, viewdirs, dot_product, m, X, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_pe_concat_backward(const float *features, const float *viewdirs, const float *grad_X, int64_t m, int32_t with_dot, float *grad_features,
                           size_t grad_features_bytes, float *grad_viewdirs, float *grad_dot, void *stream)
{
    if (m == 0) return TVR_OK;
    if (m > 0) NEED("grad_features [m,27]", grad_features_bytes, m, TVR_APPDIM);
    if (!features || !viewdirs || !grad_X || !grad_features || m < 0) return fail(TVR_ERR_INVALID, "NULL argument or m < 0");
    HIP_TRY(launch_pe_concat_backward(features, viewdirs, grad_X, m, with_dot ? 1 : 0, grad_features, grad_viewdirs, grad_dot, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_tv_loss(const float *x, int32_t C, int32_t H, int32_t W, float weight, float *value, float *grad, void *scratch, size_t scratch_bytes,
                void *stream)
{
    if (!x || !value || !grad || C < 1 || H < 1 || W < 1) return fail(TVR_ERR_INVALID, "x/value/grad NULL or bad shape");
    if (!scratch || scratch_bytes < 2048) return fail(TVR_ERR_SCRATCH, "tvr_tv_loss needs 2048 bytes of scratch");
    HIP_TRY(launch_tv_loss(x, C, H, W, weight, value, grad, (float *)scratch, (hipStream_t)stream));
    return TVR_OK;
}

static int reg_list(RegList &L, const float *const *xs, float *const *grads, const int64_t *counts, const int32_t *rows, int32_t n, bool need_grads)
{
    if (n < 1 || n > TVR_REG_MAX) return fail(TVR_ERR_INVALID, "1..%d tensors per call", TVR_REG_MAX);
    if (!xs || !counts || (need_grads && !grads)) return fail(TVR_ERR_INVALID, "xs/counts/grads NULL");
    L.n = n;
    for (int t = 0; t < n; ++t) {
        if (!xs[t] || counts[t] < 1 || (need_grads && !grads[t])) return fail(TVR_ERR_INVALID, "tensor %d: NULL pointer or empty", t);
        L.x[t] = xs[t];
        L.grad[t] = need_grads ? grads[t] : nullptr;
        L.count[t] = counts[t];
        L.rows[t] = rows ? rows[t] : 1;
        L.blocks[t] = 0;
    }
    return TVR_OK;
}

size_t tvr_l1_mean_scratch_bytes(const int64_t *counts, int32_t n)
{
    RegList L;
    if (!counts || n < 1 || n > TVR_REG_MAX) return 0;
    L.n = n;
    for (int t = 0; t < n; ++t) L.count[t] = counts[t] < 1 ? 1 : counts[t];
    return reg_l1_scratch_bytes(L);
}

int tvr_l1_mean(const float *const *xs, const int64_t *counts, int32_t n, float *value, void *scratch, size_t scratch_bytes, void *stream)
{
    RegList L;
    TRY(reg_list(L, xs, nullptr, counts, nullptr, n, false));
    if (!value) return fail(TVR_ERR_INVALID, "value NULL");
    if (!scratch || scratch_bytes < reg_l1_scratch_bytes(L)) return fail(TVR_ERR_SCRATCH, "scratch too small (tvr_l1_mean_scratch_bytes)");
    HIP_TRY(launch_l1_forward(L, value, (float *)scratch, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_l1_mean_backward(const float *const *xs, float *const *grads, const int64_t *counts, int32_t n, const float *grad_value, void *stream)
{
    RegList L;
    TRY(reg_list(L, xs, grads, counts, nullptr, n, true));
    if (!grad_value) return fail(TVR_ERR_INVALID, "grad_value NULL");
    HIP_TRY(launch_l1_backward(L, grad_value, (hipStream_t)stream));
    return TVR_OK;
}

static int ortho_list(RegList &L, const float *const *vs, float *const *grads, const int32_t *n_comp, const int32_t *n_size, int32_t n, bool need_grads)
{
    if (!n_comp || !n_size) return fail(TVR_ERR_INVALID, "n_comp/n_size NULL");
    int64_t counts[TVR_REG_MAX];
    if (n < 1 || n > TVR_REG_MAX) return fail(TVR_ERR_INVALID, "1..%d line factors per call", TVR_REG_MAX);
    for (int t = 0; t < n; ++t) {
        if (n_comp[t] < 2 || n_comp[t] > 48 || n_size[t] < 1) return fail(TVR_ERR_UNSUPPORTED, "line factor %d: %d components x %d (2..48 components)", t, n_comp[t], n_size[t]);
        counts[t] = (int64_t)n_comp[t] * n_size[t];
    }
    return reg_list(L, vs, grads, counts, n_comp, n, need_grads);
}

int tvr_line_ortho(const float *const *vs, const int32_t *n_comp, const int32_t *n_size, int32_t n, float *value, void *scratch, size_t scratch_bytes, void *stream)
{
    RegList L;
    TRY(ortho_list(L, vs, nullptr, n_comp, n_size, n, false));
    if (!value) return fail(TVR_ERR_INVALID, "value NULL");
    if (!scratch || scratch_bytes < TVR_LINE_ORTHO_SCRATCH_BYTES) return fail(TVR_ERR_SCRATCH, "tvr_line_ortho needs %d bytes of scratch", (int)TVR_LINE_ORTHO_SCRATCH_BYTES);
    HIP_TRY(launch_ortho(L, nullptr, value, (float *)scratch, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_line_ortho_backward(const float *const *vs, float *const *grads, const int32_t *n_comp, const int32_t *n_size, int32_t n, const float *grad_value, void *stream)
{
    RegList L;
    TRY(ortho_list(L, vs, grads, n_comp, n_size, n, true));
    if (!grad_value) return fail(TVR_ERR_INVALID, "grad_value NULL");
    HIP_TRY(launch_ortho(L, grad_value, nullptr, nullptr, (hipStream_t)stream));
    return TVR_OK;
}

// ---- the dense linear algebra (csrc/tvr_linear.hip, tvr_gemm.hip) ------------------------------------------------------------------------------------------------------
int tvr_linear_dx(const float *dY, int32_t ldy, int32_t N, const float *W, int32_t ldw, int32_t n_valid, int32_t K, const float *mask, int32_t ldm,
                  const uint64_t *mask_bits, float *dX, int32_t ldx, size_t dX_bytes, int64_t M, const float *scale_dev, uint32_t *sat_flag_dev, void *stream)
{
    if (mask && mask_bits) return fail(TVR_ERR_INVALID, "mask and mask_bits are alternatives");
    if ((uintptr_t)mask_bits & 7) return fail(TVR_ERR_INVALID, "mask_bits is not 8-B aligned");
    if (scale_dev && (N & 15)) return fail(TVR_ERR_INVALID, "the fp16-split form (scale_dev) takes N in multiples of 16 (N = %d)", N);
    if (M < 0) return fail(TVR_ERR_INVALID, "M < 0");
    if (N < 8 || N > 128 || (N & 7) || n_valid < 1 || n_valid > N) return fail(TVR_ERR_UNSUPPORTED, "N = %d (a multiple of 8 in [8,128]) / n_valid = %d", N, n_valid);
    if (K != 32 && K != 64 && K != 96 && K != 128) return fail(TVR_ERR_UNSUPPORTED, "K = %d (32, 64, 96 or 128)", K);
    if (ldy < N || ldx < K || ldw < K || (mask && ldm < K) || (ldy & 3) || (ldx & 3) || (mask && (ldm & 3))) return fail(TVR_ERR_INVALID, "row strides: >= the row length and multiples of 4");
    if (M == 0) return TVR_OK;
    if (!dY || !W || !dX || ((uintptr_t)dY & 15) || ((uintptr_t)dX & 15) || ((uintptr_t)mask & 15)) return fail(TVR_ERR_INVALID, "dY / W / dX NULL or not 16-B aligned");
    if (dX_bytes < ((size_t)(M - 1) * ldx + K) * sizeof(float)) return fail(TVR_ERR_SCRATCH, "dX holds fewer than M rows");
    HIP_TRY(launch_linear_dx(dY, ldy, N, W, ldw, n_valid, K, mask, ldm, dX, ldx, M, (hipStream_t)stream, scale_dev, sat_flag_dev,
                             (const unsigned long long *)mask_bits));
    return TVR_OK;
}

size_t tvr_colsum_scratch_bytes(void) { return colsum_scratch_bytes(); }

int tvr_colsum(const float *A, int32_t lda, int32_t K, int64_t M, float *out, void *scratch, size_t scratch_bytes, void *stream)
{
    if (M < 0 || K < 1 || K > 128 || lda < K) return fail(TVR_ERR_INVALID, "bad M / K / lda (K <= 128)");
    if (!out || (M > 0 && !A)) return fail(TVR_ERR_INVALID, "A / out NULL");
    if (!scratch || scratch_bytes < colsum_scratch_bytes()) return fail(TVR_ERR_SCRATCH, "scratch too small (tvr_colsum_scratch_bytes)");
    HIP_TRY(launch_colsum(A, lda, K, M, nullptr, out, (float *)scratch, (hipStream_t)stream));
    return TVR_OK;
}

static int gemm_tn_check(int32_t Ka, int32_t Kb, int64_t M)
{
    if (M < 0 || Ka < 1 || Kb < 1) return fail(TVR_ERR_INVALID, "bad Ka/Kb/M");
    if (((Ka + 31) / 32) * ((Kb + 31) / 32) > 20) return fail(TVR_ERR_UNSUPPORTED, "Ka x Kb = %d x %d exceeds the 20 32x32 tiles of a workgroup", Ka, Kb);
    return TVR_OK;
}

size_t tvr_gemm_tn_scratch_bytes(int32_t Ka, int32_t Kb, int64_t M)
{
    if (gemm_tn_check(Ka, Kb, M) != TVR_OK) return 0;
    return gemm_tn_scratch_bytes(Ka, Kb, M);
}

// C = A^T B in its three forms.  PLAIN: colsum_A and scale_dev are NULL.  SCALED: the fp16-split products at *scale_dev, the column sums of A if colsum_A is given.
// BIAS: fp32 products and the column sums, always.  The sums ride along as a ones column of B (`ones`), which the tile count and the scratch are sized for
enum GemmForm { GEMM_PLAIN, GEMM_SCALED, GEMM_BIAS };
static int gemm_tn_impl(GemmForm form, const float *A, int32_t lda, int32_t Ka, const float *B, int32_t ldb, int32_t Kb, int64_t M, float *C, float *colsum_A,
                        const float *scale_dev, void *scratch, size_t scratch_bytes, void *stream)
{
    static const char *const kNull[] = {"A/B/C NULL", "A/B/C/scale_dev NULL", "A/B/C/colsum_A NULL"};
    const int ones = colsum_A || form == GEMM_BIAS ? 1 : 0;
    TRY(gemm_tn_check(Ka, Kb + ones, M));
    const bool own_null = (form == GEMM_SCALED && !scale_dev) || (form == GEMM_BIAS && !colsum_A);
    if (!C || own_null || (M > 0 && (!A || !B))) return fail(TVR_ERR_INVALID, "%s", kNull[form]);
    if (lda < Ka || ldb < Kb) return fail(TVR_ERR_INVALID, "lda/ldb smaller than the row length");
    if (form == GEMM_SCALED && (Ka > 128 || 16 * (Ka + Kb) > 256 * 20)) return fail(TVR_ERR_UNSUPPORTED, "the fp16-split form takes Ka <= 128 and Ka + Kb <= 320 (Ka = %d, Kb = %d)", Ka, Kb);
    if (form == GEMM_BIAS && 16 * (Ka + Kb) > 256 * 20) return fail(TVR_ERR_UNSUPPORTED, "Ka + Kb = %d exceeds the 320 staged columns of the kernel that carries the ones column", Ka + Kb);
    if (M > 0 && (!scratch || scratch_bytes < gemm_tn_scratch_bytes(Ka, Kb + ones, M))) return fail(TVR_ERR_SCRATCH, "scratch too small (tvr_gemm_tn_scratch_bytes%s)", form == GEMM_PLAIN ? "" : "(Ka, Kb + 1, M)");
    HIP_TRY(launch_gemm_tn(A, lda, Ka, B, ldb, Kb, M, C, (float *)scratch, (hipStream_t)stream, nullptr, colsum_A, scale_dev));
    return TVR_OK;
}

int tvr_gemm_tn(const float *A, int32_t lda, int32_t Ka, const float *B, int32_t ldb, int32_t Kb, int64_t M, float *C, void *scratch,
                size_t scratch_bytes, void *stream)
{
    return gemm_tn_impl(GEMM_PLAIN, A, lda, Ka, B, ldb, Kb, M, C, nullptr, nullptr, scratch, scratch_bytes, stream);
}

int tvr_gemm_tn_scaled(const float *A, int32_t lda, int32_t Ka, const float *B, int32_t ldb, int32_t Kb, int64_t M, float *C, float *colsum_A, const float *scale_dev,
                       void *scratch, size_t scratch_bytes, void *stream)
{
    return gemm_tn_impl(GEMM_SCALED, A, lda, Ka, B, ldb, Kb, M, C, colsum_A, scale_dev, scratch, scratch_bytes, stream);
}

int tvr_gemm_tn_bias(const float *A, int32_t lda, int32_t Ka, const float *B, int32_t ldb, int32_t Kb, int64_t M, float *C, float *colsum_A, void *scratch,
                     size_t scratch_bytes, void *stream)
{
    return gemm_tn_impl(GEMM_BIAS, A, lda, Ka, B, ldb, Kb, M, C, colsum_A, nullptr, scratch, scratch_bytes, stream);
}

}  // extern "C"
