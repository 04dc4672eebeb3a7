// tvr_api.hip — the C-ABI of libtvr.so (include/tvr.h) for scenes, rendering, the training marches' forward (tvr_march_forward(_z)), ray filtering, field queries,
// profiling and tvr_mesh_project (the one mesh call that reads a scene); the training entry points and the dense linear algebra are in tvr_train_api.hip, every
// other tvr_mesh_* entry point in tvr_mesh_api.hip, the NGP and background-network ones beside their kernels.  Host code only (but maxdiff_kernel):
// argument checks, packed-scene layout, scratch carving and kernel launches on the caller's stream.  No device allocation, no synchronisation.
#include "tvr_scene.h"

#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

static thread_local char g_err[512] = "";

int tvr_set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static PackedLayout packed_layout(const tvr_scene_desc &d)
{
    PackedLayout L;
    size_t off = 0;
    auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * sizeof(float), 256); return o; };
    for (int i = 0; i < 3; ++i) {
        const size_t W = d.grid[kMatH[i][0]], H = d.grid[kMatH[i][1]], Ln = d.grid[kVecH[i]];
        L.dplane[i] = take((H + 1) * (W + 1) * TVR_CD);
        L.dline[i] = take((Ln + 1) * TVR_CD);
        L.aplane[i] = take((H + 1) * (W + 1) * TVR_CA);
        L.aline[i] = take((Ln + 1) * TVR_CA);
    }
    L.mlp_image = take(TVR_MLP_IMAGE_BYTES_REF / 4);
    L.basis_frag = take(TVR_BASIS_FRAG_BYTES / 4);
    L.b3 = take(16);
    // scenes with more than two encoding frequencies (TensorBase's own default is 6 / 6: 390 MLP inputs): layer 1's fragment image, 26 k-steps, streamed through LDS
    L.w1gen = (d.view_pe > 2 || d.fea_pe > 2) ? take(TVR_W1GEN_BYTES / 4) : 0;
    // the 16x16x32 render kernel's fragment images (TensorVMSplit, at most two encoding frequencies: the shape every shipped config has)
    // (round 6: REFTensoRF scenes too — check_desc admits them at the built-for shape only — with the heads' fragments beside them)
    const bool has16 = !(d.view_pe > 2 || d.fea_pe > 2);
    L.img16 = has16 ? take(TVR16_IMAGE_BYTES / 4) : 0;
    L.basg16 = has16 ? take(TVR16_BASG_BYTES / 4) : 0;
    L.refg16 = (has16 && d.variant == 1) ? take(TVR16_REFG_BYTES / 4) : 0;
    for (int i = 0; i < 3; ++i) {
        const size_t W = d.grid[kMatH[i][0]], H = d.grid[kMatH[i][1]], Ln = d.grid[kVecH[i]];
        L.aplane16[i] = take((H + 1) * (W + 1) * TVR_CA / 2);
        L.aline16[i] = take((Ln + 1) * TVR_CA / 2);
    }
    L.cp_basis = 0;
    L.total = off;
    return L;
}

// A CP scene (tvr_cp_scene_create): three lines per factor in the slots of the VM lines — [L+1][rd] / [L+1][ra] fp32 — no planes, basis_mat in fp32 for the CP feature
// kernel, and the network images exactly as a variant-0 scene has them (the 32x32x16 shade_kernel image; no 16x16x32 image: the CP path does not use shade16_kernel).
#define TVR_CP_MAX_SIGMA 96
#define TVR_CP_MAX_APP 288
static int cp_rd(const tvr_scene_desc &d) { return (d.density_n_comp[0] + 15) / 16 * 16; }     // the march's quad gather reads 16 channels per step
static int cp_ra(const tvr_scene_desc &d) { return (d.app_n_comp[0] + 3) / 4 * 4; }
static PackedLayout cp_packed_layout(const tvr_scene_desc &d)
{
    PackedLayout L;
    memset(&L, 0, sizeof(L));
    size_t off = 0;
    auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * sizeof(float), 256); return o; };
    for (int i = 0; i < 3; ++i) {
        const size_t Ln = d.grid[kVecH[i]];
        L.dline[i] = take((Ln + 1) * cp_rd(d));
        L.aline[i] = take((Ln + 1) * cp_ra(d));
    }
    L.cp_basis = take((size_t)cp_ra(d) * TVR_APPDIM);
    L.mlp_image = take(TVR_MLP_IMAGE_BYTES_REF / 4);
    L.basis_frag = take(TVR_BASIS_FRAG_BYTES / 4);
    L.b3 = take(16);
    L.w1gen = (d.view_pe > 2 || d.fea_pe > 2) ? take(TVR_W1GEN_BYTES / 4) : 0;
    L.total = off;
    return L;
}

struct tvr_profile {
    std::vector<hipEvent_t> ev;   // 4 per recorded launch set (one per call; one per PIECE of a call rendered piecewise)
    int max_calls, n_calls;       // n_calls counts calls, n_sets launch sets
    int n_sets;
};

// the default piece: measured on the 800x800 bench frame (scripts/split_frame_experiment.py, profiles/r06_split_frame.txt); TVR_PIECE_RAYS overrides it for experiments
#ifndef TVR_DEFAULT_PIECE_RAYS
#define TVR_DEFAULT_PIECE_RAYS 30720
#endif
static int default_piece_rays()
{
    static int v = -1;
    if (v < 0) {
        const char *e = getenv("TVR_PIECE_RAYS");
        v = e ? atoi(e) : TVR_DEFAULT_PIECE_RAYS;
        if (v < 0) v = 0;
    }
    return v;
}

// the appearance factors as fp16, from the packed fp32 images (the one-product arithmetic gathers these: half the bytes through L1)
static int refresh_h16(tvr_scene *s, hipStream_t stream)
{
    const tvr_scene_desc &d = s->desc;
    for (int i = 0; i < 3; ++i) {
        const long long W = d.grid[kMatH[i][0]], H = d.grid[kMatH[i][1]], Ln = d.grid[kVecH[i]];
        HIP_TRY(launch_f32_to_f16((const float *)(s->packed + s->lay.aplane[i]), s->packed + s->lay.aplane16[i], (H + 1) * (W + 1) * TVR_CA, stream));
        HIP_TRY(launch_f32_to_f16((const float *)(s->packed + s->lay.aline[i]), s->packed + s->lay.aline16[i], (Ln + 1) * TVR_CA, stream));
    }
    s->h16_stale = false;
    return TVR_OK;
}

static int check_desc(const tvr_scene_desc *d, bool cp = false)
{
    if (!d) return fail(TVR_ERR_INVALID, "desc is NULL");
    if (cp) {      // a CP field has ONE component count per factor: entry [0]; [1] and [2] are ignored
        if (d->density_n_comp[0] < 1 || d->density_n_comp[0] > TVR_CP_MAX_SIGMA)
            return fail(TVR_ERR_UNSUPPORTED, "CP scene: density_n_comp[0]=%d; this build supports 1..%d", d->density_n_comp[0], TVR_CP_MAX_SIGMA);
        if (d->app_n_comp[0] < 1 || d->app_n_comp[0] > TVR_CP_MAX_APP)
            return fail(TVR_ERR_UNSUPPORTED, "CP scene: app_n_comp[0]=%d; this build supports 1..%d", d->app_n_comp[0], TVR_CP_MAX_APP);
        if (d->variant != 0) return fail(TVR_ERR_UNSUPPORTED, "CP scene: variant=%d; a CP scene is TensorCP with MLPRender_Fea, variant must be 0", d->variant);
        if (d->view_pe < 0 || d->view_pe > TVR_GEN_PE) return fail(TVR_ERR_UNSUPPORTED, "CP scene: view_pe=%d; this build supports 0..%d", d->view_pe, TVR_GEN_PE);
        if (d->fea_pe < 0 || d->fea_pe > TVR_GEN_PE) return fail(TVR_ERR_UNSUPPORTED, "CP scene: fea_pe=%d; this build supports 0..%d", d->fea_pe, TVR_GEN_PE);
    }
    for (int i = 0; i < 3; ++i) {
        if (d->grid[i] < 2 || d->grid[i] > 4096) return fail(TVR_ERR_INVALID, "grid[%d]=%d out of [2,4096]", i, d->grid[i]);
        // fewer components / narrower layers than the kernels are built for are packed with zero padding (exact); more are not supported
        if (!cp && (d->density_n_comp[i] < 1 || d->density_n_comp[i] > TVR_CD))
            return fail(TVR_ERR_UNSUPPORTED, "density_n_comp[%d]=%d; this build supports 1..%d", i, d->density_n_comp[i], TVR_CD);
        if (!cp && (d->app_n_comp[i] < 1 || d->app_n_comp[i] > TVR_CA))
            return fail(TVR_ERR_UNSUPPORTED, "appearance_n_comp[%d]=%d; this build supports 1..%d", i, d->app_n_comp[i], TVR_CA);
        if (!(d->aabb[3 + i] > d->aabb[i])) return fail(TVR_ERR_INVALID, "aabb hi <= lo on axis %d", i);
    }
    if (d->app_dim != TVR_APPDIM || d->featureC < 1 || d->featureC > TVR_FEATC || d->view_pe < 0 || d->view_pe > TVR_GEN_PE || d->fea_pe < 0 || d->fea_pe > TVR_GEN_PE)
        return fail(TVR_ERR_UNSUPPORTED, "MLP_Fea shape app_dim=%d featureC=%d view_pe=%d fea_pe=%d; this build supports app_dim 27, featureC 1..128, view_pe / fea_pe 0..%d",
                    d->app_dim, d->featureC, d->view_pe, d->fea_pe, TVR_GEN_PE);
    if (d->variant == 1) {
        bool std_shape = d->featureC == TVR_FEATC && d->view_pe == 2 && d->fea_pe == 2;
        for (int i = 0; i < 3; ++i) std_shape = std_shape && d->density_n_comp[i] == TVR_CD && d->app_n_comp[i] == TVR_CA;
        if (!std_shape) return fail(TVR_ERR_UNSUPPORTED, "REFTensoRF scenes are supported at 16 / 48 components, featureC 128, view_pe = fea_pe = 2 only");
    }
    if (d->fea2dense_act != 0 && d->fea2dense_act != 1) return fail(TVR_ERR_INVALID, "fea2dense_act must be 0 or 1");
    if (d->variant != 0 && d->variant != 1) return fail(TVR_ERR_INVALID, "variant must be 0 (TensorVMSplit) or 1 (REFTensoRF)");
    if (!(d->step_size > 0.0f)) return fail(TVR_ERR_INVALID, "step_size must be > 0");
    return TVR_OK;
}

extern "C" {

int tvr_version(void) { return TVR_VERSION; }
const char *tvr_last_error(void) { return g_err; }

size_t tvr_scene_packed_bytes(const tvr_scene_desc *desc)
{
    if (check_desc(desc) != TVR_OK) return 0;
    return packed_layout(*desc).total;
}

}  // extern "C"

static int scene_create_impl(const tvr_scene_desc *desc, void *packed_dev, size_t packed_bytes, tvr_scene **out, bool cp)
{
    if (!out) return fail(TVR_ERR_INVALID, "out is NULL");
    *out = nullptr;
    TRY(check_desc(desc, cp));
    PackedLayout L = cp ? cp_packed_layout(*desc) : packed_layout(*desc);
    if (!packed_dev || packed_bytes < L.total) return fail(TVR_ERR_SCRATCH, "packed buffer %zu B < required %zu B", packed_bytes, L.total);
    if ((uintptr_t)packed_dev % 256) return fail(TVR_ERR_SCRATCH, "packed buffer must be 256-byte aligned");
    tvr_scene *s = new (std::nothrow) tvr_scene;
    if (!s) return fail(TVR_ERR_INVALID, "out of host memory");
    s->cp = cp;
    s->cpd.rd = cp ? cp_rd(*desc) : 0;
    s->cpd.ra = cp ? cp_ra(*desc) : 0;
    s->cpd.basis = cp ? (const float4 *)((char *)packed_dev + L.cp_basis) : nullptr;
    s->desc = *desc;
    s->lay = L;
    s->packed = (char *)packed_dev;
    s->piece_rays = default_piece_rays();
    SceneDev &v = s->dev;
    memset(&v, 0, sizeof(v));
    for (int k = 0; k < 3; ++k) {
        v.lo[k] = desc->aabb[k];
        v.hi[k] = desc->aabb[3 + k];
        v.inv[k] = desc->inv_aabb_size[k];
        v.grid[k] = desc->grid[k];
        v.gm1[k] = (float)(desc->grid[k] - 1);
        v.dplane[k] = (const float4 *)(s->packed + L.dplane[k]);
        v.dline[k] = (const float4 *)(s->packed + L.dline[k]);
        v.aplane[k] = (const float4 *)(s->packed + L.aplane[k]);
        v.aline[k] = (const float4 *)(s->packed + L.aline[k]);
        v.aplane16[k] = (const uint4 *)(s->packed + L.aplane16[k]);
        v.aline16[k] = (const uint4 *)(s->packed + L.aline16[k]);
    }
    v.mlp_image = s->packed + L.mlp_image;
    v.basis_frag = s->packed + L.basis_frag;
    v.b3 = (const float *)(s->packed + L.b3);
    v.gen = (desc->view_pe > 2 || desc->fea_pe > 2) ? 1 : 0;
    v.w1gen = v.gen ? (const void *)(s->packed + L.w1gen) : nullptr;
    v.img16 = (!v.gen && !cp) ? (const void *)(s->packed + L.img16) : nullptr;
    v.basg16 = v.img16 ? (const void *)(s->packed + L.basg16) : nullptr;
    v.refg16 = (v.img16 && desc->variant == 1) ? (const void *)(s->packed + L.refg16) : nullptr;
    v.near_ = desc->near_;
    v.far_ = desc->far_;
    v.step = desc->step_size;
    v.shift = desc->density_shift;
    v.scale = desc->distance_scale;
    v.thres = desc->weight_thres;
    v.act = desc->fea2dense_act;
    v.variant = desc->variant;
    v.range_check = 1;
    v.arith = TVR_ARITH_F32;
    v.avol = nullptr;
    if (cp)
        for (int k = 0; k < 3; ++k) { v.dplane[k] = v.aplane[k] = nullptr; v.aplane16[k] = v.aline16[k] = nullptr; }
    *out = s;
    return TVR_OK;
}

extern "C" {

int tvr_scene_create(const tvr_scene_desc *desc, void *packed_dev, size_t packed_bytes, tvr_scene **out)
{
    return scene_create_impl(desc, packed_dev, packed_bytes, out, false);
}

size_t tvr_cp_scene_packed_bytes(const tvr_scene_desc *desc)
{
    if (check_desc(desc, true) != TVR_OK) return 0;
    return cp_packed_layout(*desc).total;
}

int tvr_cp_scene_create(const tvr_scene_desc *desc, void *packed_dev, size_t packed_bytes, tvr_scene **out)
{
    return scene_create_impl(desc, packed_dev, packed_bytes, out, true);
}

int tvr_scene_update(tvr_scene *s, const tvr_scene_params *p, void *stream_)
{
    if (!s || !p) return fail(TVR_ERR_INVALID, "scene/params is NULL");
    hipStream_t stream = (hipStream_t)stream_;
    const tvr_scene_desc &d = s->desc;
    for (int i = 0; i < 3 && s->cp; ++i) {              // CP: lines only ([1, R, L_i, 1]); the plane pointers are ignored
        if (!p->density_line[i] || !p->app_line[i]) return fail(TVR_ERR_INVALID, "CP scene: line pointer %d is NULL", i);
        const int Ln = d.grid[kVecH[i]];
        HIP_TRY(launch_pack_plane(p->density_line[i], (float *)(s->packed + s->lay.dline[i]), d.density_n_comp[0], s->cpd.rd, Ln, 1, stream));
        HIP_TRY(launch_pack_plane(p->app_line[i], (float *)(s->packed + s->lay.aline[i]), d.app_n_comp[0], s->cpd.ra, Ln, 1, stream));
    }
    for (int i = 0; i < 3 && !s->cp; ++i) {
        if (!p->density_plane[i] || !p->density_line[i] || !p->app_plane[i] || !p->app_line[i])
            return fail(TVR_ERR_INVALID, "plane/line pointer %d is NULL", i);
        const int W = d.grid[kMatH[i][0]], H = d.grid[kMatH[i][1]], Ln = d.grid[kVecH[i]];
        HIP_TRY(launch_pack_plane(p->density_plane[i], (float *)(s->packed + s->lay.dplane[i]), d.density_n_comp[i], TVR_CD, H, W, stream));
        HIP_TRY(launch_pack_plane(p->density_line[i], (float *)(s->packed + s->lay.dline[i]), d.density_n_comp[i], TVR_CD, Ln, 1, stream));
        HIP_TRY(launch_pack_plane(p->app_plane[i], (float *)(s->packed + s->lay.aplane[i]), d.app_n_comp[i], TVR_CA, H, W, stream));
        HIP_TRY(launch_pack_plane(p->app_line[i], (float *)(s->packed + s->lay.aline[i]), d.app_n_comp[i], TVR_CA, Ln, 1, stream));
    }
    if (!p->basis_mat || !p->W1 || !p->b1 || !p->W2 || !p->b2 || !p->W3 || !p->b3) return fail(TVR_ERR_INVALID, "MLP pointer is NULL");
    char *img = s->packed + s->lay.mlp_image;
    MlpShape sh;
    sh.featureC = d.featureC; sh.fea_pe = d.fea_pe; sh.view_pe = d.view_pe;
    sh.n_in = TVR_APPDIM + 3 + 2 * TVR_APPDIM * d.fea_pe + 6 * d.view_pe + (d.variant == 1 ? 1 : 0);
    sh.k_app = 0;
    for (int i = 0; i < 3; ++i) { sh.app_n_comp[i] = s->cp ? 0 : d.app_n_comp[i]; sh.app_off[i] = sh.k_app; sh.k_app += sh.app_n_comp[i]; }
    // (CP: the image's basis fragments are packed as zeros — shade_kernel<SH_SRC_FEAT> copies but never multiplies them — and basis_mat goes to the CP feature kernel in fp32)
    if (s->cp) HIP_TRY(launch_cp_pack_basis(p->basis_mat, d.app_n_comp[0], s->cpd.ra, (float4 *)(s->packed + s->lay.cp_basis), stream));
    if (s->dev.gen) {       // more than two frequencies: layer 1's image is the 26-k-step general one in global memory; the LDS image's W1 region is two staging slots
        HIP_TRY(launch_zero_f32((float *)(img + TVR_IMG_W1H), (TVR_IMG_W2H - TVR_IMG_W1H) / 4, stream));
        HIP_TRY(launch_pack_mlp(p->W1, p->b1, s->packed + s->lay.w1gen, nullptr, 5, sh, stream));
    } else {
        HIP_TRY(launch_pack_mlp(p->W1, p->b1, img + TVR_IMG_W1H, img + TVR_IMG_W1L, d.variant == 1 ? 4 : 0, sh, stream));
    }
    HIP_TRY(launch_pack_mlp(p->W2, nullptr, img + TVR_IMG_W2H, img + TVR_IMG_W2L, 1, sh, stream));
    // (clears and small copies as KERNELS: tvr_scene_update runs inside a captured training step, and memset / memcpy nodes of a graph replayed back to back
    //  were observed to run ahead of the previous replay's kernels — tvr_step.hip)
    HIP_TRY(launch_zero_f32((float *)(img + TVR_IMG_B1), (2 * 512 + 4 * TVR_IMG_W3_ROW) / 4, stream));       // b3 slot, b2, W3 + zero row: hidden units >= featureC stay zero
    HIP_TRY(launch_copy_f32((float *)(img + TVR_IMG_B3), p->b3, 3, stream));
    HIP_TRY(launch_copy_f32((float *)(img + TVR_IMG_B2), p->b2, d.featureC, stream));
    HIP_TRY(launch_pack_mlp(p->basis_mat, nullptr, img + TVR_IMG_BASH, s->packed + s->lay.basis_frag, 2, sh, stream));
    for (int r = 0; r < 3; ++r) HIP_TRY(launch_copy_f32((float *)(img + TVR_IMG_W3 + r * TVR_IMG_W3_ROW), p->W3 + (size_t)r * d.featureC, d.featureC, stream));
    HIP_TRY(launch_copy_f32((float *)(s->packed + s->lay.b3), p->b3, 3, stream));
    HIP_TRY(launch_zero_f32((float *)(img + TVR_MLP_IMAGE_BYTES), (TVR_MLP_IMAGE_BYTES_REF - TVR_MLP_IMAGE_BYTES) / 4, stream));
    if (d.variant == 1) {
        for (int i = 0; i < 4; ++i)
            if (!p->ref_W[i] || !p->ref_b[i]) return fail(TVR_ERR_INVALID, "REFTensoRF linear %d (normal, diffuse, specular, rho) is NULL", i);
    }
    if (s->dev.img16)
        HIP_TRY(launch_pack16(p->W1, p->b1, p->W2, p->b2, p->W3, p->b3, p->basis_mat, s->packed + s->lay.img16, s->packed + s->lay.basg16, sh, stream,
                              d.variant == 1 ? p->ref_W : nullptr, d.variant == 1 ? p->ref_b : nullptr, d.variant == 1 ? s->packed + s->lay.refg16 : nullptr));
    if (d.variant == 1) {
        HIP_TRY(launch_pack_ref(p->ref_W, p->ref_b, img + TVR_IMG_REFW, (float *)(img + TVR_IMG_REFB), stream));
    }
    s->params_set = true;
    s->h16_stale = true;                  // (the first render in TVR_ARITH_F16 converts the fp16 copies: nothing is converted for steps that never read them)
    s->dvol_stale = true;                 // (likewise the density volume: the next render bakes it — a training step that never renders pays nothing)
    s->fvol_stale = true;                 // (and the appearance volume)
    s->arith_valid = 0;                   // new parameters: a reduced arithmetic has to be measured again before it runs (tvr_scene_validate_arith)
    s->dev.arith = TVR_ARITH_F32;
    return TVR_OK;
}

size_t tvr_alpha_bits_bytes(const int32_t ag[3])
{
    if (!ag || ag[0] < 1 || ag[1] < 1 || ag[2] < 1) return 0;
    return (size_t)(((long long)ag[0] * ag[1] * ag[2] + 31) / 32) * 4;
}

int tvr_scene_set_alpha(tvr_scene *s, const float *vol, const int32_t ag[3], const float aabb[6], const float inv[3], void *bits, size_t bits_bytes,
                        void *stream)
{
    if (!s) return fail(TVR_ERR_INVALID, "scene is NULL");
    if (!vol) { s->dev.avol = nullptr; s->dev.abits = nullptr; return TVR_OK; }
    if (!ag || !aabb || !inv) return fail(TVR_ERR_INVALID, "alpha grid/aabb/inv is NULL");
    for (int k = 0; k < 3; ++k) {
        if (ag[k] < 1) return fail(TVR_ERR_INVALID, "alpha grid[%d]=%d", k, ag[k]);
        s->dev.ag[k] = ag[k];
        s->dev.alo[k] = aabb[k];
        s->dev.ainv[k] = inv[k];
        s->dev.agm1[k] = (float)(ag[k] - 1);
    }
    s->dev.avol = vol;
    s->dev.abits = nullptr;
    if (bits) {
        if (bits_bytes < tvr_alpha_bits_bytes(ag) || (uintptr_t)bits % 4) return fail(TVR_ERR_SCRATCH, "alpha bit buffer too small or misaligned");
        HIP_TRY(launch_alpha_bits(vol, (long long)ag[0] * ag[1] * ag[2], (unsigned *)bits, (hipStream_t)stream));
        s->dev.abits = (const unsigned *)bits;
    }
    return TVR_OK;
}

int tvr_scene_set_range_check(tvr_scene *s, int32_t on)
{
    if (!s) return fail(TVR_ERR_INVALID, "tvr_scene_set_range_check: scene is NULL");
    s->dev.range_check = on ? 1 : 0;
    return TVR_OK;
}

int tvr_scene_touch(tvr_scene *s)
{
    if (!s) return fail(TVR_ERR_INVALID, "tvr_scene_touch: scene is NULL");
    s->h16_stale = true;         // the next TVR_ARITH_F16 render converts the fp32 images first
    s->dvol_stale = true;        // and the next render of a scene with a density volume bakes it first
    s->fvol_stale = true;        // likewise the appearance volume
    s->arith_valid = 0;          // and a reduced arithmetic has to be validated again
    s->dev.arith = TVR_ARITH_F32;
    return TVR_OK;
}

int tvr_scene_set_arith(tvr_scene *s, int32_t mode)
{
    if (!s) return fail(TVR_ERR_INVALID, "tvr_scene_set_arith: scene is NULL");
    if (mode != TVR_ARITH_F32 && mode != TVR_ARITH_F16ACT && mode != TVR_ARITH_F16) return fail(TVR_ERR_INVALID, "tvr_scene_set_arith: mode %d is none of TVR_ARITH_*", (int)mode);
    if (mode != TVR_ARITH_F32) NOT_CP(s);
    s->arith_req = mode;
    s->dev.arith = (mode == TVR_ARITH_F32 || s->arith_valid == mode) ? mode : TVR_ARITH_F32;
    if (s->dev.arith != mode)
        tvr_set_error(TVR_OK, "tvr_scene_set_arith: mode %d is requested but NOT in effect — the kernels compute in TVR_ARITH_F32 until tvr_scene_validate_arith has measured "
                              "the mode inside its tolerance for the current parameters", (int)mode);
    return TVR_OK;
}

int tvr_scene_get_arith(const tvr_scene *s)
{
    if (!s) return fail(TVR_ERR_INVALID, "tvr_scene_get_arith: scene is NULL");
    return s->dev.arith;
}

int tvr_scene_get_arith_requested(const tvr_scene *s)
{
    if (!s) return fail(TVR_ERR_INVALID, "tvr_scene_get_arith_requested: scene is NULL");
    return s->arith_req;
}

int tvr_scene_set_render_pieces(tvr_scene *s, int32_t piece_rays)
{
    if (!s) return fail(TVR_ERR_INVALID, "tvr_scene_set_render_pieces: scene is NULL");
    if (piece_rays < 0) piece_rays = default_piece_rays();
    if (piece_rays != 0 && piece_rays < 16) return fail(TVR_ERR_INVALID, "tvr_scene_set_render_pieces: piece_rays %d (0 = off, < 0 = the library's default, else at least 16)", (int)piece_rays);
    s->piece_rays = piece_rays;
    return TVR_OK;
}

int tvr_scene_get_render_pieces(const tvr_scene *s)
{
    if (!s) return fail(TVR_ERR_INVALID, "tvr_scene_get_render_pieces: scene is NULL");
    return s->piece_rays;
}

int tvr_scene_destroy(tvr_scene *s)
{
    if (s && s->side_ready) {          // (the caller has synchronised whatever it enqueued on this scene: the side streams only ever carry work joined back to a caller's stream)
        for (int i = 0; i < 2; ++i) {
            if (s->side[i]) (void)hipStreamDestroy(s->side[i]);
            if (s->ev_join[i]) (void)hipEventDestroy(s->ev_join[i]);
        }
        if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
    }
    if (s && s->ev_dvol) (void)hipEventDestroy(s->ev_dvol);
    if (s && s->ev_fvol) (void)hipEventDestroy(s->ev_fvol);
    delete s;
    return TVR_OK;
}

}  // extern "C"

static size_t density_volume_values(const tvr_scene_desc &d)
{
    return ((size_t)d.grid[0] + 1) * ((size_t)d.grid[1] + 1) * ((size_t)d.grid[2] + 1);
}

// Called by every entry that launches the render march, on the caller's stream and in front of any fork: brings the attached density volume up to date and orders
// this stream behind the bake.  Stale: bake here (a KERNEL, see tvr_scene_update's note on graph replays) and record ev_dvol.  Fresh, but baked on another stream:
// wait on ev_dvol, so a second stream (render.FrameStream) never reads a half-baked volume.  Under stream capture (tvr.h): a stale volume's bake is captured in front of
// the march — every replay bakes again — and the flag STAYS set, because nothing has run yet: the next un-captured render bakes too; no event is recorded or waited on.
static int ensure_dvol(tvr_scene *s, hipStream_t stream)
{
    if (!s->dvol) return TVR_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    const bool capturing = cs != hipStreamCaptureStatusNone;
    if (s->dvol_stale) {
        HIP_TRY(launch_density_volume(s->dev, s->dvol, stream));
        if (capturing) return TVR_OK;
        if (!s->ev_dvol) HIP_TRY(hipEventCreateWithFlags(&s->ev_dvol, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(s->ev_dvol, stream));
        s->dvol_recorded = true;
        s->dvol_stream = stream;
        s->dvol_stale = false;
    } else if (!capturing && s->dvol_recorded && stream != s->dvol_stream) {
        HIP_TRY(hipStreamWaitEvent(stream, s->ev_dvol, 0));
    }
    return TVR_OK;
}

extern "C" {

size_t tvr_density_volume_bytes(const tvr_scene_desc *desc)
{
    if (check_desc(desc) != TVR_OK) return 0;
    return density_volume_values(*desc) * sizeof(float);
}

int tvr_scene_set_density_volume(tvr_scene *s, void *buf, size_t bytes, void *stream)
{
    if (!s) return fail(TVR_ERR_INVALID, "tvr_scene_set_density_volume: scene is NULL");
    if (!buf) {                            // detach: the shipped (factored) march runs from the next call on
        s->dvol = nullptr;
        s->dvol_stale = true;
        s->dvol_recorded = false;
        return TVR_OK;
    }
    NOT_CP(s);
    const size_t need = density_volume_values(s->desc) * sizeof(float);
    if (bytes < need) return fail(TVR_ERR_SCRATCH, "tvr_scene_set_density_volume: buffer %zu B < required %zu B", bytes, need);
    if ((uintptr_t)buf % 256) return fail(TVR_ERR_SCRATCH, "tvr_scene_set_density_volume: buffer must be 256-byte aligned");
    s->dvol = (float *)buf;
    s->dvol_stale = true;
    s->dvol_recorded = false;
    if (s->params_set) return ensure_dvol(s, (hipStream_t)stream);       // parameters are packed: bake now, on the caller's stream
    return TVR_OK;
}

}  // extern "C"

// The appearance volume (tvr.h, BAKED APPEARANCE VOLUME): one TVR16_VOL_RECORD-byte record per value of the density volume.
static size_t appearance_volume_need(const tvr_scene_desc &d) { return density_volume_values(d) * (size_t)TVR16_VOL_RECORD; }
static bool takes_appearance_volume(const tvr_scene_desc &d) { return d.variant == 0 && d.view_pe <= 2 && d.fea_pe <= 2; }     // the scenes shade16_kernel<., false> renders

// ensure_dvol for the render shade: called by render_impl on the caller's stream, in front of any fork, when the call's shade kernel reads the volume
static int ensure_fvol(tvr_scene *s, hipStream_t stream)
{
    if (!s->fvol) return TVR_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    const bool capturing = cs != hipStreamCaptureStatusNone;
    if (s->fvol_stale) {
        HIP_TRY(launch_appearance_volume(s->dev, s->fvol, stream));
        if (capturing) return TVR_OK;
        if (!s->ev_fvol) HIP_TRY(hipEventCreateWithFlags(&s->ev_fvol, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(s->ev_fvol, stream));
        s->fvol_recorded = true;
        s->fvol_stream = stream;
        s->fvol_stale = false;
    } else if (!capturing && s->fvol_recorded && stream != s->fvol_stream) {
        HIP_TRY(hipStreamWaitEvent(stream, s->ev_fvol, 0));
    }
    return TVR_OK;
}

extern "C" {

size_t tvr_appearance_volume_bytes(const tvr_scene_desc *desc)
{
    if (check_desc(desc) != TVR_OK) return 0;
    if (!takes_appearance_volume(*desc)) {
        tvr_set_error(TVR_OK, "tvr_appearance_volume_bytes: REFTensoRF scenes and scenes with more than two encoding frequencies take no appearance volume");
        return 0;
    }
    return appearance_volume_need(*desc);
}

int tvr_scene_set_appearance_volume(tvr_scene *s, void *buf, size_t bytes, void *stream)
{
    if (!s) return fail(TVR_ERR_INVALID, "tvr_scene_set_appearance_volume: scene is NULL");
    if (!buf) {                            // detach: the factored gather and the basis product run from the next call on
        s->fvol = nullptr;
        s->fvol_stale = true;
        s->fvol_recorded = false;
        return TVR_OK;
    }
    NOT_CP(s);
    if (s->desc.variant != 0) return fail(TVR_ERR_UNSUPPORTED, "tvr_scene_set_appearance_volume: a REFTensoRF scene's heads read the 144 products themselves; no volume form");
    if (!takes_appearance_volume(s->desc))
        return fail(TVR_ERR_UNSUPPORTED, "tvr_scene_set_appearance_volume: scenes with more than two encoding frequencies do not render on the kernel that reads the volume");
    const size_t need = appearance_volume_need(s->desc);
    if (need >= ((size_t)1 << 32))
        return fail(TVR_ERR_UNSUPPORTED, "tvr_scene_set_appearance_volume: the volume of this grid takes %zu B; the gather addresses it with 32-bit byte offsets (below 4 GiB)", need);
    if (bytes < need) return fail(TVR_ERR_SCRATCH, "tvr_scene_set_appearance_volume: buffer %zu B < required %zu B", bytes, need);
    if ((uintptr_t)buf % 256) return fail(TVR_ERR_SCRATCH, "tvr_scene_set_appearance_volume: buffer must be 256-byte aligned");
    s->fvol = (float4 *)buf;
    s->fvol_stale = true;
    s->fvol_recorded = false;
    if (s->params_set && s->dev.arith == TVR_ARITH_F32) return ensure_fvol(s, (hipStream_t)stream);       // parameters are packed: bake now, on the caller's stream
    return TVR_OK;
}

// Piecewise rendering: a call of n rays goes out as K = round(n / piece_rays) pieces of ceil(n / K) rays rounded up to 512 (the last one shorter), if that makes at least
// TVR_MIN_PIECES.  Measured on one box (bench.py --emulate-world N --pieces P, profiles/r06_split_frame.txt): the 640 000-ray frame -3.6 % .. -4.6 %, a 320 000-ray share
// -4.6 %, a 160 000-ray share +-0.5 %, an 80 000-ray share +0.9 % (two or three pieces do not settle into the overlap that pays): small calls stay one launch set.
#ifndef TVR_MIN_PIECES
#define TVR_MIN_PIECES 6
#endif
struct PiecePlan { int K; int64_t rays; };
static PiecePlan piece_plan(const tvr_scene *s, int64_t n_rays)
{
    PiecePlan P = {1, n_rays};
    const int64_t pr = s ? s->piece_rays : default_piece_rays();
    if (pr <= 0 || n_rays < TVR_MIN_PIECES * pr) return P;
    const int64_t K = (n_rays + pr / 2) / pr, q = pr >= 512 ? 512 : 16;          // (pieces below 512 rays: tests on tiny fixtures)
    P.rays = ((n_rays + K - 1) / K + q - 1) / q * q;
    P.K = (int)((n_rays + P.rays - 1) / P.rays);
    if (P.K < 2) { P.K = 1; P.rays = n_rays; }
    return P;
}

size_t tvr_render_scratch_bytes(const tvr_scene *s, int64_t n_rays, int32_t n_samples)
{
    if (n_rays <= 0 || n_samples <= 0) return 256;
    const bool cp = s && s->cp;
    const size_t whole = scratch_layout(n_rays, n_samples, cp).total;
    const PiecePlan P = piece_plan(s, n_rays);             // two pieces in flight, each with a scratch of its own carved from the caller's buffer
    const size_t two = P.K > 1 ? 2 * scratch_layout(P.rays, n_samples, cp).total : 0;
    return whole > two ? whole : two;
}

// What a call WITHOUT `dense` needs: a call rendered in pieces works in two pieces' scratch (1.3 GB instead of 13 GB for the 800x800 x 512 frame: the queue is sized for the
// worst case, every sample of every ray shaded); a `dense` call is one launch set over the whole batch and needs tvr_render_scratch_bytes().
size_t tvr_render_scratch_bytes_min(const tvr_scene *s, int64_t n_rays, int32_t n_samples)
{
    if (n_rays <= 0 || n_samples <= 0) return 256;
    const PiecePlan P = piece_plan(s, n_rays);
    const bool cp = s && s->cp;
    return P.K > 1 ? 2 * scratch_layout(P.rays, n_samples, cp).total : scratch_layout(n_rays, n_samples, cp).total;
}

}  // extern "C"

// one launch set (header clear, march, shade, composite) on `stream`; ev: four events or nullptr
static int render_one(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, int32_t white_bg, const MarchSampling &sm, float eps_T, float *rgb_out, float *depth_out,
                      float *lam6_out, char *b, const ScratchLayout &L, const tvr_dense_out *dense, uint64_t *stats, hipEvent_t *ev, hipStream_t stream)
{
    MarchOut mo = carve_scratch(b, L, depth_out);
    mo.q_j = (dense && dense->rgb) ? (unsigned *)(b + L.q_j) : nullptr;
    mo.stats = (unsigned long long *)stats;
    mo.lam6 = lam6_out;
    HIP_TRY(launch_zero_header(mo.counter, stream));                   // [0] queue length, [1] the march's tile counter, [2] its fault flag, [3] unused here
    if (ev) HIP_TRY(hipEventRecord(ev[0], stream));
    if (s->cp) {
        // CP: march -> features (+ the entries' view directions) -> the network on the staged features -> colours + weights into q_out; every kernel behind the march takes
        // the entry count from the device (word 0 of the header), the grids are sized for the capacity: no host read
        const long long cap = (long long)n_rays * S;
        float *feat = (float *)(b + L.cp_feat), *dir = (float *)(b + L.cp_dir), *crgb = (float *)(b + L.cp_rgb);
        HIP_TRY(launch_cp_march(s->dev, s->cpd, rays, (int)n_rays, S, sm, eps_T, mo, dense, stream));
        if (ev) HIP_TRY(hipEventRecord(ev[1], stream));
        HIP_TRY(launch_cp_app_feature(s->dev, s->cpd, (const float *)mo.q_pos, 4, cap, mo.counter, mo.q_ray, rays, feat, dir, stream));
        ShadeArgs sa;
        memset(&sa, 0, sizeof(sa));
        sa.counter = mo.counter;
        sa.n = cap;
        sa.viewdirs = dir;
        sa.feats = feat;
        sa.out = crgb;
        HIP_TRY(launch_shade(s->dev, SH_SRC_FEAT, SH_DST_RGB, sa, stream));
        HIP_TRY(launch_cp_rgbw(mo, crgb, cap, stream));
        if (ev) HIP_TRY(hipEventRecord(ev[2], stream));
        if (dense && dense->rgb) {
            HIP_TRY(hipMemsetAsync(dense->rgb, 0, (size_t)n_rays * S * 3 * sizeof(float), stream));
            HIP_TRY(launch_scatter_rgb(mo, S, dense->rgb, stream));
        }
        HIP_TRY(launch_composite(mo, (int)n_rays, white_bg, rgb_out, stream));
        if (ev) HIP_TRY(hipEventRecord(ev[3], stream));
        return TVR_OK;
    }
    HIP_TRY(launch_march(s->dev, rays, (int)n_rays, S, sm, eps_T, mo, dense, stream, s->dvol));
    if (ev) HIP_TRY(hipEventRecord(ev[1], stream));
    ShadeArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.counter = mo.counter;
    sa.q_pos = mo.q_pos;
    sa.q_out = mo.q_out;
    sa.q_ray = mo.q_ray;
    sa.rays = rays;
    sa.stats = mo.stats;
    HIP_TRY(launch_shade(s->dev, SH_SRC_QUEUE, SH_DST_QUEUE, sa, stream, s->fvol));
    if (ev) HIP_TRY(hipEventRecord(ev[2], stream));
    if (dense && dense->rgb) {
        HIP_TRY(hipMemsetAsync(dense->rgb, 0, (size_t)n_rays * S * 3 * sizeof(float), stream));
        HIP_TRY(launch_scatter_rgb(mo, S, dense->rgb, stream));
    }
    HIP_TRY(launch_composite(mo, (int)n_rays, white_bg, rgb_out, stream));
    if (ev) HIP_TRY(hipEventRecord(ev[3], stream));
    return TVR_OK;
}

static int ensure_side_streams(tvr_scene *s)
{
    if (s->side_ready) return TVR_OK;
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(hipStreamCreateWithFlags(&s->side[i], hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&s->ev_join[i], hipEventDisableTiming));
    }
    HIP_TRY(hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming));
    s->side_ready = true;
    return TVR_OK;
}

static hipEvent_t *profile_slot(tvr_profile *prof);

static int render_impl(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, int32_t white_bg, const MarchSampling &sm, float eps_T,
                       float *rgb_out, float *depth_out, float *lam6_out, void *scratch, size_t scratch_bytes, const tvr_dense_out *dense,
                       uint64_t *stats, tvr_profile *prof, void *stream_)
{
    if (!s || !s->params_set) return fail(TVR_ERR_INVALID, "scene is NULL or tvr_scene_update has not run");
    if (n_rays == 0) return TVR_OK;
    if (!rays || !rgb_out || !depth_out || n_rays < 0) return fail(TVR_ERR_INVALID, "rays/rgb_out/depth_out NULL or n_rays < 0");
    if (S <= 0 || S > 4096) return fail(TVR_ERR_INVALID, "n_samples=%d out of [1,4096]", S);
    if ((size_t)n_rays * (size_t)S >= (1ull << 32)) return fail(TVR_ERR_INVALID, "n_rays*n_samples must be < 2^32 per call (chunk the rays)");
    if (!(eps_T >= 0.0f) || eps_T > s->desc.weight_thres)
        return fail(TVR_ERR_INVALID, "eps_T=%g must be in [0, weight_thres=%g] so that no appearance sample is skipped", eps_T, s->desc.weight_thres);
    const size_t need = dense ? scratch_layout(n_rays, S, s->cp).total : tvr_render_scratch_bytes_min(s, n_rays, S);
    if (!scratch || scratch_bytes < need) return fail(TVR_ERR_SCRATCH, "scratch %zu B < required %zu B", scratch_bytes, need);
    if ((uintptr_t)scratch % 256) return fail(TVR_ERR_SCRATCH, "scratch must be 256-byte aligned");
    if (prof && prof->n_calls >= prof->max_calls) return fail(TVR_ERR_INVALID, "profile is full (%d calls)", prof->max_calls);
    hipStream_t stream = (hipStream_t)stream_;
    if (s->dev.arith == TVR_ARITH_F16 && !s->dev.gen && s->h16_stale) TRY(refresh_h16(s, stream));        // the mode was set after the last tvr_scene_update
    if (!s->cp) {                          // the density volume, if one is attached: current, and this stream behind its bake, before anything forks
        TRY(ensure_dvol(s, stream));
        if (s->dev.arith == TVR_ARITH_F32) TRY(ensure_fvol(s, stream));          // (the reduced arithmetics shade on the factored kernels: nothing to bake for them)
    }
    // the per-sample outputs of `dense` are a debugging / parity surface ([n,S,*] arrays): such calls stay one launch set
    const PiecePlan P = dense ? PiecePlan{1, n_rays} : piece_plan(s, n_rays);
    if (P.K == 1) {
        hipEvent_t *ev = nullptr;
        if (prof && !(ev = profile_slot(prof))) return fail(TVR_ERR_HIP, "tvr_profile: hipEventCreate failed");
        int rc = render_one(s, rays, n_rays, S, white_bg, sm, eps_T, rgb_out, depth_out, lam6_out, (char *)scratch, scratch_layout(n_rays, S, s->cp), dense, stats, ev, stream);
        if (rc != TVR_OK) return rc;
        if (prof) prof->n_calls++;
        return TVR_OK;
    }
    // Piecewise (round 6): the overlap measured ACROSS frames with two frames in flight (round 5, render.FrameStream: 18.8 vs 19.7 ms) inside ONE call.  Piece k runs on
    // library-owned stream k & 1 in that stream's half of the caller's scratch; the two streams fork from the caller's stream by an event and are joined back into it by
    // two more, so the caller sees what it saw before: everything ordered on its stream.  The persistent kernels of one piece take the CUs the other piece's kernels leave
    // as they drain, and a march (L1-bound, 2.1 GHz) beside a shade kernel (matrix-bound, 1.75 GHz) shares the chip's power budget better than either alone.  Every ray's
    // result is independent of the batch it arrives in (bit for bit: tests/test_gpu_parity.py), so the pixels are those of the one-piece call.
    int rc = ensure_side_streams(s);
    if (rc != TVR_OK) return rc;
    const ScratchLayout Lp = scratch_layout(P.rays, S, s->cp);
    HIP_TRY(hipEventRecord(s->ev_fork, stream));
    for (int i = 0; i < 2; ++i) HIP_TRY(hipStreamWaitEvent(s->side[i], s->ev_fork, 0));
    // (equal pieces: a half- or third-size first piece on stream 1 — a stagger from the start — measured 18.71 - 18.76 ms against 18.64 - 18.67, profiles/r06_split_frame.txt)
    int64_t a = 0;
    for (int k = 0; a < n_rays && rc == TVR_OK; ++k) {
        const int64_t m = (a + P.rays <= n_rays) ? P.rays : n_rays - a;
        const MarchSampling smk = {sm.jitter ? sm.jitter + a : nullptr, sm.zv ? sm.zv + (size_t)a * S : nullptr};
        hipEvent_t *ev = nullptr;
        if (prof && !(ev = profile_slot(prof))) { rc = fail(TVR_ERR_HIP, "tvr_profile: hipEventCreate failed"); break; }
        rc = render_one(s, rays + 6 * a, m, S, white_bg, smk, eps_T, rgb_out + 3 * a, depth_out + a, lam6_out ? lam6_out + a : nullptr,
                        (char *)scratch + (size_t)(k & 1) * Lp.total, Lp, nullptr, stats, ev, s->side[k & 1]);
        a += m;
    }
    // the join is enqueued whatever happened above: whatever DID go out on the two streams is ordered in front of the caller's next work (an error leaves the outputs
    // undefined, never a side stream still writing them behind the caller's back)
    for (int i = 0; i < 2; ++i) {
        const hipError_t e1 = hipEventRecord(s->ev_join[i], s->side[i]);
        const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(stream, s->ev_join[i], 0) : e1;
        if (e2 != hipSuccess && rc == TVR_OK) rc = fail(TVR_ERR_HIP, "tvr_render: joining the piece streams: %s", hipGetErrorString(e2));
    }
    if (rc != TVR_OK) return rc;
    if (prof) prof->n_calls++;
    return TVR_OK;
}

extern "C" {

int tvr_render(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, int32_t white_bg, const float *jitter, float eps_T,
               float *rgb_out, float *depth_out, void *scratch, size_t scratch_bytes, const tvr_dense_out *dense,
               uint64_t *stats, tvr_profile *prof, void *stream)
{
    const MarchSampling sm = {jitter, nullptr};
    return render_impl(s, rays, n_rays, S, white_bg, sm, eps_T, rgb_out, depth_out, nullptr, scratch, scratch_bytes, dense, stats, prof, stream);
}

int tvr_render_z(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, int32_t white_bg, const float *z_vals, float eps_T,
                 float *rgb_out, float *depth_out, float *t_last_tiny_out, void *scratch, size_t scratch_bytes, const tvr_dense_out *dense,
                 uint64_t *stats, void *stream)
{
    NOT_CP(s);
    if (!z_vals) return fail(TVR_ERR_INVALID, "z_vals is NULL");
    const MarchSampling sm = {nullptr, z_vals};
    return render_impl(s, rays, n_rays, S, white_bg, sm, eps_T, rgb_out, depth_out, t_last_tiny_out, scratch, scratch_bytes, dense, stats, nullptr, stream);
}

int tvr_scratch_describe(int64_t n_rays, int32_t n_samples, tvr_scratch_layout *out)
{
    if (!out || n_rays <= 0 || n_samples <= 0) return fail(TVR_ERR_INVALID, "bad arguments");
    ScratchLayout L = scratch_layout(n_rays, n_samples);
    out->counter = L.counter; out->ray_off = L.ray_off; out->ray_cnt = L.ray_cnt; out->acc = L.acc;
    out->q_pos = L.q_pos; out->q_out = L.q_out; out->q_ray = L.q_ray; out->q_j = L.q_j; out->total = L.total;
    return TVR_OK;
}

}  // extern "C"

// (declared in tvr_scene.h: tvr_train_api.hip's tvr_train_forward begins with this march)
int march_forward_impl(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, const MarchSampling &sm, float eps_T, float *depth_out,
                       float *lam6_out, void *scratch, size_t scratch_bytes, void *stream_)
{
    NOT_CP(s);
    TRY(scene_ready(s));
    if (!rays || !depth_out || n_rays <= 0) return fail(TVR_ERR_INVALID, "rays/depth_out NULL or n_rays <= 0");
    TRY(march_args_ok(s, n_rays, S, eps_T, scratch, scratch_bytes, "scratch too small (%zu < %zu) or misaligned"));
    ScratchLayout L = scratch_layout(n_rays, S);
    hipStream_t stream = (hipStream_t)stream_;
    MarchOut mo = carve_scratch((char *)scratch, L, depth_out);
    mo.lam6 = lam6_out;
    HIP_TRY(launch_zero_header(mo.counter, stream));                   // [0] queue length, [1] the march's tile counter, [2] its fault flag, [3] workspace overflow
    HIP_TRY(launch_march(s->dev, rays, (int)n_rays, S, sm, eps_T, mo, nullptr, stream));
    // a training queue is put into ray order (the q_out / q_j regions are unused on this path): the weight gradients then do not depend on the order the
    // march kernel's waves finished in.  Small batches only — the training path's own (train.py draws 4096 rays); a caller that marches a whole frame through
    // this entry point keeps the kernel's order and rounding-level reproducibility.
    if (n_rays <= TVR_RAY_ORDER_MAX_RAYS)
        HIP_TRY(launch_queue_ray_order(mo, (unsigned *)((char *)scratch + L.ray_new), mo.q_out, (unsigned *)((char *)scratch + L.q_j), (int)n_rays, stream));
    return TVR_OK;
}

extern "C" {

// max |a - b| over n floats -> out[0] (as the bits of a non-negative float: integer max); a NaN on either side counts as +inf
__global__ __launch_bounds__(256) void maxdiff_kernel(const float *__restrict__ a, const float *__restrict__ b, long long n, unsigned *__restrict__ out)
{
    float m = 0.0f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float d = fabsf(a[i] - b[i]);
        m = (d == d) ? fmaxf(m, d) : INFINITY;
    }
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));
}

int tvr_scene_validate_arith(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, int32_t white_bg, float eps_T, float tol, void *scratch, size_t scratch_bytes,
                             float *work, size_t work_bytes, float *max_diff_out, int64_t *probe_app_samples_out, void *stream_)
{
    NOT_CP(s);
    if (!s || !s->params_set) return fail(TVR_ERR_INVALID, "tvr_scene_validate_arith: scene is NULL or tvr_scene_update has not run");
    if (!max_diff_out) return fail(TVR_ERR_INVALID, "tvr_scene_validate_arith: max_diff_out is NULL");
    *max_diff_out = 0.0f;
    if (probe_app_samples_out) *probe_app_samples_out = 0;
    if (s->arith_req == TVR_ARITH_F32) return TVR_OK;                                    // nothing to validate
    if (s->dev.gen) {                                   // more than two encoding frequencies: the lockstep kernels compute with three products whatever the mode says
        tvr_set_error(TVR_OK, "tvr_scene_validate_arith: scenes with more than two encoding frequencies compute in TVR_ARITH_F32 whatever the mode says");
        return TVR_OK;
    }
    if (n_rays <= 0 || !rays || !work) return fail(TVR_ERR_INVALID, "tvr_scene_validate_arith: rays / work NULL or n_rays <= 0");
    if ((uintptr_t)work % 16) return fail(TVR_ERR_SCRATCH, "tvr_scene_validate_arith: work must be 16-byte aligned");
    if (!(tol > 0.0f)) return fail(TVR_ERR_INVALID, "tvr_scene_validate_arith: tol must be positive");
    if (work_bytes < (size_t)n_rays * 8 * sizeof(float) + 256) return fail(TVR_ERR_SCRATCH, "tvr_scene_validate_arith: work %zu B < required %zu B", work_bytes, (size_t)n_rays * 32 + 256);
    hipStream_t stream = (hipStream_t)stream_;
    float *rgb0 = work, *dep0 = work + 3 * n_rays, *rgb1 = work + 4 * n_rays, *dep1 = work + 7 * n_rays;
    unsigned *mx = (unsigned *)(work + 8 * n_rays);
    const MarchSampling sm = {nullptr, nullptr};
    s->dev.arith = TVR_ARITH_F32;
    int rc = render_impl(s, rays, n_rays, S, white_bg, sm, eps_T, rgb0, dep0, nullptr, scratch, scratch_bytes, nullptr, nullptr, nullptr, stream_);
    if (rc != TVR_OK) return rc;
    s->dev.arith = s->arith_req;
    rc = render_impl(s, rays, n_rays, S, white_bg, sm, eps_T, rgb1, dep1, nullptr, scratch, scratch_bytes, nullptr, nullptr, nullptr, stream_);
    s->dev.arith = TVR_ARITH_F32;
    if (rc != TVR_OK) return rc;
    HIP_TRY(launch_zero_f32((float *)mx, 4, stream));                                   // (float4 granules: the 256 B behind the eight arrays are for this)
    hipLaunchKernelGGL(maxdiff_kernel, dim3(256), dim3(256), 0, stream, rgb0, rgb1, (long long)n_rays * 3, mx);
    HIP_TRY(hipGetLastError());
    unsigned bits = 0, shaded = 0;
    HIP_TRY(hipMemcpyAsync(&bits, mx, sizeof(bits), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&shaded, scratch, sizeof(shaded), hipMemcpyDeviceToHost, stream));   // word 0 of the scratch header: the probe's appearance-sample count
    HIP_TRY(hipStreamSynchronize(stream));
    float d;
    memcpy(&d, &bits, sizeof(d));
    *max_diff_out = d;
    if (probe_app_samples_out) *probe_app_samples_out = (int64_t)shaded;
    // A probe that shaded (almost) nothing measured nothing: rays that miss the box or cross empty space give two background pictures, d = 0.  Such a
    // probe neither validates nor refuses — the mode stays un-measured and the caller probes again with rays that hit something.
    const int64_t need = 2 * n_rays < TVR_ARITH_MIN_PROBE_SAMPLES ? 2 * n_rays : TVR_ARITH_MIN_PROBE_SAMPLES;      // (a probe of a few dozen rays: two samples per ray)
    if ((int64_t)shaded < need) {
        s->arith_valid = 0;
        tvr_set_error(TVR_OK, "tvr_scene_validate_arith: mode %d NOT MEASURED — the %lld probe rays shaded %u appearance samples, fewer than the %lld a measurement needs; "
                              "the scene computes in TVR_ARITH_F32 until a probe that hits the scene validates the mode", s->arith_req, (long long)n_rays, shaded,
                      (long long)need);
        return TVR_OK;
    }
    if (d <= tol) {
        s->arith_valid = s->arith_req;
        s->dev.arith = s->arith_req;
        return TVR_OK;
    }
    s->arith_valid = 0;
    tvr_set_error(TVR_OK, "tvr_scene_validate_arith: mode %d REFUSED for these parameters — its picture differs from TVR_ARITH_F32's by %.3g on the %lld probe rays, the tolerance is %.3g; "
                          "the scene computes in TVR_ARITH_F32", s->arith_req, (double)d, (long long)n_rays, (double)tol);
    return TVR_OK;
}

int tvr_march_forward(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, const float *jitter, float eps_T, float *depth_out,
                      void *scratch, size_t scratch_bytes, void *stream)
{
    const MarchSampling sm = {jitter, nullptr};
    return march_forward_impl(s, rays, n_rays, S, sm, eps_T, depth_out, nullptr, scratch, scratch_bytes, stream);
}

int tvr_march_forward_z(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, const float *z_vals, float eps_T, float *depth_out,
                        float *t_last_tiny_out, void *scratch, size_t scratch_bytes, void *stream)
{
    if (!z_vals) return fail(TVR_ERR_INVALID, "z_vals is NULL");
    const MarchSampling sm = {nullptr, z_vals};
    return march_forward_impl(s, rays, n_rays, S, sm, eps_T, depth_out, t_last_tiny_out, scratch, scratch_bytes, stream);
}

int tvr_filter_rays(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, int32_t bbox_only, uint8_t *mask, size_t mask_bytes, void *stream)
{
    if (!s) return fail(TVR_ERR_INVALID, "scene is NULL");
    if (n_rays < 0 || (!bbox_only && S < 1)) return fail(TVR_ERR_INVALID, "n_rays < 0 or N_samples < 1");
    if (n_rays == 0) return TVR_OK;
    if (!rays || !mask) return fail(TVR_ERR_INVALID, "rays / mask NULL");
    if (mask_bytes < (size_t)n_rays) return fail(TVR_ERR_SCRATCH, "mask holds fewer than n_rays bytes");
    if (!bbox_only && !s->dev.avol) return fail(TVR_ERR_INVALID, "the scene has no alpha mask (tvr_scene_set_alpha): only bbox_only filtering is defined");
    HIP_TRY(launch_filter_rays(s->dev, rays, n_rays, S, bbox_only ? 1 : 0, mask, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_density_feature(tvr_scene *s, const float *xyz, int64_t m, float *out, size_t out_bytes, void *stream)
{
    if (m > 0) NEED("out [m]", out_bytes, m, 1);
    if (!s || !s->params_set) return fail(TVR_ERR_INVALID, "scene is NULL or tvr_scene_update has not run");
    if (m == 0) return TVR_OK;
    if (!xyz || !out || m < 0) return fail(TVR_ERR_INVALID, "xyz/out NULL or m < 0");
    if (s->cp) HIP_TRY(launch_cp_density_feature(s->dev, s->cpd, xyz, m, out, (hipStream_t)stream));
    else HIP_TRY(launch_density_feature(s->dev, xyz, m, out, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_density_gradient(tvr_scene *s, const float *xyz, int64_t m, const float half_width[3], float *sigma_feature, size_t sigma_bytes, float *grad, size_t grad_bytes,
                         void *stream)
{
    if (m > 0) {
        NEED("grad [m,3]", grad_bytes, m, 3);
        if (sigma_feature) NEED("sigma_feature [m]", sigma_bytes, m, 1);
    }
    if (!s || !s->params_set) return fail(TVR_ERR_INVALID, "scene is NULL or tvr_scene_update has not run");
    if (!half_width) return fail(TVR_ERR_INVALID, "half_width is NULL");
    float inv2h[3];
    for (int k = 0; k < 3; ++k) {
        if (!(half_width[k] > 0.0f) || !(half_width[k] <= 3.4028234664e38f)) return fail(TVR_ERR_INVALID, "half_width[%d] = %g must be finite and > 0", k, half_width[k]);
        inv2h[k] = 0.5f / half_width[k];
    }
    if (m == 0) return TVR_OK;
    if (!xyz || !grad || m < 0) return fail(TVR_ERR_INVALID, "xyz/grad NULL or m < 0");
    if (m >= (1ll << 38)) return fail(TVR_ERR_INVALID, "m = %lld: at most 2^38 - 1 points per call", (long long)m);
    if (s->cp) HIP_TRY(launch_cp_density_gradient(s->dev, s->cpd, xyz, m, half_width, inv2h, sigma_feature, grad, (hipStream_t)stream));
    else HIP_TRY(launch_density_gradient(s->dev, xyz, m, half_width, inv2h, sigma_feature, grad, (hipStream_t)stream));
    return TVR_OK;
}

// projection of mesh vertices onto the iso-surface (tvr_mesh_project.hip): the one tvr_mesh_* call that reads a scene, so it lives here and not in tvr_mesh_api.hip
int tvr_mesh_project(tvr_scene *s, const float *verts, int64_t n_vertices, const uint8_t *pinned, float target_feature, int32_t iterations, const float half_width[3],
                     const float max_move[3], float tol, float *verts_out, size_t verts_out_bytes, float *residual_in, size_t residual_in_bytes, float *residual_out,
                     size_t residual_out_bytes, int64_t *counts_dev, void *stream)
{
    if (!s || !s->params_set) return fail(TVR_ERR_INVALID, "%s: scene is NULL or tvr_scene_update has not run", __func__);
    if (n_vertices < 0) return fail(TVR_ERR_INVALID, "%s: n_vertices = %lld is negative", __func__, (long long)n_vertices);
    if (n_vertices > 0x7fffffffll) return fail(TVR_ERR_UNSUPPORTED, "%s: n_vertices = %lld: at most 2^31 - 1 vertices per call", __func__, (long long)n_vertices);
    if (iterations < 0 || iterations > TVR_MESH_PROJECT_MAX_ITERATIONS)
        return fail(TVR_ERR_INVALID, "%s: iterations %d outside 0 .. %d", __func__, (int)iterations, TVR_MESH_PROJECT_MAX_ITERATIONS);
    if (!half_width || !max_move) return fail(TVR_ERR_INVALID, "%s: half_width / max_move is NULL", __func__);
    float inv2h[3];
    for (int k = 0; k < 3; ++k) {
        if (!(half_width[k] > 0.0f) || !std::isfinite(half_width[k]))
            return fail(TVR_ERR_INVALID, "%s: half_width[%d] = %g must be finite and > 0", __func__, k, (double)half_width[k]);
        if (!(max_move[k] > 0.0f) || !std::isfinite(max_move[k])) return fail(TVR_ERR_INVALID, "%s: max_move[%d] = %g must be finite and > 0", __func__, k, (double)max_move[k]);
        inv2h[k] = 0.5f / half_width[k];
    }
    if (!std::isfinite(target_feature)) return fail(TVR_ERR_INVALID, "%s: target_feature = %g must be finite", __func__, (double)target_feature);
    if (!(tol >= 0.0f)) return fail(TVR_ERR_INVALID, "%s: tol = %g must be >= 0", __func__, (double)tol);
    if (!counts_dev) return fail(TVR_ERR_INVALID, "%s: counts_dev is NULL", __func__);
    if (n_vertices > 0) {
        if (!verts || !verts_out || !residual_out) return fail(TVR_ERR_INVALID, "%s: verts / verts_out / residual_out is NULL", __func__);
        NEED("verts_out [n_vertices,3]", verts_out_bytes, n_vertices, 3);
        NEED("residual_out [n_vertices]", residual_out_bytes, n_vertices, 1);
        if (residual_in) NEED("residual_in [n_vertices]", residual_in_bytes, n_vertices, 1);
    }
    HIP_TRY(hipMemsetAsync(counts_dev, 0, 4 * sizeof(int64_t), (hipStream_t)stream));
    if (n_vertices == 0) return TVR_OK;
    HIP_TRY(launch_mesh_project(s->dev, s->cp ? &s->cpd : nullptr, verts, n_vertices, pinned, target_feature, iterations, half_width, inv2h, max_move, tol, verts_out,
                                residual_in, residual_out, (unsigned long long *)counts_dev, (hipStream_t)stream));
    return TVR_OK;
}

// tvr_render_normals' scratch: the header, the per-ray arrays the march writes (depth among them: the march writes one whether or not the caller wants it) and the
// queue's positions and ray indices; neither q_out / q_j nor a CP scene's staging regions (nothing is shaded)
struct NormalsLayout { size_t counter, ray_off, ray_cnt, acc, depth, q_pos, q_ray, total; };
static NormalsLayout normals_layout(int64_t n_rays, int32_t S)
{
    NormalsLayout L;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t cap = (size_t)n_rays * (size_t)S;
    L.counter = take(256);
    L.ray_off = take(n_rays * 4);
    L.ray_cnt = take(n_rays * 4);
    L.acc = take(n_rays * 4);
    L.depth = take(n_rays * 4);
    L.q_pos = take(cap * 16);
    L.q_ray = take(cap * 4);
    L.total = off;
    return L;
}

size_t tvr_render_normals_scratch_bytes(const tvr_scene *, int64_t n_rays, int32_t n_samples)
{
    if (n_rays <= 0 || n_samples <= 0) return 256;
    return normals_layout(n_rays, n_samples).total;
}

int tvr_render_normals(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, const float *jitter, float eps_T, const float half_width[3], float *normal_out,
                       size_t normal_bytes, float *acc_out, size_t acc_bytes, float *depth_out, size_t depth_bytes, void *scratch, size_t scratch_bytes, void *stream_)
{
    if (!s || !s->params_set) return fail(TVR_ERR_INVALID, "tvr_render_normals: scene is NULL or tvr_scene_update has not run");
    if (!half_width) return fail(TVR_ERR_INVALID, "tvr_render_normals: half_width is NULL");
    float inv2h[3];
    for (int k = 0; k < 3; ++k) {
        if (!(half_width[k] > 0.0f) || !(half_width[k] <= 3.4028234664e38f))
            return fail(TVR_ERR_INVALID, "tvr_render_normals: half_width[%d] = %g must be finite and > 0", k, half_width[k]);
        inv2h[k] = 0.5f / half_width[k];
    }
    if (n_rays < 0) return fail(TVR_ERR_INVALID, "tvr_render_normals: n_rays < 0");
    if (n_rays == 0) return TVR_OK;
    if (!rays || !normal_out) return fail(TVR_ERR_INVALID, "tvr_render_normals: rays / normal_out NULL");
    if (S <= 0 || S > 4096) return fail(TVR_ERR_INVALID, "tvr_render_normals: n_samples=%d out of [1,4096]", S);
    if ((size_t)n_rays * (size_t)S >= (1ull << 32)) return fail(TVR_ERR_INVALID, "tvr_render_normals: n_rays*n_samples must be < 2^32 per call (chunk the rays)");
    if (!(eps_T >= 0.0f) || eps_T > s->desc.weight_thres)
        return fail(TVR_ERR_INVALID, "tvr_render_normals: eps_T=%g must be in [0, weight_thres=%g] so that no appearance sample is skipped", eps_T, s->desc.weight_thres);
    NEED("normal_out [n,3]", normal_bytes, n_rays, 3);
    if (acc_out) NEED("acc_out [n]", acc_bytes, n_rays, 1);
    if (depth_out) NEED("depth_out [n]", depth_bytes, n_rays, 1);
    const NormalsLayout L = normals_layout(n_rays, S);
    if (!scratch || scratch_bytes < L.total) return fail(TVR_ERR_SCRATCH, "tvr_render_normals: scratch %zu B < required %zu B", scratch_bytes, L.total);
    if ((uintptr_t)scratch % 256) return fail(TVR_ERR_SCRATCH, "tvr_render_normals: scratch must be 256-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    if (!s->cp) TRY(ensure_dvol(s, stream));       // the same march as tvr_render's: the density volume, if one is attached
    char *b = (char *)scratch;
    MarchOut mo;
    mo.counter = (unsigned *)(b + L.counter);
    mo.ray_off = (unsigned *)(b + L.ray_off);
    mo.ray_cnt = (unsigned *)(b + L.ray_cnt);
    mo.acc = (float *)(b + L.acc);
    mo.depth = depth_out ? depth_out : (float *)(b + L.depth);
    mo.q_pos = (float4 *)(b + L.q_pos);
    mo.q_out = mo.q_pos;                                               // (nothing is shaded: the march never touches q_out)
    mo.q_ray = (unsigned *)(b + L.q_ray);
    mo.q_j = nullptr;
    mo.stats = nullptr;
    mo.lam6 = nullptr;
    const MarchSampling sm = {jitter, nullptr};
    HIP_TRY(launch_zero_header(mo.counter, stream));                   // [0] queue length, [1] the march's tile counter, [2] its fault flag, [16] the normal pass's ray tickets
    if (s->cp) HIP_TRY(launch_cp_march(s->dev, s->cpd, rays, (int)n_rays, S, sm, eps_T, mo, nullptr, stream));
    else HIP_TRY(launch_march(s->dev, rays, (int)n_rays, S, sm, eps_T, mo, nullptr, stream, s->dvol));
    HIP_TRY(launch_normals(s->dev, s->cp ? &s->cpd : nullptr, mo, (int)n_rays, half_width, inv2h, normal_out, acc_out, depth_out, stream));
    return TVR_OK;
}

int tvr_app_feature(tvr_scene *s, const float *xyz, int64_t m, float *out, size_t out_bytes, void *stream)
{
    if (m > 0) NEED("out [m,27]", out_bytes, m, TVR_APPDIM);
    if (!s || !s->params_set) return fail(TVR_ERR_INVALID, "scene is NULL or tvr_scene_update has not run");
    if (m == 0) return TVR_OK;
    if (!xyz || !out || m < 0) return fail(TVR_ERR_INVALID, "xyz/out NULL or m < 0");
    if (s->cp) {
        HIP_TRY(launch_cp_app_feature(s->dev, s->cpd, xyz, 3, m, nullptr, nullptr, nullptr, out, nullptr, (hipStream_t)stream));
        return TVR_OK;
    }
    ShadeArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.n = m;
    sa.xyz = xyz;
    sa.out = out;
    HIP_TRY(launch_shade(s->dev, SH_SRC_XYZ, SH_DST_FEAT, sa, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_app_feature_ref(tvr_scene *s, const float *xyz, int64_t m, float *features, size_t features_bytes, float *extra, size_t extra_bytes, void *stream)
{
    NOT_CP(s);
    if (m > 0) {
        NEED("features [m,27]", features_bytes, m, TVR_APPDIM);
        NEED("extra [m,8]", extra_bytes, m, 8);
    }
    TRY(scene_ready(s));
    if (s->desc.variant != 1) return fail(TVR_ERR_INVALID, "tvr_app_feature_ref needs a REFTensoRF (variant 1) scene");
    if (m == 0) return TVR_OK;
    if (!xyz || !features || !extra || m < 0) return fail(TVR_ERR_INVALID, "xyz/features/extra NULL or m < 0");
    ShadeArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.n = m;
    sa.xyz = xyz;
    sa.out = features;
    sa.out2 = extra;
    HIP_TRY(launch_shade(s->dev, SH_SRC_XYZ, SH_DST_FEAT, sa, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_mlp_render_ref(tvr_scene *s, const float *viewdirs, const float *features, const float *dot_product, int64_t m, float *rgb,
                       size_t rgb_bytes, void *stream)
{
    NOT_CP(s);
    if (m > 0) NEED("rgb [m,3]", rgb_bytes, m, 3);
    TRY(scene_ready(s));
    if (s->desc.variant != 1) return fail(TVR_ERR_INVALID, "tvr_mlp_render_ref needs a REFTensoRF (variant 1) scene");
    if (m == 0) return TVR_OK;
    if (!viewdirs || !features || !dot_product || !rgb || m < 0) return fail(TVR_ERR_INVALID, "viewdirs/features/dot_product/rgb NULL or m < 0");
    ShadeArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.n = m;
    sa.viewdirs = viewdirs;
    sa.feats = features;
    sa.dots = dot_product;
    sa.out = rgb;
    HIP_TRY(launch_shade(s->dev, SH_SRC_FEAT, SH_DST_RGB, sa, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_mlp_render(tvr_scene *s, const float *viewdirs, const float *features, int64_t m, float *rgb, size_t rgb_bytes, void *stream)
{
    if (m > 0) NEED("rgb [m,3]", rgb_bytes, m, 3);
    if (!s || !s->params_set) return fail(TVR_ERR_INVALID, "scene is NULL or tvr_scene_update has not run");
    if (s->desc.variant != 0) return fail(TVR_ERR_INVALID, "tvr_mlp_render is MLPRender_Fea; a REFTensoRF scene takes tvr_mlp_render_ref");
    if (m == 0) return TVR_OK;
    if (!viewdirs || !features || !rgb || m < 0) return fail(TVR_ERR_INVALID, "viewdirs/features/rgb NULL or m < 0");
    ShadeArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.n = m;
    sa.viewdirs = viewdirs;
    sa.feats = features;
    sa.out = rgb;
    HIP_TRY(launch_shade(s->dev, SH_SRC_FEAT, SH_DST_RGB, sa, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_alpha_sample(const float *vol, const int32_t ag[3], const float aabb[6], const float inv[3], const float *xyz,
                     int64_t m, float *out, size_t out_bytes, void *stream)
{
    if (m > 0) NEED("out [m]", out_bytes, m, 1);
    if (!vol || !ag || !aabb || !inv) return fail(TVR_ERR_INVALID, "alpha volume/grid/aabb/inv is NULL");
    if (m == 0) return TVR_OK;
    if (!xyz || !out || m < 0) return fail(TVR_ERR_INVALID, "xyz/out NULL or m < 0");
    SceneDev v;
    memset(&v, 0, sizeof(v));
    for (int k = 0; k < 3; ++k) {
        if (ag[k] < 1) return fail(TVR_ERR_INVALID, "alpha grid[%d]=%d", k, ag[k]);
        v.ag[k] = ag[k];
        v.alo[k] = aabb[k];
        v.ainv[k] = inv[k];
        v.agm1[k] = (float)(ag[k] - 1);
    }
    v.avol = vol;
    HIP_TRY(launch_alpha_sample(v, xyz, m, out, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_profile_create(int32_t max_calls, tvr_profile **out)
{
    if (!out || max_calls <= 0 || max_calls > 100000) return fail(TVR_ERR_INVALID, "bad profile arguments");
    tvr_profile *p = new (std::nothrow) tvr_profile;
    if (!p) return fail(TVR_ERR_INVALID, "out of host memory");
    p->max_calls = max_calls;
    p->n_calls = 0;
    p->n_sets = 0;
    p->ev.reserve((size_t)max_calls * 4);      // events are created as launch sets are recorded (a piecewise call records one set per piece) and kept across resets
    *out = p;
    return TVR_OK;
}

int tvr_profile_reset(tvr_profile *p)
{
    if (!p) return fail(TVR_ERR_INVALID, "profile is NULL");
    p->n_calls = 0;
    p->n_sets = 0;
    return TVR_OK;
}

int tvr_profile_read(tvr_profile *p, float ms[3])
{
    if (!p || !ms) return fail(TVR_ERR_INVALID, "profile/ms is NULL");
    ms[0] = ms[1] = ms[2] = 0.f;
    for (int c = 0; c < p->n_sets; ++c)
        for (int k = 0; k < 3; ++k) {
            float t = 0.f;
            hipError_t rc = hipEventElapsedTime(&t, p->ev[(size_t)c * 4 + k], p->ev[(size_t)c * 4 + k + 1]);
            if (rc != hipSuccess) return fail(TVR_ERR_HIP, "hipEventElapsedTime: %s", hipGetErrorString(rc));
            ms[k] += t;
        }
    return p->n_calls;
}

}  // extern "C"

// four events for the next launch set (created on first use, re-used after tvr_profile_reset)
static hipEvent_t *profile_slot(tvr_profile *prof)
{
    const size_t need = ((size_t)prof->n_sets + 1) * 4;
    while (prof->ev.size() < need) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        prof->ev.push_back(e);
    }
    return &prof->ev[(size_t)prof->n_sets++ * 4];
}

extern "C" {

int tvr_profile_destroy(tvr_profile *p)
{
    if (!p) return TVR_OK;
    for (auto &e : p->ev) (void)hipEventDestroy(e);
    delete p;
    return TVR_OK;
}

}  // extern "C"
