// tvr_scene.h — what the C-API files that take a scene (tvr_api.hip, tvr_train_api.hip) both need to know about one: the scene object and its packed layout, the
// forward scratch of a march, the refusals every scene-taking entry point begins with, and the one copy of the march-argument check.  Host code only.  Everything
// here is a macro, has internal linkage or is declared hidden: libtvr.so exports nothing from this file.
#pragma once
#include "tvr_device.h"
#include "tvr_host.h"

static const int kMatH[3][2] = {{0, 1}, {0, 2}, {1, 2}};
static const int kVecH[3] = {2, 1, 0};

struct PackedLayout {
    size_t dplane[3], dline[3], aplane[3], aline[3];
    size_t aplane16[3], aline16[3];            // fp16 copies of the appearance factors (TVR_ARITH_F16's gather), floats / 2
    size_t mlp_image, basis_frag, b3, w1gen, img16, basg16, refg16, total;
    size_t cp_basis;                           // CP scenes: basis_mat as [ra / 4][27] float4 (CpDev::basis)
};

struct tvr_scene {             // (the initialisers: what tvr_scene_create leaves until tvr_scene_update and the tvr_scene_set_* calls say otherwise)
    bool cp;                   // a CP scene (tvr_cp_scene_create): dev.dline / dev.aline hold the CP lines, `cpd` the rest; default arithmetic only; trains through tvr_cp_* only
    CpDev cpd;
    tvr_scene_desc desc;
    PackedLayout lay;
    char *packed;
    SceneDev dev;
    bool params_set = false;
    bool h16_stale = true;     // the fp16 copies of the appearance factors are older than the fp32 images
    int arith_req = TVR_ARITH_F32;     // what tvr_scene_set_arith asked for; dev.arith is what the kernels RUN: arith_req once tvr_scene_validate_arith has measured it inside
    int arith_valid = 0;               // its tolerance for the parameters as packed (0 = nothing validated), TVR_ARITH_F32 until then
    // piecewise rendering (round 6, tvr_scene_set_render_pieces): a tvr_render(_z) call of at least 2 x piece_rays rays goes out as pieces of ~piece_rays consecutive rays,
    // alternately on two library-owned streams that fork from and join the caller's stream by events
    int piece_rays;
    hipStream_t side[2] = {nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
    bool side_ready = false;
    // the baked density volume (tvr_scene_set_density_volume): the caller's memory; `dvol_stale`: the packed density factors are newer than the volume — the next call
    // that launches the render march bakes first, on ITS stream, and records ev_dvol; a later call on another stream waits on that event (ensure_dvol)
    float *dvol = nullptr;
    bool dvol_stale = true, dvol_recorded = false;
    hipStream_t dvol_stream = nullptr;
    hipEvent_t ev_dvol = nullptr;
    // the baked appearance volume (tvr_scene_set_appearance_volume): the same rules for the render shade (ensure_fvol)
    float4 *fvol = nullptr;
    bool fvol_stale = true, fvol_recorded = false;
    hipStream_t fvol_stream = nullptr;
    hipEvent_t ev_fvol = nullptr;
};

// entry points a CP scene does not have (training, explicit depths, REFTensoRF's calls, the reduced arithmetics): refused before anything is launched
static int cp_refused(const tvr_scene *s, const char *fn)
{
    if (s && s->cp) return fail(TVR_ERR_UNSUPPORTED, "%s: the scene is a CP scene (tvr_cp_scene_create) — CP scenes render and answer field queries in the default arithmetic; "
                                                     "training, explicit depths, the _ref calls and the reduced arithmetics are not built for CP", fn);
    return TVR_OK;
}
#define NOT_CP(s)                                        \
    do {                                                 \
        int rcp_ = cp_refused((s), __func__);            \
        if (rcp_ != TVR_OK) return rcp_;                 \
    } while (0)

// and the CP training entry points (include/tvr.h, CP TRAINING), which take nothing else
static int cp_required(const tvr_scene *s, const char *fn)
{
    if (!s) return fail(TVR_ERR_INVALID, "%s: scene is NULL", fn);
    if (!s->cp) return fail(TVR_ERR_UNSUPPORTED, "%s: the scene is not a CP scene (tvr_cp_scene_create); TensorVMSplit / REFTensoRF scenes train through tvr_march_forward / "
                                                 "_backward, tvr_app_h_* and tvr_train_*", fn);
    return TVR_OK;
}

static int scene_ready(const tvr_scene *s)
{
    if (!s || !s->params_set) return fail(TVR_ERR_INVALID, "scene is NULL or tvr_scene_update has not run");
    return TVR_OK;
}

// scratch carving shared by the size query, tvr_render and the training marches
#define TVR_RAY_ORDER_MAX_RAYS 65536      // march_forward_impl: batches up to this many rays get a ray-ordered queue
struct ScratchLayout { size_t counter, ray_off, ray_cnt, acc, q_pos, q_out, q_ray, q_j, ray_new, cp_feat, cp_dir, cp_rgb, total; };
static ScratchLayout scratch_layout(int64_t n_rays, int32_t S, bool cp = false)
{
    ScratchLayout L;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t cap = (size_t)n_rays * (size_t)S;
    L.counter = take(256);
    L.ray_off = take(n_rays * 4);
    L.ray_cnt = take(n_rays * 4);
    L.acc = take(n_rays * 4);
    L.q_pos = take(cap * 16);
    L.q_out = take(cap * 16);
    L.q_ray = take(cap * 4);
    L.q_j = take(cap * 4);
    L.ray_new = take(n_rays * 4);          // the training queue's ray-ordered offsets (launch_queue_ray_order); behind everything the public layout names
    // a CP scene's render stages per queue entry what its feature kernel hands the network: features [cap,27], view direction [cap,3], colour [cap,3] (132 B more per entry)
    L.cp_feat = cp ? take(cap * TVR_APPDIM * 4) : 0;
    L.cp_dir = cp ? take(cap * 12) : 0;
    L.cp_rgb = cp ? take(cap * 12) : 0;
    L.total = off;
    return L;
}

static MarchOut carve_scratch(char *b, const ScratchLayout &L, float *depth_out)
{
    MarchOut mo;
    mo.counter = (unsigned *)(b + L.counter);
    mo.ray_off = (unsigned *)(b + L.ray_off);
    mo.ray_cnt = (unsigned *)(b + L.ray_cnt);
    mo.acc = (float *)(b + L.acc);
    mo.depth = depth_out;
    mo.q_pos = (float4 *)(b + L.q_pos);
    mo.q_out = (float4 *)(b + L.q_out);
    mo.q_ray = (unsigned *)(b + L.q_ray);
    mo.q_j = nullptr;
    mo.stats = nullptr;
    mo.lam6 = nullptr;
    return mo;
}

// ---- the march arguments: one copy -----------------------------------------------------------------------------------------------------------------------------------
// the forward scratch of a march over n_rays x S: not NULL, at least scratch_layout's bytes and, with `aligned`, on a 256-byte boundary.  `text` is the calling entry
// point's own wording of the refusal: a format that takes the two byte counts (%zu, %zu) or none
static int fwd_scratch_ok(const void *scratch, size_t have, int64_t n_rays, int32_t S, bool aligned, const char *text)
{
    const size_t want = scratch_layout(n_rays, S).total;
    if (!scratch || have < want || (aligned && (uintptr_t)scratch % 256)) return fail(TVR_ERR_SCRATCH, text, have, want);
    return TVR_OK;
}

// what every training march (tvr_march_forward(_z), tvr_cp_march_forward / _backward) asks of its arguments, in this order: the range of n_samples, the 32-bit queue
// index, eps_T, the forward scratch
static int march_args_ok(const tvr_scene *s, int64_t n_rays, int32_t S, float eps_T, const void *scratch, size_t have, const char *scratch_text)
{
    if (S <= 0 || S > 4096) return fail(TVR_ERR_INVALID, "n_samples=%d out of [1,4096]", S);
    if ((size_t)n_rays * (size_t)S >= (1ull << 32)) return fail(TVR_ERR_INVALID, "n_rays*n_samples must be < 2^32 per call");
    if (!(eps_T >= 0.0f) || eps_T > s->desc.weight_thres) return fail(TVR_ERR_INVALID, "eps_T=%g must be in [0, weight_thres]", eps_T);
    return fwd_scratch_ok(scratch, have, n_rays, S, true, scratch_text);
}

// ---- defined in tvr_api.hip, called from tvr_train_api.hip as well (hidden: not in libtvr.so's dynamic symbols) --------------------------------------------------------
// the march of tvr_march_forward(_z); tvr_train_forward begins with it
__attribute__((visibility("hidden"))) int march_forward_impl(tvr_scene *s, const float *rays, int64_t n_rays, int32_t S, const MarchSampling &sm, float eps_T,
                                                             float *depth_out, float *lam6_out, void *scratch, size_t scratch_bytes, void *stream_);
