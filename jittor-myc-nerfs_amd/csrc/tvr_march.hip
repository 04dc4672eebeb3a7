// tvr_march.hip — kernel 1 of the render path: ray/AABB entry + uniform (or jittered) sampling + in-box / alpha
// mask + VM density lookup + softplus + alpha + front-to-back transmittance scan, fused.
//
// Work it replaces in the reference (paths relative to /root/reference/tensorf-myc/):
//   models/tensorBase.py:340-360 sample_ray, :491-496 alpha-mask merge, :503 normalize_coord,
//   models/tensoRF.py:209-225 compute_densityfeature, tensorBase.py:444-448 feature2density,
//   :17-24 raw2alpha, :513 app_mask, :520 acc_map, :530-531 depth_map.
//
// Launch shape: persistent workgroups, one per CU (up to 16 waves), each taking 16-ray tiles in order from one global counter;
// the waves of a group take rays from an LDS cursor, so the 16 rays of a tile are marched concurrently (shared texels
// in L1) and no wave idles while the group has rays left.  The three density LINES (3 x (L+1) x 64 B, 58 KB at 300^3) are copied
// into LDS once per group: a third of the gather's 64-B requests then go to LDS instead of the L1/TA path that bounds this kernel.
//
// Mapping (wave64): one wave marches one ray, 64 consecutive samples per chunk.  Position / mask / index math is
// lane-per-sample.  The density gather is quad-per-sample: 4 lanes each fetch one float4 (4 of the 16 channels) of
// every texel, so a wave-level dwordx4 load covers 16 samples x 64 contiguous bytes (one texel per quad) — coalesced
// 64-B segments instead of 64 unrelated 16-B pieces.  Four sub-steps cover the 64 samples (sub-step k serves
// samples 4g+k), so after the quad reduction lane 4g+k owns sample 4g+k again with no permutation.
// The transmittance is a 6-step wave scan (DPP/shuffle) with the carry in a register; the ray stops once T < eps_T
// (eps_T <= weight threshold, so no appearance sample is ever skipped).  Appearance samples (w > thres) are compacted
// with a ballot into a per-wave LDS list and flushed once per ray into a contiguous, sample-ordered segment of the
// global queue (one atomicAdd per ray; the volume marches: one for up to MARCH_PEND rays, tvr_march_body.h) -> the compositing order per ray is fixed, results are deterministic.
#include <cstdlib>
#include "tvr_device.h"
#include "tvr_kernels.h"
#include "tvr_march_body.h"
#include "tvr_gradient.h"

// (Round 5 also computed everything that depends on the sample alone once per chunk and read it through quad_perm DPP operands: -8 % VALU instructions, bit-identical,
// 1.8 % slower — DESIGN.md 4.1.  Its interpolation ops were v_mul_f32_dpp / v_fmac_f32_dpp as inline asm: hipcc's DPP combine folds a broadcast into v_mul_f32 only, and
// only in src0 position — 15 v_mov_b32_dpp per sub-step stayed with the builtins.)

template <bool DENSE, bool LDSL>
__global__ __launch_bounds__(64 * MARCH_MAX_WAVES) void march_kernel(const SceneDev sc, const float *__restrict__ rays,
                                                                     const int n_rays, const int S, const int s_cap,
                                                                     const MarchSampling sm, const float eps_T,
                                                                     MarchOut mo, const tvr_dense_out dn)
{
    constexpr bool CP = false, VOL = false;               // the body is shared with the CP march (tvr_cp.hip) and the volume march (below) as text
    const CpDev cp = {};
    const float *const dvol = nullptr;
#include "tvr_march_body.inc"
}

// The march of a scene with a baked density volume (tvr_scene_set_density_volume): the same body, the density feature from vol_density (tvr_march_body.h) — 32 B per
// sample through L1 instead of 768 B and 384 B of LDS, seven lerps instead of three 16-channel bilinear / linear products and two quad reductions.  No line image in LDS:
// a group needs its header and 6 B per sample and wave; the launch shape and why: tvr_march_body.h (MARCH_VOL_*), DESIGN.md 4.1.
// PLAIN (only with !DENSE): the instantiation the frames of a plain scene run — no alpha volume, no explicit depths, no lam6, a volume below 4 GiB (launch_march_vol
// checks); those paths are absent from it at compile time and vol_density32 addresses the volume with 32-bit offsets (tvr_march_body.h).
// BATCH: one queue reservation for several rays (MARCH_BATCH, tvr_march_body.h).  A launch with no more rays than waves (a 4096-ray chunk on 256 CUs) has nothing to batch —
// every wave marches about one ray — and the way through the waiting ray's record would add its latency to every such call (measured: 157 calls per frame, +0.08 ms), so
// launch_march_vol gives it the unbatched instantiation; the two write the same queue entries for a ray, so which one runs changes no result.
template <bool DENSE, bool PLAIN, bool BATCH>
__global__ __launch_bounds__(64 * MARCH_VOL_WAVES, DENSE ? MARCH_VOL_OCC - 1 : MARCH_VOL_OCC) void march_vol_kernel(const SceneDev sc, const float *__restrict__ dvol, const float *__restrict__ rays,
                                                                         const int n_rays, const int S, const int s_cap, const MarchSampling sm, const float eps_T,
                                                                         MarchOut mo, const tvr_dense_out dn)
{
    static_assert(!(PLAIN && DENSE), "the plain form has no dense outputs");
    constexpr bool LDSL = false, CP = false, VOL = true, MARCH_BATCH = BATCH;
    const CpDev cp = {};
#include "tvr_march_body.inc"
}

// The bake: one thread per value of D, x fastest.  The 48 products plane_i[c] * line_i[c] (i = 0, 1, 2; c = 0 .. 15, in that order) are exact in fp64 and are summed in
// fp64, one rounding to fp32 at the end.  It reads the PACKED planes and lines (zero pad texel at index grid, zero pad channels), i.e. what the factored march reads, so
// the padding layer of D is 0.
__global__ __launch_bounds__(256) void density_volume_kernel(const SceneDev sc, float *__restrict__ out)
{
    const long long gx1 = sc.grid[0] + 1, gy1 = sc.grid[1] + 1, gz1 = sc.grid[2] + 1;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= gx1 * gy1 * gz1) return;
    const long long x = t % gx1, y = (t / gx1) % gy1, z = t / (gx1 * gy1);
    // plane0 (x,y) . line0(z) ; plane1 (x,z) . line1(y) ; plane2 (y,z) . line2(x)   (matMode / vecMode); plane i is [H+1][W+1] texels of 4 float4
    const float4 *P[3] = {sc.dplane[0] + (y * gx1 + x) * 4, sc.dplane[1] + (z * gx1 + x) * 4, sc.dplane[2] + (z * gy1 + y) * 4};
    const float4 *Ln[3] = {sc.dline[0] + z * 4, sc.dline[1] + y * 4, sc.dline[2] + x * 4};
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 p = P[i][g], l = Ln[i][g];
            acc = acc + (double)p.x * (double)l.x;
            acc = acc + (double)p.y * (double)l.y;
            acc = acc + (double)p.z * (double)l.z;
            acc = acc + (double)p.w * (double)l.w;
        }
    }
    out[t] = (float)acc;
}

hipError_t launch_density_volume(const SceneDev &sc, float *out, hipStream_t stream)
{
    const long long n = ((long long)sc.grid[0] + 1) * ((long long)sc.grid[1] + 1) * ((long long)sc.grid[2] + 1);      // <= 4097^3: fewer than 2^31 blocks
    hipLaunchKernelGGL(density_volume_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sc, out);
    return hipGetLastError();
}

// composite tail (tensorBase.py:520-527): rgb_map = sum_j w_j*rgb_j (+ 1-acc if white_bg), clamp(0,1).
// Eight lanes per ray read the ray's contiguous, sample-ordered queue segment 128 B at a time (lane l sums entries l, l+8, ...),
// then a fixed butterfly adds the eight partial sums: the summation order depends on nothing but the ray -> deterministic.
#define COMP_LANES 8
__global__ __launch_bounds__(256) void composite_kernel(const MarchOut mo, const int n_rays, const int white_bg,
                                                        float *__restrict__ rgb_out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = t / COMP_LANES, l = t % COMP_LANES;
    const bool live = r < n_rays;
    const unsigned base = live ? mo.ray_off[r] : 0u, cnt = live ? mo.ray_cnt[r] : 0u;
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    // four entries in flight per lane (a 4096-ray call is one wave per 8 rays and ~11 dependent round trips per lane otherwise: 10.9 us per
    // call, rocprofv3, where the data would take 3); the additions keep their order
    unsigned i = l;
    for (; i + 3 * COMP_LANES < cnt; i += 4 * COMP_LANES) {
        const float4 e0 = mo.q_out[base + i], e1 = mo.q_out[base + i + COMP_LANES], e2 = mo.q_out[base + i + 2 * COMP_LANES],
                     e3 = mo.q_out[base + i + 3 * COMP_LANES];     // {r,g,b,w} written by the shade kernel
        c0 = c0 + e0.w * e0.x; c1 = c1 + e0.w * e0.y; c2 = c2 + e0.w * e0.z;
        c0 = c0 + e1.w * e1.x; c1 = c1 + e1.w * e1.y; c2 = c2 + e1.w * e1.z;
        c0 = c0 + e2.w * e2.x; c1 = c1 + e2.w * e2.y; c2 = c2 + e2.w * e2.z;
        c0 = c0 + e3.w * e3.x; c1 = c1 + e3.w * e3.y; c2 = c2 + e3.w * e3.z;
    }
    for (; i < cnt; i += COMP_LANES) {
        const float4 e = mo.q_out[base + i];
        c0 = c0 + e.w * e.x;
        c1 = c1 + e.w * e.y;
        c2 = c2 + e.w * e.z;
    }
#pragma unroll
    for (int off = 1; off < COMP_LANES; off <<= 1) {
        c0 = c0 + __shfl_xor(c0, off);
        c1 = c1 + __shfl_xor(c1, off);
        c2 = c2 + __shfl_xor(c2, off);
    }
    if (!live || l != 0) return;
    if (mo.counter[2] != 0u) {                        // the march raised its fault flag (tile-queue wait): no pixel of this call is trustworthy
        const float qnan = __int_as_float(0x7fc00000);
        rgb_out[(size_t)r * 3 + 0] = qnan; rgb_out[(size_t)r * 3 + 1] = qnan; rgb_out[(size_t)r * 3 + 2] = qnan;
        mo.depth[r] = qnan;
        return;
    }
    const float acc = mo.acc[r];
    if (white_bg) {
        const float bg = 1.0f - acc;
        c0 = c0 + bg; c1 = c1 + bg; c2 = c2 + bg;
    }
    rgb_out[(size_t)r * 3 + 0] = clamp01(c0);
    rgb_out[(size_t)r * 3 + 1] = clamp01(c1);
    rgb_out[(size_t)r * 3 + 2] = clamp01(c2);
}

// additional_output: scatter per-entry rgb back to the dense [n,S,3] array
__global__ __launch_bounds__(256) void scatter_rgb_kernel(const MarchOut mo, const int S, float *__restrict__ rgb_dense)
{
    const unsigned n = *mo.counter;
    for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const float4 v = mo.q_out[e];
        const size_t q = ((size_t)mo.q_ray[e] * S + mo.q_j[e]) * 3;
        rgb_dense[q] = v.x; rgb_dense[q + 1] = v.y; rgb_dense[q + 2] = v.z;
    }
}

// ---- generic feature lookups (compute_densityfeature / sample_alpha API): arbitrary coordinates, zeros padding ----
__global__ __launch_bounds__(256) void density_feature_kernel(const SceneDev sc, const float *__restrict__ xyz, const long long m,
                                                              float *__restrict__ out)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long s = t >> 2;
    const int sub = threadIdx.x & 3;
    float part = 0.0f;
    if (s < m) {
        int i0[3];
        float w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float f = unnorm(xyz[s * 3 + k], sc.gm1[k]);
            const float fl = floorf(fminf(fmaxf(f, -2.0f), sc.gm1[k] + 2.0f));
            i0[k] = (int)fl;
            w[k] = f - fl;
        }
        const float4 a = vm_term<4, true>(sc.dplane[0], sc.dline[0], sc.grid[0], sc.grid[1], sc.grid[2], i0[0], i0[1], i0[2], w[0], w[1], w[2], sub);
        const float4 b = vm_term<4, true>(sc.dplane[1], sc.dline[1], sc.grid[0], sc.grid[2], sc.grid[1], i0[0], i0[2], i0[1], w[0], w[2], w[1], sub);
        const float4 c = vm_term<4, true>(sc.dplane[2], sc.dline[2], sc.grid[1], sc.grid[2], sc.grid[0], i0[1], i0[2], i0[0], w[1], w[2], w[0], sub);
        part = ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w)) + ((c.x + c.y) + (c.z + c.w));
    }
    part += __shfl_xor(part, 1);
    part += __shfl_xor(part, 2);
    if (s < m && sub == 0) out[s] = part;
}

// ---- symmetric-difference gradient of the density feature (tvr_density_gradient) -------------------------------------------------------------------------------
//   grad[k] = (f(p + h_k e_k) - f(p - h_k e_k)) * (0.5 / h_k),   f = density_feature_kernel's value (arbitrary coordinates, zeros padding)
// Same mapping as density_feature_kernel: a quad per point, lane `sub` holds 4 of the 16 channels, quad reduction at the end.  The per-point arithmetic is
// vm_grad_point's (tvr_gradient.h), which the normal pass (tvr_normals.hip) evaluates too.
__global__ __launch_bounds__(256) void density_gradient_kernel(const SceneDev sc, const float *__restrict__ xyz, const long long m, const float3 h, const float3 inv2h,
                                                               float *__restrict__ sigma_feature, float *__restrict__ grad)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long s = t >> 2;
    const int sub = threadIdx.x & 3;
    // f[0] centre, f[1 + 2 k], f[2 + 2 k]: axis k shifted by +h_k, -h_k
    float f[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) f[j] = 0.0f;
    if (s < m) vm_grad_point(sc, xyz[s * 3], xyz[s * 3 + 1], xyz[s * 3 + 2], h, sub, f);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        f[j] += __shfl_xor(f[j], 1);
        f[j] += __shfl_xor(f[j], 2);
    }
    if (s < m && sub == 0) {
        if (sigma_feature) sigma_feature[s] = f[0];
        grad[s * 3 + 0] = (f[1] - f[2]) * inv2h.x;
        grad[s * 3 + 1] = (f[3] - f[4]) * inv2h.y;
        grad[s * 3 + 2] = (f[5] - f[6]) * inv2h.z;
    }
}

__global__ __launch_bounds__(256) void alpha_sample_kernel(const SceneDev sc, const float *__restrict__ xyz, const long long m,
                                                           float *__restrict__ out)
{
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= m) return;
    const float p[3] = {xyz[s * 3], xyz[s * 3 + 1], xyz[s * 3 + 2]};
    out[s] = alpha_lookup(sc, p);
}

// alpha volume -> bit volume (one thread per 32-voxel word)
__global__ __launch_bounds__(256) void alpha_bits_kernel(const float *__restrict__ vol, const long long n, unsigned *__restrict__ bits)
{
    const long long wd = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (wd * 32 >= n) return;
    unsigned v = 0u;
    for (int b = 0; b < 32; ++b) {
        const long long i = wd * 32 + b;
        if (i < n && vol[i] > 0.0f) v |= 1u << b;
    }
    bits[wd] = v;
}

hipError_t launch_alpha_bits(const float *vol, long long n, unsigned *bits, hipStream_t stream)
{
    const long long words = (n + 31) / 32;
    hipLaunchKernelGGL(alpha_bits_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, vol, n, bits);
    return hipGetLastError();
}

// ---- host launchers ----
template <bool DENSE, bool LDSL>
static hipError_t launch_march_t(const SceneDev &sc, const float *rays, int n_rays, int S, const MarchSampling &sm, float eps_T, const MarchOut &mo,
                                 const tvr_dense_out &dn, int waves, size_t lds, unsigned grid, hipStream_t stream)
{
    hipError_t rc = hipFuncSetAttribute((const void *)march_kernel<DENSE, LDSL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL((march_kernel<DENSE, LDSL>), dim3(grid), dim3(64 * waves), lds, stream, sc, rays, n_rays, S, S, sm, eps_T, mo, dn);
    return hipGetLastError();
}

static int device_cu_count()
{
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cus = n;
        else cus = 256;
    }
    return cus;
}

int march_cu_count() { return device_cu_count(); }

// the volume march: groups of MARCH_VOL_WAVES waves, MARCH_VOL_GROUPS of them per CU (tvr_march_body.h says why), fewer waves per group (and proportionally more
// groups) only where the appearance lists (6 B per sample and wave) do not leave room
static hipError_t launch_march_vol(const SceneDev &sc, const float *dvol, const float *rays, int n_rays, int S, const MarchSampling &sm, float eps_T, const MarchOut &mo,
                                   const tvr_dense_out *dense, hipStream_t stream)
{
    const int groups = MARCH_VOL_GROUPS;                     // per CU
    const size_t kLds = 160 * 1024 / (size_t)groups, per_list = (size_t)S * 6, fixed = MARCH_HDR + 64;
    const int n_tiles = (n_rays + MARCH_TILE - 1) / MARCH_TILE;
    int waves = 1;
    size_t lds = 0;
    long long grid = 1;
    // per wave: the list (6 B per sample) and, in a launch that batches, `per_pend` bytes behind the lists (16-byte aligned) for the records of the waiting rays
    auto shape = [&](size_t per_pend) {
        const int w = (int)((kLds - fixed - (per_pend ? 16 : 0)) / (per_list + per_pend));
        waves = w >= MARCH_VOL_WAVES ? MARCH_VOL_WAVES : (w >= 8 ? 8 : (w >= 4 ? 4 : (w >= 2 ? 2 : 1)));
        lds = per_pend ? fixed + (((size_t)waves * per_list + 15) & ~(size_t)15) + (size_t)waves * per_pend : fixed + (size_t)waves * per_list;
        grid = (long long)device_cu_count() * groups * (MARCH_VOL_WAVES / waves);
        if (grid > n_tiles) grid = n_tiles;
        if (grid < 1) grid = 1;
    };
    shape(0);                                                              // the unbatched launch: the parent's shape and LDS
    // more rays than waves: a wave marches several and reserves once for a batch of them (MARCH_BATCH, tvr_march_body.h); the records may then cost a step in waves per group
    // (512 samples: 16 waves either way; the step from 16 to 8 waves moves from 1702 to 1637 samples), with as many more groups
    const bool batch = (long long)n_rays > grid * (long long)waves;
    if (batch) shape((size_t)MARCH_PEND * MARCH_PEND_WORDS * 4);
    tvr_dense_out none = {};
    const tvr_dense_out &dn = dense ? *dense : none;
    const unsigned long long vol_bytes = 4ull * (unsigned long long)(sc.grid[0] + 1) * (unsigned long long)(sc.grid[1] + 1) * (unsigned long long)(sc.grid[2] + 1);
    const bool plain = !dense && sc.avol == nullptr && sm.zv == nullptr && mo.lam6 == nullptr && vol_bytes < (1ull << 32);
    hipError_t rc = hipSuccess;
    auto go = [&](auto kern) {
        rc = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (rc == hipSuccess) hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * waves), lds, stream, sc, dvol, rays, n_rays, S, S, sm, eps_T, mo, dn);
    };
    if (dense) batch ? go(march_vol_kernel<true, false, true>) : go(march_vol_kernel<true, false, false>);
    else if (plain) batch ? go(march_vol_kernel<false, true, true>) : go(march_vol_kernel<false, true, false>);
    else batch ? go(march_vol_kernel<false, false, true>) : go(march_vol_kernel<false, false, false>);
    if (rc != hipSuccess) return rc;
    return hipGetLastError();
}

hipError_t launch_march(const SceneDev &sc, const float *rays, int n_rays, int S, const MarchSampling &sm, float eps_T,
                        const MarchOut &mo, const tvr_dense_out *dense, hipStream_t stream, const float *dvol)
{
    if (dvol) return launch_march_vol(sc, dvol, rays, n_rays, S, sm, eps_T, mo, dense, stream);
    // LDS budget: the density lines (if they fit next to at least 4 waves' lists) + 6 B per sample and wave for the appearance lists
    const size_t kLds = 160 * 1024, line_bytes = ((size_t)sc.grid[0] + sc.grid[1] + sc.grid[2] + 3) * 16 * MARCH_LSTRIDE, per_wave = (size_t)S * 6;
    bool ldsl = MARCH_HDR + line_bytes + 4 * per_wave + 64 <= kLds;
    const size_t fixed = MARCH_HDR + (ldsl ? line_bytes : 0) + 64;
    int waves = (int)((kLds - fixed) / per_wave);
    waves = waves >= 16 ? 16 : (waves >= 12 ? 12 : (waves >= 8 ? 8 : (waves >= 4 ? 4 : (waves >= 2 ? 2 : 1))));
    const size_t lds = fixed + (size_t)waves * per_wave;
    const int n_tiles = (n_rays + MARCH_TILE - 1) / MARCH_TILE;
    // one group per CU when it holds 16 waves; proportionally more groups when the lists force smaller ones
    long long grid = (long long)device_cu_count() * (16 / waves > 0 ? 16 / waves : 1);
    if (grid > n_tiles) grid = n_tiles;
    if (grid < 1) grid = 1;
    tvr_dense_out none = {};
    const tvr_dense_out &dn = dense ? *dense : none;
    if (dense) return ldsl ? launch_march_t<true, true>(sc, rays, n_rays, S, sm, eps_T, mo, dn, waves, lds, (unsigned)grid, stream)
                           : launch_march_t<true, false>(sc, rays, n_rays, S, sm, eps_T, mo, dn, waves, lds, (unsigned)grid, stream);
    return ldsl ? launch_march_t<false, true>(sc, rays, n_rays, S, sm, eps_T, mo, dn, waves, lds, (unsigned)grid, stream)
                : launch_march_t<false, false>(sc, rays, n_rays, S, sm, eps_T, mo, dn, waves, lds, (unsigned)grid, stream);
}

hipError_t launch_composite(const MarchOut &mo, int n_rays, int white_bg, float *rgb, hipStream_t stream)
{
    const long long threads = (long long)n_rays * COMP_LANES;
    hipLaunchKernelGGL(composite_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, mo, n_rays, white_bg, rgb);
    return hipGetLastError();
}

hipError_t launch_scatter_rgb(const MarchOut &mo, int S, float *rgb_dense, hipStream_t stream)
{
    hipLaunchKernelGGL(scatter_rgb_kernel, dim3(1024), dim3(256), 0, stream, mo, S, rgb_dense);
    return hipGetLastError();
}

hipError_t launch_density_feature(const SceneDev &sc, const float *xyz, long long m, float *out, hipStream_t stream)
{
    const long long blocks = (m * 4 + 255) / 256;
    hipLaunchKernelGGL(density_feature_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, sc, xyz, m, out);
    return hipGetLastError();
}

hipError_t launch_density_gradient(const SceneDev &sc, const float *xyz, long long m, const float h[3], const float inv2h[3], float *sigma_feature, float *grad,
                                   hipStream_t stream)
{
    const long long blocks = (m * 4 + 255) / 256;
    hipLaunchKernelGGL(density_gradient_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, sc, xyz, m, make_float3(h[0], h[1], h[2]),
                       make_float3(inv2h[0], inv2h[1], inv2h[2]), sigma_feature, grad);
    return hipGetLastError();
}

hipError_t launch_alpha_sample(const SceneDev &sc, const float *xyz, long long m, float *out, hipStream_t stream)
{
    hipLaunchKernelGGL(alpha_sample_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, sc, xyz, m, out);
    return hipGetLastError();
}
