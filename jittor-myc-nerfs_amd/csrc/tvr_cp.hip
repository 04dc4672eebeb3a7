// tvr_cp.hip — the kernels of a CP-decomposed field (TensorCP, reference models/tensoRF.py:317-447): three lines per factor and no planes.
//
//   sigma_feature(p) = sum_r L0[r](p_z) L1[r](p_y) L2[r](p_x)                      (tensoRF.py:345-360; vecMode = [2, 1, 0])
//   features(p)      = basis_mat . h,  h[r] = A0[r](p_z) A1[r](p_y) A2[r](p_x)     (tensoRF.py:362-376)
// with every line interpolated linearly (grid_sample, align_corners=True, zeros padding).  Everything else is TensorBase's and runs in the kernels the
// other models use: the march body (tvr_march_body.inc) with the CP density evaluation, shade_kernel<SH_SRC_FEAT, SH_DST_RGB> on staged features, composite_kernel.
//
// Packed lines: [L+1][C] fp32, channels-last, a zero texel at index L (the +1 tap of the last cell) and zero channels behind the scene's own (exact).
// Up to 96 density / 288 appearance components at 300^3 are 0.35 MB + 1.04 MB: they live in L2, no LDS copy (3 x 301 x 384 B does not fit next to the lists).
#include "tvr_device.h"
#include "tvr_kernels.h"
#include "tvr_march_body.h"
#include "tvr_gradient.h"

// ---- a. the march: the shared body with CP = true -------------------------------------------------------------------------------------------------------------
template <bool DENSE>
__global__ __launch_bounds__(64 * MARCH_MAX_WAVES) void cp_march_kernel(const SceneDev sc, const CpDev cp, const float *__restrict__ rays, const int n_rays, const int S,
                                                                        const int s_cap, const MarchSampling sm, const float eps_T, MarchOut mo, const tvr_dense_out dn)
{
    constexpr bool LDSL = false, CP = true, VOL = false;
    const float *const dvol = nullptr;
#include "tvr_march_body.inc"
}

template <bool DENSE>
static hipError_t launch_cp_march_t(const SceneDev &sc, const CpDev &cp, const float *rays, int n_rays, int S, const MarchSampling &sm, float eps_T, const MarchOut &mo,
                                    const tvr_dense_out &dn, int waves, size_t lds, unsigned grid, hipStream_t stream)
{
    hipError_t rc = hipFuncSetAttribute((const void *)cp_march_kernel<DENSE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL((cp_march_kernel<DENSE>), dim3(grid), dim3(64 * waves), lds, stream, sc, cp, rays, n_rays, S, S, sm, eps_T, mo, dn);
    return hipGetLastError();
}

hipError_t launch_cp_march(const SceneDev &sc, const CpDev &cp, const float *rays, int n_rays, int S, const MarchSampling &sm, float eps_T, const MarchOut &mo,
                           const tvr_dense_out *dense, hipStream_t stream)
{
    // LDS: header + 6 B per sample and wave for the appearance lists (launch_march's budget without the line copy)
    const size_t kLds = 160 * 1024, per_wave = (size_t)S * 6, fixed = MARCH_HDR + 64;
    int waves = (int)((kLds - fixed) / per_wave);
    waves = waves >= 16 ? 16 : (waves >= 12 ? 12 : (waves >= 8 ? 8 : (waves >= 4 ? 4 : (waves >= 2 ? 2 : 1))));
    const size_t lds = fixed + (size_t)waves * per_wave;
    const int n_tiles = (n_rays + MARCH_TILE - 1) / MARCH_TILE;
    long long grid = (long long)march_cu_count() * (16 / waves > 0 ? 16 / waves : 1);
    if (grid > n_tiles) grid = n_tiles;
    if (grid < 1) grid = 1;
    tvr_dense_out none = {};
    if (dense) return launch_cp_march_t<true>(sc, cp, rays, n_rays, S, sm, eps_T, mo, *dense, waves, lds, (unsigned)grid, stream);
    return launch_cp_march_t<false>(sc, cp, rays, n_rays, S, sm, eps_T, mo, none, waves, lds, (unsigned)grid, stream);
}

// (cp_tap, the cell and weights of a normalised coordinate on an axis of L points, lives in tvr_gradient.h beside the gradient's per-point code)

// ---- b. compute_densityfeature at arbitrary points: one lane per point ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cp_density_feature_kernel(const SceneDev sc, const CpDev cp, const float *__restrict__ xyz, const long long m, float *__restrict__ out)
{
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= m) return;
    const CpTap tx = cp_tap(xyz[s * 3], sc.gm1[0], sc.grid[0]), ty = cp_tap(xyz[s * 3 + 1], sc.gm1[1], sc.grid[1]), tz = cp_tap(xyz[s * 3 + 2], sc.gm1[2], sc.grid[2]);
    const int tpt = cp.rd >> 2;
    const float4 *a0p = sc.dline[0] + (size_t)tz.i0 * tpt, *a1p = sc.dline[0] + (size_t)tz.i1 * tpt;
    const float4 *b0p = sc.dline[1] + (size_t)ty.i0 * tpt, *b1p = sc.dline[1] + (size_t)ty.i1 * tpt;
    const float4 *c0p = sc.dline[2] + (size_t)tx.i0 * tpt, *c1p = sc.dline[2] + (size_t)tx.i1 * tpt;
    float sum = 0.0f;
    for (int g = 0; g < tpt; ++g) {
        const float4 a = f4_fma(tz.w, a1p[g], f4_mul(tz.u, a0p[g])), b = f4_fma(ty.w, b1p[g], f4_mul(ty.u, b0p[g])), c = f4_fma(tx.w, c1p[g], f4_mul(tx.u, c0p[g]));
        const float t0 = (a.x * b.x) * c.x, t1 = (a.y * b.y) * c.y, t2 = (a.z * b.z) * c.z, t3 = (a.w * b.w) * c.w;
        sum = sum + ((t0 + t1) + (t2 + t3));
    }
    out[s] = sum;
}

hipError_t launch_cp_density_feature(const SceneDev &sc, const CpDev &cp, const float *xyz, long long m, float *out, hipStream_t stream)
{
    hipLaunchKernelGGL(cp_density_feature_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, sc, cp, xyz, m, out);
    return hipGetLastError();
}

// ---- b'. tvr_density_gradient on a CP scene: one lane per point -------------------------------------------------------------------------------------------
//   grad[k] = (f(p + h_k e_k) - f(p - h_k e_k)) * (0.5 / h_k),  f = cp_density_feature_kernel's value.  A shift along an axis moves one of the three line factors:
// each line is interpolated at {centre, +h, -h} (18 float4 taps per group of four components where seven calls of the kernel above read 42) and the seven
// products are formed and summed in that kernel's order, so the centre is bit-equal to it and the quotient is the one of its values at the shifted points.
__global__ __launch_bounds__(256) void cp_density_gradient_kernel(const SceneDev sc, const CpDev cp, const float *__restrict__ xyz, const long long m, const float3 h,
                                                                  const float3 inv2h, float *__restrict__ sigma_feature, float *__restrict__ grad)
{
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= m) return;
    float f[7];
    cp_grad_point(sc, cp, xyz[s * 3], xyz[s * 3 + 1], xyz[s * 3 + 2], h, f);
    if (sigma_feature) sigma_feature[s] = f[0];
    grad[s * 3 + 0] = (f[1] - f[2]) * inv2h.x;
    grad[s * 3 + 1] = (f[3] - f[4]) * inv2h.y;
    grad[s * 3 + 2] = (f[5] - f[6]) * inv2h.z;
}

hipError_t launch_cp_density_gradient(const SceneDev &sc, const CpDev &cp, const float *xyz, long long m, const float h[3], const float inv2h[3], float *sigma_feature,
                                      float *grad, hipStream_t stream)
{
    hipLaunchKernelGGL(cp_density_gradient_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, sc, cp, xyz, m, make_float3(h[0], h[1], h[2]),
                       make_float3(inv2h[0], inv2h[1], inv2h[2]), sigma_feature, grad);
    return hipGetLastError();
}

// ---- c. appearance features: entries in, features [., 27] out ---------------------------------------------------------------------------------------------
// One lane per entry.  Per group of four components: 6 float4 taps (3 lines x 2), 12 interpolation ops, 8 products, then 27 x 4 fp32 FMAs against the basis group,
// whose address is the same in every lane (scalar loads).  fp32 throughout: nothing passes through fp16 here; the range rule of tvr.h applies where the features
// enter the network (shade_kernel<SH_SRC_FEAT, ...> checks them).
#define CP_APP_THREADS 256
__global__ __launch_bounds__(CP_APP_THREADS) void cp_app_feature_kernel(const SceneDev sc, const CpDev cp, const float *__restrict__ xyz, const int xyz_stride, const long long m,
                                                                        const unsigned *__restrict__ m_dev, const unsigned *__restrict__ q_ray,
                                                                        const float *__restrict__ rays, float *__restrict__ feats, float *__restrict__ dirs)
{
    long long n = m;
    if (m_dev) n = (long long)(*m_dev) < m ? (long long)(*m_dev) : m;
    const int tpt = cp.ra >> 2;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const float *p = xyz + e * xyz_stride;
        const CpTap tx = cp_tap(p[0], sc.gm1[0], sc.grid[0]), ty = cp_tap(p[1], sc.gm1[1], sc.grid[1]), tz = cp_tap(p[2], sc.gm1[2], sc.grid[2]);
        const float4 *a0p = sc.aline[0] + (size_t)tz.i0 * tpt, *a1p = sc.aline[0] + (size_t)tz.i1 * tpt;
        const float4 *b0p = sc.aline[1] + (size_t)ty.i0 * tpt, *b1p = sc.aline[1] + (size_t)ty.i1 * tpt;
        const float4 *c0p = sc.aline[2] + (size_t)tx.i0 * tpt, *c1p = sc.aline[2] + (size_t)tx.i1 * tpt;
        float F[TVR_APPDIM];
#pragma unroll
        for (int c = 0; c < TVR_APPDIM; ++c) F[c] = 0.0f;
        for (int g = 0; g < tpt; ++g) {
            const float4 a = f4_fma(tz.w, a1p[g], f4_mul(tz.u, a0p[g])), b = f4_fma(ty.w, b1p[g], f4_mul(ty.u, b0p[g])), cc = f4_fma(tx.w, c1p[g], f4_mul(tx.u, c0p[g]));
            const float h0 = (a.x * b.x) * cc.x, h1 = (a.y * b.y) * cc.y, h2 = (a.z * b.z) * cc.z, h3 = (a.w * b.w) * cc.w;
            const float4 *__restrict__ bg = cp.basis + (size_t)g * TVR_APPDIM;
#pragma unroll
            for (int c = 0; c < TVR_APPDIM; ++c) {
                const float4 w = bg[c];
                F[c] = __builtin_fmaf(h3, w.w, __builtin_fmaf(h2, w.z, __builtin_fmaf(h1, w.y, __builtin_fmaf(h0, w.x, F[c]))));
            }
        }
        float *o = feats + e * TVR_APPDIM;
#pragma unroll
        for (int c = 0; c < TVR_APPDIM; ++c) o[c] = F[c];
        if (dirs) {
            const float *d = rays + (size_t)q_ray[e] * 6 + 3;
            dirs[e * 3] = d[0]; dirs[e * 3 + 1] = d[1]; dirs[e * 3 + 2] = d[2];
        }
    }
}

hipError_t launch_cp_app_feature(const SceneDev &sc, const CpDev &cp, const float *xyz, int xyz_stride, long long m, const unsigned *m_dev, const unsigned *q_ray,
                                 const float *rays, float *feats, float *dirs, hipStream_t stream)
{
    long long blocks = (m + CP_APP_THREADS - 1) / CP_APP_THREADS;
    const long long most = (long long)march_cu_count() * 8;          // a device-side count: the grid is sized for the capacity and strides
    if (blocks > most) blocks = most;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(cp_app_feature_kernel, dim3((unsigned)blocks), dim3(CP_APP_THREADS), 0, stream, sc, cp, xyz, xyz_stride, m, m_dev, q_ray, rays, feats,
                       (q_ray && rays) ? dirs : nullptr);
    return hipGetLastError();
}

// ---- d. the network's colours [cap,3] + the queue's weights -> q_out {rgb, w}, what composite_kernel and scatter_rgb_kernel read ---------------------------
__global__ __launch_bounds__(256) void cp_rgbw_kernel(const MarchOut mo, const float *__restrict__ rgb, const long long cap)
{
    const long long n = (long long)(*mo.counter) < cap ? (long long)(*mo.counter) : cap;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x)
        mo.q_out[e] = make_float4(rgb[e * 3], rgb[e * 3 + 1], rgb[e * 3 + 2], mo.q_pos[e].w);
    if (mo.stats && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd((unsigned long long *)&mo.stats[TVR_STAT_APP], (unsigned long long)n);
}

hipError_t launch_cp_rgbw(const MarchOut &mo, const float *rgb, long long cap, hipStream_t stream)
{
    long long blocks = (cap + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(cp_rgbw_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, mo, rgb, cap);
    return hipGetLastError();
}

// basis_mat [27, r_app] (reference layout) -> [ra / 4][27] float4
__global__ __launch_bounds__(256) void cp_pack_basis_kernel(const float *__restrict__ basis, const int r_app, const int ra, float *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ra * TVR_APPDIM) return;
    const int j = i & 3, c = (i >> 2) % TVR_APPDIM, g = (i >> 2) / TVR_APPDIM, r = 4 * g + j;
    out[i] = r < r_app ? basis[(size_t)c * r_app + r] : 0.0f;
}

hipError_t launch_cp_pack_basis(const float *basis, int r_app, int ra, float4 *out, hipStream_t stream)
{
    hipLaunchKernelGGL(cp_pack_basis_kernel, dim3((unsigned)((ra * TVR_APPDIM + 255) / 256)), dim3(256), 0, stream, basis, r_app, ra, (float *)out);
    return hipGetLastError();
}
