// tvr_cp_train.hip — the backward kernels of a CP-decomposed field (TensorCP, reference models/tensoRF.py:317-447; the forward half is tvr_cp.hip).
//
//   cp_march_backward_kernel : d loss / d density_line[0..2], given d loss / d w_e (per appearance sample, queue order) and d loss / d acc (per ray)
//   cp_app_backward_kernel   : d loss / d app_line[0..2] and d loss / d basis_mat, given entries xyz [m,3] and d loss / d features [m,27]
//
// Conventions are the forward's: vecMode = [2, 1, 0] (line i runs along axis 2 - i), packed lines [L+1][C] fp32 channels-last with a zero texel at index L and zero
// channels behind the scene's own (C = cp.rd / cp.ra); the gradient images have the packed lines' geometry, basis_mat's is [27][ra].
//
// Both kernels turn tvr_train.hip's RayLine by 90 degrees: a LANE is a COMPONENT, the wave (workgroup) walks samples (entries) whose cell and weights are the same in
// every lane, and each lane keeps the two taps of each line in registers while the cell stays.  A tap that leaves the window goes out with ONE atomicAdd per lane:
// 64 consecutive floats per wave-instruction.  Results are therefore reproducible to rounding, not bit for bit (include/tvr.h, CP TRAINING).
#include "tvr_device.h"
#include "tvr_kernels.h"
#include "tvr_march_body.h"
#include "tvr_gradient.h"

#define CPB_WAVES 16                     // cp_march_backward: one ray per wave, 16 rays per workgroup (march_backward_kernel's shape)
#define CPB_THREADS (64 * CPB_WAVES)
#define CPA_THREADS 320                  // cp_app_backward: thread = component, 288 of them in five waves
#define CPA_ENTRIES 256                  // consecutive entries per workgroup

__device__ __forceinline__ float cp_rdlane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// The two taps (k, k + 1) of one line for one component of this lane; k is the same in every lane of the wave (workgroup).  g: the packed gradient line, C floats per
// texel, c this lane's channel.  A tap whose sum is zero is never written (an empty window, a pad channel).
struct CpLineWin {
    int k;
    float b0, b1;
    __device__ __forceinline__ void reset() { k = 0; b0 = b1 = 0.0f; }
    __device__ __forceinline__ void flush(float *__restrict__ g, int C, int c)
    {
        if (b0 != 0.0f) atomicAdd(g + (size_t)k * C + c, b0);
        if (b1 != 0.0f) atomicAdd(g + (size_t)(k + 1) * C + c, b1);
        b0 = b1 = 0.0f;
    }
    __device__ __forceinline__ void move(float *__restrict__ g, int C, int c, int k_new)
    {
        const int dk = k_new - k;
        if (dk == 0) return;
        if (dk == 1) { if (b0 != 0.0f) atomicAdd(g + (size_t)k * C + c, b0); b0 = b1; b1 = 0.0f; }
        else if (dk == -1) { if (b1 != 0.0f) atomicAdd(g + (size_t)(k + 1) * C + c, b1); b1 = b0; b0 = 0.0f; }
        else flush(g, C, c);
        k = k_new;
    }
};

// ---- a. the march's backward -----------------------------------------------------------------------------------------------------------------------------------
// march_backward_kernel (tvr_train.hip) with the CP field in place of the VM field: the per-ray part — total, running T, the two 64-lane scans, dL/dalpha, the exits —
// is that kernel's text; phase 1 recomputes sigma_feature through cp_density_quad, so the weights it derives are the forward march's bits.  No explicit depths, no lam6,
// no fused-step capacity: those belong to NerfPlusPlus and the fused step, which are VM-only.
// Phase 2, per sample s with dL/dsf = gs and per component r, with a, b, c the three interpolated line values:
//   dL0[r][iz + t] += gs wz_t b_r c_r,   dL1[r][iy + t] += gs wy_t a_r c_r,   dL2[r][ix + t] += gs wx_t a_r b_r.
// Lane l owns components l and l + 64 (rd <= 96).  In-box samples have 0 <= i <= L - 1, so the taps i, i + 1 lie inside the packed [L+1] line — the forward's own reads.
__global__ __launch_bounds__(CPB_THREADS) void cp_march_backward_kernel(const SceneDev sc, const CpDev cp, const float *__restrict__ rays, const int n_rays, const int S,
                                                                        const float *__restrict__ jitter, const float eps_T, const MarchOut mo,
                                                                        const float *__restrict__ grad_w, const float *__restrict__ grad_acc, float *__restrict__ g0,
                                                                        float *__restrict__ g1, float *__restrict__ g2)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sub = lane & 3;
    const int rd = cp.rd;
    const int ray = blockIdx.x * CPB_WAVES + wave;
    if (ray >= n_rays) return;
    const float *__restrict__ L0 = (const float *)sc.dline[0], *__restrict__ L1 = (const float *)sc.dline[1], *__restrict__ L2 = (const float *)sc.dline[2];
    const bool on0 = lane < rd, on1 = lane + 64 < rd;
    float o[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[k] = rays[(size_t)ray * 6 + k];
        d[k] = rays[(size_t)ray * 6 + 3 + k];
    }
    const float tmin = ray_tmin(sc, o, d);
    const bool has_jit = jitter != nullptr;
    const float u = has_jit ? jitter[ray] : 0.0f;
    const unsigned base = mo.ray_off[ray], cnt = mo.ray_cnt[ray];
    const float gacc = grad_acc[ray];
    // total = sum_k dL/dw_k w_k over the whole (possibly early-terminated) ray
    float tot_l = 0.0f;
    for (unsigned i = lane; i < cnt; i += 64) tot_l += grad_w[base + i] * mo.q_pos[base + i].w;
    const float total = wave_sum(tot_l) + gacc * mo.acc[ray];

    float T = 1.0f, prefix = 0.0f;
    unsigned napp = 0;
    bool seen = false;
    CpLineWin wz0, wz1, wy0, wy1, wx0, wx1;                      // line 0 (z), 1 (y), 2 (x); components lane, lane + 64: they live for the whole ray
    wz0.reset(); wz1.reset(); wy0.reset(); wy1.reset(); wx0.reset(); wx1.reset();
    for (int c = 0; c * 64 < S; ++c) {
        const int j = c * 64 + lane;
        const bool inr = j < S;
        float fj = (float)j, fj1 = (float)(j + 1);
        if (has_jit) { fj = fj + u; fj1 = fj1 + u; }
        const float z = tmin + sc.step * fj;
        const float z1 = tmin + sc.step * fj1;
        float p[3], n[3], f[3];
        bool bbox = inr;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = o[k] + d[k] * z;
            bbox = bbox & !((sc.lo[k] > p[k]) | (p[k] > sc.hi[k]));
        }
        bool valid = bbox;
        if (sc.avol != nullptr) {
            if (bbox) valid = sc.abits ? alpha_positive(sc, p) : (alpha_lookup(sc, p) > 0.0f);
        }
        int i0[3];
        float w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            n[k] = (p[k] - sc.lo[k]) * sc.inv[k] - 1.0f;
            f[k] = unnorm(n[k], sc.gm1[k]);
            const float fl = floorf(f[k]);
            i0[k] = (int)fl;
            w[k] = f[k] - fl;
        }
        const unsigned long long mb = __ballot(bbox), mv = __ballot(valid);
        if (mv == 0ull) {
            if (mb == 0ull && seen) break;
            continue;
        }
        seen = true;
        // ---- phase 1: forward recomputation of sigma_feature (identical arithmetic to cp_march_kernel) ----
        float sf = 0.0f;
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4) {
            const bool v = quad_bcast_i((int)valid, k4) != 0;
            if (__ballot(v) == 0ull) continue;
            const int ix = quad_bcast_i(i0[0], k4), iy = quad_bcast_i(i0[1], k4), iz = quad_bcast_i(i0[2], k4);
            const float wx = quad_bcast_f(w[0], k4), wy = quad_bcast_f(w[1], k4), wz = quad_bcast_f(w[2], k4);
            float part = 0.0f;
            if (v) part = cp_density_quad(sc, cp, ix, iy, iz, wx, wy, wz, sub);
            part += quad_perm_f<QUAD_XOR1>(part);
            part += quad_perm_f<QUAD_XOR2>(part);
            if (sub == k4) sf = part;
        }
        float sigma = 0.0f, dsig_dsf = 0.0f;
        if (valid) {
            if (sc.act == 0) {
                const float x = sf + sc.shift;
                sigma = softplus_f(x);
                dsig_dsf = x > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-x));
            } else {
                sigma = fmaxf(sf, 0.0f);
                dsig_dsf = sf > 0.0f ? 1.0f : 0.0f;
            }
        }
        float dist = (j < S - 1) ? (z1 - z) : 0.0f;
        dist = dist * sc.scale;
        const float alpha = 1.0f - expf(-sigma * dist);
        const float fT = (1.0f - alpha) + 1e-10f;
        float incl = fT;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float t = __shfl_up(incl, off);
            if (lane >= off) incl = incl * t;
        }
        float excl = __shfl_up(incl, 1);
        if (lane == 0) excl = 1.0f;
        const float Tj = T * excl;
        const float wgt = alpha * Tj;
        const bool app = wgt > sc.thres;
        const unsigned long long ma = __ballot(app);
        float dLdw = gacc;
        if (app) dLdw += grad_w[base + napp + __popcll(ma & ((1ull << lane) - 1ull))];
        napp += __popcll(ma);
        // inclusive prefix of dL/dw_k w_k
        float pin = dLdw * wgt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float t = __shfl_up(pin, off);
            if (lane >= off) pin += t;
        }
        const float suffix = total - (prefix + pin);
        prefix += __shfl(pin, 63);
        const float dLda = Tj * dLdw - suffix / fT;
        const float dLdsf = valid ? dLda * dist * (1.0f - alpha) * dsig_dsf : 0.0f;
        T = T * __shfl(incl, 63);

        // ---- phase 2: one sample at a time, lane = component; cell and weights are wave-uniform (readlane), the lines are L1 / L2 hot ----
        unsigned long long todo = __ballot(dLdsf != 0.0f);
        while (todo) {
            const int src = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(todo));
            todo &= todo - 1ull;
            const float gs = cp_rdlane_f(dLdsf, src);
            const int ix = __builtin_amdgcn_readlane(i0[0], src), iy = __builtin_amdgcn_readlane(i0[1], src), iz = __builtin_amdgcn_readlane(i0[2], src);
            const float wx = cp_rdlane_f(w[0], src), wy = cp_rdlane_f(w[1], src), wz = cp_rdlane_f(w[2], src);
            const float ux = 1.0f - wx, uy = 1.0f - wy, uz = 1.0f - wz;
            wz0.move(g0, rd, lane, iz); wz1.move(g0, rd, lane + 64, iz);
            wy0.move(g1, rd, lane, iy); wy1.move(g1, rd, lane + 64, iy);
            wx0.move(g2, rd, lane, ix); wx1.move(g2, rd, lane + 64, ix);
            if (on0) {
                const size_t qz = (size_t)iz * rd + lane, qy = (size_t)iy * rd + lane, qx = (size_t)ix * rd + lane;
                const float a = __builtin_fmaf(wz, L0[qz + rd], uz * L0[qz]), b = __builtin_fmaf(wy, L1[qy + rd], uy * L1[qy]), cc = __builtin_fmaf(wx, L2[qx + rd], ux * L2[qx]);
                const float ga = gs * (b * cc), gb = gs * (a * cc), gc = gs * (a * b);
                wz0.b0 += uz * ga; wz0.b1 += wz * ga;
                wy0.b0 += uy * gb; wy0.b1 += wy * gb;
                wx0.b0 += ux * gc; wx0.b1 += wx * gc;
            }
            if (on1) {
                const size_t qz = (size_t)iz * rd + lane + 64, qy = (size_t)iy * rd + lane + 64, qx = (size_t)ix * rd + lane + 64;
                const float a = __builtin_fmaf(wz, L0[qz + rd], uz * L0[qz]), b = __builtin_fmaf(wy, L1[qy + rd], uy * L1[qy]), cc = __builtin_fmaf(wx, L2[qx + rd], ux * L2[qx]);
                const float ga = gs * (b * cc), gb = gs * (a * cc), gc = gs * (a * b);
                wz1.b0 += uz * ga; wz1.b1 += wz * ga;
                wy1.b0 += uy * gb; wy1.b1 += wy * gb;
                wx1.b0 += ux * gc; wx1.b1 += wx * gc;
            }
        }
        if (T < eps_T) break;
    }
    // (lanes that own no component hold zeros, which flush() never writes)
    wz0.flush(g0, rd, lane); wz1.flush(g0, rd, lane + 64);
    wy0.flush(g1, rd, lane); wy1.flush(g1, rd, lane + 64);
    wx0.flush(g2, rd, lane); wx1.flush(g2, rd, lane + 64);
}

hipError_t launch_cp_march_backward(const SceneDev &sc, const CpDev &cp, const float *rays, int n_rays, int S, const float *jitter, float eps_T, const MarchOut &mo,
                                    const float *grad_w, const float *grad_acc, float *const gline[3], hipStream_t stream)
{
    const unsigned grid = (unsigned)((n_rays + CPB_WAVES - 1) / CPB_WAVES);
    hipLaunchKernelGGL(cp_march_backward_kernel, dim3(grid), dim3(CPB_THREADS), 0, stream, sc, cp, rays, n_rays, S, jitter, eps_T, mo, grad_w, grad_acc, gline[0],
                       gline[1], gline[2]);
    return hipGetLastError();
}

// ---- b. the features' backward ---------------------------------------------------------------------------------------------------------------------------------
// features[e][c] = sum_r B[c][r] h_e[r],  h_e[r] = a_r b_r c_r (the three interpolated appearance lines at entry e).  With dF = d loss / d features:
//   dh[r] = sum_c dF[c] B[c][r],   dB[c][r] += dF[c] h[r],   and the three line gradients as in (a) with dh[r] in place of gs.
// A workgroup takes CPA_ENTRIES consecutive entries (the queue entries of a ray are contiguous and in sample order, so the windows slide as they do along a ray);
// thread = component; each thread holds its column of B and of dB in registers; xyz and dF of the entry are the same address in every thread.  Taps and weights are
// cp_tap's (zeros padding, indices clamped into the line): the window's key is the clamped lower tap i0 in [0, L - 1], and the upper tap is i0 + 1 (<= L, inside the
// packed gradient line) or — below the line's start, where both clamp to 0 — i0 itself.  At the end of the run the windows and the dB column go out as atomics.
__global__ __launch_bounds__(CPA_THREADS) void cp_app_backward_kernel(const SceneDev sc, const CpDev cp, const float *__restrict__ xyz, const long long m,
                                                                      const float *__restrict__ dF, float *__restrict__ g0, float *__restrict__ g1,
                                                                      float *__restrict__ g2, float *__restrict__ gB)
{
    const int r = threadIdx.x, ra = cp.ra;
    if (r >= ra) return;                                         // (no barrier in this kernel)
    const long long e0 = (long long)blockIdx.x * CPA_ENTRIES;
    const long long e1 = e0 + CPA_ENTRIES < m ? e0 + CPA_ENTRIES : m;
    const float *__restrict__ A0 = (const float *)sc.aline[0], *__restrict__ A1 = (const float *)sc.aline[1], *__restrict__ A2 = (const float *)sc.aline[2];
    float B[TVR_APPDIM], dB[TVR_APPDIM];
    {
        const float *bas = (const float *)cp.basis;              // [ra / 4][27] float4: entry (g, c) holds columns 4 g .. 4 g + 3 of row c
#pragma unroll
        for (int c = 0; c < TVR_APPDIM; ++c) {
            B[c] = bas[((size_t)(r >> 2) * TVR_APPDIM + c) * 4 + (r & 3)];
            dB[c] = 0.0f;
        }
    }
    CpLineWin w0, w1, w2;
    w0.reset(); w1.reset(); w2.reset();
    for (long long e = e0; e < e1; ++e) {
        const CpTap tx = cp_tap(xyz[e * 3], sc.gm1[0], sc.grid[0]), ty = cp_tap(xyz[e * 3 + 1], sc.gm1[1], sc.grid[1]), tz = cp_tap(xyz[e * 3 + 2], sc.gm1[2], sc.grid[2]);
        const float a = __builtin_fmaf(tz.w, A0[(size_t)tz.i1 * ra + r], tz.u * A0[(size_t)tz.i0 * ra + r]);
        const float b = __builtin_fmaf(ty.w, A1[(size_t)ty.i1 * ra + r], ty.u * A1[(size_t)ty.i0 * ra + r]);
        const float cc = __builtin_fmaf(tx.w, A2[(size_t)tx.i1 * ra + r], tx.u * A2[(size_t)tx.i0 * ra + r]);
        const float h = (a * b) * cc;
        const float *__restrict__ df = dF + e * TVR_APPDIM;
        float dh = 0.0f;
#pragma unroll
        for (int c = 0; c < TVR_APPDIM; ++c) {
            const float v = df[c];
            dh = __builtin_fmaf(v, B[c], dh);
            dB[c] = __builtin_fmaf(v, h, dB[c]);
        }
        const float ga = dh * (b * cc), gb = dh * (a * cc), gc = dh * (a * b);
        w0.move(g0, ra, r, tz.i0);
        w1.move(g1, ra, r, ty.i0);
        w2.move(g2, ra, r, tx.i0);
        if (tz.i1 == tz.i0) w0.b0 += (tz.u + tz.w) * ga; else { w0.b0 += tz.u * ga; w0.b1 += tz.w * ga; }     // (one of u, w is zero where the taps coincide)
        if (ty.i1 == ty.i0) w1.b0 += (ty.u + ty.w) * gb; else { w1.b0 += ty.u * gb; w1.b1 += ty.w * gb; }
        if (tx.i1 == tx.i0) w2.b0 += (tx.u + tx.w) * gc; else { w2.b0 += tx.u * gc; w2.b1 += tx.w * gc; }
    }
    w0.flush(g0, ra, r);
    w1.flush(g1, ra, r);
    w2.flush(g2, ra, r);
#pragma unroll
    for (int c = 0; c < TVR_APPDIM; ++c)
        if (dB[c] != 0.0f) atomicAdd(gB + (size_t)c * ra + r, dB[c]);
}

hipError_t launch_cp_app_backward(const SceneDev &sc, const CpDev &cp, const float *xyz, long long m, const float *dF, float *const gline[3], float *gbasis,
                                  hipStream_t stream)
{
    const unsigned grid = (unsigned)((m + CPA_ENTRIES - 1) / CPA_ENTRIES);
    hipLaunchKernelGGL(cp_app_backward_kernel, dim3(grid), dim3(CPA_THREADS), 0, stream, sc, cp, xyz, m, dF, gline[0], gline[1], gline[2], gbasis);
    return hipGetLastError();
}
