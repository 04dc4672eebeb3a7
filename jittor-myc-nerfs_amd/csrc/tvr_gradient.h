// tvr_gradient.h — the per-point device code of the density feature's symmetric-difference gradient, shared by the kernels that evaluate it:
// density_gradient_kernel (tvr_march.hip), cp_density_gradient_kernel (tvr_cp.hip) and the normal pass (tvr_normals.hip).  One text, one operation order: whatever a
// kernel does with the seven values, they are the same bits.
//   grad[k] = (f(p + h_k e_k) - f(p - h_k e_k)) * (0.5 / h_k),   f = tvr_density_feature's value (arbitrary coordinates, zeros padding)
#pragma once
#include "tvr_device.h"
#include "tvr_kernels.h"

// ---- VM scenes: a quad per point, lane `sub` holds 4 of the 16 channels, quad reduction by the caller ---------------------------------------------------------
// A shift along axis k moves only the factor that depends on k, so a VM term (plane over axes A, B; line over C) needs its plane at 5 positions (centre, A+-, B+-) and
// its line at 3 (centre, C+-) instead of 7 + 7: 78 float4 loads per lane where seven density_feature_kernel calls issue 126.  Each of the seven values is formed by
// vm_term's own expressions in vm_term's order and summed in density_feature_kernel's order, so the centre is bit-equal to tvr_density_feature at p and the gradient is
// bit-equal to the same difference quotient of tvr_density_feature at the shifted points (shifted coordinate and quotient in separately rounded fp32).
struct AxisTap { int i0; float w; };
__device__ __forceinline__ AxisTap axis_tap(float c, float gm1)
{
    const float f = unnorm(c, gm1);
    const float fl = floorf(fminf(fmaxf(f, -2.0f), gm1 + 2.0f));
    AxisTap t;
    t.i0 = (int)fl;
    t.w = f - fl;
    return t;
}

// vm_term<4, true>'s bilinear plane factor and linear line factor, one quad-lane's 4 channels each
__device__ __forceinline__ float4 vm_plane4(const float4 *__restrict__ P, int W, int H, AxisTap tx, AxisTap ty, int sub)
{
    const int x0 = tx.i0, y0 = ty.i0;
    const float wx = tx.w, wy = ty.w, ux = 1.0f - wx, uy = 1.0f - wy;
    const int Wp = W + 1;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool xi0 = (x0 >= 0) & (x0 < W), xi1 = (x0 + 1 >= 0) & (x0 + 1 < W);
    const bool yi0 = (y0 >= 0) & (y0 < H), yi1 = (y0 + 1 >= 0) & (y0 + 1 < H);
    const int xc = min(max(x0, 0), W - 1), yc = min(max(y0, 0), H - 1);
    const int xd = min(max(x0 + 1, 0), W - 1), yd = min(max(y0 + 1, 0), H - 1);
    // the clamped addresses are always inside the plane: load unconditionally and select (a conditional load compiles to a branch per texel and component)
    const float4 r00 = P[((size_t)yc * Wp + xc) * 4 + sub], r01 = P[((size_t)yc * Wp + xd) * 4 + sub];
    const float4 r10 = P[((size_t)yd * Wp + xc) * 4 + sub], r11 = P[((size_t)yd * Wp + xd) * 4 + sub];
    const float4 t00 = (xi0 & yi0) ? r00 : z, t01 = (xi1 & yi0) ? r01 : z, t10 = (xi0 & yi1) ? r10 : z, t11 = (xi1 & yi1) ? r11 : z;
    float4 p4 = f4_mul(ux * uy, t00);
    p4 = f4_fma(wx * uy, t01, p4);
    p4 = f4_fma(ux * wy, t10, p4);
    p4 = f4_fma(wx * wy, t11, p4);
    return p4;
}

__device__ __forceinline__ float4 vm_line4(const float4 *__restrict__ Ln, int L, AxisTap tl, int sub)
{
    const int l0 = tl.i0;
    const float wl = tl.w, ul = 1.0f - wl;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool li0 = (l0 >= 0) & (l0 < L), li1 = (l0 + 1 >= 0) & (l0 + 1 < L);
    const int lc = min(max(l0, 0), L - 1), ld = min(max(l0 + 1, 0), L - 1);
    const float4 r0 = Ln[(size_t)lc * 4 + sub], r1 = Ln[(size_t)ld * 4 + sub];
    const float4 l0v = li0 ? r0 : z, l1v = li1 ? r1 : z;
    float4 q4 = f4_mul(ul, l0v);
    q4 = f4_fma(wl, l1v, q4);
    return q4;
}

// sum of the 4 channels of plane * line in density_feature_kernel's order
__device__ __forceinline__ float vm_dot4(float4 p4, float4 q4)
{
    const float4 a = make_float4(p4.x * q4.x, p4.y * q4.y, p4.z * q4.z, p4.w * q4.w);
    return (a.x + a.y) + (a.z + a.w);
}

// One VM term at the seven positions.  ta / tb / tl: the taps of the plane's two axes and of the line's axis at {centre, +h, -h}.
// v[0] centre, v[1], v[2] the plane's first axis +-, v[3], v[4] its second axis +-, v[5], v[6] the line's axis +-.
// The scheduling barriers bound what is in flight to one group of loads (10, 8, 8 float4), so that the 78 loads of the three terms are not all hoisted to the top:
// 125 VGPRs, four waves per SIMD to hide the gather's latency behind.
__device__ __forceinline__ void vm_grad_term(const float4 *__restrict__ P, const float4 *__restrict__ Ln, int W, int H, int L, const AxisTap ta[3], const AxisTap tb[3],
                                             const AxisTap tl[3], int sub, float v[7])
{
    const float4 pc = vm_plane4(P, W, H, ta[0], tb[0], sub), lc = vm_line4(Ln, L, tl[0], sub);
    v[0] = vm_dot4(pc, lc);
    v[5] = vm_dot4(pc, vm_line4(Ln, L, tl[1], sub));
    v[6] = vm_dot4(pc, vm_line4(Ln, L, tl[2], sub));
    __builtin_amdgcn_sched_barrier(0);
    v[1] = vm_dot4(vm_plane4(P, W, H, ta[1], tb[0], sub), lc);
    v[2] = vm_dot4(vm_plane4(P, W, H, ta[2], tb[0], sub), lc);
    __builtin_amdgcn_sched_barrier(0);
    v[3] = vm_dot4(vm_plane4(P, W, H, ta[0], tb[1], sub), lc);
    v[4] = vm_dot4(vm_plane4(P, W, H, ta[0], tb[2], sub), lc);
    __builtin_amdgcn_sched_barrier(0);
}

// One quad-lane's share of the seven values at p: f[0] centre, f[1 + 2 k], f[2 + 2 k]: axis k shifted by +h_k, -h_k.  The caller adds the four lanes of the quad
// (f[j] += shfl_xor 1, then 2) and forms (f[1 + 2 k] - f[2 + 2 k]) * inv2h[k].
__device__ __forceinline__ void vm_grad_point(const SceneDev &sc, float px, float py, float pz, const float3 h, int sub, float f[7])
{
    // per axis: the taps at {centre, +h, -h}; the shifted coordinate is a separately rounded fp32 sum
    const AxisTap tp[3][3] = {{axis_tap(px, sc.gm1[0]), axis_tap(px + h.x, sc.gm1[0]), axis_tap(px - h.x, sc.gm1[0])},
                              {axis_tap(py, sc.gm1[1]), axis_tap(py + h.y, sc.gm1[1]), axis_tap(py - h.y, sc.gm1[1])},
                              {axis_tap(pz, sc.gm1[2]), axis_tap(pz + h.z, sc.gm1[2]), axis_tap(pz - h.z, sc.gm1[2])}};
    // f = (a + b) + c per position, density_feature_kernel's order
    float v[7];
    vm_grad_term(sc.dplane[0], sc.dline[0], sc.grid[0], sc.grid[1], sc.grid[2], tp[0], tp[1], tp[2], sub, v);     // plane (x, y), line z
    f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3]; f[4] = v[4]; f[5] = v[5]; f[6] = v[6];
    vm_grad_term(sc.dplane[1], sc.dline[1], sc.grid[0], sc.grid[2], sc.grid[1], tp[0], tp[2], tp[1], sub, v);     // plane (x, z), line y
    f[0] = f[0] + v[0]; f[1] = f[1] + v[1]; f[2] = f[2] + v[2]; f[3] = f[3] + v[5]; f[4] = f[4] + v[6]; f[5] = f[5] + v[3]; f[6] = f[6] + v[4];
    vm_grad_term(sc.dplane[2], sc.dline[2], sc.grid[1], sc.grid[2], sc.grid[0], tp[1], tp[2], tp[0], sub, v);     // plane (y, z), line x
    f[0] = f[0] + v[0]; f[1] = f[1] + v[5]; f[2] = f[2] + v[6]; f[3] = f[3] + v[1]; f[4] = f[4] + v[2]; f[5] = f[5] + v[3]; f[6] = f[6] + v[4];
}

// ---- CP scenes: one lane per point ------------------------------------------------------------------------------------------------------------------------------
// cell and weights of a normalised coordinate on an axis of L points, for ARBITRARY coordinates: the two taps' weights are zero where the tap lies outside the
// line (grid_sample's zeros padding), and the indices are clamped into the packed line so that nothing is read out of bounds
struct CpTap { int i0, i1; float u, w; };
__device__ __forceinline__ CpTap cp_tap(float c, float gm1, int L)
{
    const float f = unnorm(c, gm1);
    const float fl = floorf(fminf(fmaxf(f, -2.0f), gm1 + 2.0f));
    const int l0 = (int)fl;
    const float w = f - fl;
    CpTap t;
    t.u = (l0 >= 0 && l0 < L) ? 1.0f - w : 0.0f;
    t.w = (l0 + 1 >= 0 && l0 + 1 < L) ? w : 0.0f;
    t.i0 = min(max(l0, 0), L - 1);
    t.i1 = min(max(l0 + 1, 0), L - 1);
    return t;
}

__device__ __forceinline__ float4 cp_lerp4(const float4 *__restrict__ line, const CpTap t, int tpt, int g)
{
    return f4_fma(t.w, line[(size_t)t.i1 * tpt + g], f4_mul(t.u, line[(size_t)t.i0 * tpt + g]));
}
__device__ __forceinline__ float cp_dot4(float4 a, float4 b, float4 c)
{
    const float t0 = (a.x * b.x) * c.x, t1 = (a.y * b.y) * c.y, t2 = (a.z * b.z) * c.z, t3 = (a.w * b.w) * c.w;
    return (t0 + t1) + (t2 + t3);
}

// The seven values at p, in vm_grad_point's order (f[0] centre, then x+-, y+-, z+-).  A shift along an axis moves one of the three line factors: each line is
// interpolated at {centre, +h, -h} (18 float4 taps per group of four components where seven calls of cp_density_feature_kernel read 42) and the seven products are
// formed and summed in that kernel's order, so the centre is bit-equal to it and the quotient is the one of its values at the shifted points.
__device__ __forceinline__ void cp_grad_point(const SceneDev &sc, const CpDev &cp, float px, float py, float pz, const float3 h, float f[7])
{
    // [0] centre, [1] +h, [2] -h
    const CpTap tx[3] = {cp_tap(px, sc.gm1[0], sc.grid[0]), cp_tap(px + h.x, sc.gm1[0], sc.grid[0]), cp_tap(px - h.x, sc.gm1[0], sc.grid[0])};
    const CpTap ty[3] = {cp_tap(py, sc.gm1[1], sc.grid[1]), cp_tap(py + h.y, sc.gm1[1], sc.grid[1]), cp_tap(py - h.y, sc.gm1[1], sc.grid[1])};
    const CpTap tz[3] = {cp_tap(pz, sc.gm1[2], sc.grid[2]), cp_tap(pz + h.z, sc.gm1[2], sc.grid[2]), cp_tap(pz - h.z, sc.gm1[2], sc.grid[2])};
    const int tpt = cp.rd >> 2;
    float fc = 0.0f, fxp = 0.0f, fxm = 0.0f, fyp = 0.0f, fym = 0.0f, fzp = 0.0f, fzm = 0.0f;
    for (int g = 0; g < tpt; ++g) {
        const float4 a = cp_lerp4(sc.dline[0], tz[0], tpt, g), b = cp_lerp4(sc.dline[1], ty[0], tpt, g), c = cp_lerp4(sc.dline[2], tx[0], tpt, g);
        fc = fc + cp_dot4(a, b, c);
        fxp = fxp + cp_dot4(a, b, cp_lerp4(sc.dline[2], tx[1], tpt, g));
        fxm = fxm + cp_dot4(a, b, cp_lerp4(sc.dline[2], tx[2], tpt, g));
        fyp = fyp + cp_dot4(a, cp_lerp4(sc.dline[1], ty[1], tpt, g), c);
        fym = fym + cp_dot4(a, cp_lerp4(sc.dline[1], ty[2], tpt, g), c);
        fzp = fzp + cp_dot4(cp_lerp4(sc.dline[0], tz[1], tpt, g), b, c);
        fzm = fzm + cp_dot4(cp_lerp4(sc.dline[0], tz[2], tpt, g), b, c);
    }
    f[0] = fc; f[1] = fxp; f[2] = fxm; f[3] = fyp; f[4] = fym; f[5] = fzp; f[6] = fzm;
}
