// tvr_ngp_field.h — device and host code shared by the Instant-NGP translation units (tvr_ngp.hip: inference; tvr_ngp_grid.hip: the
// occupancy-grid update; tvr_ngp_geom.hip: density gradient and density lattice): the pcg32, the Morton helpers, the occupancy-cell lookup,
// the hash-grid level gather (and its tangents), SH-16, the packed weight images' layout, field_tile, the per-32-sample body of the fused
// network, and field_tile_grad, the density head with its spatial gradient.  Everything here has internal linkage or is inlined.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstdint>
#include "tvr_kernels.h"
#include "tvr_mfma.h"
#include "../../include/tvr_ngp.h"

#define NGP_G TVR_NGP_GRIDSIZE
#define NGP_CELLS (NGP_G * NGP_G * NGP_G)

// ------------------------------------------------------------------------------------------------ PCG32 (pcg32.h)
struct Pcg {
    uint64_t state, inc;
};
__device__ __forceinline__ uint32_t pcg_next(Pcg &r)
{
    const uint64_t old = r.state;
    r.state = old * 0x5851f42d4c957f2dULL + r.inc;
    const uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
    const uint32_t rot = (uint32_t)(old >> 59u);
    return (xs >> rot) | (xs << ((~rot + 1u) & 31));
}
__host__ __device__ __forceinline__ void pcg_advance(Pcg &r, uint64_t delta)
{
    uint64_t cur_mult = 0x5851f42d4c957f2dULL, cur_plus = r.inc, acc_mult = 1u, acc_plus = 0u;
    while (delta > 0) {
        if (delta & 1) {
            acc_mult *= cur_mult;
            acc_plus = acc_plus * cur_mult + cur_plus;
        }
        cur_plus = (cur_mult + 1) * cur_plus;
        cur_mult *= cur_mult;
        delta /= 2;
    }
    r.state = acc_mult * r.state + acc_plus;
}
__device__ __forceinline__ float pcg_float(Pcg &r) { return __uint_as_float((pcg_next(r) >> 9) | 0x3f800000u) - 1.0f; }

__host__ __device__ __forceinline__ uint32_t expand_bits(uint32_t v)
{
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
__host__ __device__ __forceinline__ uint32_t morton3d(uint32_t x, uint32_t y, uint32_t z) { return expand_bits(x) | (expand_bits(y) << 1) | (expand_bits(z) << 2); }
__host__ __device__ __forceinline__ uint32_t morton3d_invert(uint32_t x)
{
    x = x & 0x49249249;
    x = (x | (x >> 2)) & 0xc30c30c3;
    x = (x | (x >> 4)) & 0x0f00f00f;
    x = (x | (x >> 8)) & 0xff0000ff;
    x = (x | (x >> 16)) & 0x0000ffff;
    return x;
}
// ------------------------------------------------------------------------------------------------ occupancy cells (cascaded_grid_idx_at's rule)
__device__ __forceinline__ int frexp_exponent(float v)
{
    int e;
    (void)frexpf(v, &e);
    return e;
}
__device__ __forceinline__ int mip_from_pos(float x, float y, float z)
{
    const float m = fmaxf(fmaxf(fabsf(x - 0.5f), fabsf(y - 0.5f)), fabsf(z - 0.5f));
    return min(TVR_NGP_CASCADES - 1, max(0, frexp_exponent(m) + 1));
}
__device__ __forceinline__ bool occupied_at(float x, float y, float z, const uint8_t *__restrict__ bits, uint32_t mip)
{
    const float s = ldexpf(1.0f, -(int)mip);
    const int ix = (int)(((x - 0.5f) * s + 0.5f) * (float)NGP_G);
    const int iy = (int)(((y - 0.5f) * s + 0.5f) * (float)NGP_G);
    const int iz = (int)(((z - 0.5f) * s + 0.5f) * (float)NGP_G);
    const uint32_t idx = morton3d((uint32_t)min(max(ix, 0), NGP_G - 1), (uint32_t)min(max(iy, 0), NGP_G - 1), (uint32_t)min(max(iz, 0), NGP_G - 1));
    return bits[idx / 8 + (uint32_t)NGP_CELLS / 8 * mip] & (1u << (idx % 8));
}
// ------------------------------------------------------------------------------------------------ encoders
struct GridCfg {
    uint32_t offsets[TVR_NGP_LEVELS + 1];
    float scale[TVR_NGP_LEVELS];
    uint32_t hashed;                      // bit l: level l uses the spatial hash
};

// grid_index (HashEncode.h:75-93).  With the reference's fixed 2^19 table a level is either dense (res^3 fits: index = x + y*res +
// z*res^2, which can exceed the table by less than its size because corner coordinates reach res) or hashed (table size a power of
// two).  to_grid() checks that every level is one of the two, so the generic stride loop and the modulo reduce to this:
__device__ __forceinline__ uint32_t grid_entry(bool hashed, uint32_t size, uint32_t res, uint32_t x, uint32_t y, uint32_t z)
{
    const uint32_t dense = x + y * res + z * res * res;
    const uint32_t hash = x ^ (y * 19349663u) ^ (z * 83492791u);
    // min(): rows the sampler left unwritten (holes of rays that overflowed max_samples) hold arbitrary bits; never index outside the table
    return hashed ? (hash & (size - 1)) : min(dense - (dense >= size ? size : 0u), size - 1);
}

// one level of kernel_grid for one position: the 8 corner entries are fetched first (independent loads), then blended in corner order
__device__ __forceinline__ float2 encode_level(const float2 *__restrict__ tab, bool hashed, uint32_t size, float scale, float px, float py, float pz)
{
    const uint32_t res = (uint32_t)ceilf(scale) + 1u;
    const float x = __builtin_fmaf(px, scale, 0.5f), y = __builtin_fmaf(py, scale, 0.5f), z = __builtin_fmaf(pz, scale, 0.5f);
    const float fx0 = floorf(x), fy0 = floorf(y), fz0 = floorf(z);
    const uint32_t cx = (uint32_t)(int)fx0, cy = (uint32_t)(int)fy0, cz = (uint32_t)(int)fz0;
    const float fx = x - fx0, fy = y - fy0, fz = z - fz0;
    float2 v[8];
#pragma unroll
    for (int idx = 0; idx < 8; ++idx)
        v[idx] = tab[grid_entry(hashed, size, res, cx + (idx & 1), cy + ((idx >> 1) & 1), cz + ((idx >> 2) & 1))];
    float r0 = 0.f, r1 = 0.f;
#pragma unroll
    for (int idx = 0; idx < 8; ++idx) {
        float w = 1.0f;
        w *= (idx & 1) ? fx : 1 - fx;
        w *= (idx & 2) ? fy : 1 - fy;
        w *= (idx & 4) ? fz : 1 - fz;
        r0 = __builtin_fmaf(w, v[idx].x, r0);
        r1 = __builtin_fmaf(w, v[idx].y, r1);
    }
    return make_float2(r0, r1);
}

// encode_level plus the level's tangents d/df_k of the blend (include/tvr_ngp.h tvr_ngp_density_gradient), WITHOUT the factor scale: the caller applies it.
// v is encode_level's value bit for bit: the same fractions, the same weights in the same factor order (1 * wx is exact), the same fma chain.
// d[k] = sum over corners of (the weight with factor k replaced by +-1) * value, summed edge by edge: the four edges along axis k each contribute
// (product of the other two factors) * (far corner - near corner).  The same sum as the definition's, with the cancellation between the two corners of
// an edge taken first, on the table's own values.
struct LevelGrad {
    float2 v, d[3];
};
__device__ __forceinline__ LevelGrad encode_level_grad(const float2 *__restrict__ tab, bool hashed, uint32_t size, float scale, float px, float py, float pz)
{
    const uint32_t res = (uint32_t)ceilf(scale) + 1u;
    const float x = __builtin_fmaf(px, scale, 0.5f), y = __builtin_fmaf(py, scale, 0.5f), z = __builtin_fmaf(pz, scale, 0.5f);
    const float fx0 = floorf(x), fy0 = floorf(y), fz0 = floorf(z);
    const uint32_t cx = (uint32_t)(int)fx0, cy = (uint32_t)(int)fy0, cz = (uint32_t)(int)fz0;
    const float fx = x - fx0, fy = y - fy0, fz = z - fz0;
    float2 v[8];
#pragma unroll
    for (int idx = 0; idx < 8; ++idx)
        v[idx] = tab[grid_entry(hashed, size, res, cx + (idx & 1), cy + ((idx >> 1) & 1), cz + ((idx >> 2) & 1))];
    float r0 = 0.f, r1 = 0.f;
#pragma unroll
    for (int idx = 0; idx < 8; ++idx) {
        float w = 1.0f;
        w *= (idx & 1) ? fx : 1 - fx;
        w *= (idx & 2) ? fy : 1 - fy;
        w *= (idx & 4) ? fz : 1 - fz;
        r0 = __builtin_fmaf(w, v[idx].x, r0);
        r1 = __builtin_fmaf(w, v[idx].y, r1);
    }
    LevelGrad r;
    r.v = make_float2(r0, r1);
    const float f[3] = {fx, fy, fz};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int ka = (k + 1) % 3, kb = (k + 2) % 3;                // the two other axes
        float d0 = 0.f, d1 = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {                               // edge e: bit 0 -> axis ka, bit 1 -> axis kb
            const int near = ((e & 1) << ka) | ((e >> 1) << kb), far = near | (1 << k);
            const float w = ((e & 1) ? f[ka] : 1 - f[ka]) * ((e & 2) ? f[kb] : 1 - f[kb]);
            d0 = __builtin_fmaf(w, v[far].x - v[near].x, d0);
            d1 = __builtin_fmaf(w, v[far].y - v[near].y, d1);
        }
        r.d[k] = make_float2(d0, d1);
    }
    return r;
}

__device__ __forceinline__ void sh16(float dx, float dy, float dz, float *__restrict__ o)
{
    const float x = dx * 2.f - 1.f, y = dy * 2.f - 1.f, z = dz * 2.f - 1.f;
    const float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
    o[0] = 0.28209479177387814f;
    o[1] = -0.48860251190291987f * y;
    o[2] = 0.48860251190291987f * z;
    o[3] = -0.48860251190291987f * x;
    o[4] = 1.0925484305920792f * xy;
    o[5] = -1.0925484305920792f * yz;
    o[6] = 0.94617469575755997f * z2 - 0.31539156525251999f;
    o[7] = -1.0925484305920792f * xz;
    o[8] = 0.54627421529603959f * x2 - 0.54627421529603959f * y2;
    o[9] = 0.59004358992664352f * y * (-3.0f * x2 + y2);
    o[10] = 2.8906114426405538f * xy * z;
    o[11] = 0.45704579946446572f * y * (1.0f - 5.0f * z2);
    o[12] = 0.3731763325901154f * z * (5.0f * z2 - 3.0f);
    o[13] = 0.45704579946446572f * x * (1.0f - 5.0f * z2);
    o[14] = 1.4453057213202769f * z * (x2 - y2);
    o[15] = 0.59004358992664352f * x * (-x2 + 3.0f * y2);
}
// ------------------------------------------------------------------------------------------------ fused field kernel
// Two arithmetic variants of the five bias-free Linears, same gather, same register-resident chaining:
//   F16 = true  (default) v_mfma_f32_32x32x16_f16 with every fp32 operand split into fp16 hi + lo and three products per k-step
//                         (hi*lo, lo*hi, hi*hi; error ~2^-22 relative, i.e. fp32-grade) — 72 MFMAs x 32 cycles per 32 samples;
//   F16 = false           v_mfma_f32_32x32x2_f32, exact fp32 — 192 MFMAs x 64 cycles per 32 samples (-DTVR_NGP_MLP_F32=1).
// Chaining: the accumulator of a 32-neuron block holds, in lane (sample = lane%32, h = lane/32), register i, neuron
// (i/4)*8 + 4h + i%4.  A k-step of the next layer reads registers straight from there as its B operand, and the k order that implies
// is folded into the packed weight image (LDS), so no activation ever leaves the registers:
//   fp32 image  [layer][m_block][step][64 lanes] floats; step s pairs k = (ka, kb) for the two lane halves
//   fp16 image  [block][hi|lo][64 lanes] uint4 (8 halves); block = (layer, m_block, k-step of 16); lane half h, element j:
//                 hash features (density0)   t: level 2*(4t + j/2) + h, feature j%2
//                 previous accumulators      t: neuron (t/2)*32 + (2*(t%2) + j/4)*8 + 4h + j%4
//                 rgb0 input                 t=0: density_mlp output (j/4)*8 + 4h + j%4;  t=1: SH 8h + j
#ifndef TVR_NGP_MLP_F32
#define TVR_NGP_MLP_F32 0
#endif
#ifndef TVR_NGP_INFLIGHT          // hash levels per lane whose 8 corner loads are issued together (2 -> 16 float2 loads in flight)
#define TVR_NGP_INFLIGHT 2
#endif
#ifndef TVR_NGP_WAVES             // waves per SIMD the field kernel is compiled for
#define TVR_NGP_WAVES 2
#endif
enum { NGP_L_D0 = 0, NGP_L_D1 = 2 * 16 * 64, NGP_L_C0 = NGP_L_D1 + 32 * 64, NGP_L_C1 = NGP_L_C0 + 2 * 16 * 64, NGP_L_C2 = NGP_L_C1 + 2 * 32 * 64,
       NGP_IMAGE_FLOATS = NGP_L_C2 + 32 * 64 };
// fp16 image: first block of each layer (blocks are m_block-major, then k-step)
enum { NGP_H_D0 = 0, NGP_H_D1 = 4, NGP_H_C0 = 8, NGP_H_C1 = 12, NGP_H_C2 = 20, NGP_H_BLOCKS = 24, NGP_HIMAGE_FLOATS = NGP_H_BLOCKS * 2 * 64 * 4 };
static_assert(NGP_HIMAGE_FLOATS == NGP_IMAGE_FLOATS, "both images are 48 KiB");

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// one k-step (16 inputs) into the two 32-neuron blocks of a 64-wide layer; the two blocks alternate so that no MFMA directly follows
// the one it depends on
__device__ __forceinline__ void step2(const uint4 *__restrict__ w4, int blk0, int blk1, const Frag &b, f32x16 &a0, f32x16 &a1)
{
    AFrags<2> A;
    A.h[0] = w4[(blk0 * 2 + 0) * 64]; A.l[0] = w4[(blk0 * 2 + 1) * 64]; A.h[1] = w4[(blk1 * 2 + 0) * 64]; A.l[1] = w4[(blk1 * 2 + 1) * 64];
    f32x16 acc[2] = {a0, a1};
    mma<2>(A, b, acc);
    a0 = acc[0];
    a1 = acc[1];
}
__device__ __forceinline__ void step1(const uint4 *__restrict__ w4, int blk, const Frag &b, f32x16 &a)
{
    const AF A = {w4[(blk * 2 + 0) * 64], w4[(blk * 2 + 1) * 64]};
    mfma3(A, b, a);
}
// B fragment of k-step t (0..3) of a 64-wide activation held in two accumulators
__device__ __forceinline__ Frag relu_frag(const f32x16 &a0, const f32x16 &a1, int t)
{
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = relu_f(t < 2 ? a0[8 * (t & 1) + j] : a1[8 * (t & 1) + j]);
    return split8(v);
}

// One 32-sample column block through the encoders and both networks.  Lane (col = lane%32, hh = lane/32) holds sample col's
// position and direction; returns (rgb raw, density raw) of sample col in the lanes with hh == 0.  `lds_lane` = LDS image + lane.
// COLOUR = false stops behind density_mlp (no SH, no colour layers) and returns (0, 0, 0, density raw): the same gathers and the same
// MFMAs in the same order as the full tile's first two layers, so the density is the full tile's bit for bit.
template <bool F16, bool COLOUR = true>
__device__ __forceinline__ float4 field_tile(const GridCfg &g, const float2 *__restrict__ tab, const float *__restrict__ lds_lane, int hh, float px, float py, float pz,
                                             float dx, float dy, float dz)
{
    // ---- GATHER phase: lane half hh takes the hash levels of parity hh (8 levels x 8 corners)
    float f0[8], f1[8], shv[8];
    if (COLOUR) {
        float sh[16];
        sh16(dx, dy, dz, sh);
#pragma unroll
        for (int j = 0; j < 8; ++j) shv[j] = F16 ? (hh ? sh[8 + j] : sh[j]) : (hh ? sh[2 * j + 1] : sh[2 * j]);
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const uint32_t o0 = hh ? g.offsets[2 * p + 1] : g.offsets[2 * p];
        const uint32_t o1 = hh ? g.offsets[2 * p + 2] : g.offsets[2 * p + 1];
        const float sc = hh ? g.scale[2 * p + 1] : g.scale[2 * p];
        const bool hashed = (g.hashed >> (2 * p + hh)) & 1u;
        const float2 r = encode_level(tab + o0, hashed, o1 - o0, sc, px, py, pz);
        f0[p] = r.x;
        f1[p] = r.y;
        if ((p + 1) % TVR_NGP_INFLIGHT == 0) __builtin_amdgcn_sched_barrier(0);      // bounds the loads in flight (registers)
    }
    // ---- MATRIX phase
    float density_raw;
    f32x16 e = {0};
    if (F16) {
        const uint4 *w4 = reinterpret_cast<const uint4 *>(lds_lane);
        f32x16 a0 = {0}, a1 = {0};
        // density_mlp.0: 32 -> 64
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (j & 1) ? f1[4 * t + j / 2] : f0[4 * t + j / 2];
            step2(w4, NGP_H_D0 + t, NGP_H_D0 + 2 + t, split8(v), a0, a1);
        }
        // density_mlp.2: relu, 64 -> 16
        f32x16 d = {0};
#pragma unroll
        for (int t = 0; t < 4; ++t) step1(w4, NGP_H_D1 + t, relu_frag(a0, a1, t), d);
        density_raw = d[0];
        if (!COLOUR) return make_float4(0.f, 0.f, 0.f, density_raw);
        // rgb_mlp.0: [density(16), SH(16)] -> 64
        a0 = (f32x16){0};
        a1 = (f32x16){0};
        {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = d[j];
            step2(w4, NGP_H_C0 + 0, NGP_H_C0 + 2, split8(v), a0, a1);
            step2(w4, NGP_H_C0 + 1, NGP_H_C0 + 3, split8(shv), a0, a1);
        }
        // rgb_mlp.2: relu, 64 -> 64
        f32x16 c0 = {0}, c1 = {0};
#pragma unroll
        for (int t = 0; t < 4; ++t) step2(w4, NGP_H_C1 + t, NGP_H_C1 + 4 + t, relu_frag(a0, a1, t), c0, c1);
        // rgb_mlp.4: relu, 64 -> 3
#pragma unroll
        for (int t = 0; t < 4; ++t) step1(w4, NGP_H_C2 + t, relu_frag(c0, c1, t), e);
    } else {
        const float *wl = lds_lane;
        f32x16 a0 = {0}, a1 = {0};                              // the two 32-neuron blocks of a 64-wide layer
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const float bv = (s & 1) ? f1[s >> 1] : f0[s >> 1];
            a0 = MFMA(wl[NGP_L_D0 + (0 * 16 + s) * 64], bv, a0);
            a1 = MFMA(wl[NGP_L_D0 + (1 * 16 + s) * 64], bv, a1);
        }
        f32x16 d = {0};
#pragma unroll
        for (int s = 0; s < 32; ++s) d = MFMA(wl[NGP_L_D1 + s * 64], relu_f(s < 16 ? a0[s & 15] : a1[s & 15]), d);
        if (!COLOUR) return make_float4(0.f, 0.f, 0.f, d[0]);
        a0 = (f32x16){0};
        a1 = (f32x16){0};
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const float bv = s < 8 ? d[s & 7] : shv[s & 7];
            a0 = MFMA(wl[NGP_L_C0 + (0 * 16 + s) * 64], bv, a0);
            a1 = MFMA(wl[NGP_L_C0 + (1 * 16 + s) * 64], bv, a1);
        }
        density_raw = d[0];
        f32x16 c0 = {0}, c1 = {0};
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            const float bv = relu_f(s < 16 ? a0[s & 15] : a1[s & 15]);
            c0 = MFMA(wl[NGP_L_C1 + (0 * 32 + s) * 64], bv, c0);
            c1 = MFMA(wl[NGP_L_C1 + (1 * 32 + s) * 64], bv, c1);
        }
#pragma unroll
        for (int s = 0; s < 32; ++s) e = MFMA(wl[NGP_L_C2 + s * 64], relu_f(s < 16 ? c0[s & 15] : c1[s & 15]), e);
    }
    // rows 0..2 of the last layer and row 0 of the density head sit in accumulator regs 0..2 / 0 of the lower half-wave
    return make_float4(e[0], e[1], e[2], density_raw);
}

// ------------------------------------------------------------------------------------------------ density and its gradient, forward mode
// The power of two e for which m * 2^-e lies in [2^14, 2^15), m = the largest magnitude of one sample's operand column over BOTH lane halves (a column's 16 k
// values sit 8 and 8 in lanes col and col + 32).  A column divided by 2^e fits the fp16 hi/lo split (exact up to 65504) whatever its size, the largest element
// keeps all 22 bits of the split, and the product is linear in the column: the accumulator is multiplied by 2^e afterwards, exactly.  m = 0 or denormal gives
// e = -141: zeros stay zeros.
__device__ __forceinline__ int column_exp(float m)
{
    m = fmaxf(m, __shfl_xor(m, 32));
    return (int)((__float_as_uint(m) >> 23) & 255u) - (127 + 14);
}
// split8 with both halves rounded to NEAREST (hi = RN16(x), lo = RN16(x - hi); x - hi is exact in fp32), for operands known to be below 2^15 (RN overflows to inf
// above 65504, which is why split8 truncates).  split8's lo always has the sign of x, and so has the weights' lo: the product lo * lo that a k-step leaves out
// is then a bias of up to 2^-20 of every term, all of one sign.  Rounded to nearest the operand's lo is signed at random and half as large: no bias.
__device__ __forceinline__ Frag split8n(const float v[8])
{
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    unsigned hi[4], lo[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const f16x2 h = __builtin_convertvector((f32x2_){v[2 * p], v[2 * p + 1]}, f16x2);
        const f32x2_ r = {v[2 * p] - (float)h.x, v[2 * p + 1] - (float)h.y};
        hi[p] = __builtin_bit_cast(unsigned, h);
        lo[p] = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
    }
    Frag f;
    f.hi = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    f.lo = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    return f;
}

// field_tile<F16, false> with three tangent columns per sample beside the value column.  Returns (d raw / d p_x, d raw / d p_y, d raw / d p_z, density raw) of
// sample col in the lanes with hh == 0; the derivative is the one include/tvr_ngp.h defines (tvr_ngp_density_gradient), with respect to the unit-cube position.
// The value column runs field_tile's own gathers, fma chains and MFMAs in field_tile's order — the tangent work only sits between them — so .w is field_tile's
// density bit for bit.  Tangent k of level l is scale_l * encode_level_grad's d[k]; the three tangent encodings go through density_mlp.0 as three more B
// operands against the same LDS weight image and are masked by [h > 0] (h: see "the ReLU mask" below).  Row 0 of density_mlp.2 is 64 numbers: in the F16 build it
// is applied as an fp32 fma chain over the lane's 32 hidden units (`w1row` = that row in the accumulators' order for lane half hh: element i < 16 belongs to register i of the
// first block, 16 + i to register i of the second) and one exchange between the lane halves — exact fp32 weights, no split, no MFMA.
// RANGE (F16): scale_l reaches 2048 * aabb_scale and the table's values are the scene's, so a tangent can pass the fp16 split's 65504.  Every tangent column is
// divided by its own power of two before the split and the hidden tangents multiplied back afterwards (column_exp): no assumption on scale, table values or weights.
template <bool F16>
__device__ __forceinline__ float4 field_tile_grad(const GridCfg &g, const float2 *__restrict__ tab, const float *__restrict__ lds_lane, const float *__restrict__ w1row,
                                                  int hh, float px, float py, float pz)
{
    // ---- GATHER phase: as field_tile's; tg[k][2p + c] = tangent k of (level 2p + hh, feature c)
    float f0[8], f1[8], tg[3][16];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const uint32_t o0 = hh ? g.offsets[2 * p + 1] : g.offsets[2 * p];
        const uint32_t o1 = hh ? g.offsets[2 * p + 2] : g.offsets[2 * p + 1];
        const float sc = hh ? g.scale[2 * p + 1] : g.scale[2 * p];
        const bool hashed = (g.hashed >> (2 * p + hh)) & 1u;
        const LevelGrad r = encode_level_grad(tab + o0, hashed, o1 - o0, sc, px, py, pz);
        f0[p] = r.v.x;
        f1[p] = r.v.y;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            tg[k][2 * p] = r.d[k].x * sc;
            tg[k][2 * p + 1] = r.d[k].y * sc;
        }
        if ((p + 1) % TVR_NGP_INFLIGHT == 0) __builtin_amdgcn_sched_barrier(0);
    }
    // ---- MATRIX phase: the value column exactly as field_tile runs it
    float density_raw;
    f32x16 a0 = {0}, a1 = {0};
    if (F16) {
        const uint4 *w4 = reinterpret_cast<const uint4 *>(lds_lane);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (j & 1) ? f1[4 * t + j / 2] : f0[4 * t + j / 2];
            step2(w4, NGP_H_D0 + t, NGP_H_D0 + 2 + t, split8(v), a0, a1);
        }
        f32x16 d = {0};
#pragma unroll
        for (int t = 0; t < 4; ++t) step1(w4, NGP_H_D1 + t, relu_frag(a0, a1, t), d);
        density_raw = d[0];
    } else {
        const float *wl = lds_lane;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const float bv = (s & 1) ? f1[s >> 1] : f0[s >> 1];
            a0 = MFMA(wl[NGP_L_D0 + (0 * 16 + s) * 64], bv, a0);
            a1 = MFMA(wl[NGP_L_D0 + (1 * 16 + s) * 64], bv, a1);
        }
        f32x16 d = {0};
#pragma unroll
        for (int s = 0; s < 32; ++s) d = MFMA(wl[NGP_L_D1 + s * 64], relu_f(s < 16 ? a0[s & 15] : a1[s & 15]), d);
        density_raw = d[0];
    }
    // ---- the ReLU mask.  The value path's own h is fp32-class only relative to inputs of size 2^-14 and more: below that the fp16 split resolves an input to
    // multiples of 2^-24 (fp16's subnormal spacing), and a hidden unit of a small encoding — every vertex of the level set raw = 0 of a field whose live units
    // cross 0 there — comes out as exactly 0, which would switch its gradient off.  So the F16 build evaluates h once more for the mask alone: the encoding column
    // divided by ITS power of two, rounded to nearest, through the same weights.  Its sign is that of an fp32-class h (error ~2^-22 of sum_k |W0_jk| |enc_k|).
    f32x16 m0 = a0, m1 = a1;
    if (F16) {
        const uint4 *w4 = reinterpret_cast<const uint4 *>(lds_lane);
        float m = 0.f;
#pragma unroll
        for (int p = 0; p < 8; ++p) m = fmaxf(m, fmaxf(fabsf(f0[p]), fabsf(f1[p])));
        const int ev = column_exp(m);
        m0 = (f32x16){0};
        m1 = (f32x16){0};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = ldexpf((j & 1) ? f1[4 * t + j / 2] : f0[4 * t + j / 2], -ev);
            step2(w4, NGP_H_D0 + t, NGP_H_D0 + 2 + t, split8n(v), m0, m1);
        }
    }
    // ---- the tangent columns
    float grad[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        f32x16 b0 = {0}, b1 = {0};
        int e0 = 0;
        if (F16) {
            const uint4 *w4 = reinterpret_cast<const uint4 *>(lds_lane);
            float m = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) m = fmaxf(m, fabsf(tg[k][j]));
            e0 = column_exp(m);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = ldexpf(tg[k][8 * t + j], -e0);      // element j of k-step t: level 2 * (4t + j/2) + hh, feature j%2
                step2(w4, NGP_H_D0 + t, NGP_H_D0 + 2 + t, split8n(v), b0, b1);
            }
        } else {
            const float *wl = lds_lane;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                b0 = MFMA(wl[NGP_L_D0 + (0 * 16 + s) * 64], tg[k][s], b0);
                b1 = MFMA(wl[NGP_L_D0 + (1 * 16 + s) * 64], tg[k][s], b1);
            }
        }
        if (F16) {
            float part = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) part = __builtin_fmaf(w1row[i], m0[i] > 0.f ? b0[i] : 0.f, part);
#pragma unroll
            for (int i = 0; i < 16; ++i) part = __builtin_fmaf(w1row[16 + i], m1[i] > 0.f ? b1[i] : 0.f, part);
            grad[k] = ldexpf(part + __shfl_xor(part, 32), e0);
        } else {                                                    // exact fp32 MFMAs: the row through the matrix unit like the value's
            const float *wl = lds_lane;
            f32x16 dk = {0};
#pragma unroll
            for (int s = 0; s < 32; ++s) {
                const float hv = s < 16 ? a0[s & 15] : a1[s & 15], tv = s < 16 ? b0[s & 15] : b1[s & 15];
                dk = MFMA(wl[NGP_L_D1 + s * 64], hv > 0.f ? tv : 0.f, dk);
            }
            grad[k] = dk[0];
        }
    }
    return make_float4(grad[0], grad[1], grad[2], density_raw);
}
// fills w1rows[64] (LDS; [lane half][32]) with row 0 of density_mlp.2 in the accumulators' order, from the packed fp32 image (tvr_ngp_net_pack's first half:
// step s of that layer holds, at lanes 0 and 32, the row's weights for register s % 16 of block s / 16 in lane half 0 and 1)
__device__ __forceinline__ void load_w1rows(const float *__restrict__ image32, float *__restrict__ w1rows)
{
    if (threadIdx.x < 64) w1rows[threadIdx.x] = image32[NGP_L_D1 + (threadIdx.x & 31) * 64 + 32 * (threadIdx.x >> 5)];
}

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

static int to_grid(const tvr_ngp_grid_cfg *cfg, GridCfg &g)
{
    if (!cfg) return tvr_set_error(TVR_ERR_INVALID, "grid cfg is NULL");
    g.hashed = 0;
    for (int l = 0; l < TVR_NGP_LEVELS; ++l) {
        if (cfg->offsets[l + 1] <= cfg->offsets[l]) return tvr_set_error(TVR_ERR_INVALID, "grid offsets not increasing at level %d", l);
        if (!(cfg->scale[l] > 0.f) || cfg->scale[l] > 65000.f) return tvr_set_error(TVR_ERR_INVALID, "grid scale[%d] out of (0, 65000]", l);
        g.scale[l] = cfg->scale[l];
        // replay grid_index's stride loop (uint32 arithmetic) to classify the level
        const uint32_t size = cfg->offsets[l + 1] - cfg->offsets[l], res = (uint32_t)ceilf(cfg->scale[l]) + 1u;
        uint32_t stride = 1;
        int dims = 0;
        for (; dims < 3 && stride <= size; ++dims) stride *= res;
        if (size < stride) {
            if (size & (size - 1)) return tvr_set_error(TVR_ERR_UNSUPPORTED, "hashed level %d has a table of %u entries (not a power of two)", l, size);
            g.hashed |= 1u << l;
        } else if (dims != 3 || (uint64_t)res * res * res + (uint64_t)res * res + res >= 2ull * size) {
            return tvr_set_error(TVR_ERR_UNSUPPORTED, "level %d (res %u, %u entries) is neither dense nor hashed", l, res, size);
        }
    }
    for (int l = 0; l <= TVR_NGP_LEVELS; ++l) g.offsets[l] = cfg->offsets[l];
    return TVR_OK;
}
