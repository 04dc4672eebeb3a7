// tvr_march_body.h — what the march kernels' shared body (tvr_march_body.inc) needs in front of it: the launch constants and the density evaluations.  Included by
// tvr_march.hip (march_kernel: TensorVMSplit / REFTensoRF) and tvr_cp.hip (cp_march_kernel: TensorCP).
#pragma once
#include "tvr_device.h"
#include "tvr_kernels.h"

// Small launches (a 4096-ray training batch or render chunk, a rank's share of a split frame: 16 rays per CU, one per wave) — measured in round 3
// (scripts/march_timeline.py, profiles/r03_march_timeline.txt): a wave's chain takes 10.4 us per 64-sample chunk at 4096 rays, 8.3 at 16 384,
// 7.2 in the full frame; the kernel ends 80 us after it starts where its share of a full frame is 49 us.  Tried and dropped: staggering the
// waves' starts over a chunk period (no change: it is not a lock-step effect) and touching the next chunk's 12 plane texels per sample one
// chunk ahead (12.1 us per chunk, 32.8 vs 30.2 ms per 157-call frame: the extra loads cost more than the misses they hide).  What DID cost a
// small launch 100 us was this kernel's own statistics: three same-address global atomics per wave (4096 waves) — now one per group.
#define MARCH_MAX_WAVES 16
#define MARCH_TILE 16                     // rays per tile
#define MARCH_SPIN_LIMIT (1u << 22)       // s_sleep(1) each: ~0.15 s, against a legitimate wait of microseconds
#define MARCH_SLOTS 64u                   // ring of published handouts (a waiter's slot is reused 64 local tiles = 1024 cursor draws later)
#ifndef MARCH_CTR_WORD
#define MARCH_CTR_WORD 1                  // word of the scratch header that counts handed-out rays (its own 128-B line, word 32, measured the same: 7.55 vs 7.58 ms)
#endif
#ifndef MARCH_TAIL
#define MARCH_TAIL 4u                     // rays per handout at the end of a launch (16u = off)
#endif
// The volume march (march_vol_kernel, tvr_march.hip).  Its launch shape, measured on the 800x800 x 512 bench frame (profiles/density_volume.txt):
// alone, the kernel takes 5.15 - 5.20 ms whether a CU holds 16, 24 or 32 of its waves (5.50 with 8), so the shape was chosen on the frame rendered in pieces, where the
// other piece's shade kernel competes for the CUs: 32 / 24 / 16 waves per CU in groups of 8 gave 17.0 / 16.5 / 15.3 - 15.5 ms per frame, one group of 16 waves 15.1, two
// 16.5, and one group of 16 waves at 65 registers (the 72-register step) 16.4.  Hence ONE group of 16 waves per CU — the factored kernel's shape: a tile's 16 rays march
// concurrently and share their lines in L1 — compiled for 64 registers (the launch bound asks for 8 waves per SIMD to get that cap, not to run them); why the frame
// prefers it is not established.  LDS is the header and 6 B per sample and wave (49 KB at 512 samples, where the factored kernel holds 107 KB).  The
// DENSE form (debugging surface, 70 registers) is compiled for one wave fewer rather than spill to scratch.
#ifndef MARCH_VOL_WAVES
#define MARCH_VOL_WAVES 16                // waves per group
#endif
#ifndef MARCH_VOL_GROUPS
#define MARCH_VOL_GROUPS 1                // groups per CU
#endif
#ifndef MARCH_VOL_OCC
#define MARCH_VOL_OCC 8                   // waves per SIMD the kernel's registers are capped for (512 / 8 = 64)
#endif
#define MARCH_HDR 560                     // LDS header: ray cursor (16 B) + 64 slots of {local tile number + 1 | tail bit, first ray} (dynamic queue) + 3 u64 statistics sums + pad
#ifndef MARCH_LSTRIDE
#define MARCH_LSTRIDE 4                   // float4 per line texel in LDS.  4 = packed; 5 (80 B: the texels of 16 consecutive cells in distinct banks) removes
#endif                                    // the line taps' bank conflicts (34 % of the LDS-active cycles) and measures SLOWER: 8.2 vs 8.0 ms — the kernel sits on the L1 path

// vm_term<4, false> with the line taps taken from the LDS copy (same arithmetic, same order).
// Round 5: the plane taps are addressed as wave-uniform base + 32-BIT byte offset (global_load ... v_off, s[base] offset:imm): the 64-bit per-lane address
// arithmetic this replaced (v_mad_i64_i32, v_lshlrev_b64, 2 x v_lshl_add_u64 per plane and sub-step: multi-pass instructions) was a tenth of the kernel's VALU
// issue time.  A density plane of the largest grid the ABI admits (4097^2 texels x 64 B) is 1.07 GB: the offsets fit 32 bits.
__device__ __forceinline__ float4 vm_term_lds(const float4 *__restrict__ P, const float4 *Ls, int W, int x0, int y0, int l0,
                                              float wx, float wy, float wl, int sub)
{
    const float ux = 1.0f - wx, uy = 1.0f - wy, ul = 1.0f - wl;
    const int Wp = W + 1;
    const unsigned cell = __umul24((unsigned)y0, (unsigned)Wp) + (unsigned)x0;            // both factors below 2^24 (grid <= 4096)
    unsigned o0 = (cell << 6) + ((unsigned)sub << 4), o1 = o0 + ((unsigned)Wp << 6);
    asm volatile("" : "+v"(o0), "+v"(o1));                                                // opaque: hipcc otherwise widens the sums back into 64-bit arithmetic
    const unsigned char *pb = (const unsigned char *)P;
    const float4 t00 = *(const float4 *)(pb + (size_t)o0), t01 = *(const float4 *)(pb + (size_t)o0 + 64);
    const float4 t10 = *(const float4 *)(pb + (size_t)o1), t11 = *(const float4 *)(pb + (size_t)o1 + 64);
    const float4 *q = Ls + l0 * MARCH_LSTRIDE + sub;
    const float4 l0v = q[0], l1v = q[MARCH_LSTRIDE];
    float4 p4 = f4_mul(ux * uy, t00);
    p4 = f4_fma(wx * uy, t01, p4);
    p4 = f4_fma(ux * wy, t10, p4);
    p4 = f4_fma(wx * wy, t11, p4);
    float4 q4 = f4_mul(ul, l0v);
    q4 = f4_fma(wl, l1v, q4);
    return make_float4(p4.x * q4.x, p4.y * q4.y, p4.z * q4.z, p4.w * q4.w);
}

// One quad-lane's share of a CP density feature  sum_r L0[r](z) L1[r](y) L2[r](x)  (models/tensoRF.py:345-360) for one in-box sample: the lines are packed
// [L+1][rd] (channels-last, zero pad texel at index L, zero pad channels up to rd, a multiple of 16); lane `sub` of the quad takes float4 number 4 g + sub of every texel.
__device__ __forceinline__ float cp_density_quad(const SceneDev &sc, const CpDev &cp, int ix, int iy, int iz, float wx, float wy, float wz, int sub)
{
    const int tpt = cp.rd >> 2;                          // float4 per texel
    const float4 *__restrict__ l0 = sc.dline[0] + (size_t)iz * tpt + sub;       // line i runs along axis vecMode[i] = 2 - i
    const float4 *__restrict__ l1 = sc.dline[1] + (size_t)iy * tpt + sub;
    const float4 *__restrict__ l2 = sc.dline[2] + (size_t)ix * tpt + sub;
    const float ux = 1.0f - wx, uy = 1.0f - wy, uz = 1.0f - wz;
    float part = 0.0f;
    for (int g = 0; g < tpt; g += 4) {
        const float4 a0 = l0[g], a1 = l0[g + tpt], b0 = l1[g], b1 = l1[g + tpt], c0 = l2[g], c1 = l2[g + tpt];
        const float4 a = f4_fma(wz, a1, f4_mul(uz, a0)), b = f4_fma(wy, b1, f4_mul(uy, b0)), c = f4_fma(wx, c1, f4_mul(ux, c0));
        const float tx = (a.x * b.x) * c.x, ty = (a.y * b.y) * c.y, tz = (a.z * b.z) * c.z, tw = (a.w * b.w) * c.w;
        part = part + ((tx + ty) + (tz + tw));
    }
    return part;
}

// The baked density volume (tvr_scene_set_density_volume): D[z][y][x] = sum_i sum_c plane_i[c] * line_i[c] at the grid points, (gx+1)(gy+1)(gz+1) fp32 with x fastest.
// Inside a cell a bilinear function of two coordinates times a linear one of the third is trilinear, so the factored feature IS the trilinear interpolation of the cell's
// eight corner values — an identity in exact arithmetic; in fp32 the two forms differ by rounding.  Lane per sample: four row loads of two adjacent
// floats (4-byte aligned: the pair may start at an odd index), then seven lerps a + w (b - a) in this fixed order — x on the four rows, y on the two z layers, z last.
// A tap at index grid (the padding layer, finite) only ever meets weight 0: fmaf(0, pad - a, a) == a.
struct __attribute__((packed, aligned(4))) vol_pair { float a, b; };
__device__ __forceinline__ float vol_density(const float *__restrict__ D, int gx1, int gy1, int ix, int iy, int iz, float wx, float wy, float wz)
{
    const size_t sy = (size_t)gx1, sz = (size_t)gx1 * (size_t)gy1;        // a volume of the largest grid the ABI admits has 4097^3 values: 64-bit indices
    const float *r = D + ((size_t)iz * sz + (size_t)iy * sy + (size_t)ix);
    const vol_pair p00 = *(const vol_pair *)r, p01 = *(const vol_pair *)(r + sy);
    const vol_pair p10 = *(const vol_pair *)(r + sz), p11 = *(const vol_pair *)(r + sz + sy);
    const float c00 = __builtin_fmaf(wx, p00.b - p00.a, p00.a), c01 = __builtin_fmaf(wx, p01.b - p01.a, p01.a);
    const float c10 = __builtin_fmaf(wx, p10.b - p10.a, p10.a), c11 = __builtin_fmaf(wx, p11.b - p11.a, p11.a);
    const float c0 = __builtin_fmaf(wy, c01 - c00, c00), c1 = __builtin_fmaf(wy, c11 - c10, c10);
    return __builtin_fmaf(wz, c1 - c0, c0);
}
