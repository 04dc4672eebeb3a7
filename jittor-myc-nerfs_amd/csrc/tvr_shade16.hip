// tvr_shade16.hip — the render path's shade kernel on v_mfma_f32_16x16x32_f16 (round 5).
//
// The same work as tvr_shade.hip's shade_kernel<SH_SRC_QUEUE, SH_DST_QUEUE> for TensorVMSplit scenes in the default (fp32-class) arithmetic:
//   models/tensoRF.py:228-244 compute_appfeature, models/tensorBase.py:9-15 positional_encoding, :76-86 MLPRender_Fea.execute (paths relative to
//   /root/reference/tensorf-myc/) — appearance gather, basis product, positional encoding, the 150 -> 128 -> 128 -> 3 MLP, sigmoid; three fp16 hi/lo products per
//   fp32 product, fp32 accumulation.
// Why a second kernel: the 32x32x16 kernel runs against the chip's POWER limit (1.67 GHz on 256 CUs), and at that limit the 16x16x32 shape delivers 1.10 x the
// FLOP/s with the same LDS fragment traffic (profiles/r05_mfma_shape_probe.txt: 1641 vs 1491 TFLOP/s, cycles per MFMA 17.25 vs 32.67); a timing build of the old
// kernel with every MFMA replaced by two of this shape ran 11.28 ms against 12.42 (profiles/r05_shade_mfma_shape_diag.txt).  This is that kernel built for real.
//
// Tile: 32 queue entries per wave as TWO 16-column B tiles that share every A fragment.  Lane (c = lane & 15, g = lane >> 4) serves entries eA = 32 tile + c
// and eB = eA + 16 and holds, of each, k-group g (8 of the 32 k values of a k-step) as B operand and rows 4g .. 4g+3 of every 16-row block as accumulators.
//   GATHER phase  every lane gathers for ITS OWN entry (groups 0, 1: A; groups 2, 3: B): nine units of 6 taps x 2 float4 (the 32x32 kernel's count), unit u = channels
//                 16u + 8 (g & 1) .. + 7 of the 144 = of plane u / 3; offsets and weights once per plane.  A unit's fragment holds {A | B} in its lower | upper half, and
//                 v_permlane32_swap(unit 2s, unit 2s+1) IS k-step s's B operand of tile A | tile B in the natural k order; unit 8's halves are k-step 4's (the A operand of
//                 groups 2, 3 is zero there).  The interpolation is tvr_shade_common.h's taps_eval op for op: the same h values as the 32x32 kernel's.
//   MATRIX phase  (behind the SIMD's matrix token, as before)  basis 60 MFMAs -> F (8 base values per lane and entry) -> layer 1: 5 k-steps x 8 row blocks x 6
//                 MFMAs, the next k-step's [v, sin v, sin 2v, cos v, cos 2v] fragments derived under them -> layer 2: B = relu(layer-1 accumulators) as they lie
//                 (row blocks 2s, 2s+1 of lane group g = k-step s), row block by row block, layer 3 (fp32 FMAs) of row block rb-1 under the MFMAs of row block rb.
//   finish        last row block's layer 3, the sums over the four lane groups (v_permlane32_swap / v_permlane16_swap adds, fixed order), sigmoid, store.
// Per accumulator the order of the additions differs from the 32x32 kernel's (32 k per step instead of 16): results agree to fp32 rounding, not bit for bit; per ray the
// compositing order is unchanged, so every invariance the tests hold (chunking, permutation, partition) holds as before.
// Phase rule: lifted for this kernel on the round-5 evidence (profiles/r05_phase_rule_test.txt: a build with 12 global loads per lane between layer 1 and layer 2 is
// bit-identical on 8 frames x 2 and passes the reproducibility tests) — the loads are still issued in the gather phase here, nothing relies on the lift.
#include <cstdlib>
#include "tvr_device.h"
#include "tvr_kernels.h"
#include "tvr_mfma.h"
#include "tvr_shade_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define S16_WAVES 8         // the factored kernel: two waves per SIMD
#define S16_THREADS (64 * S16_WAVES)
#define S16_VOL_WAVES 12    // the volume kernel: three, their matrix phases side by side (no matrix token)
#define S16_VOL_THREADS (64 * S16_VOL_WAVES)
#define S16_TILE 32
#ifndef S16_PRIO_M
#define S16_PRIO_M 2      // s_setprio in the matrix phase / the gather phase / layer 3's tail (the 32x32 kernel's measured choice)
#endif
#ifndef S16_PRIO_G
#define S16_PRIO_G 0
#endif
#ifndef S16_PD
#define S16_PD 2          // A-fragment pairs are read this many row blocks ahead, ring of S16_PD + 2
#endif
#define S16_VOL_PD 1      // the volume kernel's: 8 registers fewer, what three waves per SIMD need (168 VGPRs)
#ifndef S16_MSLEEP
#define S16_MSLEEP 2
#endif
#ifndef S16_TOKEN_SPINS
#define S16_TOKEN_SPINS 4096
#endif
#ifndef S16_TIMING
#define S16_TIMING 0      // diagnostic build: per-phase s_memtime sums into stats[8..15] (scripts/phase_timing.py)
#endif
#if S16_TIMING
#define S16_STAMP(x) { __builtin_amdgcn_sched_barrier(0); x = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
#else
#define S16_STAMP(x)
#endif
#define S16_SB __builtin_amdgcn_sched_barrier(0)
#define S16_SG_MFMA(n) __builtin_amdgcn_sched_group_barrier(0x008, (n), 0)
#define S16_SG_VALU(n) __builtin_amdgcn_sched_group_barrier(0x402, (n), 0)      // VALU | TRANS
#define S16_SG_DSR(n) __builtin_amdgcn_sched_group_barrier(0x100, (n), 0)
// The kernel is bound by its SIMD's vector-issue port (492 MFMAs x 8 + ~1800 VALU x 4 cycles per tile against ~12 k cycles per tile and SIMD): every instruction
// removed is time.  v_sin_f32 / v_cos_f32 take revolutions; v * (1 / 2 pi) carries fp32's relative rounding, i.e. a phase error of |v| * 6e-8 rad — 2e-6 at the
// |v| <= 30 of a trained scene, 7e-5 at the |v| ~ 1100 that tests/test_gpu_parity.py::test_large_feature_magnitudes holds to the 1e-3 bar (its docstring prices exactly
// this error); fract keeps the argument inside the instructions' domain for any magnitude.  tvr_shade.hip's other modes keep sincos_pe's Cody-Waite form.
__device__ __forceinline__ void sincos_pe16(float x, float &s, float &c)
{
    const float t = __builtin_amdgcn_fractf(x * 0.15915494309189535f);
    s = __builtin_amdgcn_sinf(t);
    c = __builtin_amdgcn_cosf(t);
}
#ifndef S16_TICKET
#define S16_TICKET 4      // tiles per ticket of the dynamic tile hand-out
#endif
#ifndef S16_TICKET_MIN
#define S16_TICKET_MIN 256  // tiles per wave from which the tickets are used
#endif
#ifndef S16_GDEPTH
#define S16_GDEPTH 1      // units of the gather in flight ahead of the one being interpolated (24 registers each)
#endif

struct AF16 { uint4 h, l; };
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, (a)), __builtin_bit_cast(h8, (b)), (c), 0, 0, 0)
// one {hi, lo} A pair x two B tiles x three products (l*hi, h*lo, h*hi per accumulator: the order mfma3 of the 32x32 kernel has)
__device__ __forceinline__ void mfma6(const AF16 &A, const Frag &bA, const Frag &bB, f32x4 &accA, f32x4 &accB)
{
    accA = MFMA16(A.l, bA.hi, accA);
    accB = MFMA16(A.l, bB.hi, accB);
    accA = MFMA16(A.h, bA.lo, accA);
    accB = MFMA16(A.h, bB.lo, accB);
    accA = MFMA16(A.h, bA.hi, accA);
    accB = MFMA16(A.h, bB.hi, accB);
}
// an LDS pointer held in ONE register the compiler cannot see through (base + 16-bit immediates instead of one address register per read)
#define S16_LDS_BASE(name, expr)                                                                                    \
    unsigned name##_a = (unsigned)(size_t)(expr);                                                                   \
    asm volatile("" : "+v"(name##_a));                                                                              \
    const unsigned char *name = (const unsigned char *)(const void __attribute__((address_space(3))) *)(size_t)name##_a

// lower / upper 32 lanes of v in every lane (v_permlane32_swap: vdst' = {vdst.lo, src.lo}, src' = {vdst.hi, src.hi}; profiles/r05_permlane_semantics.txt)
__device__ __forceinline__ void halves_u(unsigned v, unsigned &lo, unsigned &hi)
{
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    lo = r[0]; hi = r[1];
}
__device__ __forceinline__ void halves_f(float v, float &lo, float &hi)
{
    unsigned a, b;
    halves_u(__float_as_uint(v), a, b);
    lo = __uint_as_float(a); hi = __uint_as_float(b);
}
// sum over the four lane groups of two per-entry partial sums: a (entry A) and b (entry B) -> lanes of groups 0, 1 hold A's total, groups 2, 3 B's.
// Fixed order: (g + (g ^ 2)) first, then the two 16-lane rows of a half.
__device__ __forceinline__ float group_sum2(float a, float b)
{
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);       // r0 = {a.lo, b.lo}, r1 = {a.hi, b.hi}
    const float z = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    const auto q = __builtin_amdgcn_permlane16_swap(__float_as_uint(z), __float_as_uint(z), false, false);       // q0 = {z0, z0, z2, z2}, q1 = {z1, z1, z3, z3}
    return __uint_as_float(q[0]) + __uint_as_float(q[1]);
}
__device__ __forceinline__ float group_max2(float a, float b)
{
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    const float z = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    const auto q = __builtin_amdgcn_permlane16_swap(__float_as_uint(z), __float_as_uint(z), false, false);
    return fmaxf(__uint_as_float(q[0]), __uint_as_float(q[1]));
}

// value of lane group 0's 16-lane row in every lane group (two swaps: 16-lane rows inside a half, then the halves)
__device__ __forceinline__ float bcast_g0(float v)
{
    const auto q = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);      // q0 = {v0, v0, v2, v2}
    unsigned lo, hi;
    halves_u(q[0], lo, hi);
    return __uint_as_float(lo);
}
// value of lane group 1's row in lane groups 0 and 1 (and group 3's in 2 and 3)
__device__ __forceinline__ float from_g1(float v)
{
    const auto q = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);      // q1 = {v1, v1, v3, v3}
    return __uint_as_float(q[1]);
}

// take the SIMD's matrix token (bounded: a stuck token costs speed, never a hang or a pixel) and raise the wave's priority for the matrix phase
__device__ __forceinline__ bool take_matrix_token(int *mtok, int lane)
{
    int got, n = 0;
    do {
        int r = 1;
        if (lane == 0) r = atomicCAS(mtok, 0, 1);
        got = __builtin_amdgcn_readfirstlane(r);
        if (got) __builtin_amdgcn_s_sleep(S16_MSLEEP);
    } while (got && ++n < S16_TOKEN_SPINS);
    __builtin_amdgcn_s_setprio(S16_PRIO_M);
    return !got;
}

// ---- the baked appearance volume (include/tvr.h, BAKED APPEARANCE VOLUME) ----
// One record per grid vertex, (gx+1)(gy+1)(gz+1) records, x fastest, 32 fp32 = 128 B = one cache line.  Slot 8 g + j holds feature row 4 g + j (j < 4) or
// 16 + 4 g + j - 4 (j >= 4): the 32-B segment g of a record is what lane group g holds of an entry as layer 1's base values (FA / FB below), in that order.
// Rows 27..31 (view direction, unused, constant) hold 0: the kernel fills them as it does behind the basis product.
#ifndef S16_VDEPTH
#define S16_VDEPTH 3      // (entry, z layer) units of the volume gather in flight ahead of the one being interpolated (32 registers each): all four, below the matrix phase's register peak
#endif
__host__ __device__ __forceinline__ constexpr int vol_slot_row(int slot) { return (slot & 7) < 4 ? 4 * (slot >> 3) + (slot & 7) : 16 + 4 * (slot >> 3) + (slot & 7) - 4; }

// The features of both entries of a lane's column from the volume: cell and weights of the lane's OWN entry exactly as plane_params forms them (the same unnorm, the
// same floorf: on an upper face the cell is grid - 1 with weight 0 and the +1 corner is the zero padding layer), handed to the other half of the wave by four swaps;
// then per entry four units of one z layer each — 4 corners x 2 float4 of the lane's segment, the four lanes of a column share the corners' lines — and seven lerps
// fmaf(w, b - a, a) per channel: x on the four rows, y on the two layers, z.  32-bit byte offsets against the volume's wave-uniform base (the ABI refuses volumes
// of 4 GiB and more).
__device__ __forceinline__ void vol_features(const float4 *__restrict__ vol, const SceneDev &sc, const float4 &qe, int g, float FA[8], float FB[8])
{
    const float fx = unnorm(qe.x, sc.gm1[0]), fy = unnorm(qe.y, sc.gm1[1]), fz = unnorm(qe.z, sc.gm1[2]);
    const float x0f = floorf(fx), y0f = floorf(fy), z0f = floorf(fz);
    const unsigned gx1 = (unsigned)sc.grid[0] + 1u, gy1 = (unsigned)sc.grid[1] + 1u;
    const unsigned cell = (__umul24((unsigned)(int)z0f, gy1) + (unsigned)(int)y0f) * gx1 + (unsigned)(int)x0f;      // fewer than 2^25 records
    unsigned own = cell * (unsigned)TVR16_VOL_RECORD;
    asm volatile("" : "+v"(own));                      // opaque, as plane_params' offsets: no 64-bit address arithmetic per lane
    unsigned o[2];
    float wx[2], wy[2], wz[2];
    halves_u(own, o[0], o[1]);
    halves_f(fx - x0f, wx[0], wx[1]); halves_f(fy - y0f, wy[0], wy[1]); halves_f(fz - z0f, wz[0], wz[1]);
    const unsigned sy = gx1 * (unsigned)TVR16_VOL_RECORD, sz = sy * gy1;
    o[0] += 32u * (unsigned)g; o[1] += 32u * (unsigned)g;
    struct Unit { float4 c[2][2][2]; };                // [y][x][float4 of the segment]
    auto ld = [](const float4 *base, unsigned byteoff, int imm) { return *(const float4 *)((const unsigned char *)base + (size_t)byteoff + imm); };
    auto issue = [&](Unit &U, int u) {                 // u = 2 entry + z layer
        const unsigned b0 = o[u >> 1] + ((u & 1) ? sz : 0u), b1 = b0 + sy;
        U.c[0][0][0] = ld(vol, b0, 0); U.c[0][0][1] = ld(vol, b0, 16); U.c[0][1][0] = ld(vol, b0, TVR16_VOL_RECORD); U.c[0][1][1] = ld(vol, b0, TVR16_VOL_RECORD + 16);
        U.c[1][0][0] = ld(vol, b1, 0); U.c[1][0][1] = ld(vol, b1, 16); U.c[1][1][0] = ld(vol, b1, TVR16_VOL_RECORD); U.c[1][1][1] = ld(vol, b1, TVR16_VOL_RECORD + 16);
    };
    auto lerp = [](float w, float a0, float a1) { return __builtin_fmaf(w, a1 - a0, a0); };
    auto eval = [&](const Unit &U, float w_x, float w_y, float out[8]) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float a0[4] = {U.c[0][0][q].x, U.c[0][0][q].y, U.c[0][0][q].z, U.c[0][0][q].w}, a1[4] = {U.c[0][1][q].x, U.c[0][1][q].y, U.c[0][1][q].z, U.c[0][1][q].w};
            const float b0[4] = {U.c[1][0][q].x, U.c[1][0][q].y, U.c[1][0][q].z, U.c[1][0][q].w}, b1[4] = {U.c[1][1][q].x, U.c[1][1][q].y, U.c[1][1][q].z, U.c[1][1][q].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) out[4 * q + j] = lerp(w_y, lerp(w_x, a0[j], a1[j]), lerp(w_x, b0[j], b1[j]));
            asm volatile("" : "+v"(out[4 * q]), "+v"(out[4 * q + 1]), "+v"(out[4 * q + 2]), "+v"(out[4 * q + 3]));      // one pin per float4, as eval_unit
        }
    };
    Unit U[S16_VDEPTH + 1];
#pragma unroll
    for (int u0 = 0; u0 < S16_VDEPTH; ++u0) issue(U[u0], u0);
    float lz[2][8];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (u + S16_VDEPTH < 4) issue(U[(u + S16_VDEPTH) % (S16_VDEPTH + 1)], u + S16_VDEPTH);
        eval(U[u % (S16_VDEPTH + 1)], wx[u >> 1], wy[u >> 1], lz[u & 1]);
        if (u & 1) {
            float *F = (u >> 1) ? FB : FA;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
#pragma unroll
                for (int j = 0; j < 4; ++j) F[4 * q + j] = lerp(wz[u >> 1], lz[0][4 * q + j], lz[1][4 * q + j]);
                asm volatile("" : "+v"(F[4 * q]), "+v"(F[4 * q + 1]), "+v"(F[4 * q + 2]), "+v"(F[4 * q + 3]));
            }
        }
        S16_SB;
    }
}

// REF (round 6): REFTensoRF's render path (models/REFTensoRF.py:107-133, 174-256; what configs/Scar.txt:28 runs) on the same tiles.  The four heads on h (normal 3, specular
// tint 1, diffuse 3, rho 1) are a THIRD 16-row block of the basis product — 30 more MFMAs, A fragments from global memory (10 KB, L1 / L2 resident; the LDS is full),
// requested behind the phase boundary and used after the two feature blocks; the normalised normal gives d.n and the reflection direction, which take the places of the
// view direction (base rows 27..29) and of the unused row 30 (-d.n: MLPRender_Fea_Ref's input 0) in layer 1's B operands; the colour is relu(tint) * rgb_s + rgb_d.
// VOL: the scene's baked appearance volume (include/tvr.h, BAKED APPEARANCE VOLUME; launch_appearance_volume below) — the gather phase is vol_features() and the
// basis product with its fragments is absent; everything from layer 1 on is the same text: tvr_shade16_body.inc, included by shade16_kernel and shade16_vol_kernel.
template <bool RC, bool REF>
__global__ __launch_bounds__(S16_THREADS, 2) void shade16_kernel(const SceneDev sc, const ShadeArgs a)
{
    constexpr bool VOL = false;
    constexpr int NW = S16_WAVES, PD = S16_PD;
    constexpr bool TOKEN = true;
    const float4 *const fvol = nullptr;
#include "tvr_shade16_body.inc"
}

template <bool RC>
__global__ __launch_bounds__(S16_VOL_THREADS, 3) void shade16_vol_kernel(const SceneDev sc, const ShadeArgs a, const float4 *__restrict__ fvol)
{
    constexpr bool REF = false, VOL = true;
    constexpr int NW = S16_VOL_WAVES, PD = S16_VOL_PD;
    // A matrix phase alone keeps the vector-issue port 58 % busy (6.0 k issue cycles in 10.3 k: MFMA -> VALU chains, fragment reads), and behind the token a SIMD is in
    // exactly one matrix phase at a time: the gather was hidden already, the slack sat inside the phase.  Three waves without the token fill each other's gaps
    // (profiles/shade_vol_overlap.txt: 10.2 -> 9.3 ms; three waves WITH the token: 10.4).
    constexpr bool TOKEN = false;
#include "tvr_shade16_body.inc"
}

// fvol: the scene's baked appearance volume (tvr_scene_set_appearance_volume: TensorVMSplit scenes only) or nullptr
hipError_t launch_shade16(const SceneDev &sc, const ShadeArgs &a, hipStream_t stream, const float4 *fvol)
{
    const bool rc = sc.range_check != 0, ref = sc.variant == 1;
    if (fvol && ref) return hipErrorInvalidValue;
    const int lds = (fvol ? TVR16_BASH : TVR16_IMAGE_BYTES) + 16;
    const void *kf = fvol ? (rc ? (const void *)shade16_vol_kernel<true> : (const void *)shade16_vol_kernel<false>)
                   : ref  ? (rc ? (const void *)shade16_kernel<true, true> : (const void *)shade16_kernel<false, true>)
                          : (rc ? (const void *)shade16_kernel<true, false> : (const void *)shade16_kernel<false, false>);
    hipError_t e = hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
    unsigned grid = 256;       // one workgroup per CU (the LDS holds the weights), persistent over 32-entry tiles
    if (fvol) {
        if (rc) hipLaunchKernelGGL((shade16_vol_kernel<true>), dim3(grid), dim3(S16_VOL_THREADS), lds, stream, sc, a, fvol);
        else hipLaunchKernelGGL((shade16_vol_kernel<false>), dim3(grid), dim3(S16_VOL_THREADS), lds, stream, sc, a, fvol);
    } else if (ref) {
        if (rc) hipLaunchKernelGGL((shade16_kernel<true, true>), dim3(grid), dim3(S16_THREADS), lds, stream, sc, a);
        else hipLaunchKernelGGL((shade16_kernel<false, true>), dim3(grid), dim3(S16_THREADS), lds, stream, sc, a);
    } else {
        if (rc) hipLaunchKernelGGL((shade16_kernel<true, false>), dim3(grid), dim3(S16_THREADS), lds, stream, sc, a);
        else hipLaunchKernelGGL((shade16_kernel<false, false>), dim3(grid), dim3(S16_THREADS), lds, stream, sc, a);
    }
    return hipGetLastError();
}

// ---- the bake of the appearance volume.  One thread per record, x fastest.  F[row] = sum_k B[row][k] h_k over k = 48 plane + channel in that order, h_k = plane_k * line_k
// (exact in fp64), every term one fp64 FMA, ONE rounding to fp32 at the end.  It reads what the factored kernel reads: the PACKED planes and lines (zero pad texel at index
// grid, zero pad channels: the padding layer of the volume is 0) and basis_mat as the kernel's A operands hold it — the fp16 hi + lo parts of the fragment image
// (pack16_kernel mode 2), whose sum is basis_mat truncated to 22 bits.  The 27 x 144 sums hi + lo sit in LDS as fp64, [k][28]: every lane of a wave reads the same address.
#define VOLB_THREADS 256
#define VOLB_LD 28
__global__ __launch_bounds__(VOLB_THREADS) void appearance_volume_kernel(const SceneDev sc, float4 *__restrict__ out)
{
    __shared__ double Bs[TVR_KAPP * VOLB_LD];
    {
        const unsigned char *img = (const unsigned char *)sc.img16, *basg = (const unsigned char *)sc.basg16;
        for (int i = threadIdx.x; i < TVR_KAPP * VOLB_LD; i += VOLB_THREADS) {
            const int k = i / VOLB_LD, row = i - k * VOLB_LD;
            double w = 0.0;
            if (row < TVR_APPDIM) {                    // pack16_kernel's addresses of (row, k): fragment (s, rb), lane (ci, g), element j
                const int s = k >> 5, gq = (k >> 3) & 3, j = k & 7, rb = row >> 4, ci = row & 15;
                const int off = (s < 4 ? s * TVR16_BAS_STEP : TVR16_BAS_S4) + (rb == 0 ? (gq * 16 + ci) * 16 : (s < 4 ? TVR16_BAS_RB1 : TVR16_BAS_S4_RB1) + (gq * TVR16_BAS_ROWS1 + ci) * 16);
                const __fp16 hi = ((const __fp16 *)(img + TVR16_BASH + off))[j];
                const __fp16 lo = s == 3 ? ((const __fp16 *)(basg + rb * TVR16_FRAG + (gq * 16 + ci) * 16))[j]
                                         : ((const __fp16 *)(img + TVR16_BASL + (s < 3 ? off : off - TVR16_BAS_S4 + TVR16_BASL_S4)))[j];
                w = (double)(float)hi + (double)(float)lo;
            }
            Bs[i] = w;
        }
        __syncthreads();
    }
    const long long gx1 = sc.grid[0] + 1, gy1 = sc.grid[1] + 1, gz1 = sc.grid[2] + 1;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= gx1 * gy1 * gz1) return;
    const long long x = t % gx1, y = (t / gx1) % gy1, z = t / (gx1 * gy1);
    // plane0 (x,y) . line0(z) ; plane1 (x,z) . line1(y) ; plane2 (y,z) . line2(x)   (matMode / vecMode); a texel is 12 float4
    const float4 *P[3] = {sc.aplane[0] + (y * gx1 + x) * 12, sc.aplane[1] + (z * gx1 + x) * 12, sc.aplane[2] + (z * gy1 + y) * 12};
    const float4 *Ln[3] = {sc.aline[0] + z * 12, sc.aline[1] + y * 12, sc.aline[2] + x * 12};
    double acc[TVR_APPDIM];
#pragma unroll
    for (int r = 0; r < TVR_APPDIM; ++r) acc[r] = 0.0;
#pragma unroll 1
    for (int i = 0; i < 3; ++i) {
#pragma unroll 1
        for (int q = 0; q < TVR_CA / 4; ++q) {
            const float4 p = P[i][q], l = Ln[i][q];
            const double h[4] = {(double)p.x * (double)l.x, (double)p.y * (double)l.y, (double)p.z * (double)l.z, (double)p.w * (double)l.w};
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                const double *Bk = Bs + (TVR_CA * i + 4 * q + c4) * VOLB_LD;
#pragma unroll
                for (int r = 0; r < TVR_APPDIM; ++r) acc[r] = __builtin_fma(Bk[r], h[c4], acc[r]);
            }
        }
    }
    float4 *rec = out + t * (TVR16_VOL_RECORD / 16);
#pragma unroll
    for (int q = 0; q < TVR16_VOL_RECORD / 16; ++q) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = vol_slot_row(4 * q + j);
            v[j] = row < TVR_APPDIM ? (float)acc[row < TVR_APPDIM ? row : 0] : 0.0f;
        }
        rec[q] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

hipError_t launch_appearance_volume(const SceneDev &sc, void *out, hipStream_t stream)
{
    const long long n = ((long long)sc.grid[0] + 1) * ((long long)sc.grid[1] + 1) * ((long long)sc.grid[2] + 1);      // fewer than 2^25 records (the volume stays below 4 GiB)
    hipLaunchKernelGGL(appearance_volume_kernel, dim3((unsigned)((n + VOLB_THREADS - 1) / VOLB_THREADS)), dim3(VOLB_THREADS), 0, stream, sc, (float4 *)out);
    return hipGetLastError();
}

// ---- weights -> the fragment images (tvr_device.h, TVR16_*).  One thread per (fragment, lane, j). ----
//  mode 0: W1 [5][8] fragments; mode 1: W2 [4][8]; mode 2: basis [5][2] (compact, hi -> the image, lo -> the image or the global k-step-3 fragments)
//  mode 3 (REFTensoRF): the heads' fragments -> refg [5 k-steps][hi | lo] as full fragments: row ci < 8 = {normal 0..2, specular, diffuse 0..2, rho}, k natural as mode 2
struct RefHeads { const float *W[4]; };      // tvr_scene_params.ref_W order: normal [3,144], diffuse [3,144], specular [1,144], rho [1,144]
__global__ __launch_bounds__(256) void pack16_kernel(const float *__restrict__ W, const float *__restrict__ bias, unsigned char *__restrict__ img,
                                                     unsigned char *__restrict__ basg, int mode, const MlpShape sh, const RefHeads rh, int ref)
{
    const int nfr = mode == 0 ? 40 : (mode == 1 ? 32 : (mode == 3 ? 5 : 10));
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nfr * 512) return;
    const int fr = i >> 9, lane = (i >> 3) & 63, j = i & 7, ci = lane & 15, g = lane >> 4;
    float w = 0.0f;
    unsigned short *ph = nullptr, *pl = nullptr;
    if (mode == 0) {
        const int s = fr >> 3, rb = fr & 7, row = 16 * rb + ci, ii = 8 * s + j, r = ii / 5, t = ii % 5;
        const int cbase = r < 4 ? 4 * g + r : 16 + 4 * g + (r - 4);
        int idx = ref_in_index(cbase, t, sh.fea_pe, sh.view_pe);
        if (ref) idx = cbase == 30 ? (t == 0 ? 0 : -1) : (idx >= 0 ? idx + 1 : -1);        // MLPRender_Fea_Ref (REFTensoRF.py:19-24): input 0 is the dot product, everything else moves up by one
        if (idx >= 0 && row < sh.featureC) w = W[(size_t)row * sh.n_in + idx];
        if (cbase == 31 && t == 0 && row < sh.featureC) w = bias[row];          // the constant-1 input: b1 rides in the weight image
        ph = (unsigned short *)(img + TVR16_W1H + fr * TVR16_FRAG + lane * 16) + j;
        pl = (unsigned short *)(img + TVR16_W1L + fr * TVR16_FRAG + lane * 16) + j;
    } else if (mode == 1) {
        const int s = fr >> 3, rb = fr & 7, row = 16 * rb + ci;
        const int u = j < 4 ? 32 * s + 4 * g + j : 32 * s + 16 + 4 * g + (j - 4);
        if (row < sh.featureC && u < sh.featureC) w = W[(size_t)row * sh.featureC + u];
        ph = (unsigned short *)(img + TVR16_W2H + fr * TVR16_FRAG + lane * 16) + j;
        pl = (unsigned short *)(img + TVR16_W2L + fr * TVR16_FRAG + lane * 16) + j;
    } else if (mode == 3) {
        const int s = fr, k = 32 * s + 8 * g + j;
        if (k < TVR_KAPP && ci < 8) {
            const float *Wh = ci < 3 ? rh.W[0] + (size_t)ci * TVR_KAPP : (ci == 3 ? rh.W[2] : (ci < 7 ? rh.W[1] + (size_t)(ci - 4) * TVR_KAPP : rh.W[3]));
            w = Wh[k];
        }
        ph = (unsigned short *)(basg + (2 * s) * TVR16_FRAG + lane * 16) + j;          // (`basg` is the heads' buffer in this mode)
        pl = (unsigned short *)(basg + (2 * s + 1) * TVR16_FRAG + lane * 16) + j;
    } else {
        // k slot (s, g, j) = 32 s + 8 g + j, the kernels' natural k = 48 * plane + channel (k-step 4: groups 0, 1 only — the kernel reads zeros in groups 2, 3)
        const int s = fr >> 1, rb = fr & 1, row = 16 * rb + ci, k = 32 * s + 8 * g + j;
        if (k < TVR_KAPP && row < TVR_APPDIM) {
            const int pl_ = k / TVR_CA, ch = k - pl_ * TVR_CA;                  // basis_mat's column = its plane's offset + channel
            if (ch < sh.app_n_comp[pl_]) w = W[(size_t)row * sh.k_app + sh.app_off[pl_] + ch];
        }
        const bool in_img = (rb == 0 || ci < TVR16_BAS_ROWS1) && (s < 4 || g < 2);
        const int off = (s < 4 ? s * TVR16_BAS_STEP : TVR16_BAS_S4) + (rb == 0 ? (g * 16 + ci) * 16 : (s < 4 ? TVR16_BAS_RB1 : TVR16_BAS_S4_RB1) + (g * TVR16_BAS_ROWS1 + ci) * 16);
        if (in_img) {
            ph = (unsigned short *)(img + TVR16_BASH + off) + j;
            if (s != 3) pl = (unsigned short *)(img + TVR16_BASL + (s < 3 ? off : off - TVR16_BAS_S4 + TVR16_BASL_S4)) + j;
        }
        if (s == 3) pl = (unsigned short *)(basg + rb * TVR16_FRAG + lane * 16) + j;       // full fragments: rows >= 27 are zero
    }
    unsigned hi, lo;
    split2(w, 0.0f, hi, lo);
    if (ph) *ph = (unsigned short)hi;
    if (pl) *pl = (unsigned short)lo;
}

// the heads' biases as the initial accumulators of the third row block: [4 groups][4 rows] floats behind the ten fragments (groups 2, 3: zeros)
__global__ void pack16_ref_bias_kernel(const float *__restrict__ bn, const float *__restrict__ bd, const float *__restrict__ bs, const float *__restrict__ br, float *__restrict__ out)
{
    const int i = threadIdx.x;
    if (i >= 16) return;
    out[i] = i < 3 ? bn[i] : (i == 3 ? bs[0] : (i < 7 ? bd[i - 4] : (i == 7 ? br[0] : 0.0f)));
}

hipError_t launch_pack16(const float *W1, const float *b1, const float *W2, const float *b2, const float *W3, const float *b3, const float *basis, void *img, void *basg,
                         const MlpShape &sh, hipStream_t stream, const float *const *ref_W, const float *const *ref_b, void *refg)
{
    unsigned char *im = (unsigned char *)img;
    hipError_t e;
    // b2, b3, W3, the zero bytes (hidden units >= featureC stay zero), then the copies — as kernels: tvr_scene_update runs inside captured training steps (tvr_step.hip)
    if ((e = launch_zero_f32((float *)(im + TVR16_B2), (TVR16_BASH - TVR16_B2) / 4, stream)) != hipSuccess) return e;
    if ((e = launch_copy_f32((float *)(im + TVR16_B2), b2, sh.featureC, stream)) != hipSuccess) return e;
    if ((e = launch_copy_f32((float *)(im + TVR16_B3), b3, 3, stream)) != hipSuccess) return e;
    for (int r = 0; r < 3; ++r)
        if ((e = launch_copy_f32((float *)(im + TVR16_W3 + r * 512), W3 + (size_t)r * sh.featureC, sh.featureC, stream)) != hipSuccess) return e;
    RefHeads rh = {{nullptr, nullptr, nullptr, nullptr}};
    const int ref = refg != nullptr;
    if (ref) for (int i = 0; i < 4; ++i) rh.W[i] = ref_W[i];
    hipLaunchKernelGGL(pack16_kernel, dim3(40 * 512 / 256), dim3(256), 0, stream, W1, b1, im, (unsigned char *)basg, 0, sh, rh, ref);
    hipLaunchKernelGGL(pack16_kernel, dim3(32 * 512 / 256), dim3(256), 0, stream, W2, nullptr, im, (unsigned char *)basg, 1, sh, rh, ref);
    hipLaunchKernelGGL(pack16_kernel, dim3(10 * 512 / 256), dim3(256), 0, stream, basis, nullptr, im, (unsigned char *)basg, 2, sh, rh, ref);
    if (ref) {
        hipLaunchKernelGGL(pack16_kernel, dim3(5 * 512 / 256), dim3(256), 0, stream, nullptr, nullptr, im, (unsigned char *)refg, 3, sh, rh, ref);
        hipLaunchKernelGGL(pack16_ref_bias_kernel, dim3(1), dim3(64), 0, stream, ref_b[0], ref_b[1], ref_b[2], ref_b[3], (float *)((unsigned char *)refg + 10 * TVR16_FRAG));
    }
    return hipGetLastError();
}
