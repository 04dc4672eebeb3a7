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
// After the trim (profiles/march_trim.txt) the plain form holds 39 registers and the shape was measured again on the frame in pieces: 1 x 16 waves 12.76 - 12.77 ms,
// 1 x 8 13.5, 2 x 8 13.3, 2 x 16 14.1.  The launch bound now matters for the SCALAR file: bound (1024, 7) gives the plain form 96 SGPRs and no spill, and the frame
// 13.95 ms instead of 12.5 — the ten values that spill under (1024, 8) are all outside the chunk loop and stay spilled.
// With the queue reservations batched (MARCH_BATCH below; profiles/march_batch.txt) the kernel is no longer pinned by the queue counter's line — which is why it had
// ignored occupancy — and the shape and the hand-out word were measured once more on the frame in pieces: 1 x 16 waves 11.86 - 11.99 ms (kept), 1 x 8 12.06 - 12.10, 2 x 8
// 12.00 - 12.20, 2 x 16 12.31 - 12.33; MARCH_CTR_WORD 32 11.78 - 12.02 (inside the spread: word 1 stays, although the march ALONE gains 0.3 ms with its hand-out on a
// line of its own, 2.46 -> 2.15 ms).  One group of 16 waves wins by less than before, and 2 x 16 still loses to the co-scheduled shade kernel.
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

// The plain form of the volume march (march_vol_kernel<false, true>: no alpha volume, no explicit depths, no lam6, a volume below 4 GiB — launch_march_vol checks) is
// compiled without those paths; kernels that do not name PLAIN themselves (march_kernel, cp_march_kernel) see this `false`.
constexpr bool PLAIN = false;

// Queue reservations of the volume marches (march_vol_kernel, all three forms).  A returning atomicAdd on the queue counter per ray with appearance samples pinned
// the kernel: 384 000 of them per bench frame plus 40 000 tile hand-outs on one 128-byte line, at the ~88 per microsecond one word sustains, are 4.8 ms of a 4.95 ms
// kernel (profiles/march_batch.txt, block A: 1.63 ms with the reservations off that line).  So a wave keeps the lists of up to MARCH_PEND finished rays in the list
// it already owns (bufw / bufj: a RING of s_cap entries, the ray in progress appending at the tail) and reserves ONCE for all of them:
//   - a ray's record {o, d, tmin, jitter, ray, first entry within the batch} waits in LDS (MARCH_PEND_WORDS words; MARCH_PEND of them per wave) — not in scalar
//     registers, which the chunk loop has none to spare of (the scalar budget above);
//   - the flush adds the batch's total to the counter, writes ray_off of its rays and the entries: a lane finds its entry's ray by comparing its index with the
//     <= MARCH_PEND first-entry numbers, and recomputes q_pos from the record with the expressions (and therefore the bits) of the unbatched write;
//   - it runs when MARCH_PEND rays wait, when the ray in progress needs room the waiting rays hold (a ray alone never exceeds s_cap, so it fits afterwards and nothing
//     is copied), and behind the ray loop, which every exit — queue exhausted, both fault breaks — leaves through.
// acc, depth, ray_cnt (and ray_off = 0 of a ray without entries) are written when the ray ends, as before.  The queue stays contiguous, *counter exact, a ray's
// segment contiguous and in sample order; only the order of the segments changes, which already depended on which wave finished first.
// Kernels that do not name MARCH_BATCH themselves (march_kernel, cp_march_kernel) see this `false` and compile to what they were; march_vol_kernel names it after its BATCH
// parameter, which launch_march_vol sets for launches with more rays than waves (tvr_march.hip).
constexpr bool MARCH_BATCH = false;
#define MARCH_PEND 8                      // rays per reservation at most
#define MARCH_PEND_WORDS 12               // a waiting ray's record, 32-bit words: o[3], d[3], tmin, jitter, ray, first entry, 2 of padding

// What a march touches once per ray — the ray and jitter arrays in front of the chunk loop, the outputs behind it — costs the chunk loop scalar registers for nothing:
// kernel arguments are loaded at the kernel's entry and stay live (march_vol_kernel<false> kept 100 of them in spilled lanes, 40 v_readlane_b32 inside the chunk loop).
// The plain form reads these pointers from the kernel-argument segment where it uses them: MarchVolArgs restates march_vol_kernel's parameter list (arguments are
// laid out like the members of a struct), and the empty asm keeps the loads from being hoisted back out of the ray loop.  Every other kernel takes its arguments.
struct MarchVolArgs {
    SceneDev sc;
    const float *dvol, *rays;
    int n_rays, S, s_cap;
    MarchSampling sm;
    float eps_T;
    MarchOut mo;
    tvr_dense_out dn;
};
template <bool ON_DEMAND, typename T>
__device__ __forceinline__ T march_arg_now(const T &arg, unsigned offset)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (ON_DEMAND) {
        const __attribute__((address_space(4))) unsigned char *ka = (const __attribute__((address_space(4))) unsigned char *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        return *(const __attribute__((address_space(4))) T *)(ka + offset);
    }
#endif
    return arg;
}

// vol_density for a volume below 4 GiB: the same four loads and seven lerps, addressed as vm_term_lds addresses its planes — ONE opaque 32-bit byte offset per sample
// against four wave-uniform row bases r00 = D, r01 = D + sy, r10 = D + sz, r11 = D + sz + sy (global_load_dwordx2 v, v_off, s[base]); no 64-bit VALU.  The row number
// iz (gy + 1) + iy has both factors below 2^24 (grid <= 4096); its product with gx + 1 is a full 32-bit multiply, since a flat volume's row count may pass 2^24.
__device__ __forceinline__ float vol_density32(const unsigned char *r00, const unsigned char *r01, const unsigned char *r10, const unsigned char *r11, unsigned gx1,
                                               unsigned gy1, int ix, int iy, int iz, float wx, float wy, float wz)
{
    const unsigned row = __umul24((unsigned)iz, gy1) + (unsigned)iy;
    unsigned o = (row * gx1 + (unsigned)ix) << 2;
    asm volatile("" : "+v"(o));                                                           // opaque: hipcc otherwise widens the sums back into 64-bit arithmetic
    const vol_pair p00 = *(const vol_pair *)(r00 + (size_t)o), p01 = *(const vol_pair *)(r01 + (size_t)o);
    const vol_pair p10 = *(const vol_pair *)(r10 + (size_t)o), p11 = *(const vol_pair *)(r11 + (size_t)o);
    const float c00 = __builtin_fmaf(wx, p00.b - p00.a, p00.a), c01 = __builtin_fmaf(wx, p01.b - p01.a, p01.a);
    const float c10 = __builtin_fmaf(wx, p10.b - p10.a, p10.a), c11 = __builtin_fmaf(wx, p11.b - p11.a, p11.a);
    const float c0 = __builtin_fmaf(wy, c01 - c00, c00), c1 = __builtin_fmaf(wy, c11 - c10, c10);
    return __builtin_fmaf(wz, c1 - c0, c0);
}

// exp and softplus of the volume marches (all three forms, so that one scene has one evaluator).  The arguments are bounded where they are used — softplus takes the
// branch below only for x <= 20, and -sigma * dist <= 0, where underflow to 0 is the right answer — so OCML's range clamps and its double-float log1pf (some 110
// instructions) are not needed:
//   march_expf   OCML's own expf without the clamps: p = x log2(e), the fma-compensated low part, v_exp_f32 of the reduced argument, v_ldexp_f32 — the same bits as
//                expf for every finite x <= 88.7
//   march_softplus   log1p(t), t = e^x in (0, e^20]: u = 1 + t, d = u - 1 (exact), log(u) (t / d) — the rounding of 1 + t cancels in the quotient; v_log_f32, and
//                v_rcp_f32 with one residual step for t / d.  d == 0 (x < -16.6): log1p(t) = t to fp32.  x > 20 as softplus_f.
#ifndef MARCH_VOL_LEAN
#define MARCH_VOL_LEAN 1                  // 0: the volume marches call expf / softplus_f like every other kernel (the stage that changes no bit)
#endif
__device__ __forceinline__ float march_expf(float x)
{
    const float p = x * 0x1.715476p+0f;
    const float r = __builtin_rintf(p);
    float lo = __builtin_fmaf(x, 0x1.715476p+0f, -p);
    lo = __builtin_fmaf(x, 0x1.4ae0bep-26f, lo);
    return __builtin_ldexpf(__builtin_amdgcn_exp2f((p - r) + lo), (int)r);
}
__device__ __forceinline__ float march_softplus(float x)
{
    if (x > 20.0f) return x;
    const float t = march_expf(x);
    const float u = 1.0f + t, d = u - 1.0f;
    const float rc = __builtin_amdgcn_rcpf(d);
    float q = t * rc;
    q = __builtin_fmaf(__builtin_fmaf(-d, q, t), rc, q);
    const float lg = __builtin_amdgcn_logf(u) * 0x1.62e430p-1f;
    return d == 0.0f ? t : lg * q;
}

// The transmittance scan of the volume marches: x[l] <- x[l] * x[l - off] for off = 1, 2, 4, 8, 16, 32 and the lanes l >= off (Hillis-Steele) — the recurrence, the
// operands and their order of the __shfl_up form the factored marches keep, so every product has the same bits — with the data moved inside the register file instead
// of through eight ds_bpermute_b32 round trips.  A lane below `off` multiplies by 1.0f (exact: fp32 denormals are kept) instead of being skipped.
//   off 1 - 8   v_mov_b32_dpp wave_shr:1, off times: it carries across the 16-lane rows, which row_shr does not; lane 0 keeps `old` = 1.0f
//   off 16      v_permlane16_swap(x, x) = {r0 r0 r2 r2 | r1 r1 r3 r3} (rows r0 .. r3 of x), v_permlane32_swap of the two = {r0 r0 r1 r1 | r2 r2 r3 r3}: rows 1, 2
//               take the latter's first word, row 3 the former's (r2), row 0 keeps 1.0f (row-masked moves)   (profiles/r05_permlane_semantics.txt)
//   off 32      v_permlane32_swap(x, x) = {lo lo | hi hi}: the upper half takes the first
// excl = the scan shifted up one lane (lane 0: 1.0f); last = lane 63's value (v_readlane_b32).
#define MARCH_DPP_WAVE_SHR1 0x138
#define MARCH_DPP_SAME 0xE4                 // quad_perm:[0,1,2,3]
template <int CTRL, int ROWS>
__device__ __forceinline__ float march_dpp_mov(float old, float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, ROWS, 0xF, false));
}
// v shifted up N lanes, 1.0f in the lanes below N: the first move puts 1.0f into lane 0, the others run in place, where lane 0 keeps what it holds
template <int N>
__device__ __forceinline__ float march_up(float v)
{
    float t = march_dpp_mov<MARCH_DPP_WAVE_SHR1, 0xF>(1.0f, v);
#pragma unroll
    for (int i = 1; i < N; ++i) t = march_dpp_mov<MARCH_DPP_WAVE_SHR1, 0xF>(t, t);
    return t;
}
__device__ __forceinline__ void scan_mul_dpp(float &x, float &excl, float &last)
{
    x = x * march_up<1>(x);
    x = x * march_up<2>(x);
    x = x * march_up<4>(x);
    x = x * march_up<8>(x);
    {
        const auto q = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
        const auto s = __builtin_amdgcn_permlane32_swap(q[0], q[1], false, false);        // {r0 r0 r1 r1 | r2 r2 r3 r3}
        float t = march_dpp_mov<MARCH_DPP_SAME, 0x6>(1.0f, __uint_as_float(s[0]));
        t = march_dpp_mov<MARCH_DPP_SAME, 0x8>(t, __uint_as_float(q[0]));
        x = x * t;
    }
    {
        const auto h = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
        x = x * march_dpp_mov<MARCH_DPP_SAME, 0xC>(1.0f, __uint_as_float(h[0]));
    }
    excl = march_up<1>(x);
    last = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}

// The flush of MARCH_BATCH (above): one reservation for the n_pend rays whose entries stand at [ring_head, ring_head + pend_total) of the wave's ring, then their ray_off
// and entries.  The three numbers are the same in every lane (the body keeps them in vector registers); they come back as the empty set behind the flushed entries.
template <bool PLAIN_F>
__device__ __forceinline__ void march_flush(const SceneDev &sc, const MarchSampling &sm, const MarchOut &mo, const int S, const int s_cap, const int lane, const float *bufw,
                                            const unsigned short *bufj, const float *pend, int &ring_head, int &pend_total, int &n_pend)
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const MarchOut mf = march_arg_now<PLAIN_F>(mo, offsetof(MarchVolArgs, mo));
    const bool jit_f = march_arg_now<PLAIN_F>(sm.jitter, offsetof(MarchVolArgs, sm.jitter)) != nullptr;
    const int f_total = __builtin_amdgcn_readfirstlane(pend_total), f_rays = __builtin_amdgcn_readfirstlane(n_pend), f_head = __builtin_amdgcn_readfirstlane(ring_head);
    unsigned fbase = 0;
    if (lane == 0) fbase = atomicAdd(mf.counter, (unsigned)f_total);          // ONE reservation for the f_rays rays
    fbase = __builtin_amdgcn_readfirstlane(fbase);
    if (lane < f_rays) mf.ray_off[__float_as_uint(pend[lane * MARCH_PEND_WORDS + 8])] = fbase + __float_as_uint(pend[lane * MARCH_PEND_WORDS + 9]);
    for (int i = lane; i < f_total; i += 64) {
        int k = 0;                                                            // the ray of entry i: the last one whose first entry is <= i
        for (int m = 1; m < f_rays; ++m) k += (unsigned)i >= __float_as_uint(pend[m * MARCH_PEND_WORDS + 9]) ? 1 : 0;
        const float *rec = pend + k * MARCH_PEND_WORDS;
        int rp = f_head + i;
        if (rp >= s_cap) rp -= s_cap;
        const unsigned ej = bufj[rp];
        const unsigned eray = __float_as_uint(rec[8]);
        float fj = (float)ej;
        if (jit_f) fj = fj + rec[7];
        const float *__restrict__ zr = (!PLAIN_F && sm.zv) ? sm.zv + (size_t)eray * S : nullptr;
        const float z = zr ? zr[ej] : rec[6] + sc.step * fj;
        float4 qv;
        qv.x = ((rec[0] + rec[3] * z) - sc.lo[0]) * sc.inv[0] - 1.0f;
        qv.y = ((rec[1] + rec[4] * z) - sc.lo[1]) * sc.inv[1] - 1.0f;
        qv.z = ((rec[2] + rec[5] * z) - sc.lo[2]) * sc.inv[2] - 1.0f;
        qv.w = bufw[rp];
        mf.q_pos[fbase + i] = qv;
        mf.q_ray[fbase + i] = eray;
        if (mf.q_j) mf.q_j[fbase + i] = ej;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    ring_head = f_head + f_total >= s_cap ? f_head + f_total - s_cap : f_head + f_total;
    pend_total = 0;
    n_pend = 0;
    asm volatile("" : "+v"(ring_head), "+v"(pend_total), "+v"(n_pend));
}
