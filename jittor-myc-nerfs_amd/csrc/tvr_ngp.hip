// tvr_ngp.hip — the alt path: JNeRF Instant-NGP inference on MI355X.  Kernels + the C-ABI of include/tvr_ngp.h.
//
//   ngp_march_kernel          one lane per ray: AABB slab test, jittered start (PCG32), occupancy-bitfield march ONCE, recording each
//                             step's t; an exclusive scan hands out bases IN RAY ORDER; ngp_expand_kernel (one wave per ray) writes the rows.
//   ngp_field_kernel          fused NGPNetworks.execute_: per wave 32 samples at a time; each half-wave gathers the even / odd hash
//                             levels of its 32 samples (8 corners x float2), and the five bias-free Linears run as fp32 MFMAs
//                             (v_mfma_f32_32x32x2_f32) with activations register-resident between layers: the accumulator layout
//                             of one layer IS the B-operand layout of the next once the k index is paired (r, r+4), and that
//                             pairing is folded into the packed weight image (LDS, one ds_read_b32 per MFMA).
//   ngp_composite_kernel      compute_rgbs_inference: one lane per ray over its contiguous rows.
//   ngp_render_kernel         the whole frame in one kernel after the march (tvr_ngp_render): a wave walks a ray's recorded steps 32 at a
//                             time through the same field_tile code and composites in order, stopping at the compositor's T < 1e-4 break.
//   + stand-alone hash / SH encoders (the reference's separate ops) and update_bitfield.
//
// Compiled with -ffp-contract=off; FMAs are explicit where the reference's compiler contracts (see oracle/ngp_oracle.c header).
#include "tvr_ngp_field.h"
#include "tvr_ngp_composite.h"


// ------------------------------------------------------------------------------------------------ march helpers
struct MarchCfg {
    float lo[3], hi[3];
    float near_distance, cone_angle;
    int const_dt;
    uint64_t rng_state, rng_inc;
    uint32_t slab_rays;
};

__device__ __forceinline__ float max_cone_step() { return min_cone_step() * 16.0f * 1024.0f / 128.0f; }
__device__ __forceinline__ float calc_dt(const MarchCfg &c, float t)
{
    if (c.const_dt) return min_cone_step() * 0.5f;
    const float v = t * c.cone_angle;
    return v < min_cone_step() ? min_cone_step() : (max_cone_step() < v ? max_cone_step() : v);
}
__device__ __forceinline__ int mip_from_dt(float dt, float x, float y, float z)
{
    const int mip = mip_from_pos(x, y, z);
    dt *= (float)(2 * NGP_G);
    if (dt < 1.f) return mip;
    return min(TVR_NGP_CASCADES - 1, max(frexp_exponent(dt), mip));
}
__device__ __forceinline__ float dist_axis(float pos, float dir, float idir, float res)
{
    const float p = res * pos;
    return (floorf(p + 0.5f + 0.5f * copysignf(1.0f, dir)) - p) * idir;
}

// `do { t += dt; } while (t < target);` with a constant dt (advance_to_next_voxel, ray_sampler_header.h:739-753, const_dt mode), in closed
// form and bit for bit.  While t stays inside one binade (ulp u, t = M u with 2^23 <= M < 2^24) every fp32 addition of dt adds the same
// integer q = RN(dt / u) to M, so the loop's j-th value is (M + j q) u and the first one >= target follows from one division.  The
// addition that leaves the binade is done by the hardware (it rounds at the coarser ulp), then the next binade is handled the same
// way.  Ties (dt / u ending in exactly .5: round-to-even then depends on M's parity), non-finite or non-positive operands and
// exponents outside the comfortable range take the plain additions.  Empty space costs a few dozen instructions per voxel instead of
// ~150 dependent additions per coarse voxel.
__device__ __forceinline__ float advance_const(float t, float target, float dt)
{
    t += dt;
    const uint32_t db = __float_as_uint(dt), m_dt = (db & 0x7fffffu) | 0x800000u;
    const int e_dt = (int)((db >> 23) & 0xff);
    while (t < target) {
        const uint32_t tb = __float_as_uint(t), gb = __float_as_uint(target);
        const int e = (int)((tb >> 23) & 0xff), eg = (int)((gb >> 23) & 0xff), s = e - e_dt;
        bool fast = (tb >> 31) == 0 && (gb >> 31) == 0 && e > 0 && e < 0xfe && eg != 0xff && s >= 1 && s <= 22 && e_dt > 0;
        uint32_t q = 0;
        if (fast) {
            const uint32_t rem = m_dt & ((1u << s) - 1u), half = 1u << (s - 1);
            q = (m_dt >> s) + (rem > half ? 1u : 0u);
            fast = rem != half && q > 0;
        }
        if (!fast) {
            t += dt;
            continue;
        }
        const uint32_t M = (tb & 0x7fffffu) | 0x800000u;
        const uint32_t j_stay = (0xffffffu - M) / q;               // most additions that keep M + j q <= 2^24 - 1
        uint32_t j = 0xffffffffu;                                   // target beyond this binade
        if (eg == e) j = (((gb & 0x7fffffu) | 0x800000u) - M + q - 1u) / q;
        if (j <= j_stay) return __uint_as_float((tb & 0xff800000u) | ((M + j * q) & 0x7fffffu));
        t = __uint_as_float((tb & 0xff800000u) | ((M + j_stay * q) & 0x7fffffu));
        t += dt;                                                    // the addition that crosses into the next binade
    }
    return t;
}

struct RayState {
    float o[3], d[3], idir[3];
};

// rays_sampler's march (its two while loops are the same walk): every occupied step's t goes to the ray's slab; returns the step count
__device__ __forceinline__ uint32_t march_ray(const MarchCfg &c, const RayState &r, const uint8_t *__restrict__ bits, float startt, float *__restrict__ tslab)
{
    uint32_t j = 0;
    float t = startt;
    for (;;) {
        const float x = __builtin_fmaf(t, r.d[0], r.o[0]), y = __builtin_fmaf(t, r.d[1], r.o[1]), z = __builtin_fmaf(t, r.d[2], r.o[2]);
        const bool inside = x >= c.lo[0] && x <= c.hi[0] && y >= c.lo[1] && y <= c.hi[1] && z >= c.lo[2] && z <= c.hi[2];
        if (!(inside && j < (uint32_t)TVR_NGP_STEPS)) break;
        const float dt = calc_dt(c, t);
        const uint32_t mip = (uint32_t)mip_from_dt(dt, x, y, z);
        if (occupied_at(x, y, z, bits, mip)) {
            tslab[j] = t;
            ++j;
            t += dt;
        } else {
            const float res = (float)(NGP_G >> mip);
            const float tx = dist_axis(x, r.d[0], r.idir[0], res), ty = dist_axis(y, r.d[1], r.idir[1], res), tz = dist_axis(z, r.d[2], r.idir[2], res);
            const float t_target = t + fmaxf(fminf(fminf(tx, ty), tz) / res, 0.0f);
            if (c.const_dt) {
                t = advance_const(t, t_target, calc_dt(c, t));
            } else {
                do {
                    t += calc_dt(c, t);
                } while (t < t_target);
            }
        }
    }
    return j;
}

__device__ __forceinline__ float ray_entry(const MarchCfg &c, const RayState &r)
{
    float tmin = (c.lo[0] - r.o[0]) / r.d[0], tmax = (c.hi[0] - r.o[0]) / r.d[0], s;
    if (tmin > tmax) { s = tmin; tmin = tmax; tmax = s; }
    float tymin = (c.lo[1] - r.o[1]) / r.d[1], tymax = (c.hi[1] - r.o[1]) / r.d[1];
    if (tymin > tymax) { s = tymin; tymin = tymax; tymax = s; }
    if (tmin > tymax || tymin > tmax) return FLT_MAX;
    if (tymin > tmin) tmin = tymin;
    if (tymax < tmax) tmax = tymax;
    float tzmin = (c.lo[2] - r.o[2]) / r.d[2], tzmax = (c.hi[2] - r.o[2]) / r.d[2];
    if (tzmin > tzmax) { s = tzmin; tzmin = tzmax; tzmax = s; }
    if (tmin > tzmax || tzmin > tmax) return FLT_MAX;
    if (tzmin > tmin) tmin = tzmin;
    return tmin;
}

__device__ __forceinline__ void load_ray(const float *__restrict__ rays_o, const float *__restrict__ rays_d, long long i, RayState &r)
{
    for (int k = 0; k < 3; ++k) {
        r.o[k] = rays_o[3 * i + k];
        r.d[k] = rays_d[3 * i + k];
        r.idir[k] = 1.0f / r.d[k];
    }
}

// the march: step count of every ray, and the t of every step in the ray's 1024-float slab
__global__ void __launch_bounds__(256) ngp_march_kernel(MarchCfg c, const float *__restrict__ rays_o, const float *__restrict__ rays_d, long long n_rays,
                                                        const uint8_t *__restrict__ bits, uint32_t *__restrict__ counts, float *__restrict__ tslab)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays) return;
    RayState r;
    load_ray(rays_o, rays_d, i, r);
    Pcg rng = {c.rng_state, c.rng_inc};
    // N_MAX_RANDOM_SAMPLES_PER_RAY = 8 draws reserved per ray; one 2^32 advance of the global generator per slab of rays
    const uint32_t slab = c.slab_rays ? (uint32_t)(i / c.slab_rays) : 0u, in_slab = c.slab_rays ? (uint32_t)(i % c.slab_rays) : (uint32_t)i;
    pcg_advance(rng, ((uint64_t)slab << 32) + (uint64_t)(uint32_t)(in_slab * 8u));
    float t0 = fmaxf(ray_entry(c, r), c.near_distance);
    t0 = __builtin_fmaf(calc_dt(c, t0), pcg_float(rng), t0);
    counts[i] = march_ray(c, r, bits, t0, tslab + (size_t)i * TVR_NGP_STEPS);
}

// exclusive scan of counts in ray order: (a) per 1024-ray block, (b) the block totals, (c) folded into pass 2
__global__ void __launch_bounds__(1024) ngp_scan_block_kernel(const uint32_t *__restrict__ counts, long long n, uint32_t *__restrict__ local, uint32_t *__restrict__ block_sum)
{
    __shared__ uint32_t wsum[16];
    const long long i = (long long)blockIdx.x * 1024 + threadIdx.x;
    const uint32_t v = i < n ? counts[i] : 0u;
    uint32_t s = v;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(s, d, 64);
        if (lane >= d) s += u;
    }
    if (lane == 63) wsum[w] = s;
    __syncthreads();
    uint32_t before = 0;
    for (int k = 0; k < w; ++k) before += wsum[k];
    if (i < n) local[i] = before + s - v;
    if (threadIdx.x == 1023) block_sum[blockIdx.x] = before + s;
}
__global__ void __launch_bounds__(1024) ngp_scan_top_kernel(uint32_t *__restrict__ block_sum, int n_blocks, uint32_t *__restrict__ total)
{
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int base = 0; base < n_blocks; base += 1024) {
        const int i = base + threadIdx.x;
        const uint32_t v = i < n_blocks ? block_sum[i] : 0u;
        uint32_t s = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t u = __shfl_up(s, d, 64);
            if (lane >= d) s += u;
        }
        if (lane == 63) wsum[w] = s;
        __syncthreads();
        uint32_t before = carry;
        for (int k = 0; k < w; ++k) before += wsum[k];
        if (i < n_blocks) block_sum[i] = before + s - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = before + s;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// rows from the recorded t: one wave per ray, lane j writes row base+j (consecutive rows: the stores of a wave cover one contiguous
// span).  Also numsteps and the "got a slab" flag whose scan gives ray_index (rank among rays with a slab; informational, unused by
// inference).
__global__ void __launch_bounds__(256) ngp_expand_kernel(MarchCfg c, const float *__restrict__ rays_o, const float *__restrict__ rays_d, long long n_rays,
                                                         const uint32_t *__restrict__ counts, const float *__restrict__ tslab, const uint32_t *__restrict__ local,
                                                         const uint32_t *__restrict__ block_sum, long long max_samples, float *__restrict__ coords,
                                                         int *__restrict__ numsteps, uint32_t *__restrict__ got_slab)
{
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n_rays) return;
    const uint32_t n = counts[i];
    const uint32_t base = local[i] + block_sum[i >> 10];
    const bool over = (long long)base + n > max_samples;
    if (lane == 0) {
        numsteps[2 * i] = over ? 0 : (int)n;
        numsteps[2 * i + 1] = (int)base;
        if (got_slab) got_slab[i] = over ? 0u : 1u;
    }
    if (over || n == 0) return;
    const float o0 = rays_o[3 * i], o1 = rays_o[3 * i + 1], o2 = rays_o[3 * i + 2], d0 = rays_d[3 * i], d1 = rays_d[3 * i + 1], d2 = rays_d[3 * i + 2];
    const float w0 = (d0 + 1.0f) * 0.5f, w1 = (d1 + 1.0f) * 0.5f, w2 = (d2 + 1.0f) * 0.5f;
    const float max_step = min_cone_step() * 16.0f;
    const float *ts = tslab + (size_t)i * TVR_NGP_STEPS;
    for (uint32_t j = lane; j < n; j += 64) {
        const float t = ts[j];
        const float x = __builtin_fmaf(t, d0, o0), y = __builtin_fmaf(t, d1, o1), z = __builtin_fmaf(t, d2, o2);
        float *q = coords + 7 * ((size_t)base + j);
        q[0] = (x - c.lo[0]) / (c.hi[0] - c.lo[0]);
        q[1] = (y - c.lo[1]) / (c.hi[1] - c.lo[1]);
        q[2] = (z - c.lo[2]) / (c.hi[2] - c.lo[2]);
        q[3] = (calc_dt(c, t) - min_cone_step()) / (max_step - min_cone_step());
        q[4] = w0;
        q[5] = w1;
        q[6] = w2;
    }
}
__global__ void __launch_bounds__(256) ngp_ray_index_kernel(const uint32_t *__restrict__ got_slab, const uint32_t *__restrict__ local, const uint32_t *__restrict__ block_sum,
                                                            const uint32_t *__restrict__ counts, const uint32_t *__restrict__ slab_total,
                                                            const uint32_t *__restrict__ step_total, long long n_rays, int *__restrict__ ray_index,
                                                            uint32_t *__restrict__ counter)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        counter[0] = *slab_total;
        counter[1] = *step_total;
    }
    if (i >= n_rays) return;
    ray_index[i] = (got_slab[i] && counts[i]) ? (int)(local[i] + block_sum[i >> 10]) : -1;
}
__global__ void ngp_counter_kernel(const uint32_t *__restrict__ step_total, uint32_t *__restrict__ counter)
{
    counter[0] = 0u;
    counter[1] = *step_total;
}

// ------------------------------------------------------------------------------------------------ update_bitfield
__global__ void __launch_bounds__(1024) ngp_mean_kernel(const float *__restrict__ grid, float *__restrict__ mean_out)
{
    __shared__ float part[1024];
    float s = 0.f;
    for (uint32_t i = threadIdx.x; i < (uint32_t)NGP_CELLS; i += 1024) s += fmaxf(grid[i], 0.f) / (float)NGP_CELLS;
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 512; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) *mean_out = part[0];
}
__global__ void __launch_bounds__(256) ngp_grid_to_bits_kernel(const float *__restrict__ grid, uint8_t *__restrict__ bitfield, const float *__restrict__ mean)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)NGP_CELLS / 8 * TVR_NGP_CASCADES) return;
    const float thresh = 0.01f < *mean ? 0.01f : *mean;             // NERF_MIN_OPTICAL_THICKNESS
    uint32_t b = 0;
    for (int j = 0; j < 8; ++j) b |= grid[(size_t)i * 8 + j] > thresh ? (1u << j) : 0u;
    bitfield[i] = (uint8_t)b;
}
__global__ void __launch_bounds__(256) ngp_max_pool_kernel(const uint8_t *__restrict__ prev, uint8_t *__restrict__ next)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)NGP_CELLS / 64) return;
    uint32_t b = 0;
    for (int j = 0; j < 8; ++j) b |= prev[(size_t)i * 8 + j] > 0 ? (1u << j) : 0u;
    const uint32_t x = morton3d_invert(i >> 0) + NGP_G / 8, y = morton3d_invert(i >> 1) + NGP_G / 8, z = morton3d_invert(i >> 2) + NGP_G / 8;
    next[morton3d(x, y, z)] |= (uint8_t)b;
}

__global__ void __launch_bounds__(256) ngp_hash_encode_kernel(GridCfg g, const float *__restrict__ grid, const float *__restrict__ pos, int pos_stride, long long n,
                                                              float *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int l = blockIdx.y;
    if (i >= n) return;
    const float2 r = encode_level(reinterpret_cast<const float2 *>(grid) + g.offsets[l], (g.hashed >> l) & 1u, g.offsets[l + 1] - g.offsets[l], g.scale[l],
                                  pos[i * pos_stride], pos[i * pos_stride + 1], pos[i * pos_stride + 2]);
    reinterpret_cast<float2 *>(out)[i * TVR_NGP_LEVELS + l] = r;
}

__global__ void __launch_bounds__(256) ngp_sh_encode_kernel(const float *__restrict__ dirs, int stride, long long n, float *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float o[16];
    sh16(dirs[i * stride], dirs[i * stride + 1], dirs[i * stride + 2], o);
    float4 *q = reinterpret_cast<float4 *>(out + 16 * i);
    for (int k = 0; k < 4; ++k) q[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
}

// tvr_device.h's acc_row(i, 0), kept in this form: with the shared one (shifts and masks on a signed int) ngp_pack_f32_kernel compiles to other instructions
__device__ __forceinline__ int acc_row(int i) { return (i / 4) * 8 + i % 4; }

__global__ void __launch_bounds__(256) ngp_pack_f32_kernel(const float *__restrict__ d0, const float *__restrict__ d1, const float *__restrict__ c0, const float *__restrict__ c1,
                                                           const float *__restrict__ c2, float *__restrict__ image)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= NGP_IMAGE_FLOATS) return;
    const float *W;
    int off, n_in, n_out, steps, kind;
    if (e < NGP_L_D1) { W = d0; off = NGP_L_D0; n_in = 32; n_out = 64; steps = 16; kind = 0; }
    else if (e < NGP_L_C0) { W = d1; off = NGP_L_D1; n_in = 64; n_out = 16; steps = 32; kind = 1; }
    else if (e < NGP_L_C1) { W = c0; off = NGP_L_C0; n_in = 32; n_out = 64; steps = 16; kind = 2; }
    else if (e < NGP_L_C2) { W = c1; off = NGP_L_C1; n_in = 64; n_out = 64; steps = 32; kind = 1; }
    else { W = c2; off = NGP_L_C2; n_in = 64; n_out = 3; steps = 32; kind = 1; }
    const int r = e - off, l = r & 63, s = (r >> 6) % steps, mb = (r >> 6) / steps;
    int ka, kb;
    if (kind == 0) { ka = 4 * (s >> 1) + (s & 1); kb = ka + 2; }
    else if (kind == 1) { ka = (s >> 4) * 32 + acc_row(s & 15); kb = ka + 4; }
    else if (s < 8) { ka = acc_row(s); kb = ka + 4; }
    else { ka = 16 + 2 * (s - 8); kb = ka + 1; }
    const int row = mb * 32 + (l & 31), k = l < 32 ? ka : kb;
    image[e] = row < n_out ? W[row * n_in + k] : 0.f;
}

// one thread per (block, lane): the 8 weights of that lane's A fragment, split into hi / lo
__global__ void __launch_bounds__(256) ngp_pack_f16_kernel(const float *__restrict__ d0, const float *__restrict__ d1, const float *__restrict__ c0, const float *__restrict__ c1,
                                                           const float *__restrict__ c2, uint4 *__restrict__ image)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= NGP_H_BLOCKS * 64) return;
    const int blk = e >> 6, l = e & 63, h = l >> 5;
    const float *W;
    int first, n_in, n_out, steps, kind;
    if (blk < NGP_H_D1) { W = d0; first = NGP_H_D0; n_in = 32; n_out = 64; steps = 2; kind = 0; }
    else if (blk < NGP_H_C0) { W = d1; first = NGP_H_D1; n_in = 64; n_out = 16; steps = 4; kind = 1; }
    else if (blk < NGP_H_C1) { W = c0; first = NGP_H_C0; n_in = 32; n_out = 64; steps = 2; kind = 2; }
    else if (blk < NGP_H_C2) { W = c1; first = NGP_H_C1; n_in = 64; n_out = 64; steps = 4; kind = 1; }
    else { W = c2; first = NGP_H_C2; n_in = 64; n_out = 3; steps = 4; kind = 1; }
    const int mb = (blk - first) / steps, t = (blk - first) % steps, row = mb * 32 + (l & 31);
    float v[8];
    for (int j = 0; j < 8; ++j) {
        int k;
        if (kind == 0) k = 2 * (2 * (4 * t + j / 2) + h) + (j & 1);
        else if (kind == 1) k = (t / 2) * 32 + (2 * (t & 1) + j / 4) * 8 + 4 * h + (j & 3);
        else k = t == 0 ? (j / 4) * 8 + 4 * h + (j & 3) : 16 + 8 * h + j;
        v[j] = row < n_out ? W[row * n_in + k] : 0.f;
    }
    const Frag f = split8(v);
    image[(blk * 2 + 0) * 64 + l] = f.hi;
    image[(blk * 2 + 1) * 64 + l] = f.lo;
}


template <bool F16>
__global__ void __launch_bounds__(256, TVR_NGP_WAVES) ngp_field_kernel(GridCfg g, const float *__restrict__ grid, const float *__restrict__ image,
                                                           const float *__restrict__ positions, int pos_stride, const float *__restrict__ dirs, int dir_stride,
                                                           long long n_max, const uint32_t *__restrict__ n_dev, float4 *__restrict__ out)
{
    __shared__ float lds[NGP_IMAGE_FLOATS];
    for (int e = threadIdx.x; e < NGP_IMAGE_FLOATS / 4; e += 256) reinterpret_cast<float4 *>(lds)[e] = reinterpret_cast<const float4 *>(image)[e];
    __syncthreads();
    long long n = n_max;
    if (n_dev) n = min((long long)*n_dev, n_max);
    if (n <= 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, col = lane & 31;
    const long long n_tiles = (n + 31) / 32;
    const float2 *__restrict__ tab = reinterpret_cast<const float2 *>(grid);

    for (long long tile = (long long)blockIdx.x * 4 + wave; tile < n_tiles; tile += (long long)gridDim.x * 4) {
        int hh = h, lane_off = lane;
        asm volatile("" : "+v"(hh), "+v"(lane_off));                // opaque per tile: nothing below may be hoisted out of the loop (registers)
        const long long sidx = tile * 32 + col;
        const long long srow = min(sidx, n - 1);
        const float *q = positions + pos_stride * srow, *qd = dirs + dir_stride * srow;
        const float4 r = field_tile<F16>(g, tab, lds + (F16 ? 4 : 1) * lane_off, hh, q[0], q[1], q[2], qd[0], qd[1], qd[2]);
        if (h == 0 && sidx < n) out[sidx] = r;
    }
}

// ------------------------------------------------------------------------------------------------ fused frame kernel
// render_img's picture without rows, network outputs or slabs in between: a wave takes a ray (dynamic queue), walks its recorded
// steps 32 at a time through field_tile, composites them in order, and STOPS at the sample where compute_rgbs_inference breaks
// (T < 1e-4): the samples behind it never contribute, so skipping their gathers and networks changes nothing.
// T is advanced serially in sample order (the same multiplications as the reference's loop, so the break lands on the same
// sample); colour is accumulated per lane and reduced once per ray (a different summation order: ~1e-7).
template <bool F16>
__global__ void __launch_bounds__(256, TVR_NGP_WAVES) ngp_render_kernel(MarchCfg c, GridCfg g, const float *__restrict__ grid, const float *__restrict__ image,
                                                            const float *__restrict__ rays_o, const float *__restrict__ rays_d, long long n_rays,
                                                            const uint32_t *__restrict__ counts, const float *__restrict__ tslab, unsigned long long *__restrict__ queue,
                                                            float bg0, float bg1, float bg2, float *__restrict__ rgb, unsigned long long *__restrict__ evaluated)
{
    __shared__ float lds[NGP_IMAGE_FLOATS];
    for (int e = threadIdx.x; e < NGP_IMAGE_FLOATS / 4; e += 256) reinterpret_cast<float4 *>(lds)[e] = reinterpret_cast<const float4 *>(image)[e];
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5, col = lane & 31;
    const float2 *__restrict__ tab = reinterpret_cast<const float2 *>(grid);
    const float max_step = min_cone_step() * 16.0f;
    unsigned long long done_samples = 0, all_samples = 0;
    for (;;) {
        // a ticket covers 64 consecutive rays: one atomic and one coalesced read of their step counts per 64 rays; rays without
        // steps (a third of a typical frame) are finished right here
        unsigned long long ticket = 0;
        if (lane == 0) ticket = atomicAdd(queue, 1ull);
        const long long first = (long long)__shfl(ticket, 0, 64) * 64;
        if (first >= n_rays) break;
        const long long mine = first + lane;
        const uint32_t my_n = mine < n_rays ? counts[mine] : 0u;
        if (mine < n_rays && my_n == 0) {
            rgb[3 * mine] = bg0;
            rgb[3 * mine + 1] = bg1;
            rgb[3 * mine + 2] = bg2;
        }
        unsigned long long todo = __ballot(my_n != 0);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const long long i = __shfl(mine, src, 64);
            const uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)my_n, src);
            all_samples += n;
            const float o0 = rays_o[3 * i], o1 = rays_o[3 * i + 1], o2 = rays_o[3 * i + 2], d0 = rays_d[3 * i], d1 = rays_d[3 * i + 1], d2 = rays_d[3 * i + 2];
            const float w0 = (d0 + 1.0f) * 0.5f, w1 = (d1 + 1.0f) * 0.5f, w2 = (d2 + 1.0f) * 0.5f;
            const float *ts = tslab + (size_t)i * TVR_NGP_STEPS;
            float T = 1.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
            bool broke = false;
            for (uint32_t s0 = 0; s0 < n && !broke; s0 += 32) {
                int hh = h, lane_off = lane;
                asm volatile("" : "+v"(hh), "+v"(lane_off));        // opaque per tile (see ngp_field_kernel)
                const uint32_t valid = min(32u, n - s0);
                const float t = ts[min(s0 + (uint32_t)col, n - 1)];
                const float x = __builtin_fmaf(t, d0, o0), y = __builtin_fmaf(t, d1, o1), z = __builtin_fmaf(t, d2, o2);
                const float px = (x - c.lo[0]) / (c.hi[0] - c.lo[0]), py = (y - c.lo[1]) / (c.hi[1] - c.lo[1]), pz = (z - c.lo[2]) / (c.hi[2] - c.lo[2]);
                const float4 r = field_tile<F16>(g, tab, lds + (F16 ? 4 : 1) * lane_off, hh, px, py, pz, w0, w1, w2);
                // the row's dt as compute_rgbs_inference sees it: warped by the sampler, unwarped by the compositor
                const float dtw = (calc_dt(c, t) - min_cone_step()) / (max_step - min_cone_step());
                const float dt = dtw * (max_step - min_cone_step()) + min_cone_step();
                const float alpha = 1.f - __expf(-__expf(r.w) * dt);
                const int oma_bits = __float_as_int(1.f - alpha);
                // T before each sample, multiplied up serially in sample order (the reference's products, so the break lands on the
                // same sample); branch-free: the break is located afterwards
                float Tk = 0.f;
#pragma unroll
                for (int k = 0; k < 32; ++k) {
                    Tk = lane == k ? T : Tk;
                    T *= (uint32_t)k < valid ? __int_as_float(__builtin_amdgcn_readlane(oma_bits, k)) : 1.0f;   // lanes past the ray's end hold a repeat of its last step
                }
                const unsigned long long dead = __ballot(h == 0 && (uint32_t)col < valid && Tk < 1e-4f);   // T is non-increasing: a prefix survives
                const uint32_t n_live = dead ? (uint32_t)(__ffsll((long long)dead) - 1) : valid;
                broke = dead != 0;
                if (h == 0 && (uint32_t)col < n_live) {
                    const float w = alpha * Tk;
                    c0 += w * (1.0f / (1.0f + __expf(-r.x)));
                    c1 += w * (1.0f / (1.0f + __expf(-r.y)));
                    c2 += w * (1.0f / (1.0f + __expf(-r.z)));
                }
                done_samples += valid;
            }
#pragma unroll
            for (int m = 16; m >= 1; m >>= 1) {                     // lanes 0..31 hold the partial sums
                c0 += __shfl_xor(c0, m, 64);
                c1 += __shfl_xor(c1, m, 64);
                c2 += __shfl_xor(c2, m, 64);
            }
            if (lane == 0) {
                if (!broke) { c0 += T * bg0; c1 += T * bg1; c2 += T * bg2; }
                rgb[3 * i] = c0;
                rgb[3 * i + 1] = c1;
                rgb[3 * i + 2] = c2;
            }
        }
    }
    if (evaluated && lane == 0) {
        if (done_samples) atomicAdd(evaluated, done_samples);
        if (all_samples) atomicAdd(evaluated + 1, all_samples);
    }
}

// ------------------------------------------------------------------------------------------------ compositing
__global__ void __launch_bounds__(256) ngp_composite_kernel(const float4 *__restrict__ net_out, const float *__restrict__ coords, const int *__restrict__ numsteps,
                                                            long long n_rays, float bg0, float bg1, float bg2, float *__restrict__ rgb)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays) return;
    const uint32_t n = (uint32_t)numsteps[2 * i], base = (uint32_t)numsteps[2 * i + 1];
    float T = 1.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
    uint32_t j = 0;
    for (; j < n; ++j) {
        if (T < 1e-4f) break;
        const float4 o = net_out[(size_t)base + j];
        const float alpha = ngp_alpha(o.w, ngp_row_dt(coords[7 * ((size_t)base + j) + 3]));
        const float w = alpha * T;
        c0 += w * ngp_logistic(o.x);
        c1 += w * ngp_logistic(o.y);
        c2 += w * ngp_logistic(o.z);
        T *= (1.f - alpha);
    }
    if (j == n) {
        c0 += T * bg0;
        c1 += T * bg1;
        c2 += T * bg2;
    }
    rgb[3 * i] = c0;
    rgb[3 * i + 1] = c1;
    rgb[3 * i + 2] = c2;
}

// ------------------------------------------------------------------------------------------------ C-ABI
static int to_cfg(const tvr_ngp_march_cfg *cfg, MarchCfg &c)
{
    if (!cfg) return tvr_set_error(TVR_ERR_INVALID, "march cfg is NULL");
    for (int k = 0; k < 3; ++k) {
        if (!(cfg->aabb_hi[k] > cfg->aabb_lo[k])) return tvr_set_error(TVR_ERR_INVALID, "aabb_hi <= aabb_lo on axis %d", k);
        c.lo[k] = cfg->aabb_lo[k];
        c.hi[k] = cfg->aabb_hi[k];
    }
    if ((cfg->rng_inc & 1u) == 0) return tvr_set_error(TVR_ERR_INVALID, "rng_inc must be odd (pcg32 stream)");
    c.near_distance = cfg->near_distance;
    c.cone_angle = cfg->cone_angle;
    c.const_dt = cfg->const_dt;
    c.rng_state = cfg->rng_state;
    c.rng_inc = cfg->rng_inc;
    c.slab_rays = cfg->slab_rays;
    return TVR_OK;
}
extern "C" {

int tvr_ngp_update_bitfield(const void *density_grid, void *bitfield, void *mean_out, void *scratch, size_t scratch_bytes, void *stream)
{
    (void)scratch;
    (void)scratch_bytes;
    if (!density_grid || !bitfield || !mean_out) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_update_bitfield: NULL argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ngp_mean_kernel, dim3(1), dim3(1024), 0, st, static_cast<const float *>(density_grid), static_cast<float *>(mean_out));
    const unsigned nb = NGP_CELLS / 8 * TVR_NGP_CASCADES;
    hipLaunchKernelGGL(ngp_grid_to_bits_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, static_cast<const float *>(density_grid),
                       static_cast<uint8_t *>(bitfield), static_cast<const float *>(mean_out));
    for (int level = 1; level < TVR_NGP_CASCADES; ++level)
        hipLaunchKernelGGL(ngp_max_pool_kernel, dim3((NGP_CELLS / 64 + 255) / 256), dim3(256), 0, st,
                           static_cast<const uint8_t *>(bitfield) + (size_t)NGP_CELLS / 8 * (level - 1),
                           static_cast<uint8_t *>(bitfield) + (size_t)NGP_CELLS / 8 * level);
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

// scratch: counts, local, flags, flag-local [n] each + two block-sum arrays + 2 totals + the t slabs [n, 1024]
static size_t scan_blocks(int64_t n) { return (size_t)((n + 1023) / 1024); }
size_t tvr_ngp_sample_scratch_bytes(int64_t n_rays)
{
    if (n_rays < 0) return 0;
    const size_t n = align_up((size_t)n_rays * 4, 256), nb = align_up(scan_blocks(n_rays) * 4 + 4, 256);
    return 4 * n + 2 * nb + 256 + (size_t)n_rays * TVR_NGP_STEPS * sizeof(float);
}

int tvr_ngp_sample(const tvr_ngp_march_cfg *cfg, const void *rays_o, const void *rays_d, int64_t n_rays, const void *bitfield,
                   void *coords, int64_t max_samples, void *numsteps, void *ray_index, void *counter,
                   void *scratch, size_t scratch_bytes, void *stream)
{
    MarchCfg c;
    if (int rc = to_cfg(cfg, c)) return rc;
    if (n_rays < 0 || max_samples < 0 || max_samples > 0xFFFFFFFFll) return tvr_set_error(TVR_ERR_INVALID, "n_rays / max_samples out of range");
    if (!counter) return tvr_set_error(TVR_ERR_INVALID, "counter is NULL");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_rays == 0) {
        HIP_TRY(hipMemsetAsync(counter, 0, 8, st));
        return TVR_OK;
    }
    if (!rays_o || !rays_d || !bitfield || !numsteps || (!coords && max_samples > 0)) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_sample: NULL argument");
    if (n_rays > (1ll << 31)) return tvr_set_error(TVR_ERR_INVALID, "n_rays > 2^31");
    if (scratch_bytes < tvr_ngp_sample_scratch_bytes(n_rays) || !scratch || misaligned(scratch))
        return tvr_set_error(TVR_ERR_SCRATCH, "tvr_ngp_sample: scratch too small or misaligned (%zu < %zu)", scratch_bytes, tvr_ngp_sample_scratch_bytes(n_rays));
    const size_t n = align_up((size_t)n_rays * 4, 256), nbb = align_up(scan_blocks(n_rays) * 4 + 4, 256);
    char *p = static_cast<char *>(scratch);
    uint32_t *counts = reinterpret_cast<uint32_t *>(p);
    uint32_t *local = reinterpret_cast<uint32_t *>(p + n);
    uint32_t *flags = reinterpret_cast<uint32_t *>(p + 2 * n);
    uint32_t *flocal = reinterpret_cast<uint32_t *>(p + 3 * n);
    uint32_t *bsum = reinterpret_cast<uint32_t *>(p + 4 * n);
    uint32_t *fsum = reinterpret_cast<uint32_t *>(p + 4 * n + nbb);
    uint32_t *totals = reinterpret_cast<uint32_t *>(p + 4 * n + 2 * nbb);          // [0] steps, [1] rays with a slab
    float *tslab = reinterpret_cast<float *>(p + 4 * n + 2 * nbb + 256);
    const int nb = (int)scan_blocks(n_rays);
    const dim3 rg((unsigned)((n_rays + 255) / 256)), wg((unsigned)((n_rays + 3) / 4));
    const float *o = static_cast<const float *>(rays_o), *d = static_cast<const float *>(rays_d);
    const uint8_t *bits = static_cast<const uint8_t *>(bitfield);
    hipLaunchKernelGGL(ngp_march_kernel, rg, dim3(256), 0, st, c, o, d, (long long)n_rays, bits, counts, tslab);
    hipLaunchKernelGGL(ngp_scan_block_kernel, dim3(nb), dim3(1024), 0, st, counts, (long long)n_rays, local, bsum);
    hipLaunchKernelGGL(ngp_scan_top_kernel, dim3(1), dim3(1024), 0, st, bsum, nb, totals);
    hipLaunchKernelGGL(ngp_expand_kernel, wg, dim3(256), 0, st, c, o, d, (long long)n_rays, counts, tslab, local, bsum, (long long)max_samples,
                       static_cast<float *>(coords), static_cast<int *>(numsteps), ray_index ? flags : nullptr);
    if (ray_index) {
        hipLaunchKernelGGL(ngp_scan_block_kernel, dim3(nb), dim3(1024), 0, st, flags, (long long)n_rays, flocal, fsum);
        hipLaunchKernelGGL(ngp_scan_top_kernel, dim3(1), dim3(1024), 0, st, fsum, nb, totals + 1);
        hipLaunchKernelGGL(ngp_ray_index_kernel, rg, dim3(256), 0, st, flags, flocal, fsum, counts, totals + 1, totals, (long long)n_rays,
                           static_cast<int *>(ray_index), static_cast<uint32_t *>(counter));
    } else {
        hipLaunchKernelGGL(ngp_counter_kernel, dim3(1), dim3(1), 0, st, totals, static_cast<uint32_t *>(counter));
    }
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

int tvr_ngp_hash_encode(const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *positions, int32_t pos_stride, int64_t n, void *out, void *stream)
{
    GridCfg g;
    if (int rc = to_grid(grid_cfg, g)) return rc;
    if (n < 0 || pos_stride < 3) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_hash_encode: n < 0 or pos_stride < 3");
    if (n == 0) return TVR_OK;
    if (!grid || !positions || !out) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_hash_encode: NULL argument");
    hipLaunchKernelGGL(ngp_hash_encode_kernel, dim3((unsigned)((n + 255) / 256), TVR_NGP_LEVELS), dim3(256), 0, static_cast<hipStream_t>(stream), g,
                       static_cast<const float *>(grid), static_cast<const float *>(positions), (int)pos_stride, (long long)n, static_cast<float *>(out));
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

int tvr_ngp_sh_encode(const void *dirs, int32_t dir_stride, int64_t n, void *out, void *stream)
{
    if (n < 0 || dir_stride < 3) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_sh_encode: n < 0 or dir_stride < 3");
    if (n == 0) return TVR_OK;
    if (!dirs || !out || misaligned(out)) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_sh_encode: NULL or misaligned argument");
    hipLaunchKernelGGL(ngp_sh_encode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const float *>(dirs),
                       (int)dir_stride, (long long)n, static_cast<float *>(out));
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

size_t tvr_ngp_net_packed_bytes(void) { return 2 * (size_t)NGP_IMAGE_FLOATS * sizeof(float); }      // fp32 image, then fp16 hi/lo image

int tvr_ngp_net_pack(const tvr_ngp_net_params *p, void *packed, size_t packed_bytes, void *stream)
{
    if (!p || !p->density0 || !p->density1 || !p->rgb0 || !p->rgb1 || !p->rgb2) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_net_pack: NULL weights");
    if (!packed || misaligned(packed) || packed_bytes < tvr_ngp_net_packed_bytes()) return tvr_set_error(TVR_ERR_SCRATCH, "tvr_ngp_net_pack: packed buffer too small or misaligned");
    const float *d0 = static_cast<const float *>(p->density0), *d1 = static_cast<const float *>(p->density1), *c0 = static_cast<const float *>(p->rgb0),
                *c1 = static_cast<const float *>(p->rgb1), *c2 = static_cast<const float *>(p->rgb2);
    hipLaunchKernelGGL(ngp_pack_f32_kernel, dim3((NGP_IMAGE_FLOATS + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), d0, d1, c0, c1, c2,
                       static_cast<float *>(packed));
    hipLaunchKernelGGL(ngp_pack_f16_kernel, dim3((NGP_H_BLOCKS * 64 + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), d0, d1, c0, c1, c2,
                       reinterpret_cast<uint4 *>(static_cast<float *>(packed) + NGP_IMAGE_FLOATS));
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

int tvr_ngp_network(const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *net_packed, const void *positions, int32_t pos_stride,
                    const void *dirs, int32_t dir_stride, int64_t n_max, const void *n_dev, void *out, void *stream)
{
    GridCfg g;
    if (int rc = to_grid(grid_cfg, g)) return rc;
    if (n_max < 0 || pos_stride < 3 || dir_stride < 3) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_network: n_max < 0 or a stride < 3");
    if (n_max == 0) return TVR_OK;
    if (!grid || !net_packed || !positions || !dirs || !out || misaligned(out) || misaligned(net_packed))
        return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_network: NULL or misaligned argument");
    const long long tiles = (n_max + 31) / 32;
    unsigned blocks = (unsigned)(tiles < 4 * 2048 ? (tiles + 3) / 4 : 2048);
    const bool f16 = !TVR_NGP_MLP_F32;
    hipLaunchKernelGGL(f16 ? ngp_field_kernel<true> : ngp_field_kernel<false>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), g,
                       static_cast<const float *>(grid), static_cast<const float *>(net_packed) + (f16 ? NGP_IMAGE_FLOATS : 0), static_cast<const float *>(positions),
                       (int)pos_stride, static_cast<const float *>(dirs), (int)dir_stride, (long long)n_max, static_cast<const uint32_t *>(n_dev),
                       static_cast<float4 *>(out));
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

int tvr_ngp_composite(const void *net_out, const void *coords, const void *numsteps, int64_t n_rays, const float background[3], void *rgb, void *stream)
{
    if (n_rays < 0 || !background) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_composite: n_rays < 0 or background NULL");
    if (n_rays == 0) return TVR_OK;
    if (!numsteps || !rgb) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_composite: NULL argument");
    hipLaunchKernelGGL(ngp_composite_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const float4 *>(net_out),
                       static_cast<const float *>(coords), static_cast<const int *>(numsteps), (long long)n_rays, background[0], background[1], background[2],
                       static_cast<float *>(rgb));
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

// scratch of the fused frame call: step counts [n], the ray queue + 2 statistics words, the t slabs [n, 1024]
size_t tvr_ngp_render_scratch_bytes(int64_t n_rays)
{
    if (n_rays < 0) return 0;
    return align_up((size_t)n_rays * 4, 256) + 256 + (size_t)n_rays * TVR_NGP_STEPS * sizeof(float);
}

}  // extern "C" — closed here: the body shared by tvr_ngp_render / tvr_ngp_render_profiled has internal linkage

static int ngp_render_impl(const tvr_ngp_march_cfg *cfg, const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *net_packed, const void *rays_o,
                           const void *rays_d, int64_t n_rays, const void *bitfield, const float background[3], void *rgb, void *stats,
                           void *scratch, size_t scratch_bytes, void *stream, hipEvent_t *ev)
{
    MarchCfg c;
    GridCfg g;
    if (int rc = to_cfg(cfg, c)) return rc;
    if (int rc = to_grid(grid_cfg, g)) return rc;
    if (n_rays < 0 || n_rays > (1ll << 31) || !background) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_render: n_rays out of range or background NULL");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (stats) HIP_TRY(hipMemsetAsync(stats, 0, 16, st));
    if (n_rays == 0) return TVR_OK;
    if (!grid || !net_packed || !rays_o || !rays_d || !bitfield || !rgb || misaligned(net_packed)) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_render: NULL or misaligned argument");
    if (scratch_bytes < tvr_ngp_render_scratch_bytes(n_rays) || !scratch || misaligned(scratch))
        return tvr_set_error(TVR_ERR_SCRATCH, "tvr_ngp_render: scratch too small or misaligned (%zu < %zu)", scratch_bytes, tvr_ngp_render_scratch_bytes(n_rays));
    char *p = static_cast<char *>(scratch);
    const size_t n = align_up((size_t)n_rays * 4, 256);
    uint32_t *counts = reinterpret_cast<uint32_t *>(p);
    unsigned long long *queue = reinterpret_cast<unsigned long long *>(p + n);
    float *tslab = reinterpret_cast<float *>(p + n + 256);
    HIP_TRY(hipMemsetAsync(queue, 0, 8, st));
    const float *o = static_cast<const float *>(rays_o), *d = static_cast<const float *>(rays_d);
    if (ev) HIP_TRY(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(ngp_march_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, st, c, o, d, (long long)n_rays, static_cast<const uint8_t *>(bitfield), counts, tslab);
    if (ev) HIP_TRY(hipEventRecord(ev[1], st));
    const bool f16 = !TVR_NGP_MLP_F32;
    const unsigned blocks = (unsigned)(n_rays < 4 * 512 ? (n_rays + 3) / 4 : 512);         // 256 CUs x 2 blocks (LDS image + 2 waves / SIMD)
    hipLaunchKernelGGL(f16 ? ngp_render_kernel<true> : ngp_render_kernel<false>, dim3(blocks), dim3(256), 0, st, c, g, static_cast<const float *>(grid),
                       static_cast<const float *>(net_packed) + (f16 ? NGP_IMAGE_FLOATS : 0), o, d, (long long)n_rays, counts, tslab, queue, background[0],
                       background[1], background[2], static_cast<float *>(rgb), static_cast<unsigned long long *>(stats));
    if (ev) HIP_TRY(hipEventRecord(ev[2], st));
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}


extern "C" {

int tvr_ngp_render(const tvr_ngp_march_cfg *cfg, const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *net_packed, const void *rays_o,
                   const void *rays_d, int64_t n_rays, const void *bitfield, const float background[3], void *rgb, void *stats,
                   void *scratch, size_t scratch_bytes, void *stream)
{
    return ngp_render_impl(cfg, grid_cfg, grid, net_packed, rays_o, rays_d, n_rays, bitfield, background, rgb, stats, scratch, scratch_bytes, stream, nullptr);
}

int tvr_ngp_render_profiled(const tvr_ngp_march_cfg *cfg, const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *net_packed, const void *rays_o,
                            const void *rays_d, int64_t n_rays, const void *bitfield, const float background[3], void *rgb, void *stats,
                            void *scratch, size_t scratch_bytes, void *stream, float ms_out[2])
{
    if (!ms_out) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_render_profiled: ms_out is NULL");
    hipEvent_t ev[3];
    for (int k = 0; k < 3; ++k) HIP_TRY(hipEventCreate(&ev[k]));
    int rc = ngp_render_impl(cfg, grid_cfg, grid, net_packed, rays_o, rays_d, n_rays, bitfield, background, rgb, stats, scratch, scratch_bytes, stream, ev);
    ms_out[0] = ms_out[1] = 0.f;
    if (rc == TVR_OK && n_rays > 0) {
        hipError_t e = hipEventSynchronize(ev[2]);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms_out[0], ev[0], ev[1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms_out[1], ev[1], ev[2]);
        if (e != hipSuccess) rc = tvr_set_error(TVR_ERR_HIP, "tvr_ngp_render_profiled: %s", hipGetErrorString(e));
    }
    for (int k = 0; k < 3; ++k) (void)hipEventDestroy(ev[k]);
    return rc;
}

}  // extern "C"
