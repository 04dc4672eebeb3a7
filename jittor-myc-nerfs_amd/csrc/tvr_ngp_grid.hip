// tvr_ngp_grid.hip — the occupancy grid of the Instant-NGP alt path, built and refreshed FROM THE NETWORK (DensityGridSampler.update_density_grid /
// update_density_grid_nerf, density_grid_sampler.py:200-259; definitions in include/tvr_ngp.h).
//
//   ngp_grid_mark_kernel      mark_untrained_density_grid: one lane per cell against every camera.
//   ngp_grid_samples_kernel   generate_grid_samples_nerf_nonuniform on its own: one lane per sample, positions and indices to memory.
//   ngp_density_kernel        the density head of the fused network (field_tile<F16, COLOUR = false>): hash gather + density_mlp only.
//   ngp_grid_splat_kernel     splat_grid_samples_nerf_max_nearest_neighbor, ngp_grid_ema_kernel: ema_grid_samples_nerf.
//   ngp_grid_update_kernel    the product path: per wave 32 samples at a time, drawn in registers (grid_sample), through the same density tile,
//                             one atomicMax per sample from the lanes that hold the result.  Both sample populations share the launch: their
//                             reads of density_grid do not depend on the splat, which goes to density_grid_tmp.
//
// Compiled with -ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt: every fp32 operation below is rounded on its own, in the order written.
#include "tvr_ngp_field.h"

struct GridBox {
    float lo[3], hi[3];
};
struct GridGen {                          // one sample population of generate_grid_samples_nerf_nonuniform
    uint64_t state, inc;                  // the generator as this population sees it
    uint32_t n;
    float thresh;
};
struct GridSample {
    float p[3];                           // warped to [0,1] of the aabb
    uint32_t idx;
};

#define GRID_HASH_MUL 56924617u
#define GRID_HASH_MUL_INV 53369u           // GRID_HASH_MUL * GRID_HASH_MUL_INV == 1 (mod 2^21)
static_assert(((GRID_HASH_MUL * GRID_HASH_MUL_INV) & (uint32_t)(NGP_CELLS - 1)) == 1u, "inverse of the index hash's multiplier modulo the cells of a cascade");

__device__ __forceinline__ float grid_min_cone_step() { return 1.73205080757f / 1024.0f; }
__device__ __forceinline__ float pow2_level(uint32_t level) { return __uint_as_float((127u + level) << 23); }      // scalbnf(1.0f, level), level 0..4

// Sample i of a population of n, `rng` already advanced by 4 * i.  The ten candidate cells do not depend on one another: the first is read alone
// (on a grid without negative cells the uniform population always keeps it), the other nine together when it fails.
__device__ __forceinline__ GridSample grid_sample(Pcg rng, uint32_t i, uint32_t n, uint32_t ema_step, uint32_t n_cascades, float thresh, const GridBox &b,
                                                  const float *__restrict__ grid)
{
    const uint32_t level = (uint32_t)(pcg_float(rng) * (float)n_cascades) % n_cascades;
    const uint32_t h0 = (i + ema_step * n) * GRID_HASH_MUL + 96925573u;
    uint32_t idx = h0 % (uint32_t)NGP_CELLS + level * (uint32_t)NGP_CELLS;
    if (!(grid[idx] > thresh)) {
        uint32_t cand[9];
        float v[9];
#pragma unroll
        for (uint32_t j = 1; j < 10; ++j) {
            cand[j - 1] = (h0 + j * 19349663u) % (uint32_t)NGP_CELLS + level * (uint32_t)NGP_CELLS;
            v[j - 1] = grid[cand[j - 1]];
        }
        idx = cand[8];                                              // none breaks: the tenth index is kept
#pragma unroll
        for (int j = 7; j >= 0; --j) idx = v[j] > thresh ? cand[j] : idx;
    }
    const uint32_t pos_idx = idx % (uint32_t)NGP_CELLS;
    const uint32_t c[3] = {morton3d_invert(pos_idx >> 0), morton3d_invert(pos_idx >> 1), morton3d_invert(pos_idx >> 2)};
    const float s = pow2_level(level);
    GridSample r;
    r.idx = idx;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float u = pcg_float(rng);
        const float pos = (((float)c[k] + u) / (float)NGP_G - 0.5f) * s + 0.5f;
        r.p[k] = (pos - b.lo[k]) / (b.hi[k] - b.lo[k]);
    }
    return r;
}

__device__ __forceinline__ uint32_t splat_bits(float raw) { return __float_as_uint(__expf(raw) * grid_min_cone_step()); }    // level 0 for every cascade

// ------------------------------------------------------------------------------------------------ mark_untrained_density_grid
__global__ void __launch_bounds__(256) ngp_grid_mark_kernel(float *__restrict__ grid, int n_images, const float *__restrict__ focal, const float *__restrict__ xforms,
                                                            float half_w, float half_h)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)NGP_CELLS * TVR_NGP_CASCADES) return;
    const uint32_t level = i / (uint32_t)NGP_CELLS, pos_idx = i % (uint32_t)NGP_CELLS;
    const float s = pow2_level(level);
    const float px = (((float)morton3d_invert(pos_idx >> 0) + 0.5f) / (float)NGP_G - 0.5f) * s + 0.5f;
    const float py = (((float)morton3d_invert(pos_idx >> 1) + 0.5f) / (float)NGP_G - 0.5f) * s + 0.5f;
    const float pz = (((float)morton3d_invert(pos_idx >> 2) + 0.5f) / (float)NGP_G - 0.5f) * s + 0.5f;
    const float r = 0.5f * 1.73205080757f * s / (float)NGP_G;
    bool seen = false;
    for (int j = 0; j < n_images && !seen; ++j) {
        const float *m = xforms + 12 * (size_t)j;                   // row-major [3,4]: columns 0..2 the camera axes, column 3 the origin
        const float p0 = px - m[3], p1 = py - m[7], p2 = pz - m[11];
        const float x = (p0 * m[0] + p1 * m[4]) + p2 * m[8];
        const float y = (p0 * m[1] + p1 * m[5]) + p2 * m[9];
        const float z = (p0 * m[2] + p1 * m[6]) + p2 * m[10];
        seen = z > 0.f && fabsf(x) - r < z / focal[2 * j] * half_w && fabsf(y) - r < z / focal[2 * j + 1] * half_h;
    }
    if ((grid[i] < 0.f) != !seen) grid[i] = seen ? 0.f : -1.f;
}

// ------------------------------------------------------------------------------------------------ the pieces
__global__ void __launch_bounds__(256) ngp_grid_samples_kernel(GridGen gen, uint32_t ema_step, uint32_t n_cascades, GridBox b, const float *__restrict__ grid,
                                                               float *__restrict__ positions, uint32_t *__restrict__ indices)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= gen.n) return;
    Pcg rng = {gen.state, gen.inc};
    pcg_advance(rng, (uint64_t)(4u * i));                          // 1 draw selects the level, 3 the position
    const GridSample r = grid_sample(rng, i, gen.n, ema_step, n_cascades, gen.thresh, b, grid);
    positions[3 * (size_t)i] = r.p[0];
    positions[3 * (size_t)i + 1] = r.p[1];
    positions[3 * (size_t)i + 2] = r.p[2];
    indices[i] = r.idx;
}

template <bool F16>
__global__ void __launch_bounds__(256, TVR_NGP_WAVES) ngp_density_kernel(GridCfg g, const float *__restrict__ grid, const float *__restrict__ image,
                                                                         const float *__restrict__ positions, int pos_stride, long long n_max,
                                                                         const uint32_t *__restrict__ n_dev, float *__restrict__ out)
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
        asm volatile("" : "+v"(hh), "+v"(lane_off));                // opaque per tile, as in ngp_field_kernel
        const long long sidx = tile * 32 + col;
        const float *q = positions + pos_stride * min(sidx, n - 1);
        const float4 r = field_tile<F16, false>(g, tab, lds + (F16 ? 4 : 1) * lane_off, hh, q[0], q[1], q[2], 0.f, 0.f, 0.f);
        if (h == 0 && sidx < n) out[sidx] = r.w;
    }
}

__global__ void __launch_bounds__(256) ngp_grid_splat_kernel(const uint32_t *__restrict__ indices, const float *__restrict__ raw, long long n, uint32_t *__restrict__ tmp)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t idx = indices[i];
    if (idx >= (uint32_t)NGP_CELLS * TVR_NGP_CASCADES) return;    // caller-made indices: never outside the grid
    // positive floats are ordered like their bit patterns
    atomicMax(tmp + idx, splat_bits(raw[i]));
}

__global__ void __launch_bounds__(256) ngp_grid_ema_kernel(const float *__restrict__ tmp, float *__restrict__ grid, float decay)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)NGP_CELLS * TVR_NGP_CASCADES) return;
    const float prev = grid[i];
    grid[i] = prev < 0.f ? prev : fmaxf(prev * decay, tmp[i]);    // maximum instead of an average: a cell turns on as soon as anything visible is in it
}

// ------------------------------------------------------------------------------------------------ the fused update
// Tiles [0, tiles0) belong to population 0, the rest to population 1; a tile's population and generator are wave-uniform.  Both half-waves
// draw the same 32 samples (the gather wants the position in either half); the lower half issues the atomic.
//
// WHICH 32 samples share a tile is free — the splat is a maximum, so the order of the samples changes no bit — and is chosen for the gathers:
// sample i's first candidate cell, ((i + ema_step * n) * 56924617 + 96925573) mod 2^21, is a bijection of any 2^21 consecutive i onto the cells of
// a cascade (the multiplier is odd), so within every whole block of 2^21 samples work slot w takes the sample whose first candidate is Morton
// cell w mod 2^21: a tile's 32 samples then sit in a 4 x 4 x 2 block of neighbouring cells (of up to n_cascades cascades) whenever the first
// probe is kept, and concurrently running tiles in neighbouring blocks, instead of 32 cells spread over the whole volume.  The samples behind
// the last whole block keep their own order.

// rng advanced by delta (delta <= max_delta, wave-uniform): pcg_advance's jump, applied to the state bit by bit — the per-bit multiplier and
// increment depend on the stream alone (scalar unit), a lane multiplies once per set bit.  Same state: all the maps are powers of one step.
// The loop runs on shrinking copies, as pcg_advance's does: at most 32 rounds whatever max_delta holds (bit 31 is set from n = 2^29 + 2 on),
// and no shift by a variable amount.
__device__ __forceinline__ void pcg_advance_lane(Pcg &r, uint32_t delta, uint32_t max_delta)
{
    uint64_t cur_mult = 0x5851f42d4c957f2dULL, cur_plus = r.inc;
    for (; max_delta != 0u; max_delta >>= 1, delta >>= 1) {
        if (delta & 1u) r.state = r.state * cur_mult + cur_plus;
        cur_plus = (cur_mult + 1) * cur_plus;
        cur_mult *= cur_mult;
    }
}
template <bool F16>
__global__ void __launch_bounds__(256, TVR_NGP_WAVES) ngp_grid_update_kernel(GridCfg g, const float *__restrict__ hash, const float *__restrict__ image, GridGen gen0,
                                                                             GridGen gen1, uint32_t ema_step, uint32_t n_cascades, GridBox b,
                                                                             const float *__restrict__ density_grid, uint32_t *__restrict__ tmp)
{
    __shared__ float lds[NGP_IMAGE_FLOATS];
    for (int e = threadIdx.x; e < NGP_IMAGE_FLOATS / 4; e += 256) reinterpret_cast<float4 *>(lds)[e] = reinterpret_cast<const float4 *>(image)[e];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, col = lane & 31;
    const uint32_t tiles0 = (gen0.n + 31u) / 32u, n_tiles = tiles0 + (gen1.n + 31u) / 32u;
    const float2 *__restrict__ tab = reinterpret_cast<const float2 *>(hash);

    for (uint32_t tile = blockIdx.x * 4u + (uint32_t)wave; tile < n_tiles; tile += gridDim.x * 4u) {
        int hh = h, lane_off = lane;
        asm volatile("" : "+v"(hh), "+v"(lane_off));                // opaque per tile, as in ngp_field_kernel
        const uint32_t ut = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile);
        const bool second = ut >= tiles0;
        const uint32_t t = second ? ut - tiles0 : ut, n = second ? gen1.n : gen0.n;
        const float thresh = second ? gen1.thresh : gen0.thresh;
        Pcg rng = {second ? gen1.state : gen0.state, second ? gen1.inc : gen0.inc};
        const uint32_t sidx = t * 32u + (uint32_t)col, whole = n & ~(uint32_t)(NGP_CELLS - 1);
        uint32_t i = min(sidx, n - 1u);                             // lanes behind the population's end repeat its last sample and write nothing
        if (sidx < whole)                                           // whole blocks end on a tile boundary: wave-uniform
            i = (((sidx - 96925573u) * GRID_HASH_MUL_INV - ema_step * n) & (uint32_t)(NGP_CELLS - 1)) + (sidx & ~(uint32_t)(NGP_CELLS - 1));
        pcg_advance_lane(rng, 4u * i, 4u * (n - 1u));
        const GridSample s = grid_sample(rng, i, n, ema_step, n_cascades, thresh, b, density_grid);
        const float4 r = field_tile<F16, false>(g, tab, lds + (F16 ? 4 : 1) * lane_off, hh, s.p[0], s.p[1], s.p[2], 0.f, 0.f, 0.f);
        if (h == 0 && sidx < n) atomicMax(tmp + s.idx, splat_bits(r.w));
    }
}

// ------------------------------------------------------------------------------------------------ C-ABI
static const size_t GRID_CELLS_ALL = (size_t)NGP_CELLS * TVR_NGP_CASCADES;
static const int64_t GRID_MAX_SAMPLES = (1ll << 30) - 1;          // 4 * i is the reference's uint32 product

static int to_box(const char *who, const float *lo, const float *hi, GridBox &b)
{
    if (!lo || !hi) return tvr_set_error(TVR_ERR_INVALID, "%s: aabb is NULL", who);
    for (int k = 0; k < 3; ++k) {
        if (!(hi[k] > lo[k])) return tvr_set_error(TVR_ERR_INVALID, "%s: aabb_hi <= aabb_lo on axis %d", who, k);
        b.lo[k] = lo[k];
        b.hi[k] = hi[k];
    }
    return TVR_OK;
}

static int check_gen(const char *who, int64_t n, int32_t n_cascades, uint64_t rng_inc)
{
    if (n < 0 || n > GRID_MAX_SAMPLES) return tvr_set_error(TVR_ERR_INVALID, "%s: sample count %lld outside [0, 2^30)", who, (long long)n);
    if (n_cascades < 1 || n_cascades > TVR_NGP_CASCADES) return tvr_set_error(TVR_ERR_INVALID, "%s: n_cascades %d outside 1..%d", who, (int)n_cascades, TVR_NGP_CASCADES);
    if ((rng_inc & 1u) == 0) return tvr_set_error(TVR_ERR_INVALID, "%s: rng_inc must be odd (pcg32 stream)", who);
    return TVR_OK;
}

extern "C" {

int tvr_ngp_grid_mark_untrained(void *density_grid, int32_t n_images, const void *focal_lengths, const void *xforms, int32_t res_w, int32_t res_h, void *stream)
{
    if (n_images < 0 || res_w <= 0 || res_h <= 0) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_grid_mark_untrained: n_images < 0 or a resolution <= 0");
    if (!density_grid || (n_images > 0 && (!focal_lengths || !xforms))) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_grid_mark_untrained: NULL argument");
    hipLaunchKernelGGL(ngp_grid_mark_kernel, dim3((unsigned)((GRID_CELLS_ALL + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<float *>(density_grid),
                       (int)n_images, static_cast<const float *>(focal_lengths), static_cast<const float *>(xforms), (float)res_w * 0.5f, (float)res_h * 0.5f);
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

int tvr_ngp_grid_samples(int64_t n, uint32_t ema_step, int32_t n_cascades, float thresh, uint64_t rng_state, uint64_t rng_inc, const float aabb_lo[3],
                         const float aabb_hi[3], const void *density_grid, void *positions_out, void *indices_out, void *stream)
{
    GridBox b;
    if (int rc = check_gen("tvr_ngp_grid_samples", n, n_cascades, rng_inc)) return rc;
    if (int rc = to_box("tvr_ngp_grid_samples", aabb_lo, aabb_hi, b)) return rc;
    if (n == 0) return TVR_OK;
    if (!density_grid || !positions_out || !indices_out) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_grid_samples: NULL argument");
    const GridGen gen = {rng_state, rng_inc, (uint32_t)n, thresh};
    hipLaunchKernelGGL(ngp_grid_samples_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), gen, ema_step, (uint32_t)n_cascades, b,
                       static_cast<const float *>(density_grid), static_cast<float *>(positions_out), static_cast<uint32_t *>(indices_out));
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

int tvr_ngp_density(const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *net_packed, const void *positions, int32_t pos_stride, int64_t n_max,
                    const void *n_dev, void *out, void *stream)
{
    GridCfg g;
    if (int rc = to_grid(grid_cfg, g)) return rc;
    if (n_max < 0 || pos_stride < 3) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_density: n_max < 0 or pos_stride < 3");
    if (n_max == 0) return TVR_OK;
    if (!grid || !net_packed || !positions || !out || misaligned(net_packed)) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_density: NULL or misaligned argument");
    const long long tiles = (n_max + 31) / 32;
    const unsigned blocks = (unsigned)(tiles < 4 * 2048 ? (tiles + 3) / 4 : 2048);
    const bool f16 = !TVR_NGP_MLP_F32;
    hipLaunchKernelGGL(f16 ? ngp_density_kernel<true> : ngp_density_kernel<false>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), g,
                       static_cast<const float *>(grid), static_cast<const float *>(net_packed) + (f16 ? NGP_IMAGE_FLOATS : 0), static_cast<const float *>(positions),
                       (int)pos_stride, (long long)n_max, static_cast<const uint32_t *>(n_dev), static_cast<float *>(out));
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

int tvr_ngp_grid_splat(const void *indices, const void *raw, int64_t n, void *grid_tmp, void *stream)
{
    if (n < 0) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_grid_splat: n < 0");
    if (n == 0) return TVR_OK;
    if (!indices || !raw || !grid_tmp) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_grid_splat: NULL argument");
    hipLaunchKernelGGL(ngp_grid_splat_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint32_t *>(indices),
                       static_cast<const float *>(raw), (long long)n, static_cast<uint32_t *>(grid_tmp));
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

int tvr_ngp_grid_ema(const void *grid_tmp, void *density_grid, float decay, void *stream)
{
    if (!grid_tmp || !density_grid) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_grid_ema: NULL argument");
    hipLaunchKernelGGL(ngp_grid_ema_kernel, dim3((unsigned)((GRID_CELLS_ALL + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float *>(grid_tmp), static_cast<float *>(density_grid), decay);
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

int tvr_ngp_grid_update(const float aabb_lo[3], const float aabb_hi[3], const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *net_packed, void *density_grid,
                        void *density_grid_tmp, size_t tmp_bytes, void *bitfield, void *mean_out, int64_t n_uniform, int64_t n_nonuniform, uint32_t ema_step,
                        int32_t n_cascades, float decay, uint64_t rng_state, uint64_t rng_inc, void *stream)
{
    GridCfg g;
    GridBox b;
    if (int rc = to_box("tvr_ngp_grid_update", aabb_lo, aabb_hi, b)) return rc;
    if (int rc = to_grid(grid_cfg, g)) return rc;
    if (int rc = check_gen("tvr_ngp_grid_update", n_uniform, n_cascades, rng_inc)) return rc;
    if (int rc = check_gen("tvr_ngp_grid_update", n_nonuniform, n_cascades, rng_inc)) return rc;
    if (!grid || !net_packed || !density_grid || !bitfield || !mean_out || misaligned(net_packed))
        return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_grid_update: NULL or misaligned argument");
    if (!density_grid_tmp || tmp_bytes < GRID_CELLS_ALL * sizeof(float))
        return tvr_set_error(TVR_ERR_SCRATCH, "tvr_ngp_grid_update: density_grid_tmp too small (%zu < %zu)", tmp_bytes, GRID_CELLS_ALL * sizeof(float));
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(density_grid_tmp, 0, GRID_CELLS_ALL * sizeof(float), st));
    Pcg later = {rng_state, rng_inc};
    pcg_advance(later, 1ull << 32);                                 // the second generate call sees the generator one host advance later
    const GridGen gen0 = {rng_state, rng_inc, (uint32_t)n_uniform, -0.01f}, gen1 = {later.state, rng_inc, (uint32_t)n_nonuniform, 0.01f};   // NERF_MIN_OPTICAL_THICKNESS
    const long long tiles = (n_uniform + 31) / 32 + (n_nonuniform + 31) / 32;
    if (tiles > 0) {
        const unsigned blocks = (unsigned)(tiles < 4 * 2048 ? (tiles + 3) / 4 : 2048);
        const bool f16 = !TVR_NGP_MLP_F32;
        hipLaunchKernelGGL(f16 ? ngp_grid_update_kernel<true> : ngp_grid_update_kernel<false>, dim3(blocks), dim3(256), 0, st, g, static_cast<const float *>(grid),
                           static_cast<const float *>(net_packed) + (f16 ? NGP_IMAGE_FLOATS : 0), gen0, gen1, ema_step, (uint32_t)n_cascades, b,
                           static_cast<const float *>(density_grid), static_cast<uint32_t *>(density_grid_tmp));
    }
    hipLaunchKernelGGL(ngp_grid_ema_kernel, dim3((unsigned)((GRID_CELLS_ALL + 255) / 256)), dim3(256), 0, st, static_cast<const float *>(density_grid_tmp),
                       static_cast<float *>(density_grid), decay);
    HIP_TRY(hipGetLastError());
    return tvr_ngp_update_bitfield(density_grid, bitfield, mean_out, nullptr, 0, stream);
}

}  // extern "C"
