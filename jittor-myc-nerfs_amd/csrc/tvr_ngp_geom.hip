// tvr_ngp_geom.hip — geometry from an Instant-NGP field (definitions in include/tvr_ngp.h, "geometry"):
//
//   ngp_density_gradient_kernel   raw density and its analytic spatial gradient at points: ngp_density_kernel's tile loop around field_tile_grad
//                                 (tvr_ngp_field.h) — forward mode, three tangent columns per sample through the same LDS weight image, then row 0 of
//                                 density_mlp.2 in fp32 (64 more floats of LDS, from the packed fp32 image).
//   ngp_density_grid_kernel       the raw density on a lattice: a tile is a 2 x 4 x 4 brick of lattice points (x, y, z; z is the volume's fastest axis),
//                                 positions formed in registers, points outside the unit cube or in unoccupied cells answered without evaluation, a brick
//                                 without a live point skipped before any gather or MFMA.  The value path is field_tile<F16, false>, the density kernel's.
//
// No atomics in either kernel, one owner per output word: the same bytes on every run.  Compiled with -ffp-contract=off like the rest of the library.
#include "tvr_ngp_field.h"

template <bool F16>
__global__ void __launch_bounds__(256, TVR_NGP_WAVES) ngp_density_gradient_kernel(GridCfg g, const float *__restrict__ grid, const float *__restrict__ image,
                                                                                  const float *__restrict__ image32, const float *__restrict__ positions, int pos_stride, long long n_max,
                                                                                  const uint32_t *__restrict__ n_dev, float *__restrict__ raw_out,
                                                                                  float *__restrict__ grad_out)
{
    __shared__ float lds[NGP_IMAGE_FLOATS + 64];
    for (int e = threadIdx.x; e < NGP_IMAGE_FLOATS / 4; e += 256) reinterpret_cast<float4 *>(lds)[e] = reinterpret_cast<const float4 *>(image)[e];
    load_w1rows(image32, lds + NGP_IMAGE_FLOATS);
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
        asm volatile("" : "+v"(hh), "+v"(lane_off));                // opaque per tile, as in ngp_density_kernel
        const long long sidx = tile * 32 + col;
        const float *q = positions + pos_stride * min(sidx, n - 1);
        const float4 r = field_tile_grad<F16>(g, tab, lds + (F16 ? 4 : 1) * lane_off, lds + NGP_IMAGE_FLOATS + 32 * hh, hh, q[0], q[1], q[2]);
        if (h == 0 && sidx < n) {
            if (raw_out) raw_out[sidx] = r.w;
            grad_out[3 * sidx] = r.x;
            grad_out[3 * sidx + 1] = r.y;
            grad_out[3 * sidx + 2] = r.z;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the lattice
#define BRICK_X 2
#define BRICK_Y 4
#define BRICK_Z 4
static_assert(BRICK_X * BRICK_Y * BRICK_Z == 32, "a brick is one 32-sample tile");

struct Lattice {
    int n[3];                             // lattice points per axis
    unsigned by, bz;                      // bricks along y and z
    long long bricks;
    float origin[3], spacing[3];
    float lo[3], ext[3];                  // unit cube -> NGP position: p * ext + lo (read only with a bitfield)
    float empty;
};

template <bool F16>
__global__ void __launch_bounds__(256, TVR_NGP_WAVES) ngp_density_grid_kernel(GridCfg g, const float *__restrict__ grid, const float *__restrict__ image,
                                                                              const uint8_t *__restrict__ bits, Lattice L, float *__restrict__ out)
{
    __shared__ float lds[NGP_IMAGE_FLOATS];
    for (int e = threadIdx.x; e < NGP_IMAGE_FLOATS / 4; e += 256) reinterpret_cast<float4 *>(lds)[e] = reinterpret_cast<const float4 *>(image)[e];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, col = lane & 31;
    const float2 *__restrict__ tab = reinterpret_cast<const float2 *>(grid);

    // consecutive tiles are neighbouring bricks along z, then y, then x: the four waves of a workgroup and the workgroups in flight gather from one neighbourhood
    for (long long tile = (long long)blockIdx.x * 4 + wave; tile < L.bricks; tile += (long long)gridDim.x * 4) {
        int hh = h, lane_off = lane;
        asm volatile("" : "+v"(hh), "+v"(lane_off));                // opaque per tile, as in ngp_density_kernel
        const unsigned tz = (unsigned)(tile % L.bz), ty = (unsigned)((tile / L.bz) % L.by), tx = (unsigned)(tile / ((long long)L.bz * L.by));
        const int i = (int)(tx * BRICK_X) + (col >> 4), j = (int)(ty * BRICK_Y) + ((col >> 2) & 3), k = (int)(tz * BRICK_Z) + (col & 3);
        const bool inside = i < L.n[0] && j < L.n[1] && k < L.n[2];
        const float px = __builtin_fmaf((float)i, L.spacing[0], L.origin[0]), py = __builtin_fmaf((float)j, L.spacing[1], L.origin[1]),
                    pz = __builtin_fmaf((float)k, L.spacing[2], L.origin[2]);
        bool live = inside && px >= 0.f && px <= 1.f && py >= 0.f && py <= 1.f && pz >= 0.f && pz <= 1.f;
        if (bits && live) {
            const float x = px * L.ext[0] + L.lo[0], y = py * L.ext[1] + L.lo[1], z = pz * L.ext[2] + L.lo[2];
            live = occupied_at(x, y, z, bits, (uint32_t)mip_from_pos(x, y, z));
        }
        const long long o = ((long long)i * L.n[1] + j) * L.n[2] + k;
        if (__ballot(live) == 0ull) {                               // wave-uniform: no gather, no MFMA
            if (h == 0 && inside) out[o] = L.empty;
            continue;
        }
        // lanes without a live point run the tile on a position clamped into the cube (a neighbour's cell) and store the empty value
        const float4 r = field_tile<F16, false>(g, tab, lds + (F16 ? 4 : 1) * lane_off, hh, fminf(fmaxf(px, 0.f), 1.f), fminf(fmaxf(py, 0.f), 1.f),
                                                fminf(fmaxf(pz, 0.f), 1.f), 0.f, 0.f, 0.f);
        if (h == 0 && inside) out[o] = live ? r.w : L.empty;
    }
}

// ------------------------------------------------------------------------------------------------ C-ABI
extern "C" {

int tvr_ngp_density_gradient(const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *net_packed, const void *positions, int32_t pos_stride, int64_t n_max,
                             const void *n_dev, void *raw_out, void *grad_out, void *stream)
{
    GridCfg g;
    if (int rc = to_grid(grid_cfg, g)) return rc;
    if (n_max < 0 || pos_stride < 3) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_density_gradient: n_max < 0 or pos_stride < 3");
    if (n_max == 0) return TVR_OK;
    if (!grid || !net_packed || !positions || !grad_out || misaligned(net_packed))
        return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_density_gradient: NULL or misaligned argument");
    const long long tiles = (n_max + 31) / 32;
    const unsigned blocks = (unsigned)(tiles < 4 * 2048 ? (tiles + 3) / 4 : 2048);
    const bool f16 = !TVR_NGP_MLP_F32;
    hipLaunchKernelGGL(f16 ? ngp_density_gradient_kernel<true> : ngp_density_gradient_kernel<false>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), g,
                       static_cast<const float *>(grid), static_cast<const float *>(net_packed) + (f16 ? NGP_IMAGE_FLOATS : 0), static_cast<const float *>(net_packed),
                       static_cast<const float *>(positions), (int)pos_stride, (long long)n_max, static_cast<const uint32_t *>(n_dev), static_cast<float *>(raw_out),
                       static_cast<float *>(grad_out));
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

int tvr_ngp_density_grid(const tvr_ngp_grid_cfg *grid_cfg, const void *grid, const void *net_packed, const void *bitfield, const float aabb_lo[3],
                         const float aabb_hi[3], const int32_t dims[3], const float origin[3], const float spacing[3], float empty_value, void *volume_out,
                         void *stream)
{
    GridCfg g;
    Lattice L;
    if (int rc = to_grid(grid_cfg, g)) return rc;
    if (!dims || !origin || !spacing) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_density_grid: dims, origin or spacing is NULL");
    long long points = 1;
    for (int k = 0; k < 3; ++k) {
        if (dims[k] <= 0) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_density_grid: dims[%d] = %d, the volume would be empty", k, (int)dims[k]);
        if (!(fabsf(origin[k]) <= FLT_MAX) || !(fabsf(spacing[k]) <= FLT_MAX)) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_density_grid: origin or spacing not finite on axis %d", k);
        points *= dims[k];                                          // at most 2^31 * 2^31 before the check below: no overflow
        if (points > (1ll << 31)) return tvr_set_error(TVR_ERR_UNSUPPORTED, "tvr_ngp_density_grid: more than 2^31 lattice points");
        L.n[k] = dims[k];
        L.origin[k] = origin[k];
        L.spacing[k] = spacing[k];
        L.lo[k] = 0.f;
        L.ext[k] = 1.f;
    }
    if (bitfield) {
        if (!aabb_lo || !aabb_hi) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_density_grid: a bitfield needs the aabb");
        for (int k = 0; k < 3; ++k) {
            if (!(aabb_hi[k] > aabb_lo[k])) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_density_grid: aabb_hi <= aabb_lo on axis %d", k);
            L.lo[k] = aabb_lo[k];
            L.ext[k] = aabb_hi[k] - aabb_lo[k];
        }
    }
    if (!grid || !net_packed || !volume_out || misaligned(net_packed)) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_density_grid: NULL or misaligned argument");
    const long long bx = (dims[0] + BRICK_X - 1) / BRICK_X, by = (dims[1] + BRICK_Y - 1) / BRICK_Y, bz = (dims[2] + BRICK_Z - 1) / BRICK_Z;
    L.by = (unsigned)by;
    L.bz = (unsigned)bz;
    L.bricks = bx * by * bz;
    L.empty = empty_value;
    const unsigned blocks = (unsigned)(L.bricks < 4 * 2048 ? (L.bricks + 3) / 4 : 2048);
    const bool f16 = !TVR_NGP_MLP_F32;
    hipLaunchKernelGGL(f16 ? ngp_density_grid_kernel<true> : ngp_density_grid_kernel<false>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), g,
                       static_cast<const float *>(grid), static_cast<const float *>(net_packed) + (f16 ? NGP_IMAGE_FLOATS : 0), static_cast<const uint8_t *>(bitfield), L,
                       static_cast<float *>(volume_out));
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

}  // extern "C"
