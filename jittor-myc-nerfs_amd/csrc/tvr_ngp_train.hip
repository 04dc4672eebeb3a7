// tvr_ngp_train.hip — what Instant-NGP training adds to the row-level alt path (include/tvr_ngp.h, "training" section): the compositor of
// CalcRgb.execute with a per-ray background and a row capacity, its backward, and the hash grid's scatter-add backward (kernel_grid_backward).
// The five Linears train through tvr_linear_dx / tvr_gemm_tn (autograd_ops._LinearFn); nothing here touches them.
//
//   ngp_composite_train_kernel      one lane per ray over its contiguous rows: tvr_ngp.hip's ngp_composite_kernel with bg[i] and the capacity clamp.
//   ngp_composite_backward_kernel   one lane per ray walks the same rows again with the same roundings (tvr_ngp_composite.h), forward for T and then from
//                                   the back for the suffix, and writes each composited row's gradient; the buffer is zeroed first, so every other row
//                                   is exactly 0.  One owner per row.
//   ngp_hash_backward_*_kernel      grad_grid += w * grad_enc with the forward's cell, fractions and factor order (tvr_ngp_field.h).  Three
//                                   variants, selectable for measurement (tvr_ngp_hash_encode_backward_variant):
//                                     0  one lane per (sample, level): 16 atomics per lane, 64 lanes in 64 different entries per instruction;
//                                     1  four lanes per (sample, level) = (corner x, feature): the four lanes add into 16 contiguous bytes in a dense
//                                        level, and into one aligned 16-byte block in a hashed level when the cell's x is even (x ^ 1 only flips bit 0);
//                                     2  variant 1 for the levels whose table exceeds NGP_LDS_ENTRIES; the smaller ones (level 0: 16^3 entries, which
//                                        takes 512 adds per entry at 2^18 rows) are summed per workgroup in LDS and flushed with one atomic per entry
//                                        that received anything, 256 contiguous bytes per wave-instruction.
// Compiled with -ffp-contract=off like tvr_ngp.hip: the compositor's products and sums are those of ngp_composite_kernel bit for bit.
#include "tvr_ngp_field.h"
#include "tvr_ngp_composite.h"

// ------------------------------------------------------------------------------------------------ training compositor
__device__ __forceinline__ uint32_t rows_of_ray(uint32_t n, uint32_t base, long long n_rows)
{
    const long long b = (long long)base < n_rows ? (long long)base : n_rows;       // min(n_rows, base)
    const long long room = n_rows - b;
    return room < (long long)n ? (uint32_t)room : n;
}

__global__ void __launch_bounds__(256) ngp_composite_train_kernel(const float4 *__restrict__ net_out, const float *__restrict__ coords, const int *__restrict__ numsteps,
                                                                  long long n_rays, long long n_rows, const float *__restrict__ bg, float *__restrict__ rgb)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays) return;
    const uint32_t n = (uint32_t)numsteps[2 * i], base = (uint32_t)numsteps[2 * i + 1];
    const uint32_t nc = rows_of_ray(n, base, n_rows);
    float T = 1.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
    uint32_t j = 0;
    for (; j < nc; ++j) {
        if (T < 1e-4f) break;
        const float4 o = net_out[(size_t)base + j];
        const float alpha = ngp_alpha(o.w, ngp_row_dt(coords[7 * ((size_t)base + j) + 3]));
        const float w = alpha * T;
        c0 += w * ngp_logistic(o.x);
        c1 += w * ngp_logistic(o.y);
        c2 += w * ngp_logistic(o.z);
        T *= (1.f - alpha);
    }
    if (j == n) {                                   // walked every uncompacted step: no break, not cut by the capacity
        c0 += T * bg[3 * i];
        c1 += T * bg[3 * i + 1];
        c2 += T * bg[3 * i + 2];
    }
    rgb[3 * i] = c0;
    rgb[3 * i + 1] = c1;
    rgb[3 * i + 2] = c2;
}

// d rgb / d out of the rows the forward composited (the stop index is held fixed).  With suffix_j = everything behind sample j (the background term included
// where the forward added it):
//   d / d out[0:3] = g * alpha T c (1 - c)            d / d out[3] = sigma dt * dot(g, T (1 - alpha) c - suffix)
// suffix_j equals rgb_out - (the colour summed up to and including j), but formed that way it cancels where little is left behind j while sigma dt, which
// multiplies it, is large.  So the lane walks its ray twice: forward with the compositor's own products, parking T_j in the row's fourth gradient slot (the
// row is this lane's to write), then from the last composited sample back to the first, summing the suffix directly and overwriting the row with its gradient.
__global__ void __launch_bounds__(256) ngp_composite_backward_kernel(const float4 *__restrict__ net_out, const float *__restrict__ coords, const int *__restrict__ numsteps,
                                                                     long long n_rays, long long n_rows, const float *__restrict__ bg,
                                                                     const float *__restrict__ grad_rgb, float4 *grad_net_out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays) return;
    const uint32_t n = (uint32_t)numsteps[2 * i], base = (uint32_t)numsteps[2 * i + 1];
    const uint32_t nc = rows_of_ray(n, base, n_rows);
    const float g0 = grad_rgb[3 * i], g1 = grad_rgb[3 * i + 1], g2 = grad_rgb[3 * i + 2];
    float T = 1.f;
    uint32_t stop = 0;
    for (; stop < nc; ++stop) {
        if (T < 1e-4f) break;
        const size_t row = (size_t)base + stop;
        grad_net_out[row].w = T;
        T *= (1.f - ngp_alpha(net_out[row].w, ngp_row_dt(coords[7 * row + 3])));
    }
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    if (stop == n) {                                // the forward added the background behind the last sample
        s0 = T * bg[3 * i];
        s1 = T * bg[3 * i + 1];
        s2 = T * bg[3 * i + 2];
    }
    for (uint32_t j = stop; j-- > 0;) {
        const size_t row = (size_t)base + j;
        const float4 o = net_out[row];
        const float dt = ngp_row_dt(coords[7 * row + 3]);
        const float alpha = ngp_alpha(o.w, dt);
        const float Tj = grad_net_out[row].w;
        const float w = alpha * Tj, Tn = Tj * (1.f - alpha);
        const float c0 = ngp_logistic(o.x), c1 = ngp_logistic(o.y), c2 = ngp_logistic(o.z);
        const float d = g0 * (Tn * c0 - s0) + g1 * (Tn * c1 - s1) + g2 * (Tn * c2 - s2);
        grad_net_out[row] = make_float4(g0 * w * (c0 * (1.f - c0)), g1 * w * (c1 * (1.f - c1)), g2 * w * (c2 * (1.f - c2)), __expf(o.w) * dt * d);
        s0 += w * c0;
        s1 += w * c1;
        s2 += w * c2;
    }
}

// ------------------------------------------------------------------------------------------------ hash grid backward
#define NGP_LDS_ENTRIES 6144      // a level whose table has at most this many entries (48 KiB of float2) is pre-summed in LDS by variant 2

struct HashCell {
    uint32_t res, cx, cy, cz;
    float fx, fy, fz;
};
// the forward's cell and fractions (encode_level: the same fma, floor and subtraction)
__device__ __forceinline__ HashCell hash_cell(float scale, float px, float py, float pz)
{
    HashCell c;
    c.res = (uint32_t)ceilf(scale) + 1u;
    const float x = __builtin_fmaf(px, scale, 0.5f), y = __builtin_fmaf(py, scale, 0.5f), z = __builtin_fmaf(pz, scale, 0.5f);
    const float fx0 = floorf(x), fy0 = floorf(y), fz0 = floorf(z);
    c.cx = (uint32_t)(int)fx0;
    c.cy = (uint32_t)(int)fy0;
    c.cz = (uint32_t)(int)fz0;
    c.fx = x - fx0;
    c.fy = y - fy0;
    c.fz = z - fz0;
    return c;
}
// the forward's weight of corner idx, in its factor order
__device__ __forceinline__ float corner_weight(const HashCell &c, int idx)
{
    float w = 1.0f;
    w *= (idx & 1) ? c.fx : 1 - c.fx;
    w *= (idx & 2) ? c.fy : 1 - c.fy;
    w *= (idx & 4) ? c.fz : 1 - c.fz;
    return w;
}

// variant 0: one lane per (sample, level)
__global__ void __launch_bounds__(256) ngp_hash_backward_lane_kernel(GridCfg g, const float *__restrict__ pos, int pos_stride, long long n, const float *__restrict__ grad_enc,
                                                                     float *__restrict__ grad_grid)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int l = blockIdx.y;
    if (i >= n) return;
    const uint32_t off = g.offsets[l], size = g.offsets[l + 1] - off;
    const bool hashed = (g.hashed >> l) & 1u;
    const HashCell c = hash_cell(g.scale[l], pos[i * pos_stride], pos[i * pos_stride + 1], pos[i * pos_stride + 2]);
    const float2 ge = reinterpret_cast<const float2 *>(grad_enc)[i * TVR_NGP_LEVELS + l];
    float *tab = grad_grid + 2 * (size_t)off;
#pragma unroll
    for (int idx = 0; idx < 8; ++idx) {
        const uint32_t e = grid_entry(hashed, size, c.res, c.cx + (idx & 1), c.cy + ((idx >> 1) & 1), c.cz + ((idx >> 2) & 1));
        const float w = corner_weight(c, idx);
        atomicAdd(tab + 2 * (size_t)e, w * ge.x);
        atomicAdd(tab + 2 * (size_t)e + 1, w * ge.y);
    }
}

// variants 1 and 2: four lanes per (sample, level) = (corner x, feature); blockIdx.y indexes `levels` (a packed list of 4-bit level numbers)
__global__ void __launch_bounds__(256) ngp_hash_backward_quad_kernel(GridCfg g, unsigned long long levels, const float *__restrict__ pos, int pos_stride, long long n,
                                                                     const float *__restrict__ grad_enc, float *__restrict__ grad_grid)
{
    const long long i = (long long)blockIdx.x * 64 + (threadIdx.x >> 2);
    const int l = (int)((levels >> (4 * blockIdx.y)) & 15u);
    if (i >= n) return;
    const int f = threadIdx.x & 1, dx = (threadIdx.x >> 1) & 1;
    const uint32_t off = g.offsets[l], size = g.offsets[l + 1] - off;
    const bool hashed = (g.hashed >> l) & 1u;
    const HashCell c = hash_cell(g.scale[l], pos[i * pos_stride], pos[i * pos_stride + 1], pos[i * pos_stride + 2]);
    const float ge = grad_enc[i * (2 * TVR_NGP_LEVELS) + 2 * l + f];
    float *tab = grad_grid + 2 * (size_t)off + f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = dx | (k << 1);
        const uint32_t e = grid_entry(hashed, size, c.res, c.cx + dx, c.cy + (k & 1), c.cz + (k >> 1));
        atomicAdd(tab + 2 * (size_t)e, corner_weight(c, idx) * ge);
    }
}

// variant 2, small levels: a workgroup sums the contributions of its slice of the samples in LDS, then adds every entry that received anything once
__global__ void __launch_bounds__(256) ngp_hash_backward_lds_kernel(GridCfg g, unsigned long long levels, const float *__restrict__ pos, int pos_stride, long long n,
                                                                    long long per_block, const float *__restrict__ grad_enc, float *__restrict__ grad_grid)
{
    __shared__ float acc[2 * NGP_LDS_ENTRIES];
    const int l = (int)((levels >> (4 * blockIdx.y)) & 15u);
    const uint32_t off = g.offsets[l], size = g.offsets[l + 1] - off;      // size <= NGP_LDS_ENTRIES (checked by the host)
    const bool hashed = (g.hashed >> l) & 1u;
    for (uint32_t e = threadIdx.x; e < 2 * size; e += 256) acc[e] = 0.f;
    __syncthreads();
    const long long first = (long long)blockIdx.x * per_block, last = first + per_block < n ? first + per_block : n;
    const int f = threadIdx.x & 1, dx = (threadIdx.x >> 1) & 1;
    for (long long i = first + (threadIdx.x >> 2); i < last; i += 64) {
        const HashCell c = hash_cell(g.scale[l], pos[i * pos_stride], pos[i * pos_stride + 1], pos[i * pos_stride + 2]);
        const float ge = grad_enc[i * (2 * TVR_NGP_LEVELS) + 2 * l + f];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t e = grid_entry(hashed, size, c.res, c.cx + dx, c.cy + (k & 1), c.cz + (k >> 1));
            atomicAdd(&acc[2 * e + f], corner_weight(c, dx | (k << 1)) * ge);
        }
    }
    __syncthreads();
    float *tab = grad_grid + 2 * (size_t)off;
    for (uint32_t e = threadIdx.x; e < 2 * size; e += 256) {
        const float v = acc[e];
        if (v != 0.f) atomicAdd(tab + e, v);
    }
}

static int hash_backward(const tvr_ngp_grid_cfg *grid_cfg, const void *positions, int32_t pos_stride, int64_t n, const void *grad_enc, void *grad_grid, int variant,
                         void *stream)
{
    GridCfg g;
    if (int rc = to_grid(grid_cfg, g)) return rc;
    if (n < 0 || pos_stride < 3) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_hash_encode_backward: n < 0 or pos_stride < 3");
    if (variant < 0 || variant > 2) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_hash_encode_backward: variant %d is not 0, 1 or 2", variant);
    if (n >= (1ll << 31) * 64) return tvr_set_error(TVR_ERR_UNSUPPORTED, "tvr_ngp_hash_encode_backward: n too large for one launch");
    if (n == 0) return TVR_OK;
    if (!positions || !grad_enc || !grad_grid || (reinterpret_cast<uintptr_t>(grad_enc) & 7u) || (reinterpret_cast<uintptr_t>(grad_grid) & 7u))
        return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_hash_encode_backward: NULL or misaligned argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float *p = static_cast<const float *>(positions), *ge = static_cast<const float *>(grad_enc);
    float *gg = static_cast<float *>(grad_grid);
    if (variant == 0) {
        hipLaunchKernelGGL(ngp_hash_backward_lane_kernel, dim3((unsigned)((n + 255) / 256), TVR_NGP_LEVELS), dim3(256), 0, s, g, p, (int)pos_stride, (long long)n, ge, gg);
        HIP_TRY(hipGetLastError());
        return TVR_OK;
    }
    unsigned long long big = 0, small = 0;
    unsigned n_big = 0, n_small = 0;
    for (int l = 0; l < TVR_NGP_LEVELS; ++l) {
        if (variant == 2 && g.offsets[l + 1] - g.offsets[l] <= NGP_LDS_ENTRIES) small |= (unsigned long long)l << (4 * n_small++);
        else big |= (unsigned long long)l << (4 * n_big++);
    }
    if (n_big) hipLaunchKernelGGL(ngp_hash_backward_quad_kernel, dim3((unsigned)((n + 63) / 64), n_big), dim3(256), 0, s, g, big, p, (int)pos_stride, (long long)n, ge, gg);
    if (n_small) {
        // slices of at least 1024 samples, at most 512 workgroups per level: the flush costs one table's worth of atomics per workgroup
        long long blocks = (n + 1023) / 1024;
        if (blocks > 512) blocks = 512;
        const long long per_block = (n + blocks - 1) / blocks;
        hipLaunchKernelGGL(ngp_hash_backward_lds_kernel, dim3((unsigned)blocks, n_small), dim3(256), 0, s, g, small, p, (int)pos_stride, (long long)n, per_block, ge, gg);
    }
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

#ifndef TVR_NGP_HASH_BWD_VARIANT      // what tvr_ngp_hash_encode_backward runs (DESIGN.md §10.2 has the measurements)
#define TVR_NGP_HASH_BWD_VARIANT 2
#endif

static int composite_args(const char *who, const void *net_out, const void *coords, const void *numsteps, int64_t n_rays, int64_t n_rows, const void *bg)
{
    if (n_rays < 0 || n_rows < 0) return tvr_set_error(TVR_ERR_INVALID, "%s: n_rays < 0 or n_rows < 0", who);
    if (n_rays == 0) return TVR_OK;
    if (!numsteps || !bg) return tvr_set_error(TVR_ERR_INVALID, "%s: NULL argument", who);
    if (n_rows > 0 && (!net_out || !coords || misaligned(net_out))) return tvr_set_error(TVR_ERR_INVALID, "%s: NULL or misaligned rows", who);
    return TVR_OK;
}

extern "C" {

int tvr_ngp_composite_train(const void *net_out, const void *coords, const void *numsteps, int64_t n_rays, int64_t n_rows, const void *bg, void *rgb_out, void *stream)
{
    if (int rc = composite_args("tvr_ngp_composite_train", net_out, coords, numsteps, n_rays, n_rows, bg)) return rc;
    if (n_rays == 0) return TVR_OK;
    if (!rgb_out) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_composite_train: rgb_out NULL");
    hipLaunchKernelGGL(ngp_composite_train_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float4 *>(net_out), static_cast<const float *>(coords), static_cast<const int *>(numsteps), (long long)n_rays, (long long)n_rows,
                       static_cast<const float *>(bg), static_cast<float *>(rgb_out));
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

int tvr_ngp_composite_backward(const void *net_out, const void *coords, const void *numsteps, int64_t n_rays, int64_t n_rows, const void *bg, const void *rgb_out,
                               const void *grad_rgb, void *grad_net_out, void *stream)
{
    if (int rc = composite_args("tvr_ngp_composite_backward", net_out, coords, numsteps, n_rays, n_rows, bg)) return rc;
    (void)rgb_out;                                  // part of the signature; the suffix is summed from the back, not formed from it
    if (n_rows > 0 && (!grad_net_out || misaligned(grad_net_out))) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_composite_backward: grad_net_out NULL or misaligned");
    if (n_rays > 0 && !grad_rgb) return tvr_set_error(TVR_ERR_INVALID, "tvr_ngp_composite_backward: grad_rgb NULL");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_rows > 0) HIP_TRY(hipMemsetAsync(grad_net_out, 0, (size_t)n_rows * 16, s));       // rows behind a break, behind the cut and rows no ray owns
    if (n_rays == 0 || n_rows == 0) return TVR_OK;
    hipLaunchKernelGGL(ngp_composite_backward_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, s, static_cast<const float4 *>(net_out),
                       static_cast<const float *>(coords), static_cast<const int *>(numsteps), (long long)n_rays, (long long)n_rows, static_cast<const float *>(bg),
                       static_cast<const float *>(grad_rgb), static_cast<float4 *>(grad_net_out));
    HIP_TRY(hipGetLastError());
    return TVR_OK;
}

int tvr_ngp_hash_encode_backward(const tvr_ngp_grid_cfg *grid_cfg, const void *positions, int32_t pos_stride, int64_t n, const void *grad_enc, void *grad_grid, void *stream)
{
    return hash_backward(grid_cfg, positions, pos_stride, n, grad_enc, grad_grid, TVR_NGP_HASH_BWD_VARIANT, stream);
}

// Measurement hook, NOT part of the C-ABI (no declaration in include/tvr_ngp.h): the same sums through a named kernel variant, for
// scripts/ngp_train_timing.py and the variant cases of tests/test_gpu_ngp_train.py (ngp_train.hash_encode_backward binds it by name).
int tvr_ngp_hash_encode_backward_variant(const tvr_ngp_grid_cfg *grid_cfg, const void *positions, int32_t pos_stride, int64_t n, const void *grad_enc, void *grad_grid,
                                         int32_t variant, void *stream)
{
    return hash_backward(grid_cfg, positions, pos_stride, n, grad_enc, grad_grid, variant, stream);
}

}  // extern "C"
