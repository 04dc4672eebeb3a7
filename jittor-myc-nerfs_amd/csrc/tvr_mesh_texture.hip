// tvr_mesh_texture.hip — the per-triangle texture atlas of an indexed triangle mesh: where every texel lies on the mesh (the bake's sample points) and what a rasterised
// hit reads back from a baked atlas (mesh.atlas_points, mesh.sample_texture, TensorBase.bake_texture, reconstruct --mesh_texture).  include/tvr.h tvr_mesh_atlas_points
// holds the definition (placement, texel to point, sampling); this file is its one implementation.  DESIGN.md §4.16.
//
//   check    per triangle of the square rows the texel range touches: an index outside 0 .. V-1 raises the fault flag
//   points   one lane per texel of the range: owner (square, half, local coordinates), barycentric weights, point; returns at once when the flag is up
//   sample   one lane per pixel: the four taps of the hit in its triangle's half, the bilinear blend
//
// Both are gathers without atomics, LDS or cross-lane traffic; fp contraction is off and the divisions are correctly rounded (csrc/Makefile), so the numpy restatement
// of tests/mesh_texture_common.py gives the same bits.  The atlas has fewer than 2^31 texels (checked by the host), so every texel index is an unsigned below that;
// every texel of the range is below Ha * Wa (host), so its square column is below C by construction (Wa = C * P); a triangle index is compared with F, its three vertex
// indices with V, a tap's index with Ha * Wa, before anything is loaded through them: no load or store leaves the caller's buffers whatever faces, tri and bary hold.
#include "tvr_kernels.h"

#define TX_THREADS 256

struct TxLayout {
    unsigned F;            // triangles
    unsigned P, C, Wa;     // patch side, squares per row, atlas width C * P
    float L;               // P - 4 as a float (exact)
};

__global__ __launch_bounds__(TX_THREADS) void tx_check_kernel(const int *__restrict__ faces, unsigned t0, unsigned t1, unsigned V, unsigned *__restrict__ fault)
{
    const unsigned t = t0 + blockIdx.x * TX_THREADS + threadIdx.x;
    if (t >= t1) return;
    const int *f = faces + (size_t)t * 3;
    if ((unsigned)f[0] >= V || (unsigned)f[1] >= V || (unsigned)f[2] >= V) *fault = 1u;        // (a negative index is a huge unsigned one)
}

__global__ __launch_bounds__(TX_THREADS) void tx_points_kernel(const float *__restrict__ verts, const int *__restrict__ faces, unsigned V, TxLayout a, unsigned texel0,
                                                               unsigned n, float *__restrict__ pos, int *__restrict__ tri, const unsigned *__restrict__ fault)
{
    if (*fault) return;                                        // the check kernel (or the caller) raised it: nothing is written
    const unsigned e = blockIdx.x * TX_THREADS + threadIdx.x;
    if (e >= n) return;
    const unsigned idx = texel0 + e, Y = idx / a.Wa, X = idx % a.Wa;
    const unsigned ca = X % a.P, cb = Y % a.P, s = (Y / a.P) * a.C + X / a.P;
    const unsigned h = ca + cb <= a.P - 1u ? 0u : 1u;
    const unsigned x = h ? a.P - 1u - ca : ca, y = h ? a.P - 1u - cb : cb;
    const unsigned long long t = 2ull * s + h;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    int owner = -1;
    if (t < a.F) {
        const int *f = faces + (size_t)t * 3;
        const int v0 = f[0], v1 = f[1], v2 = f[2];
        if ((unsigned)v0 >= V || (unsigned)v1 >= V || (unsigned)v2 >= V) return;       // (checked again: this kernel indexes verts with them)
        const float *p0 = verts + (size_t)v0 * 3, *p1 = verts + (size_t)v1 * 3, *p2 = verts + (size_t)v2 * 3;
        const float b1 = (float)x / a.L, b2 = (float)y / a.L, b0 = (1.0f - b1) - b2;
        px = (b0 * p0[0] + b1 * p1[0]) + b2 * p2[0];
        py = (b0 * p0[1] + b1 * p1[1]) + b2 * p2[1];
        pz = (b0 * p0[2] + b1 * p1[2]) + b2 * p2[2];
        owner = (int)t;
    }
    pos[(size_t)e * 3 + 0] = px; pos[(size_t)e * 3 + 1] = py; pos[(size_t)e * 3 + 2] = pz;
    tri[e] = owner;
}

// texel (x, y) in the local coordinates of half h of the square whose corner texel is (X0, Y0) -> its linear index in the atlas
__device__ __forceinline__ unsigned tx_tap(const TxLayout &a, unsigned X0, unsigned Y0, unsigned h, unsigned x, unsigned y)
{
    const unsigned ca = h ? a.P - 1u - x : x, cb = h ? a.P - 1u - y : y;
    return (Y0 + cb) * a.Wa + (X0 + ca);
}

template <typename T>
__device__ __forceinline__ float tx_load(const T *__restrict__ atlas, unsigned texel, unsigned n_texels, int k)
{
    return texel < n_texels ? (float)atlas[(size_t)texel * 3 + k] : 0.0f;
}

template <typename T>
__global__ __launch_bounds__(TX_THREADS) void tx_sample_kernel(const int *__restrict__ tri, const float *__restrict__ bary, unsigned n_pix, const T *__restrict__ atlas,
                                                               unsigned n_texels, TxLayout a, float *__restrict__ out)
{
    const unsigned p = blockIdx.x * TX_THREADS + threadIdx.x;
    if (p >= n_pix) return;
    float r[3] = {0.0f, 0.0f, 0.0f};
    const int t = tri[p];
    if (t >= 0 && (unsigned)t < a.F) {
        const float x = fminf(fmaxf(bary[(size_t)p * 3 + 1] * a.L, 0.0f), a.L), y = fminf(fmaxf(bary[(size_t)p * 3 + 2] * a.L, 0.0f), a.L);     // (a NaN becomes 0)
        const float fi = floorf(x), fj = floorf(y), fx = x - fi, fy = y - fj;
        const unsigned i = (unsigned)fi, j = (unsigned)fj;                          // 0 .. L = P - 4: i + 1, j + 1 <= P - 3 stay inside the square
        const unsigned s = (unsigned)t >> 1, h = (unsigned)t & 1u, X0 = (s % a.C) * a.P, Y0 = (s / a.C) * a.P;
        const unsigned e00 = tx_tap(a, X0, Y0, h, i, j), e10 = tx_tap(a, X0, Y0, h, i + 1u, j), e01 = tx_tap(a, X0, Y0, h, i, j + 1u),
                       e11 = tx_tap(a, X0, Y0, h, i + 1u, j + 1u);
        for (int k = 0; k < 3; ++k) {
            const float T00 = tx_load(atlas, e00, n_texels, k), T10 = tx_load(atlas, e10, n_texels, k), T01 = tx_load(atlas, e01, n_texels, k),
                        T11 = tx_load(atlas, e11, n_texels, k);
            const float top = T00 + fx * (T10 - T00), bot = T01 + fx * (T11 - T01);
            r[k] = top + fy * (bot - top);
        }
    }
    out[(size_t)p * 3 + 0] = r[0]; out[(size_t)p * 3 + 1] = r[1]; out[(size_t)p * 3 + 2] = r[2];
}

static TxLayout tx_layout(long long n_triangles, int P, int C)
{
    TxLayout a;
    a.F = (unsigned)n_triangles; a.P = (unsigned)P; a.C = (unsigned)C; a.Wa = (unsigned)C * (unsigned)P; a.L = (float)(P - 4);
    return a;
}

hipError_t launch_mesh_atlas_points(const float *verts, long long n_vertices, const int *faces, long long n_triangles, int P, int C, long long texel0, long long n,
                                    float *pos, int *tri, unsigned *fault, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const TxLayout a = tx_layout(n_triangles, P, C);
    // the triangles a texel of the range can belong to: those of the square rows its atlas rows lie in
    const long long r0 = texel0 / a.Wa / P, r1 = (texel0 + n - 1) / a.Wa / P;
    long long t0 = 2 * r0 * C, t1 = 2 * (r1 + 1) * C;
    if (t1 > n_triangles) t1 = n_triangles;
    if (t0 < t1) {
        const unsigned fb = (unsigned)((t1 - t0 + TX_THREADS - 1) / TX_THREADS);
        hipLaunchKernelGGL(tx_check_kernel, dim3(fb), dim3(TX_THREADS), 0, stream, faces, (unsigned)t0, (unsigned)t1, (unsigned)n_vertices, fault);
    }
    const unsigned pb = (unsigned)((n + TX_THREADS - 1) / TX_THREADS);
    hipLaunchKernelGGL(tx_points_kernel, dim3(pb), dim3(TX_THREADS), 0, stream, verts, faces, (unsigned)n_vertices, a, (unsigned)texel0, (unsigned)n, pos, tri, fault);
    return hipGetLastError();
}

hipError_t launch_mesh_texture_sample(const int *tri, const float *bary, long long n_pix, const void *atlas, int fmt, long long n_texels, int P, int C,
                                      long long n_triangles, float *out, hipStream_t stream)
{
    if (n_pix <= 0) return hipSuccess;
    const TxLayout a = tx_layout(n_triangles, P, C);
    const unsigned pb = (unsigned)((n_pix + TX_THREADS - 1) / TX_THREADS);
    if (fmt == 0)
        hipLaunchKernelGGL(tx_sample_kernel<unsigned char>, dim3(pb), dim3(TX_THREADS), 0, stream, tri, bary, (unsigned)n_pix, (const unsigned char *)atlas,
                           (unsigned)n_texels, a, out);
    else
        hipLaunchKernelGGL(tx_sample_kernel<float>, dim3(pb), dim3(TX_THREADS), 0, stream, tri, bary, (unsigned)n_pix, (const float *)atlas, (unsigned)n_texels, a, out);
    return hipGetLastError();
}
