// tvr_mesh_project.hip — Newton projection of mesh vertices onto the iso-surface f(p) = f* of the density feature: what puts an exported mesh's vertices back on the
// surface after marching cubes' linear interpolation, clustering and smoothing moved them off it (TensorBase.project_to_isosurface, export_mesh(refine=)).
// include/tvr.h tvr_mesh_project holds the definition; this file is its one implementation.
//
//   per vertex, k = 0 .. N:   n_k = (p_k - lo) * inv - 1,   (f_k, g_k) = tvr_density_gradient's value at n_k,   r_k = f_k - f*
//                             gw = g_k * inv,  s = r_k / max(|gw|^2, 1e-30),  q = p_k - s * gw,  p_{k+1} = clamp(clamp(q, p_0 -+ max_move), lo, hi)
// The gradient is evaluated by the per-point code tvr_density_gradient runs (tvr_gradient.h), in its mapping: VM scenes a quad per vertex (4 lanes x 4 of the 16
// channels, quad reduction), CP scenes a lane per vertex.  Nothing per iteration goes to memory: a vertex is read once, iterated in registers and written once.
//
// The loop runs N + 1 evaluations in EVERY lane: a vertex that has converged, is pinned, was frozen by a non-finite value or lies behind the end of the array is HELD
// by selection (its state is no longer written) and does not leave the loop, so the trip count is wave-uniform and the quad shuffles always meet all four lanes.
// No position depends on an atomic or on another vertex: the output is a function of the arguments alone.  The four counters are summed per wave (ballot + popcount)
// and added with one 64-bit vector atomic per counter and wave; integer sums do not depend on the order they land in.
#include "tvr_device.h"
#include "tvr_kernels.h"
#include "tvr_gradient.h"

struct ProjectArgs {
    const float *verts;                // [V,3]
    const unsigned char *pinned;       // [V] or nullptr
    long long n_vertices;
    float target;                      // f*
    int iterations;                    // N
    float3 h, inv2h;                   // tvr_density_gradient's half width and 0.5 / h
    float3 max_move;
    float tol;
    float *verts_out;                  // [V,3]
    float *residual_in;                // [V] or nullptr
    float *residual_out;               // [V]
    unsigned long long *counts;        // [4] converged, moved, clamped, non-finite
};

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.4028234664e38f; }       // false for NaN and +-inf
__device__ __forceinline__ float clamp_f(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

template <bool CP>
__global__ __launch_bounds__(256) void mesh_project_kernel(const SceneDev sc, const CpDev cp, const ProjectArgs a)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long v = CP ? t : (t >> 2);
    const int sub = threadIdx.x & 3;
    const bool have = v < a.n_vertices;
    const bool owner = have && (CP || sub == 0);             // the lane that writes the vertex and is counted
    // a lane behind the end iterates the box's centre (every load stays inside the packed images whatever the coordinate: axis_tap / cp_tap clamp) and writes nothing
    float p0x = 0.0f, p0y = 0.0f, p0z = 0.0f;
    bool pin = false;
    if (have) {
        p0x = a.verts[(size_t)v * 3 + 0]; p0y = a.verts[(size_t)v * 3 + 1]; p0z = a.verts[(size_t)v * 3 + 2];
        pin = a.pinned != nullptr && a.pinned[v] != 0;
    }
    // the trust box about p_0 (rounded fp32 bounds)
    const float bxl = p0x - a.max_move.x, bxh = p0x + a.max_move.x, byl = p0y - a.max_move.y, byh = p0y + a.max_move.y, bzl = p0z - a.max_move.z, bzh = p0z + a.max_move.z;
    float px = p0x, py = p0y, pz = p0z;                      // p_k
    float bx = p0x, by = p0y, bz = p0z;                      // the best iterate so far (the result when the loop ends)
    float best_r = 0.0f, best_a = 0.0f, r0 = 0.0f;
    bool have_best = false, held = false, converged = false, clamped = false, nonfinite = false;
    if (!(finite_f(p0x) && finite_f(p0y) && finite_f(p0z))) { nonfinite = true; held = true; }       // (k = 0 is still evaluated: its r is the vertex's residual)

#pragma unroll 1
    for (int k = 0; k <= a.iterations; ++k) {
        const float nx = (px - sc.lo[0]) * sc.inv[0] - 1.0f, ny = (py - sc.lo[1]) * sc.inv[1] - 1.0f, nz = (pz - sc.lo[2]) * sc.inv[2] - 1.0f;
        float f[7];
        if (CP) {
            cp_grad_point(sc, cp, nx, ny, nz, a.h, f);
        } else {
            vm_grad_point(sc, nx, ny, nz, a.h, sub, f);
#pragma unroll
            for (int j = 0; j < 7; ++j) {                    // density_gradient_kernel's quad reduction: every lane of the quad ends with the same bits
                f[j] += __shfl_xor(f[j], 1);
                f[j] += __shfl_xor(f[j], 2);
            }
        }
        const float r = f[0] - a.target;
        if (k == 0) { r0 = r; best_r = r; }
        if (!held) {
            if (!finite_f(r)) {
                nonfinite = true; held = true;
            } else {
                const float ar = fabsf(r);
                if (!have_best || ar < best_a) { bx = px; by = py; bz = pz; best_r = r; best_a = ar; have_best = true; }
                if (ar <= a.tol) { converged = true; held = true; }
                else if (pin) held = true;
            }
        }
        if (!held && k < a.iterations) {
            const float gx = (f[1] - f[2]) * a.inv2h.x, gy = (f[3] - f[4]) * a.inv2h.y, gz = (f[5] - f[6]) * a.inv2h.z;
            const float wx = gx * sc.inv[0], wy = gy * sc.inv[1], wz = gz * sc.inv[2];
            const float s = r / fmaxf((wx * wx + wy * wy) + wz * wz, 1e-30f);
            const float qx = px - s * wx, qy = py - s * wy, qz = pz - s * wz;
            if (!(finite_f(qx) && finite_f(qy) && finite_f(qz))) {
                nonfinite = true; held = true;
            } else {
                const float cx = clamp_f(clamp_f(qx, bxl, bxh), sc.lo[0], sc.hi[0]);
                const float cy = clamp_f(clamp_f(qy, byl, byh), sc.lo[1], sc.hi[1]);
                const float cz = clamp_f(clamp_f(qz, bzl, bzh), sc.lo[2], sc.hi[2]);
                clamped = clamped || cx != qx || cy != qy || cz != qz;
                px = cx; py = cy; pz = cz;
            }
        }
    }

    // moved: the result differs from p_0 in some bit (a frozen or pinned vertex never does: its best iterate is p_0 or none)
    const bool moved = __float_as_uint(bx) != __float_as_uint(p0x) || __float_as_uint(by) != __float_as_uint(p0y) || __float_as_uint(bz) != __float_as_uint(p0z);
    if (owner) {
        a.verts_out[(size_t)v * 3 + 0] = bx; a.verts_out[(size_t)v * 3 + 1] = by; a.verts_out[(size_t)v * 3 + 2] = bz;
        if (a.residual_in) a.residual_in[v] = r0;
        a.residual_out[v] = best_r;
    }
    const unsigned long long m0 = __ballot(owner && converged), m1 = __ballot(owner && moved), m2 = __ballot(owner && clamped), m3 = __ballot(owner && nonfinite);
    if ((threadIdx.x & 63) == 0) {
        if (m0) atomicAdd(a.counts + 0, (unsigned long long)__popcll(m0));
        if (m1) atomicAdd(a.counts + 1, (unsigned long long)__popcll(m1));
        if (m2) atomicAdd(a.counts + 2, (unsigned long long)__popcll(m2));
        if (m3) atomicAdd(a.counts + 3, (unsigned long long)__popcll(m3));
    }
}

hipError_t launch_mesh_project(const SceneDev &sc, const CpDev *cp, const float *verts, long long n_vertices, const unsigned char *pinned, float target_feature,
                               int iterations, const float h[3], const float inv2h[3], const float max_move[3], float tol, float *verts_out, float *residual_in,
                               float *residual_out, unsigned long long *counts, hipStream_t stream)
{
    ProjectArgs a;
    a.verts = verts; a.pinned = pinned; a.n_vertices = n_vertices; a.target = target_feature; a.iterations = iterations;
    a.h = make_float3(h[0], h[1], h[2]); a.inv2h = make_float3(inv2h[0], inv2h[1], inv2h[2]); a.max_move = make_float3(max_move[0], max_move[1], max_move[2]);
    a.tol = tol; a.verts_out = verts_out; a.residual_in = residual_in; a.residual_out = residual_out; a.counts = counts;
    const long long lanes = cp ? n_vertices : n_vertices * 4;
    const long long blocks = (lanes + 255) / 256;
    const CpDev none = {};
    if (cp) hipLaunchKernelGGL((mesh_project_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, stream, sc, *cp, a);
    else hipLaunchKernelGGL((mesh_project_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, stream, sc, none, a);
    return hipGetLastError();
}
