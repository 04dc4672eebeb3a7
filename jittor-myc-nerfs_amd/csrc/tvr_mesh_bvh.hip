// tvr_mesh_bvh.hip — a linear bounding-volume hierarchy over the triangles of an indexed mesh and the ray queries that walk it: closest hit, any hit, and the
// cosine-weighted openness of points on the mesh (mesh.build_bvh / cast_rays / ambient_occlusion, TensorBase.export_mesh(ao=), reconstruct --mesh_ao).  include/tvr.h
// tvr_mesh_bvh_* holds the definition; DESIGN.md §4.17 the reasoning.  A (ray, triangle) pair is judged by the rasteriser's expressions (tvr_mesh_raster.hip rs_setup /
// rs_pixel) with the camera rotation taken as the identity and the camera centre at the ray's origin; they are restated in bv_triangle (tvr_mesh_bvh_tree.h), fp contraction is off, and
// tests/test_gpu_mesh_bvh.py ties the two files together.
//
//   keys     bbox_init, bbox (finite extent of the triangles that count: a wave-level min / max, then one atomic per wave and component on order-preserving integer
//            images of the floats — min and max do not depend on the order they land in), keys (30-bit Morton code of the centroid << 32 | triangle)
//   build    check (keys strictly ascending, codes below 2^30, every triangle exactly once, face indices inside 0 .. V-1), leaves (exact min / max boxes in key order),
//            topology (Karras 2012: every internal node finds its range and split from the sorted keys alone), 62 refit passes, finish (header, counts, root check)
//   cast     one lane per ray, a 64-entry stack per lane in LDS, nearer child first; occlusion: one lane per point, its K rays in table order
//   nearest  the closest point of the mesh to a point (mesh.closest_points / mesh_distance): the cast's walk with the boxes ordered and pruned by a
//            padded lower bound of their squared distance; a (point, triangle) pair by Ericson's regions in the frame translated to the point
//   signed   the same walk, then the sign from the pseudo-normal of the feature under the closest point (tvr_mesh_pseudo.hip's table; mesh.signed_distance,
//            DESIGN.md §4.19); the points come from an array or from a lattice
//   (the winding numbers of DESIGN.md §4.20 walk the same blob from tvr_mesh_winding.hip, the triangle pairs of §4.21 from tvr_mesh_crossings.hip; tvr_mesh_bvh_tree.h
//   holds what the files share, bv_triangle and bv_ray — the (ray, triangle) pair — among it)
//
// REFIT.  No workgroup hands data to another inside a launch.  `pass` [F-1] holds, per internal node, the number of the launch that computed its box (0 = not yet; leaves
// count as pass 1).  Launch p = 2 .. 63 computes a node iff it has no box and both children carry a pass number in 1 .. p-1, i.e. were finished by an EARLIER launch:
// a number p written by a neighbour during this launch is ignored whether the load sees it or not, so every box that is read was complete before the launch began and the
// kernel boundary is the only ordering.  The tree's height is at most 62 (keys have 62 significant bits and every level of the topology splits on one of them), so 62
// launches always finish the root; a root left without a box raises the fault flag.  pass[0] - 1 is the height.
//
// Every index read from the blob or the faces is compared with its bound before it is used (node < 2F-1, leaf < F, triangle < F, vertex < V) and every stack push with
// the stack's size: no load or store leaves the caller's buffers whatever the blob, the keys and the faces hold.
#include "tvr_mesh_bvh_tree.h"          // the blob's header, BvTree, BvLattice, BvRay, BV_PAD, bv_finite, bv_dot, bv_tree, bv_blob_ok, bv_triangle, bv_ray: shared

struct BvBuildScratch {
    unsigned *header;                   // [64]: word 0 bad, word 1 skipped triangles
    unsigned *pass;                     // [F-1]
    unsigned *seen;                     // [(F+31)/32] bits
};

// order-preserving image of a float in the unsigned integers (for atomicMin / atomicMax)
__device__ __forceinline__ unsigned bv_order(float x) { const unsigned u = __float_as_uint(x); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float bv_unorder(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// the three corners of triangle t (< F): false when an index is outside 0 .. V-1 or a coordinate is not finite
__device__ __forceinline__ bool bv_corners(const float *__restrict__ verts, const int *__restrict__ faces, unsigned V, unsigned t, float c[9], bool &bad_index)
{
    const int *f = faces + (size_t)t * 3;
    const int v0 = f[0], v1 = f[1], v2 = f[2];
    bad_index = (unsigned)v0 >= V || (unsigned)v1 >= V || (unsigned)v2 >= V;
    if (bad_index) return false;
    bool fin = true;
    for (int k = 0; k < 3; ++k) {
        c[k] = verts[(size_t)v0 * 3 + k]; c[3 + k] = verts[(size_t)v1 * 3 + k]; c[6 + k] = verts[(size_t)v2 * 3 + k];
        fin = fin && bv_finite(c[k]) && bv_finite(c[3 + k]) && bv_finite(c[6 + k]);
    }
    return fin;
}

// ---- keys -----------------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ void bv_bbox_init_kernel(unsigned *__restrict__ s)
{
    if (threadIdx.x < 3) s[threadIdx.x] = 0xffffffffu;              // running minima
    else if (threadIdx.x < 6) s[threadIdx.x] = 0u;                   // running maxima
}

__global__ __launch_bounds__(BV_THREADS) void bv_bbox_kernel(const float *__restrict__ verts, unsigned V, const int *__restrict__ faces, unsigned F, unsigned *__restrict__ s,
                                                             unsigned *__restrict__ fault)
{
    const unsigned t = blockIdx.x * BV_THREADS + threadIdx.x;
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    if (t < F) {
        float c[9];
        bool bad;
        if (bv_corners(verts, faces, V, t, c, bad))
            for (int k = 0; k < 3; ++k) {
                lo[k] = bv_order(fminf(fminf(c[k], c[3 + k]), c[6 + k]));
                hi[k] = bv_order(fmaxf(fmaxf(c[k], c[3 + k]), c[6 + k]));
            }
        if (bad) *fault = 1u;
    }
    for (int k = 0; k < 3; ++k) {
        for (int o = 32; o; o >>= 1) {
            lo[k] = min(lo[k], (unsigned)__shfl_xor((int)lo[k], o, 64));
            hi[k] = max(hi[k], (unsigned)__shfl_xor((int)hi[k], o, 64));
        }
        if ((threadIdx.x & 63u) == 0) {
            if (lo[k] != 0xffffffffu) atomicMin(s + k, lo[k]);
            if (hi[k] != 0u) atomicMax(s + 3 + k, hi[k]);
        }
    }
}

__device__ __forceinline__ unsigned bv_spread(unsigned x)           // 10 bits -> every third bit
{
    x &= 0x3ffu;
    x = (x | (x << 16)) & 0x030000ffu;
    x = (x | (x << 8)) & 0x0300f00fu;
    x = (x | (x << 4)) & 0x030c30c3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

__global__ __launch_bounds__(BV_THREADS) void bv_keys_kernel(const float *__restrict__ verts, unsigned V, const int *__restrict__ faces, unsigned F,
                                                             const unsigned *__restrict__ s, u64 *__restrict__ keys)
{
    const unsigned t = blockIdx.x * BV_THREADS + threadIdx.x;
    if (t >= F) return;
    float c[9];
    bool bad;
    unsigned code = 0x3fffffffu;                                     // skipped triangles: the largest code
    if (bv_corners(verts, faces, V, t, c, bad)) {
        unsigned q[3];
        for (int k = 0; k < 3; ++k) {
            const float lo = bv_unorder(s[k]), hi = bv_unorder(s[3 + k]);
            const float m = ((c[k] + c[3 + k]) + c[6 + k]) * 0.333333343f, ext = hi - lo;
            float u = ext > 0.0f ? ((m - lo) / ext) * 1024.0f : 0.0f;
            u = fminf(fmaxf(u, 0.0f), 1023.0f);                      // (a NaN becomes 0)
            q[k] = (unsigned)u;
        }
        code = (bv_spread(q[0]) << 2) | (bv_spread(q[1]) << 1) | bv_spread(q[2]);
    }
    keys[t] = ((u64)code << 32) | (u64)t;
}

// ---- build ----------------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BV_THREADS) void bv_check_kernel(const u64 *__restrict__ keys, const int *__restrict__ faces, unsigned F, unsigned V, BvBuildScratch s,
                                                              unsigned *__restrict__ fault)
{
    const unsigned i = blockIdx.x * BV_THREADS + threadIdx.x;
    if (i >= F) return;
    const u64 k = keys[i];
    const unsigned t = (unsigned)(k & 0xffffffffull);
    bool bad = (k >> 62) != 0 || t >= F || (i + 1 < F && !(k < keys[i + 1]));
    if (!bad) bad = (atomicOr(s.seen + (t >> 5), 1u << (t & 31u)) >> (t & 31u)) & 1u;         // a triangle named twice
    const int *f = faces + (size_t)i * 3;
    if ((unsigned)f[0] >= V || (unsigned)f[1] >= V || (unsigned)f[2] >= V) bad = true;
    if (bad) {
        s.header[0] = 1u;
        *fault = 1u;
    }
}

__global__ __launch_bounds__(BV_THREADS) void bv_leaves_kernel(const u64 *__restrict__ keys, BvTree T, BvBuildScratch s)
{
    if (s.header[0]) return;
    const unsigned i = blockIdx.x * BV_THREADS + threadIdx.x;
    bool skipped = false;
    if (i < T.F) {
        const unsigned t = (unsigned)(keys[i] & 0xffffffffull);        // < F: the check kernel saw to it
        float c[9], lo[3], hi[3];
        bool bad;
        const float inf = __uint_as_float(0x7f800000u);
        if (t < T.F && bv_corners(T.verts, T.faces, T.V, t, c, bad))
            for (int k = 0; k < 3; ++k) {
                lo[k] = fminf(fminf(c[k], c[3 + k]), c[6 + k]);
                hi[k] = fmaxf(fmaxf(c[k], c[3 + k]), c[6 + k]);
            }
        else {                                                       // never hit: the empty box, which a union ignores and no ray enters
            skipped = true;
            for (int k = 0; k < 3; ++k) { lo[k] = inf; hi[k] = -inf; }
        }
        float *b = T.box + ((size_t)(T.F - 1) + i) * 6;
        for (int k = 0; k < 3; ++k) { b[k] = lo[k]; b[3 + k] = hi[k]; }
        T.leaf_tri[i] = (int)t;
    }
    const u64 m = __ballot(skipped);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(s.header + 1, (unsigned)__popcll(m));
}

__device__ __forceinline__ int bv_delta(const u64 *__restrict__ keys, long long F, long long i, long long j)
{
    if (j < 0 || j >= F) return -1;
    return __clzll((long long)(keys[i] ^ keys[j]));                   // keys are unique: the xor is never 0
}

__global__ __launch_bounds__(BV_THREADS) void bv_topology_kernel(const u64 *__restrict__ keys, BvTree T, BvBuildScratch s)
{
    if (s.header[0]) return;
    const long long F = T.F, i = (long long)blockIdx.x * BV_THREADS + threadIdx.x;
    if (i >= F - 1) return;
    const long long d = bv_delta(keys, F, i, i + 1) > bv_delta(keys, F, i, i - 1) ? 1 : -1;
    const int dmin = bv_delta(keys, F, i, i - d);
    long long lmax = 2;
    while (bv_delta(keys, F, i, i + lmax * d) > dmin) lmax *= 2;      // (ends: beyond the array delta is -1 <= dmin)
    long long l = 0;
    for (long long t = lmax / 2; t >= 1; t /= 2)
        if (bv_delta(keys, F, i, i + (l + t) * d) > dmin) l += t;
    const long long j = i + l * d;
    const int dnode = bv_delta(keys, F, i, j);
    long long sp = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (bv_delta(keys, F, i, i + (sp + t) * d) > dnode) sp += t;
    } while (t > 1);
    const long long g = i + sp * d + (d < 0 ? -1 : 0), first = i < j ? i : j, last = i < j ? j : i;
    T.child[i * 2 + 0] = (int)(g == first ? (F - 1) + g : g);
    T.child[i * 2 + 1] = (int)(g + 1 == last ? (F - 1) + g + 1 : g + 1);
}

__global__ __launch_bounds__(BV_THREADS) void bv_refit_kernel(BvTree T, BvBuildScratch s, unsigned p)
{
    if (s.header[0]) return;
    const unsigned i = blockIdx.x * BV_THREADS + threadIdx.x;
    if (T.F < 2 || i >= T.F - 1 || s.pass[i] != 0u) return;
    const unsigned n_nodes = 2u * T.F - 1u, a = (unsigned)T.child[(size_t)i * 2], b = (unsigned)T.child[(size_t)i * 2 + 1];
    if (a >= n_nodes || b >= n_nodes) return;                        // (never: the topology kernel wrote them)
    const unsigned pa = a >= T.F - 1 ? 1u : s.pass[a], pb = b >= T.F - 1 ? 1u : s.pass[b];
    if (pa == 0u || pa >= p || pb == 0u || pb >= p) return;          // a child this very launch finishes does not count: its box may be half written
    const float *A = T.box + (size_t)a * 6, *B = T.box + (size_t)b * 6;
    float *o = T.box + (size_t)i * 6;
    for (int k = 0; k < 3; ++k) { o[k] = fminf(A[k], B[k]); o[3 + k] = fmaxf(A[3 + k], B[3 + k]); }
    s.pass[i] = p;
}

__global__ void bv_finish_kernel(BvTree T, BvBuildScratch s, int *__restrict__ counts, unsigned *__restrict__ fault)
{
    if (threadIdx.x != 0) return;
    BvHeader *h = T.h;
    h->magic = BV_MAGIC; h->F = T.F; h->bad = s.header[0];
    unsigned height = 0;
    if (!s.header[0] && T.F >= 2) {
        if (s.pass[0] == 0u) {                                       // the passes did not reach the root
            h->bad = 2u;
            *fault = 1u;
        } else
            height = s.pass[0] - 1u;
    }
    h->height = height; h->skipped = s.header[1];
    for (int k = 0; k < 3; ++k) {
        h->lo[k] = T.F && !h->bad ? T.box[k] : 0.0f;
        h->hi[k] = T.F && !h->bad ? T.box[3 + k] : 0.0f;
    }
    if (counts) { counts[0] = (int)s.header[1]; counts[1] = (int)height; counts[2] = T.F ? (int)(T.F - 1) : 0; counts[3] = (int)h->bad; }
}

size_t mesh_bvh_bytes(long long F, MeshBvhCarve *c)
{
    MeshBvhCarve L;
    const size_t n = (size_t)F;
    L.header = 0;
    L.box = MESH_BVH_HEADER_BYTES;
    L.child = L.box + bv_align((n ? 2 * n - 1 : 0) * 6 * sizeof(float));
    L.leaf_tri = L.child + bv_align((n ? n - 1 : 0) * 2 * sizeof(int));
    L.total = L.leaf_tri + bv_align(n * sizeof(int));
    if (c) *c = L;
    return L.total;
}

size_t mesh_bvh_scratch_bytes(long long F)
{
    const size_t n = (size_t)F;
    return 256 + bv_align((n ? n - 1 : 0) * sizeof(unsigned)) + bv_align((n + 31) / 32 * sizeof(unsigned));
}

hipError_t launch_mesh_bvh_keys(const float *verts, long long V, const int *faces, long long F, unsigned long long *keys, void *scratch, unsigned *fault, hipStream_t stream)
{
    const unsigned fb = (unsigned)((F + BV_THREADS - 1) / BV_THREADS);
    hipLaunchKernelGGL(bv_bbox_init_kernel, dim3(1), dim3(64), 0, stream, (unsigned *)scratch);
    if (fb) {
        hipLaunchKernelGGL(bv_bbox_kernel, dim3(fb), dim3(BV_THREADS), 0, stream, verts, (unsigned)V, faces, (unsigned)F, (unsigned *)scratch, fault);
        hipLaunchKernelGGL(bv_keys_kernel, dim3(fb), dim3(BV_THREADS), 0, stream, verts, (unsigned)V, faces, (unsigned)F, (const unsigned *)scratch, keys);
    }
    return hipGetLastError();
}

hipError_t launch_mesh_bvh_build(const float *verts, long long V, const int *faces, long long F, const unsigned long long *keys, void *bvh, void *scratch, int *counts,
                                 unsigned *fault, hipStream_t stream)
{
    const size_t n = (size_t)F;
    hipError_t e = hipMemsetAsync(bvh, 0, mesh_bvh_bytes(F, nullptr), stream);          // padding included: the blob is a function of the mesh alone
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(scratch, 0, mesh_bvh_scratch_bytes(F), stream);
    if (e != hipSuccess) return e;
    BvTree T = bv_tree(verts, V, faces, F, bvh);
    BvBuildScratch s;
    s.header = (unsigned *)scratch;
    s.pass = (unsigned *)((char *)scratch + 256);
    s.seen = (unsigned *)((char *)s.pass + bv_align((n ? n - 1 : 0) * sizeof(unsigned)));
    const unsigned fb = (unsigned)((F + BV_THREADS - 1) / BV_THREADS), ib = F > 1 ? (unsigned)((F - 1 + BV_THREADS - 1) / BV_THREADS) : 0u;
    if (fb) {
        hipLaunchKernelGGL(bv_check_kernel, dim3(fb), dim3(BV_THREADS), 0, stream, keys, faces, (unsigned)F, (unsigned)V, s, fault);
        hipLaunchKernelGGL(bv_leaves_kernel, dim3(fb), dim3(BV_THREADS), 0, stream, keys, T, s);
    }
    if (ib) {
        hipLaunchKernelGGL(bv_topology_kernel, dim3(ib), dim3(BV_THREADS), 0, stream, keys, T, s);
        for (unsigned p = 2; p < 2 + BV_PASSES; ++p) hipLaunchKernelGGL(bv_refit_kernel, dim3(ib), dim3(BV_THREADS), 0, stream, T, s, p);
    }
    hipLaunchKernelGGL(bv_finish_kernel, dim3(1), dim3(64), 0, stream, T, s, counts, fault);
    return hipGetLastError();
}

// ---- traversal ------------------------------------------------------------------------------------------------------------------------------------------------------------
struct BvHit {
    float t;                                         // the bound: t_max before a hit, the best t after
    unsigned tri;                                    // 0xffffffff before a hit
    float E0, E1, E2;
};

// The padded slab test of box b against the ray over [t_min, best]: the entry parameter in tn.  Every face of the box is moved outwards by BV_PAD x the largest
// distance, along an axis, from the origin to the box.  fminf / fmaxf drop a NaN (0 x inf: the origin in a face's plane, the direction along it).
__device__ __forceinline__ bool bv_slab(const float *__restrict__ b, const BvRay &r, float best, float &tn)
{
    const float lx = b[0] - r.ox, ly = b[1] - r.oy, lz = b[2] - r.oz, hx = b[3] - r.ox, hy = b[4] - r.oy, hz = b[5] - r.oz;
    const float m = fmaxf(fmaxf(fmaxf(fabsf(lx), fabsf(hx)), fmaxf(fabsf(ly), fabsf(hy))), fmaxf(fabsf(lz), fabsf(hz)));
    const float pad = m * BV_PAD;
    const float ax = (lx - pad) * r.ix, bx = (hx + pad) * r.ix, ay = (ly - pad) * r.iy, by = (hy + pad) * r.iy, az = (lz - pad) * r.iz, bz = (hz + pad) * r.iz;
    tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
    const float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
    return tn <= tf && tf >= r.t_min && !(tn > best) && lx <= hx;        // (an empty box has lo = +inf, hi = -inf: lx <= hx is false)
}

// Walk the tree for one ray.  stack: this lane's BV_STACK entries, `stride` words apart.  H.t holds t_max on entry.  Returns whether anything was hit.
template <bool ANY>
__device__ __forceinline__ bool bv_walk(const BvTree &T, const BvRay &r, float t_max, BvHit &H, unsigned *stack, unsigned stride, unsigned &node_tests, unsigned &tri_tests,
                                        unsigned *__restrict__ fault)
{
    H.t = t_max; H.tri = 0xffffffffu; H.E0 = H.E1 = H.E2 = 0.0f;
    if (T.F == 0) return false;
    const unsigned n_nodes = 2u * T.F - 1u, first_leaf = T.F - 1u;
    unsigned sp = 0, node = 0;
    float tn;
    ++node_tests;
    if (!bv_slab(T.box, r, H.t, tn)) return false;
    for (unsigned budget = n_nodes;; --budget) {
        if (budget == 0u) {                                          // a tree visits every node at most once: a blob with a cycle in it ends here
            *fault = 1u;
            return H.tri != 0xffffffffu;
        }
        bool pop = true;
        if (node >= first_leaf) {
            const unsigned t = (unsigned)T.leaf_tri[node - first_leaf];
            if (t < T.F) {
                float E[3], tt;
                ++tri_tests;
                if (bv_triangle(T, t, r, t_max, E, tt, fault) && (tt < H.t || (tt == H.t && t < H.tri))) {
                    H.t = tt; H.tri = t; H.E0 = E[0]; H.E1 = E[1]; H.E2 = E[2];
                    if (ANY) return true;
                }
            } else
                *fault = 1u;
        } else {
            const unsigned a = (unsigned)T.child[(size_t)node * 2], b = (unsigned)T.child[(size_t)node * 2 + 1];
            if (a < n_nodes && b < n_nodes) {
                float ta, tb;
                node_tests += 2;
                const bool ha = bv_slab(T.box + (size_t)a * 6, r, H.t, ta), hb = bv_slab(T.box + (size_t)b * 6, r, H.t, tb);
                if (ha && hb) {
                    const bool a_first = ta <= tb;                   // the nearer child first, the farther one waits: at most one entry per level
                    const unsigned far_ = a_first ? b : a;
                    node = a_first ? a : b;
                    if (sp < BV_STACK) stack[(sp++) * stride] = far_;
                    else *fault = 1u;                                // (never: the height is at most 62)
                    pop = false;
                } else if (ha || hb) {
                    node = ha ? a : b;
                    pop = false;
                }
            } else
                *fault = 1u;
        }
        while (pop) {
            if (sp == 0) return H.tri != 0xffffffffu;
            node = stack[(--sp) * stride];
            if (node >= n_nodes) { *fault = 1u; continue; }
            ++node_tests;
            pop = !bv_slab(T.box + (size_t)node * 6, r, H.t, tn);    // the bound may have dropped since the push
        }
    }
}

// the wave's sums of the four counters: one atomic per wave and counter
__device__ __forceinline__ void bv_count(unsigned long long *__restrict__ counts, bool hit, bool refused, unsigned node_tests, unsigned tri_tests)
{
    if (!counts) return;
    const u64 mh = __ballot(hit), mr = __ballot(refused);
    for (int o = 32; o; o >>= 1) {
        node_tests += (unsigned)__shfl_xor((int)node_tests, o, 64);   // (a ray makes far fewer than 2^32 / 64 tests)
        tri_tests += (unsigned)__shfl_xor((int)tri_tests, o, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (mh) atomicAdd(counts + 0, (unsigned long long)__popcll(mh));
        if (mr) atomicAdd(counts + 1, (unsigned long long)__popcll(mr));
        if (node_tests) atomicAdd(counts + 2, (unsigned long long)node_tests);
        if (tri_tests) atomicAdd(counts + 3, (unsigned long long)tri_tests);
    }
}

template <bool ANY>
__global__ __launch_bounds__(BV_CAST_THREADS) void bv_cast_kernel(BvTree T, const float *__restrict__ origins, const float *__restrict__ dirs, unsigned N, float t_min,
                                                                  float t_max, int cull, float *__restrict__ t_out, int *__restrict__ tri_out, float *__restrict__ bary_out,
                                                                  unsigned char *__restrict__ hit_out, unsigned long long *__restrict__ counts,
                                                                  unsigned *__restrict__ fault)
{
    __shared__ unsigned stack[BV_STACK * BV_CAST_THREADS];            // entry e of lane l at [e * BV_CAST_THREADS + l]: a wave's accesses to one depth are contiguous
    const bool ok = bv_blob_ok(T, fault);
    const unsigned i = blockIdx.x * BV_CAST_THREADS + threadIdx.x;
    bool hit = false, refused = false;
    unsigned node_tests = 0, tri_tests = 0;
    if (i < N) {
        BvRay r;
        BvHit H;
        H.t = t_max; H.tri = 0xffffffffu; H.E0 = H.E1 = H.E2 = 0.0f;
        const float *o = origins + (size_t)i * 3, *d = dirs + (size_t)i * 3;
        refused = !bv_ray(r, o[0], o[1], o[2], d[0], d[1], d[2], t_min, cull);
        if (ok && !refused) hit = bv_walk<ANY>(T, r, t_max, H, stack + threadIdx.x, BV_CAST_THREADS, node_tests, tri_tests, fault);
        if (ANY)
            hit_out[i] = hit ? 1 : 0;
        else {
            const float sum = (H.E0 + H.E1) + H.E2;
            t_out[i] = hit ? H.t : __uint_as_float(0x7f800000u);
            tri_out[i] = hit ? (int)H.tri : -1;
            bary_out[(size_t)i * 3 + 0] = hit ? H.E0 / sum : 0.0f;
            bary_out[(size_t)i * 3 + 1] = hit ? H.E1 / sum : 0.0f;
            bary_out[(size_t)i * 3 + 2] = hit ? H.E2 / sum : 0.0f;
        }
    }
    bv_count(counts, hit, refused, node_tests, tri_tests);
}

// ---- closest point (tvr_mesh_bvh_nearest) ------------------------------------------------------------------------------------------------------------------
struct BvNear {
    float D;                                         // the bound: max_dist^2 before a candidate, the best squared distance after
    unsigned tri;                                    // 0xffffffff before a candidate
    float w0, w1, w2;
};

// A lower bound of the squared distance from p to box b, every face of the box moved outwards by BV_PAD x the largest distance, along an axis, from p to the box.
// false for an empty box (lo = +inf, hi = -inf) and for a bound STRICTLY above `best` (an equal D may still win on the index).
__device__ __forceinline__ bool bv_near_box(const float *__restrict__ b, float px, float py, float pz, float best, float &lb)
{
    const float lx = b[0] - px, ly = b[1] - py, lz = b[2] - pz, hx = b[3] - px, hy = b[4] - py, hz = b[5] - pz;
    const float m = fmaxf(fmaxf(fmaxf(fabsf(lx), fabsf(hx)), fmaxf(fabsf(ly), fabsf(hy))), fmaxf(fabsf(lz), fabsf(hz)));
    const float pad = m * BV_PAD;
    const float gx = fmaxf(fmaxf(lx - pad, -(hx + pad)), 0.0f), gy = fmaxf(fmaxf(ly - pad, -(hy + pad)), 0.0f), gz = fmaxf(fmaxf(lz - pad, -(hz + pad)), 0.0f);
    lb = bv_dot(gx, gy, gz, gx, gy, gz);
    return !(lb > best) && lx <= hx;
}

// (point, triangle t): the definition of include/tvr.h tvr_mesh_bvh_nearest — Ericson's regions in the frame translated to p.  false when D is not finite.
// region: which of the seven held (1 .. 7); xo: the closest point in the translated frame (p - closest = -xo) — what the signed query reads; the walk drops both.
__device__ __forceinline__ bool bv_near_pair(const BvTree &T, unsigned t, float px, float py, float pz, float &D, float w[3], int &region, float xo[3],
                                             unsigned *__restrict__ fault)
{
    region = 0; xo[0] = xo[1] = xo[2] = 0.0f;
    const int *f = T.faces + (size_t)t * 3;
    const int v0 = f[0], v1 = f[1], v2 = f[2];
    if ((unsigned)v0 >= T.V || (unsigned)v1 >= T.V || (unsigned)v2 >= T.V) {
        *fault = 1u;
        return false;
    }
    const float *p0 = T.verts + (size_t)v0 * 3, *p1 = T.verts + (size_t)v1 * 3, *p2 = T.verts + (size_t)v2 * 3;
    const float ax = p0[0] - px, ay = p0[1] - py, az = p0[2] - pz;
    const float bx = p1[0] - px, by = p1[1] - py, bz = p1[2] - pz;
    const float cx = p2[0] - px, cy = p2[1] - py, cz = p2[2] - pz;
    const bool finite = bv_finite(ax) && bv_finite(ay) && bv_finite(az) && bv_finite(bx) && bv_finite(by) && bv_finite(bz) && bv_finite(cx) && bv_finite(cy) && bv_finite(cz);
    if (!finite) return false;
    const float abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
    const float d1 = -bv_dot(abx, aby, abz, ax, ay, az), d2 = -bv_dot(acx, acy, acz, ax, ay, az);
    const float d3 = -bv_dot(abx, aby, abz, bx, by, bz), d4 = -bv_dot(acx, acy, acz, bx, by, bz);
    const float d5 = -bv_dot(abx, aby, abz, cx, cy, cz), d6 = -bv_dot(acx, acy, acz, cx, cy, cz);
    // va, vb, vc: the triple products of the corners with the normal — Ericson's d-products in exact arithmetic, without their cancellation on thin triangles
    const float bcx = cx - bx, bcy = cy - by, bcz = cz - bz;
    const float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    const float va = bv_dot(by * bcz - bz * bcy, bz * bcx - bx * bcz, bx * bcy - by * bcx, nx, ny, nz);            // (b x bc) . n
    const float vb = bv_dot(acy * az - acz * ay, acz * ax - acx * az, acx * ay - acy * ax, nx, ny, nz);            // (ac x a) . n
    const float vc = bv_dot(ay * abz - az * aby, az * abx - ax * abz, ax * aby - ay * abx, nx, ny, nz);            // (a x ab) . n
    float x, y, z;
    if (d1 <= 0.0f && d2 <= 0.0f) {                                  // 1: vertex A
        x = ax; y = ay; z = az; region = 1;
        w[0] = 1.0f; w[1] = 0.0f; w[2] = 0.0f;
    } else if (d3 >= 0.0f && d4 <= d3) {                             // 2: vertex B
        x = bx; y = by; z = bz; region = 2;
        w[0] = 0.0f; w[1] = 1.0f; w[2] = 0.0f;
    } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {             // 3: edge AB
        const float v = d1 / (d1 - d3);
        x = ax + v * abx; y = ay + v * aby; z = az + v * abz; region = 3;
        w[0] = 1.0f - v; w[1] = v; w[2] = 0.0f;
    } else if (d6 >= 0.0f && d5 <= d6) {                             // 4: vertex C
        x = cx; y = cy; z = cz; region = 4;
        w[0] = 0.0f; w[1] = 0.0f; w[2] = 1.0f;
    } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {             // 5: edge AC
        const float u = d2 / (d2 - d6);
        x = ax + u * acx; y = ay + u * acy; z = az + u * acz; region = 5;
        w[0] = 1.0f - u; w[1] = 0.0f; w[2] = u;
    } else if (va <= 0.0f && d4 - d3 >= 0.0f && d5 - d6 >= 0.0f) {   // 6: edge BC
        const float u = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        x = bx + u * bcx; y = by + u * bcy; z = bz + u * bcz; region = 6;
        w[0] = 0.0f; w[1] = 1.0f - u; w[2] = u;
    } else {                                                         // 7: the face
        const float den = (va + vb) + vc, v = vb / den, u = vc / den;
        x = (ax + v * abx) + u * acx; y = (ay + v * aby) + u * acy; z = (az + v * abz) + u * acz; region = 7;
        w[0] = (1.0f - v) - u; w[1] = v; w[2] = u;
    }
    xo[0] = x; xo[1] = y; xo[2] = z;
    D = bv_dot(x, y, z, x, y, z);
    return bv_finite(D);                                             // (a NaN is not finite: a zero-area triangle in region 7)
}

__device__ __forceinline__ bool bv_near_triangle(const BvTree &T, unsigned t, float px, float py, float pz, float &D, float w[3], unsigned *__restrict__ fault)
{
    int region;
    float x[3];
    return bv_near_pair(T, t, px, py, pz, D, w, region, x, fault);
}

// Walk the tree for one point.  H.D holds max_dist^2 on entry.  The shape of bv_walk: the nearer box first, the other pushed, a popped node tested again.
__device__ __forceinline__ void bv_near_walk(const BvTree &T, float px, float py, float pz, BvNear &H, unsigned *stack, unsigned stride, unsigned &node_tests,
                                             unsigned &tri_tests, unsigned *__restrict__ fault)
{
    if (T.F == 0) return;
    const unsigned n_nodes = 2u * T.F - 1u, first_leaf = T.F - 1u;
    unsigned sp = 0, node = 0;
    float lb;
    ++node_tests;
    if (!bv_near_box(T.box, px, py, pz, H.D, lb)) return;
    for (unsigned budget = n_nodes;; --budget) {
        if (budget == 0u) {                                          // a tree visits every node at most once: a blob with a cycle in it ends here
            *fault = 1u;
            return;
        }
        bool pop = true;
        if (node >= first_leaf) {
            const unsigned t = (unsigned)T.leaf_tri[node - first_leaf];
            if (t < T.F) {
                float w[3], D;
                ++tri_tests;
                if (bv_near_triangle(T, t, px, py, pz, D, w, fault) && (D < H.D || (D == H.D && t < H.tri))) {
                    H.D = D; H.tri = t; H.w0 = w[0]; H.w1 = w[1]; H.w2 = w[2];
                }
            } else
                *fault = 1u;
        } else {
            const unsigned a = (unsigned)T.child[(size_t)node * 2], b = (unsigned)T.child[(size_t)node * 2 + 1];
            if (a < n_nodes && b < n_nodes) {
                float la, lbb;
                node_tests += 2;
                const bool ha = bv_near_box(T.box + (size_t)a * 6, px, py, pz, H.D, la), hb = bv_near_box(T.box + (size_t)b * 6, px, py, pz, H.D, lbb);
                if (ha && hb) {
                    const bool a_first = la <= lbb;                  // the nearer child first, the farther one waits: at most one entry per level
                    const unsigned far_ = a_first ? b : a;
                    node = a_first ? a : b;
                    if (sp < BV_STACK) stack[(sp++) * stride] = far_;
                    else *fault = 1u;                                // (never: the height is at most 62)
                    pop = false;
                } else if (ha || hb) {
                    node = ha ? a : b;
                    pop = false;
                }
            } else
                *fault = 1u;
        }
        while (pop) {
            if (sp == 0) return;
            node = stack[(--sp) * stride];
            if (node >= n_nodes) { *fault = 1u; continue; }
            ++node_tests;
            pop = !bv_near_box(T.box + (size_t)node * 6, px, py, pz, H.D, lb);      // the bound may have dropped since the push
        }
    }
}

__global__ __launch_bounds__(BV_CAST_THREADS) void bv_nearest_kernel(BvTree T, const float *__restrict__ points, unsigned N, float max_sq, float *__restrict__ dist_out,
                                                                     int *__restrict__ tri_out, float *__restrict__ bary_out, unsigned long long *__restrict__ counts,
                                                                     unsigned *__restrict__ fault)
{
    __shared__ unsigned stack[BV_STACK * BV_CAST_THREADS];            // entry e of lane l at [e * BV_CAST_THREADS + l]
    const bool ok = bv_blob_ok(T, fault);
    const unsigned i = blockIdx.x * BV_CAST_THREADS + threadIdx.x;
    bool answered = false, refused = false;
    unsigned node_tests = 0, tri_tests = 0;
    if (i < N) {
        const float *p = points + (size_t)i * 3;
        const float px = p[0], py = p[1], pz = p[2];
        BvNear H;
        H.D = max_sq; H.tri = 0xffffffffu; H.w0 = H.w1 = H.w2 = 0.0f;
        refused = !(bv_finite(px) && bv_finite(py) && bv_finite(pz));
        if (ok && !refused) bv_near_walk(T, px, py, pz, H, stack + threadIdx.x, BV_CAST_THREADS, node_tests, tri_tests, fault);
        answered = H.tri != 0xffffffffu;
        dist_out[i] = answered ? sqrtf(H.D) : __uint_as_float(0x7f800000u);
        tri_out[i] = answered ? (int)H.tri : -1;
        bary_out[(size_t)i * 3 + 0] = answered ? H.w0 : 0.0f;
        bary_out[(size_t)i * 3 + 1] = answered ? H.w1 : 0.0f;
        bary_out[(size_t)i * 3 + 2] = answered ? H.w2 : 0.0f;
    }
    bv_count(counts, answered, refused, node_tests, tri_tests);
}

// ---- signed distance (tvr_mesh_bvh_signed) ------------------------------------------------------------------------------------------------------------------
struct BvNormals {                                   // the pseudo-normal table of tvr_mesh_pseudo.hip
    const MeshPseudoHeader *h;
    const float *face_n, *edge_n, *vert_n;           // [F][3], [F][3][3], [V][3]
};

__device__ __forceinline__ bool bv_table_ok(const BvTree &T, const BvNormals &P, unsigned *__restrict__ fault)
{
    const bool ok = P.h->magic == MESH_PSEUDO_MAGIC && P.h->F == T.F && P.h->V == T.V && P.h->bad == 0u;
    if (!ok && threadIdx.x == 0) *fault = 1u;
    return ok;
}

// bv_nearest_kernel's walk, then the winner's pair once more for its region and closest point x (the same expressions: the same bits), the normal N of the feature
// under x from the table, and the sign of s = -(N . x) = N . (p - closest).
__global__ __launch_bounds__(BV_CAST_THREADS) void bv_signed_kernel(BvTree T, BvNormals P, const float *__restrict__ points, BvLattice G, unsigned N, float max_sq,
                                                                    float *__restrict__ sdist_out, int *__restrict__ tri_out, float *__restrict__ bary_out,
                                                                    signed char *__restrict__ feature_out, unsigned long long *__restrict__ counts,
                                                                    unsigned *__restrict__ fault)
{
    __shared__ unsigned stack[BV_STACK * BV_CAST_THREADS];            // entry e of lane l at [e * BV_CAST_THREADS + l]
    const bool blob_ok = bv_blob_ok(T, fault), table_ok = bv_table_ok(T, P, fault), ok = blob_ok && table_ok;
    const unsigned i = blockIdx.x * BV_CAST_THREADS + threadIdx.x;
    bool answered = false, refused = false, undecided = false;
    unsigned node_tests = 0, tri_tests = 0;
    if (i < N) {
        float px, py, pz;
        if (points) {
            const float *p = points + (size_t)i * 3;
            px = p[0]; py = p[1]; pz = p[2];
        } else {
            const unsigned plane = G.ny * G.nz, ix = i / plane, r = i - ix * plane, iy = r / G.nz, iz = r - iy * G.nz;
            px = G.ox + (float)ix * G.sx; py = G.oy + (float)iy * G.sy; pz = G.oz + (float)iz * G.sz;
        }
        BvNear H;
        H.D = max_sq; H.tri = 0xffffffffu; H.w0 = H.w1 = H.w2 = 0.0f;
        refused = !(bv_finite(px) && bv_finite(py) && bv_finite(pz));
        if (ok && !refused) bv_near_walk(T, px, py, pz, H, stack + threadIdx.x, BV_CAST_THREADS, node_tests, tri_tests, fault);
        answered = H.tri != 0xffffffffu;
        float dist = __uint_as_float(0x7f800000u);
        int region = 0;
        if (answered) {
            float D, w[3], x[3];
            bv_near_pair(T, H.tri, px, py, pz, D, w, region, x, fault);
            dist = sqrtf(H.D);
            const int *f = T.faces + (size_t)H.tri * 3;
            const unsigned corner = region == 1 ? 0u : region == 2 ? 1u : 2u, v = (unsigned)f[corner];
            const float *n = P.face_n + (size_t)H.tri * 3;                                        // 7: the face
            if (region == 3) n = P.edge_n + ((size_t)H.tri * 3 + 2) * 3;                          // AB is edge 2 (from corner 0 to corner 1)
            else if (region == 5) n = P.edge_n + ((size_t)H.tri * 3 + 1) * 3;                     // AC is edge 1
            else if (region == 6) n = P.edge_n + ((size_t)H.tri * 3 + 0) * 3;                     // BC is edge 0
            else if (region == 1 || region == 2 || region == 4) n = v < T.V ? P.vert_n + (size_t)v * 3 : nullptr;
            float s = 0.0f;
            bool usable = false;
            if (n && region >= 1) {
                const float nx = n[0], ny = n[1], nz = n[2];
                usable = bv_finite(nx) && bv_finite(ny) && bv_finite(nz) && !(nx == 0.0f && ny == 0.0f && nz == 0.0f);
                s = -bv_dot(nx, ny, nz, x[0], x[1], x[2]);
            }
            undecided = dist > 0.0f && !(usable && (s < 0.0f || s > 0.0f));
            if (dist > 0.0f && usable && s < 0.0f) dist = -dist;
        }
        sdist_out[i] = dist;
        if (tri_out) tri_out[i] = answered ? (int)H.tri : -1;
        if (bary_out) {
            bary_out[(size_t)i * 3 + 0] = answered ? H.w0 : 0.0f;
            bary_out[(size_t)i * 3 + 1] = answered ? H.w1 : 0.0f;
            bary_out[(size_t)i * 3 + 2] = answered ? H.w2 : 0.0f;
        }
        if (feature_out) feature_out[i] = (signed char)(answered ? region - 1 : -1);
    }
    bv_count(counts, answered, refused, node_tests, tri_tests);
    if (counts) {
        const u64 mu = __ballot(undecided);
        if ((threadIdx.x & 63u) == 0 && mu) atomicAdd(counts + 4, (unsigned long long)__popcll(mu));
    }
}

__global__ __launch_bounds__(BV_CAST_THREADS) void bv_occlusion_kernel(BvTree T, const float *__restrict__ points, const float *__restrict__ normals, unsigned M,
                                                                       const float *__restrict__ dirs, unsigned K, float bias, float t_max, float *__restrict__ out,
                                                                       unsigned long long *__restrict__ counts, unsigned *__restrict__ fault)
{
    __shared__ unsigned stack[BV_STACK * BV_CAST_THREADS];
    const bool ok = bv_blob_ok(T, fault);
    const unsigned i = blockIdx.x * BV_CAST_THREADS + threadIdx.x;
    unsigned node_tests = 0, tri_tests = 0, hits = 0, refusals = 0;
    if (i < M) {
        const float *p = points + (size_t)i * 3, *n = normals + (size_t)i * 3;
        const float nx = n[0], ny = n[1], nz = n[2];
        float res = 1.0f;
        if (ok && bv_finite(nx) && bv_finite(ny) && bv_finite(nz) && !(nx == 0.0f && ny == 0.0f && nz == 0.0f)) {
            const float ox = p[0] + bias * nx, oy = p[1] + bias * ny, oz = p[2] + bias * nz;
            float num = 0.0f, den = 0.0f;
            for (unsigned k = 0; k < K; ++k) {                       // k is the same in every lane: the wave walks one direction of the table at a time
                float dx = dirs[(size_t)k * 3], dy = dirs[(size_t)k * 3 + 1], dz = dirs[(size_t)k * 3 + 2];
                float w = bv_dot(dx, dy, dz, nx, ny, nz);
                if (!(w >= 0.0f)) { dx = -dx; dy = -dy; dz = -dz; w = -w; }
                BvRay r;
                BvHit H;
                bool hit = false;
                if (bv_ray(r, ox, oy, oz, dx, dy, dz, 0.0f, 0)) hit = bv_walk<true>(T, r, t_max, H, stack + threadIdx.x, BV_CAST_THREADS, node_tests, tri_tests, fault);
                else ++refusals;
                hits += hit ? 1u : 0u;
                num += hit ? 0.0f : w;
                den += w;
            }
            if (den > 0.0f) res = num / den;
        }
        out[i] = res;
    }
    if (counts) {
        for (int o = 32; o; o >>= 1) {
            hits += (unsigned)__shfl_xor((int)hits, o, 64);
            refusals += (unsigned)__shfl_xor((int)refusals, o, 64);
            node_tests += (unsigned)__shfl_xor((int)node_tests, o, 64);
            tri_tests += (unsigned)__shfl_xor((int)tri_tests, o, 64);
        }
        if ((threadIdx.x & 63u) == 0) {
            if (hits) atomicAdd(counts + 0, (unsigned long long)hits);
            if (refusals) atomicAdd(counts + 1, (unsigned long long)refusals);
            if (node_tests) atomicAdd(counts + 2, (unsigned long long)node_tests);
            if (tri_tests) atomicAdd(counts + 3, (unsigned long long)tri_tests);
        }
    }
}

hipError_t launch_mesh_bvh_cast(const float *verts, long long V, const int *faces, long long F, const void *bvh, const float *origins, const float *dirs, long long N,
                                float t_min, float t_max, int any_hit, int cull, float *t, int *tri, float *bary, unsigned char *hit, unsigned long long *counts,
                                unsigned *fault, hipStream_t stream)
{
    if (counts) {
        hipError_t e = hipMemsetAsync(counts, 0, 4 * sizeof(unsigned long long), stream);
        if (e != hipSuccess) return e;
    }
    if (N <= 0) return hipSuccess;
    const BvTree T = bv_tree(verts, V, faces, F, const_cast<void *>(bvh));
    const unsigned nb = (unsigned)((N + BV_CAST_THREADS - 1) / BV_CAST_THREADS);
    if (any_hit)
        hipLaunchKernelGGL(bv_cast_kernel<true>, dim3(nb), dim3(BV_CAST_THREADS), 0, stream, T, origins, dirs, (unsigned)N, t_min, t_max, cull, t, tri, bary, hit, counts, fault);
    else
        hipLaunchKernelGGL(bv_cast_kernel<false>, dim3(nb), dim3(BV_CAST_THREADS), 0, stream, T, origins, dirs, (unsigned)N, t_min, t_max, cull, t, tri, bary, hit, counts, fault);
    return hipGetLastError();
}

hipError_t launch_mesh_bvh_occlusion(const float *verts, long long V, const int *faces, long long F, const void *bvh, const float *points, const float *normals, long long M,
                                     const float *dirs, int K, float bias, float t_max, float *out, unsigned long long *counts, unsigned *fault, hipStream_t stream)
{
    if (counts) {
        hipError_t e = hipMemsetAsync(counts, 0, 4 * sizeof(unsigned long long), stream);
        if (e != hipSuccess) return e;
    }
    if (M <= 0) return hipSuccess;
    const BvTree T = bv_tree(verts, V, faces, F, const_cast<void *>(bvh));
    const unsigned nb = (unsigned)((M + BV_CAST_THREADS - 1) / BV_CAST_THREADS);
    hipLaunchKernelGGL(bv_occlusion_kernel, dim3(nb), dim3(BV_CAST_THREADS), 0, stream, T, points, normals, (unsigned)M, dirs, (unsigned)K, bias, t_max, out, counts, fault);
    return hipGetLastError();
}

hipError_t launch_mesh_bvh_nearest(const float *verts, long long V, const int *faces, long long F, const void *bvh, const float *points, long long N, float max_dist,
                                   float *dist, int *tri, float *bary, unsigned long long *counts, unsigned *fault, hipStream_t stream)
{
    if (counts) {
        hipError_t e = hipMemsetAsync(counts, 0, 4 * sizeof(unsigned long long), stream);
        if (e != hipSuccess) return e;
    }
    if (N <= 0) return hipSuccess;
    const BvTree T = bv_tree(verts, V, faces, F, const_cast<void *>(bvh));
    const unsigned nb = (unsigned)((N + BV_CAST_THREADS - 1) / BV_CAST_THREADS);
    const float max_sq = max_dist * max_dist;                        // fp32, rounded once (+inf for +inf or an overflow)
    hipLaunchKernelGGL(bv_nearest_kernel, dim3(nb), dim3(BV_CAST_THREADS), 0, stream, T, points, (unsigned)N, max_sq, dist, tri, bary, counts, fault);
    return hipGetLastError();
}

hipError_t launch_mesh_bvh_signed(const float *verts, long long V, const int *faces, long long F, const void *bvh, const void *table, const float *points,
                                  const float *origin, const float *spacing, const int *dims, long long N, float max_dist, float *sdist, int *tri, float *bary,
                                  signed char *feature, unsigned long long *counts, unsigned *fault, hipStream_t stream)
{
    if (counts) {
        hipError_t e = hipMemsetAsync(counts, 0, 5 * sizeof(unsigned long long), stream);
        if (e != hipSuccess) return e;
    }
    if (N <= 0) return hipSuccess;
    const BvTree T = bv_tree(verts, V, faces, F, const_cast<void *>(bvh));
    MeshPseudoCarve L;
    mesh_pseudo_bytes(V, F, &L);
    BvNormals P;
    P.h = (const MeshPseudoHeader *)table;
    P.face_n = (const float *)((const char *)table + L.face_n); P.edge_n = (const float *)((const char *)table + L.edge_n);
    P.vert_n = (const float *)((const char *)table + L.vert_n);
    BvLattice G = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1u, 1u};
    if (!points) {
        G.ox = origin[0]; G.oy = origin[1]; G.oz = origin[2]; G.sx = spacing[0]; G.sy = spacing[1]; G.sz = spacing[2];
        G.ny = (unsigned)dims[1]; G.nz = (unsigned)dims[2];
    }
    const unsigned nb = (unsigned)((N + BV_CAST_THREADS - 1) / BV_CAST_THREADS);
    const float max_sq = max_dist * max_dist;                        // fp32, rounded once (+inf for +inf or an overflow)
    hipLaunchKernelGGL(bv_signed_kernel, dim3(nb), dim3(BV_CAST_THREADS), 0, stream, T, P, points, G, (unsigned)N, max_sq, sdist, tri, bary, feature, counts, fault);
    return hipGetLastError();
}
