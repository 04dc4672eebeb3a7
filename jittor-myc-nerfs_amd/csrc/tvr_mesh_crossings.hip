// tvr_mesh_crossings.hip — which triangles cut through which: the triangle-pair query on the tree of tvr_mesh_bvh.hip, over one mesh (every unordered pair i < j: its
// self-intersections) or with a second mesh as the query (every pair (q, a): the collision test) (mesh.self_intersections / mesh_intersections / mesh_check,
// reconstruct --mesh_check).  include/tvr.h tvr_mesh_crossings_* holds the definition; DESIGN.md §4.21 the reasoning.  Two triangles cross iff a side of one pierces the
// other: six (segment, triangle) tests per pair, each the cast's (ray, triangle) pair — bv_triangle of tvr_mesh_bvh_tree.h — over 0 < t <= 1.  fp contraction is off and
// t is a correctly rounded division (csrc/Makefile), so pairs, piercing counts and piercing points are the same bits as a numpy fp32 restatement.
//
//   walk     one lane per query triangle, the cast's 64-entry stack per lane in LDS: a node is entered iff its box overlaps the query triangle's box (both padded), left
//            child first, the right one waits; a leaf's triangle is evaluated (in a self query only when its index is above the lane's).
//   count    the walk, writing per query triangle how many triangles it crosses; the caller scans the counts into offsets
//   emit     the same walk again, writing pair k of query triangle i at offsets[i] + k: the order within a triangle is the walk's (the same on every run), the caller
//            sorts by (first, second).  No float atomics, no atomics on the output order.
//
// Every index read from the blob, the offsets and either mesh's faces is compared with its bound before it is used, and every push with the stack's size.
#include "tvr_mesh_bvh_tree.h"

struct CxTriangle {
    int f[3];
    float c[9];                         // corner k at c[3k .. 3k+2]
};

struct CxPair {
    unsigned n;                         // how many of the six tests pierce
    float p[6];                         // the first two piercing points in test order
};

// triangle t (< T.F) of T's mesh: false when an index is outside 0 .. V-1 (bad_index) or a coordinate is not finite
__device__ __forceinline__ bool cx_load(const BvTree &T, unsigned t, CxTriangle &A, bool &bad_index)
{
    const int *f = T.faces + (size_t)t * 3;
    A.f[0] = f[0]; A.f[1] = f[1]; A.f[2] = f[2];
    bad_index = (unsigned)A.f[0] >= T.V || (unsigned)A.f[1] >= T.V || (unsigned)A.f[2] >= T.V;
    if (bad_index) return false;
    bool fin = true;
    for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 3; ++j) {
            A.c[3 * k + j] = T.verts[(size_t)A.f[k] * 3 + j];
            fin = fin && bv_finite(A.c[3 * k + j]);
        }
    return fin;
}

__device__ __forceinline__ bool cx_same(const float *a, const float *b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }

// sides 0, 1, 2 of S against triangle t of T's mesh, whose corners are B.c: side k runs between corners (k+1)%3 and (k+2)%3, from the smaller vertex index to the larger
__device__ __forceinline__ void cx_sides(const CxTriangle &S, const BvTree &T, unsigned t, const CxTriangle &B, CxPair &P, unsigned *__restrict__ fault)
{
    for (int k = 0; k < 3; ++k) {
        const int i1 = (k + 1) % 3, i2 = (k + 2) % 3;
        const bool fwd = S.f[i1] < S.f[i2];
        const float *o = S.c + 3 * (fwd ? i1 : i2), *e = S.c + 3 * (fwd ? i2 : i1);
        bool share = false;
        for (int c = 0; c < 3; ++c) share = share || cx_same(o, B.c + 3 * c) || cx_same(e, B.c + 3 * c);
        if (share) continue;                                         // by position: a neighbour, welded or not
        const float dx = e[0] - o[0], dy = e[1] - o[1], dz = e[2] - o[2];
        BvRay r;
        float E[3], tt;
        if (!bv_ray(r, o[0], o[1], o[2], dx, dy, dz, 0.0f, 0)) continue;
        if (!bv_triangle(T, t, r, 1.0f, E, tt, fault)) continue;
        const float px = o[0] + tt * dx, py = o[1] + tt * dy, pz = o[2] + tt * dz;
        if (P.n == 0u) { P.p[0] = px; P.p[1] = py; P.p[2] = pz; }
        else if (P.n == 1u) { P.p[3] = px; P.p[4] = py; P.p[5] = pz; }
        ++P.n;
    }
}

// Do the boxes overlap?  b: a node's box; lo / hi: the query triangle's.  Both are widened by BV_PAD x the largest distance, along an axis, between a face of one and
// the opposite face of the other (a margin for pairs the fp32 test reports although the exact triangles miss by a rounding error, not a proof).
__device__ __forceinline__ bool cx_overlap(const float *__restrict__ b, const float lo[3], const float hi[3])
{
    const float gx = lo[0] - b[3], gy = lo[1] - b[4], gz = lo[2] - b[5], hx = b[0] - hi[0], hy = b[1] - hi[1], hz = b[2] - hi[2];
    const float m = fmaxf(fmaxf(fmaxf(fabsf(gx), fabsf(hx)), fmaxf(fabsf(gy), fabsf(hy))), fmaxf(fabsf(gz), fabsf(hz)));
    const float pad = m * BV_PAD;
    return gx <= pad && hx <= pad && gy <= pad && hy <= pad && gz <= pad && hz <= pad && b[0] <= b[3];      // (an empty box has lo = +inf, hi = -inf)
}

// EMIT false: count_out[i] = the number of triangles query triangle i crosses.  EMIT true: offsets [Nq+1] is the caller's exclusive scan of those counts; pair k of
// triangle i goes to row offsets[i] + k.  A walk that finds another number than the scan says raises the fault flag and writes nothing outside its rows.
template <bool EMIT>
__global__ __launch_bounds__(BV_CAST_THREADS) void cx_kernel(BvTree T, BvTree Q, int self, int *__restrict__ count_out, const long long *__restrict__ offsets,
                                                             long long n_pairs, int *__restrict__ pairs, int *__restrict__ n_pierce, float *__restrict__ points,
                                                             unsigned long long *__restrict__ total, unsigned long long *__restrict__ counts,
                                                             unsigned *__restrict__ fault)
{
    __shared__ unsigned stack[BV_STACK * BV_CAST_THREADS];            // entry e of lane l at [e * BV_CAST_THREADS + l]: a wave's accesses to one depth are contiguous
    const bool ok = bv_blob_ok(T, fault);
    const unsigned i = blockIdx.x * BV_CAST_THREADS + threadIdx.x;
    bool refused = false;
    u64 found = 0, node_tests = 0, pair_tests = 0;
    if (i < Q.F) {
        CxTriangle A;
        bool bad;
        refused = !cx_load(Q, i, A, bad);
        long long row = 0, row_end = 0;
        if (EMIT) {
            row = offsets[i]; row_end = offsets[i + 1];
            if (row < 0 || row_end < row || row_end > n_pairs) {
                *fault = 1u;
                row = row_end = 0;
            }
        }
        if (ok && !refused && T.F > 0) {
            float lo[3], hi[3];
            for (int k = 0; k < 3; ++k) {
                lo[k] = fminf(fminf(A.c[k], A.c[3 + k]), A.c[6 + k]);
                hi[k] = fmaxf(fmaxf(A.c[k], A.c[3 + k]), A.c[6 + k]);
            }
            const unsigned n_nodes = 2u * T.F - 1u, first_leaf = T.F - 1u, stride = BV_CAST_THREADS;
            unsigned *st = stack + threadIdx.x;
            unsigned sp = 0, node = 0;
            ++node_tests;
            bool walking = cx_overlap(T.box, lo, hi);
            for (unsigned budget = n_nodes; walking; --budget) {
                if (budget == 0u) {                                  // a tree visits every node at most once: a blob with a cycle in it ends here
                    *fault = 1u;
                    break;
                }
                bool pop = true;
                if (node >= first_leaf) {
                    const unsigned t = (unsigned)T.leaf_tri[node - first_leaf];
                    if (t >= T.F)
                        *fault = 1u;
                    else if (!self || t > i) {
                        CxTriangle B;
                        if (cx_load(T, t, B, bad)) {
                            CxPair P;
                            P.n = 0u;
                            for (int k = 0; k < 6; ++k) P.p[k] = 0.0f;
                            ++pair_tests;
                            cx_sides(A, T, t, B, P, fault);          // sides 0, 1, 2 of a against b, then those of b against a
                            cx_sides(B, Q, i, A, P, fault);
                            if (P.n) {
                                if (EMIT) {
                                    const long long at = row + (long long)found;
                                    if (at < row_end) {
                                        pairs[at * 2] = (int)i; pairs[at * 2 + 1] = (int)t;
                                        n_pierce[at] = (int)P.n;
                                        if (points)
                                            for (int k = 0; k < 3; ++k) {
                                                points[at * 6 + k] = P.p[k];
                                                points[at * 6 + 3 + k] = P.n == 1u ? P.p[k] : P.p[3 + k];
                                            }
                                    }
                                }
                                ++found;
                            }
                        } else if (bad)
                            *fault = 1u;
                    }
                } else {
                    const unsigned a = (unsigned)T.child[(size_t)node * 2], b = (unsigned)T.child[(size_t)node * 2 + 1];
                    if (a < n_nodes && b < n_nodes) {
                        node_tests += 2;
                        const bool ha = cx_overlap(T.box + (size_t)a * 6, lo, hi), hb = cx_overlap(T.box + (size_t)b * 6, lo, hi);
                        if (ha && hb) {
                            node = a;                                // left first, the right child waits: at most one entry per level
                            if (sp < BV_STACK) st[(sp++) * stride] = b;
                            else *fault = 1u;                        // (never: the height is at most 62)
                            pop = false;
                        } else if (ha || hb) {
                            node = ha ? a : b;
                            pop = false;
                        }
                    } else
                        *fault = 1u;
                }
                if (pop) {
                    if (sp == 0) break;
                    node = st[(--sp) * stride];
                    if (node >= n_nodes) {                           // (never: only checked numbers are pushed)
                        *fault = 1u;
                        break;
                    }
                }
            }
        }
        if (EMIT) {
            if ((long long)found != row_end - row) *fault = 1u;
        } else
            count_out[i] = found > 0x7fffffffull ? 0x7fffffff : (int)found;
    }
    if (total || counts) {
        const u64 mr = __ballot(refused);
        found = bv_wave_sum(found); node_tests = bv_wave_sum(node_tests); pair_tests = bv_wave_sum(pair_tests);
        if ((threadIdx.x & 63u) == 0) {
            if (total && found) atomicAdd(total, found);
            if (counts) {
                if (found) atomicAdd(counts + 0, found);
                if (mr) atomicAdd(counts + 1, (unsigned long long)__popcll(mr));
                if (node_tests) atomicAdd(counts + 2, node_tests);
                if (pair_tests) atomicAdd(counts + 3, pair_tests);
            }
        }
    }
}

// the query mesh as the fields of a BvTree that cx_load and bv_triangle read (verts, faces, V, F); the mesh itself in a self query
static BvTree cx_query(const BvTree &T, const float *verts_q, long long Vq, const int *faces_q, long long Fq, int self)
{
    BvTree Q = T;
    if (!self) { Q.verts = verts_q; Q.faces = faces_q; Q.V = (unsigned)Vq; Q.F = (unsigned)Fq; }
    return Q;
}

hipError_t launch_mesh_crossings_count(const float *verts, long long V, const int *faces, long long F, const void *bvh, const float *verts_q, long long Vq,
                                       const int *faces_q, long long Fq, int self, int *count_out, unsigned long long *total, unsigned long long *counts, unsigned *fault,
                                       hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(total, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    if (counts) {
        e = hipMemsetAsync(counts, 0, 4 * sizeof(unsigned long long), stream);
        if (e != hipSuccess) return e;
    }
    const BvTree T = bv_tree(verts, V, faces, F, const_cast<void *>(bvh)), Q = cx_query(T, verts_q, Vq, faces_q, Fq, self);
    if (Q.F == 0u) return hipSuccess;
    const unsigned nb = (Q.F + BV_CAST_THREADS - 1u) / BV_CAST_THREADS;
    hipLaunchKernelGGL(cx_kernel<false>, dim3(nb), dim3(BV_CAST_THREADS), 0, stream, T, Q, self, count_out, (const long long *)nullptr, 0ll, (int *)nullptr, (int *)nullptr,
                       (float *)nullptr, total, counts, fault);
    return hipGetLastError();
}

hipError_t launch_mesh_crossings_emit(const float *verts, long long V, const int *faces, long long F, const void *bvh, const float *verts_q, long long Vq,
                                      const int *faces_q, long long Fq, int self, const long long *offsets, long long n_pairs, int *pairs, int *n_pierce, float *points,
                                      unsigned *fault, hipStream_t stream)
{
    const BvTree T = bv_tree(verts, V, faces, F, const_cast<void *>(bvh)), Q = cx_query(T, verts_q, Vq, faces_q, Fq, self);
    if (Q.F == 0u) return hipSuccess;
    const unsigned nb = (Q.F + BV_CAST_THREADS - 1u) / BV_CAST_THREADS;
    hipLaunchKernelGGL(cx_kernel<true>, dim3(nb), dim3(BV_CAST_THREADS), 0, stream, T, Q, self, (int *)nullptr, offsets, n_pairs, pairs, n_pierce, points,
                       (unsigned long long *)nullptr, (unsigned long long *)nullptr, fault);
    return hipGetLastError();
}
