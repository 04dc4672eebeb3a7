// tvr_mesh_winding.hip — the generalized winding number of a triangle soup (Jacobson et al. 2013) by its hierarchical evaluation (Barill et al. 2018, dipole order) on the
// tree of tvr_mesh_bvh.hip: inside / outside for meshes the pseudo-normal sign of tvr_mesh_pseudo.hip cannot judge — open, non-manifold, self-intersecting, unwelded
// (mesh.build_winding / winding_number / winding_contains / winding_number_grid / signed_distance_winding / remesh_watertight).  include/tvr.h tvr_mesh_winding_* holds
// the definition; DESIGN.md §4.20 the reasoning.  fp contraction is off and divisions and square roots are correctly rounded (csrc/Makefile), so the table is the same
// bits as a numpy fp32 restatement and every accept decision of the query can be restated.
//
//   table    one row per internal node: the sum A of the area vectors below it, their area-weighted centroid c, the radius r about c that holds the node's box, the
//            summed area a.  62 passes in the refit's discipline (tvr_mesh_bvh.hip, REFIT): launch p computes a node iff both children were finished by an EARLIER
//            launch, as (left child) + (right child); a leaf's moments are computed from its triangle where they are needed (the same expressions, the same bits).
//            The unnormalised moment m = sum |A_t| centroid_t lives in scratch.  No float atomics: the order is the tree's, not the scheduler's.
//   query    one lane per point, the cast's 64-entry stack per lane in LDS: a node far enough away (|c - q| > beta r) adds its dipole, any other is opened, left child
//            first; a leaf adds its triangle's exact solid angle.  fp32 terms, an fp64 sum.
//
// Every index read from the blob, the table and the faces is compared with its bound before it is used, and every push with the stack's size.
#include "tvr_mesh_bvh_tree.h"

struct WnTable {
    MeshWindingHeader *h;
    float *rows;                        // [F-1][8]: A xyz, c xyz, r, a
};

struct WnScratch {
    unsigned *pass;                     // [F-1]: the launch that finished the node (0 = not yet; leaves count as pass 1)
    float *moment;                      // [F-1][4]: m xyz, one word of padding
};

struct WnMoments {
    float A[3], m[3], a;
};

__device__ __forceinline__ bool wn_tree_ok(const BvTree &T) { return T.h->magic == BV_MAGIC && T.h->F == T.F && T.h->bad == 0u; }

// the moments of leaf node `node` (first_leaf <= node < 2F-1): zeros for a triangle the hierarchy skipped (an index outside the vertices, a non-finite coordinate)
__device__ __forceinline__ WnMoments wn_leaf(const BvTree &T, unsigned node)
{
    WnMoments M = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0.0f};
    const unsigned t = (unsigned)T.leaf_tri[node - (T.F - 1u)];
    if (t >= T.F) return M;
    const int *f = T.faces + (size_t)t * 3;
    const unsigned v0 = (unsigned)f[0], v1 = (unsigned)f[1], v2 = (unsigned)f[2];
    if (v0 >= T.V || v1 >= T.V || v2 >= T.V) return M;
    const float *p0 = T.verts + (size_t)v0 * 3, *p1 = T.verts + (size_t)v1 * 3, *p2 = T.verts + (size_t)v2 * 3;
    bool fin = true;
    for (int k = 0; k < 3; ++k) fin = fin && bv_finite(p0[k]) && bv_finite(p1[k]) && bv_finite(p2[k]);
    if (!fin) return M;
    const float abx = p1[0] - p0[0], aby = p1[1] - p0[1], abz = p1[2] - p0[2], acx = p2[0] - p0[0], acy = p2[1] - p0[1], acz = p2[2] - p0[2];
    M.A[0] = 0.5f * (aby * acz - abz * acy); M.A[1] = 0.5f * (abz * acx - abx * acz); M.A[2] = 0.5f * (abx * acy - aby * acx);
    M.a = sqrtf(bv_dot(M.A[0], M.A[1], M.A[2], M.A[0], M.A[1], M.A[2]));
    for (int k = 0; k < 3; ++k) M.m[k] = M.a * (((p0[k] + p1[k]) + p2[k]) / 3.0f);
    return M;
}

__global__ __launch_bounds__(BV_THREADS) void wn_refit_kernel(BvTree T, WnTable W, WnScratch s, unsigned p)
{
    if (!wn_tree_ok(T)) return;
    const unsigned i = blockIdx.x * BV_THREADS + threadIdx.x;
    if (T.F < 2 || i >= T.F - 1 || s.pass[i] != 0u) return;
    const unsigned n_nodes = 2u * T.F - 1u, first_leaf = T.F - 1u;
    const unsigned ch[2] = {(unsigned)T.child[(size_t)i * 2], (unsigned)T.child[(size_t)i * 2 + 1]};
    if (ch[0] >= n_nodes || ch[1] >= n_nodes) return;
    const unsigned pa = ch[0] >= first_leaf ? 1u : s.pass[ch[0]], pb = ch[1] >= first_leaf ? 1u : s.pass[ch[1]];
    if (pa == 0u || pa >= p || pb == 0u || pb >= p) return;          // a child this very launch finishes does not count: its row may be half written
    WnMoments M[2];
    for (int k = 0; k < 2; ++k) {
        if (ch[k] >= first_leaf)
            M[k] = wn_leaf(T, ch[k]);
        else {
            const float *row = W.rows + (size_t)ch[k] * 8, *mo = s.moment + (size_t)ch[k] * 4;
            for (int j = 0; j < 3; ++j) { M[k].A[j] = row[j]; M[k].m[j] = mo[j]; }
            M[k].a = row[7];
        }
    }
    float A[3], m[3], c[3], e[3];
    for (int j = 0; j < 3; ++j) { A[j] = M[0].A[j] + M[1].A[j]; m[j] = M[0].m[j] + M[1].m[j]; }
    const float a = M[0].a + M[1].a;
    const bool ok = a > 0.0f && bv_finite(a);
    const float *box = T.box + (size_t)i * 6;
    for (int j = 0; j < 3; ++j) {
        c[j] = ok ? m[j] / a : 0.0f;
        e[j] = fmaxf(c[j] - box[j], box[3 + j] - c[j]);
    }
    float r = sqrtf(bv_dot(e[0], e[1], e[2], e[0], e[1], e[2]));
    if (!ok || !bv_finite(r)) r = __uint_as_float(0x7f800000u);     // never approximated (a NaN r included)
    float *row = W.rows + (size_t)i * 8, *mo = s.moment + (size_t)i * 4;
    for (int j = 0; j < 3; ++j) { row[j] = A[j]; row[3 + j] = c[j]; mo[j] = m[j]; }
    row[6] = r; row[7] = a;
    s.pass[i] = p;
}

__global__ void wn_finish_kernel(BvTree T, WnTable W, WnScratch s, unsigned *__restrict__ fault)
{
    if (threadIdx.x != 0) return;
    unsigned bad = 0u;
    if (!wn_tree_ok(T)) bad = 1u;                                    // the hierarchy does not belong to this mesh
    else if (T.F >= 2 && s.pass[0] == 0u) bad = 2u;                  // the passes did not reach the root
    if (bad) *fault = 1u;
    W.h->magic = MESH_WINDING_MAGIC; W.h->F = T.F; W.h->bad = bad;
}

size_t mesh_winding_bytes(long long F, MeshWindingCarve *c)
{
    MeshWindingCarve L;
    const size_t n = (size_t)F;
    L.header = 0;
    L.rows = MESH_WINDING_HEADER_BYTES;
    L.total = L.rows + bv_align((n ? n - 1 : 0) * 8 * sizeof(float));
    if (c) *c = L;
    return L.total;
}

size_t mesh_winding_scratch_bytes(long long F)
{
    const size_t n = (size_t)F;
    const size_t b = bv_align((n ? n - 1 : 0) * sizeof(unsigned)) + bv_align((n ? n - 1 : 0) * 4 * sizeof(float));
    return b ? b : 256;                                              // never 0: the query reports an error that way
}

static WnTable wn_table(void *table)
{
    WnTable W;
    W.h = (MeshWindingHeader *)table;
    W.rows = (float *)((char *)table + MESH_WINDING_HEADER_BYTES);
    return W;
}

hipError_t launch_mesh_winding_build(const float *verts, long long V, const int *faces, long long F, const void *bvh, void *table, void *scratch, unsigned *fault,
                                     hipStream_t stream)
{
    const size_t n = (size_t)F;
    hipError_t e = hipMemsetAsync(table, 0, mesh_winding_bytes(F, nullptr), stream);    // padding included: the table is a function of the mesh alone
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(scratch, 0, mesh_winding_scratch_bytes(F), stream);
    if (e != hipSuccess) return e;
    const BvTree T = bv_tree(verts, V, faces, F, const_cast<void *>(bvh));
    const WnTable W = wn_table(table);
    WnScratch s;
    s.pass = (unsigned *)scratch;
    s.moment = (float *)((char *)s.pass + bv_align((n ? n - 1 : 0) * sizeof(unsigned)));
    const unsigned ib = F > 1 ? (unsigned)((F - 1 + BV_THREADS - 1) / BV_THREADS) : 0u;
    if (ib)
        for (unsigned p = 2; p < 2 + BV_PASSES; ++p) hipLaunchKernelGGL(wn_refit_kernel, dim3(ib), dim3(BV_THREADS), 0, stream, T, W, s, p);
    hipLaunchKernelGGL(wn_finish_kernel, dim3(1), dim3(64), 0, stream, T, W, s, fault);
    return hipGetLastError();
}

// ---- the query ------------------------------------------------------------------------------------------------------------------------------------------------------------
// the solid angle of triangle t seen from q (Van Oosterom & Strackee 1983); 0 for a triangle the hierarchy skipped
__device__ __forceinline__ float wn_solid_angle(const BvTree &T, unsigned t, float qx, float qy, float qz, bool &counted, unsigned *__restrict__ fault)
{
    counted = false;
    const int *f = T.faces + (size_t)t * 3;
    const unsigned v0 = (unsigned)f[0], v1 = (unsigned)f[1], v2 = (unsigned)f[2];
    if (v0 >= T.V || v1 >= T.V || v2 >= T.V) {
        *fault = 1u;
        return 0.0f;
    }
    const float *p0 = T.verts + (size_t)v0 * 3, *p1 = T.verts + (size_t)v1 * 3, *p2 = T.verts + (size_t)v2 * 3;
    bool fin = true;
    for (int k = 0; k < 3; ++k) fin = fin && bv_finite(p0[k]) && bv_finite(p1[k]) && bv_finite(p2[k]);
    if (!fin) return 0.0f;
    counted = true;
    const float ax = p0[0] - qx, ay = p0[1] - qy, az = p0[2] - qz;
    const float bx = p1[0] - qx, by = p1[1] - qy, bz = p1[2] - qz;
    const float cx = p2[0] - qx, cy = p2[1] - qy, cz = p2[2] - qz;
    const float la = sqrtf(bv_dot(ax, ay, az, ax, ay, az)), lb = sqrtf(bv_dot(bx, by, bz, bx, by, bz)), lc = sqrtf(bv_dot(cx, cy, cz, cx, cy, cz));
    const float num = bv_dot(ax, ay, az, by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx);
    const float den = (((la * lb) * lc + bv_dot(ax, ay, az, bx, by, bz) * lc) + bv_dot(bx, by, bz, cx, cy, cz) * la) + bv_dot(cx, cy, cz, ax, ay, az) * lb;
    return 2.0f * atan2f(num, den);
}

__global__ __launch_bounds__(BV_CAST_THREADS) void wn_query_kernel(BvTree T, WnTable W, const float *__restrict__ points, BvLattice G, unsigned N, float beta,
                                                                   float *__restrict__ w_out, unsigned long long *__restrict__ counts, unsigned *__restrict__ fault)
{
    __shared__ unsigned stack[BV_STACK * BV_CAST_THREADS];            // entry e of lane l at [e * BV_CAST_THREADS + l]
    const bool blob_ok = bv_blob_ok(T, fault);
    const bool table_ok = W.h->magic == MESH_WINDING_MAGIC && W.h->F == T.F && W.h->bad == 0u;
    if (!table_ok && threadIdx.x == 0) *fault = 1u;
    const bool ok = blob_ok && table_ok;
    const unsigned i = blockIdx.x * BV_CAST_THREADS + threadIdx.x;
    bool answered = false, refused = false;
    u64 node_visits = 0, dipole_terms = 0, tri_terms = 0;
    if (i < N) {
        float qx, qy, qz;
        if (points) {
            const float *p = points + (size_t)i * 3;
            qx = p[0]; qy = p[1]; qz = p[2];
        } else {
            const unsigned plane = G.ny * G.nz, ix = i / plane, r = i - ix * plane, iy = r / G.nz, iz = r - iy * G.nz;
            qx = G.ox + (float)ix * G.sx; qy = G.oy + (float)iy * G.sy; qz = G.oz + (float)iz * G.sz;
        }
        refused = !(bv_finite(qx) && bv_finite(qy) && bv_finite(qz));
        double acc = 0.0;
        if (ok && !refused && T.F > 0) {
            const unsigned n_nodes = 2u * T.F - 1u, first_leaf = T.F - 1u, stride = BV_CAST_THREADS;
            unsigned *st = stack + threadIdx.x;
            unsigned sp = 0, node = 0;
            for (unsigned budget = n_nodes;; --budget) {
                if (budget == 0u) {                                  // a tree visits every node at most once: a blob with a cycle in it ends here
                    *fault = 1u;
                    break;
                }
                bool pop = true;
                if (node >= first_leaf) {
                    const unsigned t = (unsigned)T.leaf_tri[node - first_leaf];
                    if (t < T.F) {
                        bool counted;
                        acc += (double)wn_solid_angle(T, t, qx, qy, qz, counted, fault);
                        tri_terms += counted ? 1u : 0u;
                    } else
                        *fault = 1u;
                } else {
                    const float *row = W.rows + (size_t)node * 8;
                    const float dx = row[3] - qx, dy = row[4] - qy, dz = row[5] - qz;
                    const float d2 = bv_dot(dx, dy, dz, dx, dy, dz), br = beta * row[6];
                    ++node_visits;
                    if (d2 > br * br) {
                        acc += (double)(bv_dot(dx, dy, dz, row[0], row[1], row[2]) / (d2 * sqrtf(d2)));
                        ++dipole_terms;
                    } else {
                        const unsigned a = (unsigned)T.child[(size_t)node * 2], b = (unsigned)T.child[(size_t)node * 2 + 1];
                        if (a < n_nodes && b < n_nodes) {
                            node = a;                                // left first, the right child waits: at most one entry per level
                            if (sp < BV_STACK) st[(sp++) * stride] = b;
                            else *fault = 1u;                        // (never: the height is at most 62)
                            pop = false;
                        } else
                            *fault = 1u;
                    }
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
        answered = ok && !refused;
        w_out[i] = answered ? (float)(acc / 12.566370614359172) : __uint_as_float(0x7fc00000u);
    }
    if (counts) {
        const u64 ma = __ballot(answered), mr = __ballot(refused);
        node_visits = bv_wave_sum(node_visits); dipole_terms = bv_wave_sum(dipole_terms); tri_terms = bv_wave_sum(tri_terms);
        if ((threadIdx.x & 63u) == 0) {
            if (ma) atomicAdd(counts + 0, (unsigned long long)__popcll(ma));
            if (mr) atomicAdd(counts + 1, (unsigned long long)__popcll(mr));
            if (node_visits) atomicAdd(counts + 2, node_visits);
            if (dipole_terms) atomicAdd(counts + 3, dipole_terms);
            if (tri_terms) atomicAdd(counts + 4, tri_terms);
        }
    }
}

hipError_t launch_mesh_winding_query(const float *verts, long long V, const int *faces, long long F, const void *bvh, const void *table, const float *points,
                                     const float *origin, const float *spacing, const int *dims, long long N, float beta, float *w, unsigned long long *counts,
                                     unsigned *fault, hipStream_t stream)
{
    if (counts) {
        hipError_t e = hipMemsetAsync(counts, 0, 5 * sizeof(unsigned long long), stream);
        if (e != hipSuccess) return e;
    }
    if (N <= 0) return hipSuccess;
    const BvTree T = bv_tree(verts, V, faces, F, const_cast<void *>(bvh));
    const WnTable W = wn_table(const_cast<void *>(table));
    BvLattice G = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1u, 1u};
    if (!points) {
        G.ox = origin[0]; G.oy = origin[1]; G.oz = origin[2]; G.sx = spacing[0]; G.sy = spacing[1]; G.sz = spacing[2];
        G.ny = (unsigned)dims[1]; G.nz = (unsigned)dims[2];
    }
    const unsigned nb = (unsigned)((N + BV_CAST_THREADS - 1) / BV_CAST_THREADS);
    hipLaunchKernelGGL(wn_query_kernel, dim3(nb), dim3(BV_CAST_THREADS), 0, stream, T, W, points, G, (unsigned)N, beta, w, counts, fault);
    return hipGetLastError();
}
