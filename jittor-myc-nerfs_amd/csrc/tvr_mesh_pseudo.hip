// tvr_mesh_pseudo.hip — the pseudo-normal table of an indexed triangle mesh: a unit normal per face, the sum of the adjoining faces' normals per edge and the
// angle-weighted sum of the fan's normals per vertex (Baerentzen & Aanaes 2005).  The signed closest-point query of tvr_mesh_bvh.hip (bv_signed_kernel) takes the normal
// of the feature under the closest point from it: that normal, unlike a face normal, gives the right side of a closed surface at edges and vertices too.
// include/tvr.h tvr_mesh_pseudonormals_* holds the definition; DESIGN.md §4.19 the reasoning.  fp contraction is off and divisions and square roots are correctly
// rounded (csrc/Makefile), so face_n and edge_n are the same bits as a numpy fp32 restatement; vert_n goes through atan2f and is compared as a direction.
//
//   keys     one launch: per corner c = 3 f + k the key (vertex << 32 | c) — unique — and per half-edge h = 3 f + k (edge k of face f runs from corner (k+1)%3 to
//            corner (k+2)%3) the key (smaller vertex << 32 | larger vertex), which the two sides of an edge share.  The caller sorts both (the second stably, with
//            the permutation), as for the hierarchy.
//   build    faces (face_n, degenerate faces, index check), check (both sorted arrays: ascending, truthful against the faces, every corner and half-edge exactly once),
//            vertices and edges (the first entry of every run of equal vertices / equal edges walks its run in order and writes the sum), finish (header, counts)
//
// No float atomics: every sum is formed by one thread in ascending face order, so the table is a function of (verts, faces) alone.  The integer counters are summed
// with atomics, which commute.  Every index read from the keys, the order and the faces is compared with its bound before it is used.
#include "tvr_kernels.h"

#define PN_THREADS 256

typedef unsigned long long u64;

struct PnTable {
    MeshPseudoHeader *h;
    float *face_n;                      // [F][3]
    float *edge_n;                      // [F][3][3]
    float *vert_n;                      // [V][3]
    unsigned F, V;
    const float *verts;
    const int *faces;
};

struct PnScratch {
    unsigned *header;                   // [64]: word 0 bad, 1 degenerate faces, 2 open edges, 3 non-manifold edges, 4 inconsistent edges
    unsigned *seen_c;                   // [(3F+31)/32] bits: corners named by the corner keys
    unsigned *seen_e;                   // [(3F+31)/32] bits: half-edges named by the edge order
};

static size_t pn_align(size_t v) { return (v + 255) / 256 * 256; }

__device__ __forceinline__ bool pn_finite(float x) { return fabsf(x) <= 3.4028234664e38f; }
__device__ __forceinline__ float pn_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// the key of half-edge h (< 3F): false when one of its two vertices lies outside 0 .. V-1; from = the vertex it leaves
__device__ __forceinline__ bool pn_edge_key(const int *__restrict__ faces, unsigned V, unsigned h, u64 &key, unsigned &from)
{
    const unsigned f = h / 3u, k = h - f * 3u;
    const unsigned a = (unsigned)faces[(size_t)f * 3 + (k + 1u) % 3u], b = (unsigned)faces[(size_t)f * 3 + (k + 2u) % 3u];
    from = a;
    if (a >= V || b >= V) {
        key = 0x7fffffff7fffffffull;
        return false;
    }
    key = ((u64)(a < b ? a : b) << 32) | (u64)(a < b ? b : a);
    return true;
}

// ---- keys -----------------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PN_THREADS) void pn_keys_kernel(const int *__restrict__ faces, unsigned V, unsigned n, u64 *__restrict__ corner_keys, u64 *__restrict__ edge_keys,
                                                             unsigned *__restrict__ fault)
{
    const unsigned c = blockIdx.x * PN_THREADS + threadIdx.x;          // n = 3F <= 3 * 2^30 < 2^32
    if (c >= n) return;
    const unsigned v = (unsigned)faces[c];
    const bool bad = v >= V;
    corner_keys[c] = ((u64)(bad ? 0x7fffffffu : v) << 32) | (u64)c;
    u64 key;
    unsigned from;
    const bool ok = pn_edge_key(faces, V, c, key, from);
    edge_keys[c] = key;
    if (bad || !ok) *fault = 1u;
}

// ---- build ----------------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PN_THREADS) void pn_faces_kernel(PnTable T, PnScratch s, unsigned *__restrict__ fault)
{
    const unsigned t = blockIdx.x * PN_THREADS + threadIdx.x;
    bool degenerate = false;
    if (t < T.F) {
        const int *f = T.faces + (size_t)t * 3;
        const unsigned v0 = (unsigned)f[0], v1 = (unsigned)f[1], v2 = (unsigned)f[2];
        if (v0 >= T.V || v1 >= T.V || v2 >= T.V) {
            s.header[0] = 1u;
            *fault = 1u;
        } else {
            const float *p0 = T.verts + (size_t)v0 * 3, *p1 = T.verts + (size_t)v1 * 3, *p2 = T.verts + (size_t)v2 * 3;
            bool fin = true;
            for (int k = 0; k < 3; ++k) fin = fin && pn_finite(p0[k]) && pn_finite(p1[k]) && pn_finite(p2[k]);
            const float abx = p1[0] - p0[0], aby = p1[1] - p0[1], abz = p1[2] - p0[2], acx = p2[0] - p0[0], acy = p2[1] - p0[1], acz = p2[2] - p0[2];
            const float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
            const float len = sqrtf(pn_dot(nx, ny, nz, nx, ny, nz));
            const bool ok = fin && len > 0.0f && pn_finite(len);     // (a NaN length is not > 0)
            degenerate = !ok;
            float *o = T.face_n + (size_t)t * 3;
            o[0] = ok ? nx / len : 0.0f; o[1] = ok ? ny / len : 0.0f; o[2] = ok ? nz / len : 0.0f;
        }
    }
    const u64 m = __ballot(degenerate);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(s.header + 1, (unsigned)__popcll(m));
}

__global__ __launch_bounds__(PN_THREADS) void pn_check_kernel(const u64 *__restrict__ ck, const u64 *__restrict__ ek, const long long *__restrict__ eo, PnTable T, PnScratch s,
                                                              unsigned *__restrict__ fault)
{
    const unsigned n = 3u * T.F, i = blockIdx.x * PN_THREADS + threadIdx.x;
    if (i >= n) return;
    // the corner keys: strictly ascending, each names a corner below 3F once and the vertex the faces hold there
    const u64 k = ck[i];
    const unsigned c = (unsigned)(k & 0xffffffffull), v = (unsigned)(k >> 32);
    bool bad = c >= n || v >= T.V || (i + 1 < n && !(k < ck[i + 1]));
    if (!bad) bad = (unsigned)T.faces[c] != v;
    if (!bad) bad = (atomicOr(s.seen_c + (c >> 5), 1u << (c & 31u)) >> (c & 31u)) & 1u;
    // the edge keys with their order: ascending, equal keys in ascending half-edge order, each half-edge below 3F once under the key the faces give it
    const u64 e = ek[i], h64 = (u64)eo[i];
    if (h64 >= (u64)n)
        bad = true;
    else {
        const unsigned h = (unsigned)h64;
        u64 want;
        unsigned from;
        if (!pn_edge_key(T.faces, T.V, h, want, from) || want != e) bad = true;
        if (i + 1 < n && !(e < ek[i + 1] || (e == ek[i + 1] && h64 < (u64)eo[i + 1]))) bad = true;
        if ((atomicOr(s.seen_e + (h >> 5), 1u << (h & 31u)) >> (h & 31u)) & 1u) bad = true;
    }
    if (bad) {
        s.header[0] = 1u;
        *fault = 1u;
    }
}

// vert_n: the first entry of every run of corners of one vertex walks the run — corners in ascending order, i.e. faces in ascending index
__global__ __launch_bounds__(PN_THREADS) void pn_vertex_kernel(const u64 *__restrict__ ck, PnTable T, PnScratch s)
{
    if (s.header[0]) return;
    const unsigned n = 3u * T.F, i = blockIdx.x * PN_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned v = (unsigned)(ck[i] >> 32);
    if (v >= T.V || (i > 0 && (unsigned)(ck[i - 1] >> 32) == v)) return;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (unsigned j = i; j < n && (unsigned)(ck[j] >> 32) == v; ++j) {
        const unsigned c = (unsigned)(ck[j] & 0xffffffffull);
        if (c >= n) continue;                                        // (never: the check kernel saw to it)
        const unsigned f = c / 3u, k = c - f * 3u;
        const float *nf = T.face_n + (size_t)f * 3;
        const float nx = nf[0], ny = nf[1], nz = nf[2];
        if (nx == 0.0f && ny == 0.0f && nz == 0.0f) continue;        // a degenerate face has no angle
        const unsigned v1 = (unsigned)T.faces[(size_t)f * 3 + (k + 1u) % 3u], v2 = (unsigned)T.faces[(size_t)f * 3 + (k + 2u) % 3u];
        if (v1 >= T.V || v2 >= T.V) continue;                        // (never: the faces kernel would have set `bad`)
        const float *p0 = T.verts + (size_t)v * 3, *p1 = T.verts + (size_t)v1 * 3, *p2 = T.verts + (size_t)v2 * 3;
        const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2], bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        const float angle = atan2f(sqrtf(pn_dot(cx, cy, cz, cx, cy, cz)), pn_dot(ax, ay, az, bx, by, bz));
        sx = sx + angle * nx; sy = sy + angle * ny; sz = sz + angle * nz;
    }
    float *o = T.vert_n + (size_t)v * 3;
    o[0] = sx; o[1] = sy; o[2] = sz;
}

// edge_n: the first entry of every run of half-edges of one undirected edge sums the run's face normals in ascending half-edge (so face) order, writes the sum to
// every half-edge of the run and classifies the edge by the number of half-edges on it
__global__ __launch_bounds__(PN_THREADS) void pn_edge_kernel(const u64 *__restrict__ ek, const long long *__restrict__ eo, PnTable T, PnScratch s)
{
    const unsigned n = 3u * T.F, i = blockIdx.x * PN_THREADS + threadIdx.x;
    bool open = false, nonmanifold = false, inconsistent = false;
    if (!s.header[0] && i < n && (i == 0 || ek[i - 1] != ek[i])) {
        const u64 e = ek[i];
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;
        unsigned m = 0, from0 = 0, from1 = 0;
        for (unsigned j = i; j < n && ek[j] == e; ++j) {
            const u64 h = (u64)eo[j];
            if (h >= (u64)n) continue;                               // (never: the check kernel saw to it)
            u64 key;
            unsigned from;
            pn_edge_key(T.faces, T.V, (unsigned)h, key, from);
            const float *nf = T.face_n + (size_t)(h / 3u) * 3;
            sx = sx + nf[0]; sy = sy + nf[1]; sz = sz + nf[2];
            if (m == 0) from0 = from;
            if (m == 1) from1 = from;
            ++m;
        }
        for (unsigned j = i; j < n && ek[j] == e; ++j) {
            const u64 h = (u64)eo[j];
            if (h >= (u64)n) continue;
            float *o = T.edge_n + (size_t)h * 3;
            o[0] = sx; o[1] = sy; o[2] = sz;
        }
        open = m == 1;
        nonmanifold = m > 2;
        inconsistent = m == 2 && from0 == from1;                     // two faces that run the edge in the same direction
    }
    const u64 mo = __ballot(open), mn = __ballot(nonmanifold), mi = __ballot(inconsistent);
    if ((threadIdx.x & 63u) == 0) {
        if (mo) atomicAdd(s.header + 2, (unsigned)__popcll(mo));
        if (mn) atomicAdd(s.header + 3, (unsigned)__popcll(mn));
        if (mi) atomicAdd(s.header + 4, (unsigned)__popcll(mi));
    }
}

__global__ void pn_finish_kernel(PnTable T, PnScratch s, int *__restrict__ counts)
{
    if (threadIdx.x != 0) return;
    MeshPseudoHeader *h = T.h;
    const bool bad = s.header[0] != 0u;
    h->magic = MESH_PSEUDO_MAGIC; h->F = T.F; h->V = T.V; h->bad = s.header[0];
    h->degenerate_faces = bad ? 0u : s.header[1]; h->open_edges = bad ? 0u : s.header[2];
    h->nonmanifold_edges = bad ? 0u : s.header[3]; h->inconsistent_edges = bad ? 0u : s.header[4];
    if (counts) {
        counts[0] = (int)h->degenerate_faces; counts[1] = (int)h->open_edges; counts[2] = (int)h->nonmanifold_edges; counts[3] = (int)h->inconsistent_edges;
    }
}

size_t mesh_pseudo_bytes(long long V, long long F, MeshPseudoCarve *c)
{
    MeshPseudoCarve L;
    L.header = 0;
    L.face_n = MESH_PSEUDO_HEADER_BYTES;
    L.edge_n = L.face_n + pn_align((size_t)F * 3 * sizeof(float));
    L.vert_n = L.edge_n + pn_align((size_t)F * 9 * sizeof(float));
    L.total = L.vert_n + pn_align((size_t)V * 3 * sizeof(float));
    if (c) *c = L;
    return L.total;
}

size_t mesh_pseudo_scratch_bytes(long long F)
{
    return 256 + 2 * pn_align(((size_t)F * 3 + 31) / 32 * sizeof(unsigned));
}

hipError_t launch_mesh_pseudo_keys(const int *faces, long long V, long long F, unsigned long long *corner_keys, unsigned long long *edge_keys, unsigned *fault,
                                   hipStream_t stream)
{
    const unsigned n = (unsigned)(3 * F), nb = (n + PN_THREADS - 1) / PN_THREADS;
    if (nb) hipLaunchKernelGGL(pn_keys_kernel, dim3(nb), dim3(PN_THREADS), 0, stream, faces, (unsigned)V, n, corner_keys, edge_keys, fault);
    return hipGetLastError();
}

hipError_t launch_mesh_pseudo_build(const float *verts, long long V, const int *faces, long long F, const unsigned long long *corner_keys,
                                    const unsigned long long *edge_keys, const long long *edge_order, void *table, void *scratch, int *counts, unsigned *fault,
                                    hipStream_t stream)
{
    MeshPseudoCarve L;
    hipError_t e = hipMemsetAsync(table, 0, mesh_pseudo_bytes(V, F, &L), stream);       // padding and unused vertices included: the blob is a function of the mesh alone
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(scratch, 0, mesh_pseudo_scratch_bytes(F), stream);
    if (e != hipSuccess) return e;
    PnTable T;
    T.h = (MeshPseudoHeader *)table;
    T.face_n = (float *)((char *)table + L.face_n); T.edge_n = (float *)((char *)table + L.edge_n); T.vert_n = (float *)((char *)table + L.vert_n);
    T.F = (unsigned)F; T.V = (unsigned)V; T.verts = verts; T.faces = faces;
    PnScratch s;
    s.header = (unsigned *)scratch;
    s.seen_c = (unsigned *)((char *)scratch + 256);
    s.seen_e = (unsigned *)((char *)s.seen_c + pn_align(((size_t)F * 3 + 31) / 32 * sizeof(unsigned)));
    const unsigned fb = (unsigned)((F + PN_THREADS - 1) / PN_THREADS), cb = (unsigned)((3 * F + PN_THREADS - 1) / PN_THREADS);
    if (fb) {
        hipLaunchKernelGGL(pn_faces_kernel, dim3(fb), dim3(PN_THREADS), 0, stream, T, s, fault);
        hipLaunchKernelGGL(pn_check_kernel, dim3(cb), dim3(PN_THREADS), 0, stream, corner_keys, edge_keys, edge_order, T, s, fault);
        hipLaunchKernelGGL(pn_vertex_kernel, dim3(cb), dim3(PN_THREADS), 0, stream, corner_keys, T, s);
        hipLaunchKernelGGL(pn_edge_kernel, dim3(cb), dim3(PN_THREADS), 0, stream, edge_keys, edge_order, T, s);
    }
    hipLaunchKernelGGL(pn_finish_kernel, dim3(1), dim3(64), 0, stream, T, s, counts);
    return hipGetLastError();
}
