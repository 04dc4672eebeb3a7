// tvr_mesh_cc.hip — connected components of an indexed triangle mesh and the filter that keeps whole components: what drops the floaters from an exported mesh
// (mesh.filter_components, TensorBase.export_mesh(min_component_faces=, keep_largest=)).  include/tvr.h tvr_mesh_components / tvr_mesh_filter_*, DESIGN.md §4.10.
//
// Labelling is a union-find over the vertices whose parent array IS the caller's vertex_label:
//
//   check    per triangle: an index outside 0 .. V-1 raises the header's `bad` word and the fault flag; every later kernel of the call returns at once on `bad`
//   init     parent[v] = v, component_faces[v] = 0, *n_components = 0
//   hook     per triangle (a, b, c): unite(a, b), unite(b, c).  unite finds both roots and hooks the LARGER root under the smaller with one atomicCAS that expects the
//            root to still be a root; when it is not (someone else hooked it first) the CAS returns the root's new parent and the union continues from THAT value
//   flatten  per vertex: parent[v] <- parent[parent[v]] until parent[v] is a root.  A thread writes its own entry only, so the entry it leaves is final; the roots are counted
//   sizes    per triangle one integer add onto component_faces[label of its first vertex], aggregated per workgroup / per wave first
//
// Invariant: parent[v] <= v, with equality exactly at roots.  init establishes it; the CAS stores lo < hi into parent[hi] only while parent[hi] == hi; the path-splitting
// store of `find` replaces parent[v] by an ancestor that was read below v.  Hence (1) a vertex that stops being a root never becomes one again, (2) indices strictly
// decrease along every walk, so walks end after at most V hops and there are no cycles, (3) the minimum vertex m of a component is never hooked (anything it could be
// hooked under is a smaller vertex of the same component) — and since every triangle's unions have completed when the hook kernel ends, the one root left in a component's
// tree is m.  That is why the labels do not depend on launch geometry or on the order the atomics land in.
//
// Reads and writes of parent[] inside the hook and flatten kernels are relaxed device-scope atomics (the eight XCDs' L2s are not coherent for plain accesses).  A value
// read late is still an ancestor; the CAS is the only authority on "is a root".  No workgroup waits for another: every loop below makes progress on its own (its index
// decreases) and carries a step bound with a give-up path that raises the fault flag.  The kernel boundary is the only ordering.
//
// The filter is the count / scan / emit of tvr_mesh.hip over ELEMENTS e = 0 .. max(V, F)-1: count byte bit 0 = vertex e survives, bit 3 = triangle e survives — the
// encoding tvr_mesh.hip's scan kernels read as "one vertex" / "one triangle", so they are reused as they are (launch_mesh_scan).
#include "tvr_kernels.h"

#define CC_THREADS 256
#define CC_PER_THREAD 4
#define CC_TILE (CC_THREADS * CC_PER_THREAD)

static_assert(TVR_MESH_TILE == CC_TILE && TVR_MESH_SCAN_CHUNK == CC_THREADS, "the filter shares tvr_mesh.hip's scan: same tile, same chunk");

typedef unsigned long long u64;

struct CcHeader {
    unsigned bad;          // a triangle index outside 0 .. V-1 was seen: nothing else of the call is written
    unsigned max_steps;    // the most steps one unite / flatten walk took (diagnostic; see tvr.h)
};

__device__ __forceinline__ int cc_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_store(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the workgroup's largest step count -> header, one atomic per wave and only when it would raise the word
__device__ __forceinline__ void cc_note_steps(unsigned steps, CcHeader *h)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)steps, d, 64);
        steps = o > steps ? o : steps;
    }
    if ((threadIdx.x & 63) == 0 && steps > h->max_steps) atomicMax(&h->max_steps, steps);
}

__global__ __launch_bounds__(CC_THREADS) void cc_check_kernel(const int *__restrict__ faces, unsigned F, unsigned V, CcHeader *__restrict__ h, unsigned *__restrict__ fault)
{
    const unsigned f = blockIdx.x * CC_THREADS + threadIdx.x;
    if (f >= F) return;
    const int *t = faces + (size_t)f * 3;
    if ((unsigned)t[0] >= V || (unsigned)t[1] >= V || (unsigned)t[2] >= V) {        // (a negative index is a huge unsigned one)
        h->bad = 1u;
        *fault = 1u;
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(int *__restrict__ parent, int *__restrict__ comp_faces, unsigned V, long long *__restrict__ n_components,
                                                             const CcHeader *__restrict__ h)
{
    if (h->bad) return;
    const unsigned v = blockIdx.x * CC_THREADS + threadIdx.x;
    if (v == 0) *n_components = 0;
    if (v >= V) return;
    parent[v] = (int)v;
    comp_faces[v] = 0;
}

// root of v's tree, splitting the path on the way (every visited vertex is re-pointed at its grandparent).  `steps` is the caller's running count against `bound`;
// false = gave up (bound reached, or an entry outside 0 .. V-1: the array was written by someone else during the call).
__device__ __forceinline__ bool cc_find(int *parent, unsigned V, int v, unsigned &steps, unsigned bound, int &root)
{
    int p = cc_load(parent + v);
    while (p != v) {
        if ((unsigned)p >= V || ++steps > bound) return false;
        const int g = cc_load(parent + p);
        if (g != p) {
            if ((unsigned)g >= V) return false;
            cc_store(parent + v, g);           // g < p < v: an ancestor, so v stays in its tree and never looks like a root
        }
        v = p;
        p = g;
    }
    root = v;
    return true;
}

__device__ __forceinline__ bool cc_unite(int *parent, unsigned V, int a, int b, unsigned &steps, unsigned bound)
{
    for (;;) {
        if (!cc_find(parent, V, a, steps, bound, a) || !cc_find(parent, V, b, steps, bound, b)) return false;
        if (a == b) return true;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return true;            // hi was still a root and now hangs under lo
        // hi had already been hooked under `old` (< hi) by someone else: hi's tree and lo's tree still have to meet, so go on with (old, lo) — never drop it.
        if ((unsigned)old >= V || ++steps > bound) return false;
        a = old;
        b = lo;
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_hook_kernel(const int *__restrict__ faces, unsigned F, unsigned V, int *parent, CcHeader *h, unsigned bound,
                                                             unsigned *__restrict__ fault)
{
    if (h->bad) return;
    const unsigned f = blockIdx.x * CC_THREADS + threadIdx.x;
    unsigned steps = 0;
    if (f < F) {
        const int *t = faces + (size_t)f * 3;
        const int a = t[0], b = t[1], c = t[2];
        if ((unsigned)a < V && (unsigned)b < V && (unsigned)c < V) {        // (checked again: `faces` is the caller's and this kernel indexes with it)
            bool ok = a == b || cc_unite(parent, V, a, b, steps, bound);
            steps = 0;
            ok = ok && (b == c || cc_unite(parent, V, b, c, steps, bound));
            if (!ok) *fault = 1u;
        } else {
            *fault = 1u;
        }
    }
    cc_note_steps(steps, h);
}

__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int *parent, unsigned V, long long *__restrict__ n_components, CcHeader *h, unsigned bound,
                                                                unsigned *__restrict__ fault)
{
    __shared__ unsigned roots[CC_THREADS / 64];
    if (h->bad) return;
    const unsigned v = blockIdx.x * CC_THREADS + threadIdx.x;
    unsigned steps = 0;
    bool is_root = false;
    if (v < V) {
        int p = cc_load(parent + v);
        is_root = p == (int)v;              // roots are final since the hook kernel ended
        bool ok = (unsigned)p < V;
        while (ok && !is_root) {
            const int g = cc_load(parent + p);
            if (g == p) break;              // p is a root: parent[v] is final
            if ((unsigned)g >= V || ++steps > bound) {
                ok = false;
                break;
            }
            cc_store(parent + v, g);        // this thread is the only writer of parent[v]; others that read it skip ahead
            p = g;
        }
        if (!ok) *fault = 1u;
    }
    const u64 m = __ballot(is_root);
    if ((threadIdx.x & 63) == 0) roots[threadIdx.x >> 6] = (unsigned)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned n = 0;
#pragma unroll
        for (int w = 0; w < CC_THREADS / 64; ++w) n += roots[w];
        if (n) atomicAdd((u64 *)n_components, (u64)n);
    }
    cc_note_steps(steps, h);
}

__global__ __launch_bounds__(CC_THREADS) void cc_sizes_kernel(const int *__restrict__ faces, unsigned F, unsigned V, const int *__restrict__ label,
                                                              int *__restrict__ comp_faces, const CcHeader *__restrict__ h)
{
    __shared__ int first_root;
    if (h->bad) return;
    const unsigned f = blockIdx.x * CC_THREADS + threadIdx.x;
    int root = -1;
    if (f < F) {
        const int a = faces[(size_t)f * 3];
        if ((unsigned)a < V) {
            root = label[a];
            if ((unsigned)root >= V) root = -1;
        }
    }
    // triangles leave marching cubes ordered by cell, so a workgroup's triangles mostly share one component: one add for the workgroup then, else one per wave and root
    if (threadIdx.x == 0) first_root = root;
    __syncthreads();
    const int r0 = first_root;
    const int same = __syncthreads_count(root == r0);
    if (same == CC_THREADS) {
        if (threadIdx.x == 0 && r0 >= 0) atomicAdd(comp_faces + r0, CC_THREADS);
        return;
    }
    bool pending = root >= 0;
    while (pending) {                        // at most 64 rounds: each retires the lanes of one root
        const int lead = __builtin_amdgcn_readfirstlane(root);
        const u64 m = __ballot(root == lead);
        if (root == lead) {
            if ((threadIdx.x & 63) == (unsigned)__ffsll((long long)m) - 1u) atomicAdd(comp_faces + lead, (int)__popcll(m));
            pending = false;
        }
    }
}

hipError_t launch_mesh_components(const int *faces, long long n_triangles, long long n_vertices, int *vertex_label, int *component_faces, long long *n_components,
                                  void *scratch, unsigned *fault, hipStream_t stream)
{
    const unsigned F = (unsigned)n_triangles, V = (unsigned)n_vertices;
    const unsigned fb = (F + CC_THREADS - 1) / CC_THREADS, vb = (V + CC_THREADS - 1) / CC_THREADS;
    const u64 b = 2ull * V + 64;
    const unsigned bound = b > 0xffffffffull ? 0xffffffffu : (unsigned)b;
    CcHeader *h = (CcHeader *)scratch;
    hipError_t e = hipMemsetAsync(scratch, 0, MESH_CC_SCRATCH_BYTES, stream);
    if (e != hipSuccess) return e;
    if (fb) hipLaunchKernelGGL(cc_check_kernel, dim3(fb), dim3(CC_THREADS), 0, stream, faces, F, V, h, fault);
    hipLaunchKernelGGL(cc_init_kernel, dim3(vb ? vb : 1), dim3(CC_THREADS), 0, stream, vertex_label, component_faces, V, n_components, h);
    if (fb && vb) hipLaunchKernelGGL(cc_hook_kernel, dim3(fb), dim3(CC_THREADS), 0, stream, faces, F, V, vertex_label, h, bound, fault);
    if (vb) hipLaunchKernelGGL(cc_flatten_kernel, dim3(vb), dim3(CC_THREADS), 0, stream, vertex_label, V, n_components, h, bound, fault);
    if (fb && vb) hipLaunchKernelGGL(cc_sizes_kernel, dim3(fb), dim3(CC_THREADS), 0, stream, faces, F, V, vertex_label, component_faces, h);
    return hipGetLastError();
}

// ---- filter ----------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_THREADS) void cc_filter_count_kernel(const int *__restrict__ faces, unsigned F, unsigned V, const int *__restrict__ label,
                                                                     const unsigned char *__restrict__ keep_root, unsigned char *__restrict__ cnt8,
                                                                     u64 *__restrict__ tile_sum, u64 *__restrict__ totals, unsigned *__restrict__ fault)
{
    __shared__ u64 lds[CC_THREADS / 64];
    u64 mine = 0;
    bool bad = false;
#pragma unroll
    for (int r = 0; r < CC_PER_THREAD; ++r) {
        const unsigned e = blockIdx.x * CC_TILE + r * CC_THREADS + threadIdx.x;          // < n_tiles * CC_TILE: inside cnt8's padded extent
        unsigned byte = 0;
        if (e < V) {
            const int l = label[e];
            if ((unsigned)l >= V) bad = true;
            else if (keep_root[l]) byte |= 1u;
        }
        if (e < F) {
            const int *t = faces + (size_t)e * 3;
            const int a = t[0];
            if ((unsigned)a >= V || (unsigned)t[1] >= V || (unsigned)t[2] >= V) {
                bad = true;
            } else {
                const int l = label[a];
                if ((unsigned)l >= V) bad = true;
                else if (keep_root[l]) byte |= 8u;
            }
        }
        cnt8[e] = (unsigned char)byte;
        mine += (u64)(byte & 1u) | ((u64)(byte >> 3) << 32);
    }
    if (bad) {
        totals[1] = 1;
        *fault = 1u;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
#pragma unroll
        for (int w = 0; w < CC_THREADS / 64; ++w) s += lds[w];
        tile_sum[blockIdx.x] = s;
    }
}

struct CcEmit {
    const float *verts;    // [V][3] or nullptr
    float *verts_out;      // [cap_v][3] or nullptr
    int *faces_out;        // [cap_f][3]
    int *kept_vertex;      // [cap_v]
    unsigned cap_v, cap_f; // declared counts = capacities: no store at or beyond them
    unsigned *fault;
};

__global__ __launch_bounds__(CC_THREADS) void cc_filter_emit_kernel(const int *__restrict__ faces, unsigned F, unsigned V, const unsigned char *__restrict__ cnt8,
                                                                    const unsigned *__restrict__ vbase, const unsigned *__restrict__ tbase,
                                                                    const u64 *__restrict__ totals, CcEmit o)
{
    const unsigned e = blockIdx.x * CC_THREADS + threadIdx.x;
    const u64 tot = totals[0];
    if (totals[1] != 0 || (unsigned)(tot & 0xffffffffull) != o.cap_v || (unsigned)(tot >> 32) != o.cap_f) {      // bad input at count time, or the declared counts are
        if (e == 0) *o.fault = 1u;                                                                                 // not the counted ones: nothing is written
        return;
    }
    if (e >= V && e >= F) return;
    const unsigned byte = cnt8[e];
    bool bad = false;
    if (e < V && (byte & 1u)) {
        const unsigned n = vbase[e];
        if (n < o.cap_v) {
            o.kept_vertex[n] = (int)e;
            if (o.verts && o.verts_out) {
                const float *s = o.verts + (size_t)e * 3;
                float *d = o.verts_out + (size_t)n * 3;
                d[0] = s[0];
                d[1] = s[1];
                d[2] = s[2];
            }
        } else {
            bad = true;
        }
    }
    if (e < F && (byte & 8u)) {
        const unsigned n = tbase[e];
        const int *t = faces + (size_t)e * 3;
        int vi[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int a = t[q];
            vi[q] = -1;
            if ((unsigned)a < V && (cnt8[a] & 1u)) vi[q] = (int)vbase[a];       // (range checked again: no load outside the scratch whatever `faces` holds now)
            if (vi[q] < 0 || (unsigned)vi[q] >= o.cap_v) bad = true;            // a corner that did not survive: the labels are not these faces'
        }
        if (n < o.cap_f && !bad) {
            int *d = o.faces_out + (size_t)n * 3;
            d[0] = vi[0];
            d[1] = vi[1];
            d[2] = vi[2];
        } else {
            bad = true;
        }
    }
    if (bad) *o.fault = 1u;
}

hipError_t launch_mesh_filter_count(const int *faces, long long n_triangles, long long n_vertices, const int *vertex_label, const unsigned char *keep_root,
                                    const MeshScratch &s, long long *counts_dev, unsigned *fault, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(s.totals, 0, 2 * sizeof(u64), stream);
    if (e != hipSuccess) return e;
    if (s.n_tiles)
        hipLaunchKernelGGL(cc_filter_count_kernel, dim3(s.n_tiles), dim3(CC_THREADS), 0, stream, faces, (unsigned)n_triangles, (unsigned)n_vertices, vertex_label, keep_root,
                           s.cnt8, s.tile_base, s.totals, fault);
    return launch_mesh_scan(s, counts_dev, stream);
}

hipError_t launch_mesh_filter_emit(const float *verts, const int *faces, long long n_triangles, long long n_vertices, const MeshScratch &s, float *verts_out,
                                   long long n_vertices_out, int *faces_out, long long n_triangles_out, int *kept_vertex, unsigned *fault, hipStream_t stream)
{
    const unsigned F = (unsigned)n_triangles, V = (unsigned)n_vertices, n = F > V ? F : V;
    CcEmit o;
    o.verts = verts;
    o.verts_out = verts_out;
    o.faces_out = faces_out;
    o.kept_vertex = kept_vertex;
    o.cap_v = (unsigned)n_vertices_out;
    o.cap_f = (unsigned)n_triangles_out;
    o.fault = fault;
    const unsigned blocks = (n + CC_THREADS - 1) / CC_THREADS;
    hipLaunchKernelGGL(cc_filter_emit_kernel, dim3(blocks ? blocks : 1), dim3(CC_THREADS), 0, stream, faces, F, V, s.cnt8, s.vbase, s.tbase, s.totals, o);
    return hipGetLastError();
}
