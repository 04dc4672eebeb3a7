// tvr_mesh_simplify.hip — vertex-clustering simplification (Rossignac–Borrel) of an indexed triangle mesh: what shrinks an exported mesh
// (mesh.simplify_clustering, TensorBase.export_mesh(simplify=)).  include/tvr.h tvr_mesh_simplify_* holds the definition the kernels match bit for bit; DESIGN.md §4.12.
//
//   count:  cell     per vertex: its lattice cell -> 64-bit key; insert into the CELL table (atomicCAS on the key claims or finds the slot, atomicMin on the slot's
//                    representative); the vertex remembers its slot.  A cell outside the lattice raises the header's `bad` word and the fault flag
//           resolve  per vertex: slot -> the slot's representative (final since the cell kernel ended)
//           tri      per triangle: corners -> representatives; two equal = collapsed.  Else the triple, rotated so that its smallest entry leads, is inserted into the
//                    TRIANGLE table: a slot holds a triangle index; claimed by atomicCAS from empty; an occupant with the same triple is joined by atomicMin, another
//                    one is probed past.  The occupant of a slot changes (downwards) but its triple never does, and nothing is deleted, so equal triples meet in one slot
//           flags    per element e: bit 0 = vertex e is its own representative, bit 3 = triangle e is the index left in its slot; tile sums; then tvr_mesh.hip's scan
//   emit:   accum    per vertex: its quantised in-cell fractions, added as INTEGERS onto the representative's sums (the order the adds land in does not matter)
//           emit     per element: vertex_map, the representatives' new positions, the surviving triangles re-indexed
//
// Every probe sequence is bounded by the table's capacity and gives up by raising the fault flag.  No workgroup waits for another; the kernel boundary is the only
// ordering (values read inside the kernel that writes them come back from the atomics themselves).  Atomics: atomicCAS, atomicMin, atomicAdd on unsigned long long.
// No float is ever added atomically.  Every kernel after `bad` was raised returns at once, and the emit kernel writes only below the declared capacities.
#include "tvr_kernels.h"

#define SP_THREADS 256
#define SP_PER_THREAD 4
#define SP_TILE (SP_THREADS * SP_PER_THREAD)
#define SP_HEADER_BYTES 256
#define SP_MIN_CAPACITY 256ull
#define SP_EMPTY_KEY 0xffffffffffffffffull          // three 21-bit cell coordinates fill 63 bits: never a key
#define SP_EMPTY 0xffffffffu                        // never an index: counts stay below 2^31
#define SP_CELL_LIMIT 2097152.0f                    // 2^21 cells per axis
#define SP_Q_SCALE 1048576.0f                       // 2^20 steps inside a cell

static_assert(TVR_MESH_TILE == SP_TILE && TVR_MESH_SCAN_CHUNK == SP_THREADS, "the flags share tvr_mesh.hip's scan: same tile, same chunk");

typedef unsigned long long u64;

static inline size_t sp_align(size_t v) { return (v + 255) / 256 * 256; }

static inline u64 sp_capacity(long long n)
{
    u64 c = SP_MIN_CAPACITY;
    while (c < 2ull * (u64)n) c <<= 1;
    return c;
}

SimplifyScratch simplify_carve(long long n_vertices, long long n_triangles, void *scratch)
{
    SimplifyScratch s;
    const size_t V = (size_t)n_vertices, F = (size_t)n_triangles;
    char *b = (char *)scratch;
    size_t off = 0;
    s.cap_v = sp_capacity(n_vertices);
    s.cap_t = sp_capacity(n_triangles);
    s.header = (unsigned *)(b + off);       off += SP_HEADER_BYTES;
    s.flags = mesh_carve(n_vertices > n_triangles ? n_vertices : n_triangles, b + off);
    off += s.flags.total;
    s.vrep = (unsigned *)(b + off);         off += sp_align(V * sizeof(unsigned));
    s.tslot = (unsigned *)(b + off);        off += sp_align(F * sizeof(unsigned));
    s.fill_off = off;
    s.cell_key = (u64 *)(b + off);          off += sp_align((size_t)s.cap_v * sizeof(u64));
    s.cell_rep = (unsigned *)(b + off);     off += sp_align((size_t)s.cap_v * sizeof(unsigned));
    s.tri_slot = (unsigned *)(b + off);     off += sp_align((size_t)s.cap_t * sizeof(unsigned));
    s.fill_bytes = off - s.fill_off;
    s.sums_off = off;
    s.sums = (u64 *)(b + off);              off += sp_align(V * 4 * sizeof(u64));
    s.sums_bytes = off - s.sums_off;
    s.total = off;
    return s;
}

// splitmix64's finaliser
__device__ __forceinline__ u64 sp_mix(u64 x)
{
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

// the workgroup's longest probe sequence -> header[1], one lane per wave and only when it would raise the word.  The loop is a maximum by atomicCAS: the word only
// grows, so every failed exchange brings a larger value back and the loop ends after at most `steps` rounds — it waits for nobody.
__device__ __forceinline__ void sp_note_probe(unsigned steps, unsigned *header)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)steps, d, 64);
        steps = o > steps ? o : steps;
    }
    if ((threadIdx.x & 63) == 0) {
        unsigned cur = header[1];
        while (steps > cur) {
            const unsigned old = atomicCAS(header + 1, cur, steps);
            if (old == cur) break;
            cur = old;
        }
    }
}

// lattice coordinates of a point: g = (p - origin) * inv_cell, c = floorf(g), each operation rounded on its own; false = outside 0 .. 2^21-1 on an axis (NaN included)
__device__ __forceinline__ bool sp_cell_of(const float *__restrict__ p, const SimplifyLattice &l, float g[3], float c[3])
{
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float d = p[a] - l.origin[a];
        g[a] = d * l.inv_cell[a];
        c[a] = floorf(g[a]);
        ok = ok && (c[a] >= 0.0f && c[a] < SP_CELL_LIMIT);
    }
    return ok;
}

__global__ __launch_bounds__(SP_THREADS) void sp_cell_kernel(const float *__restrict__ verts, unsigned V, SimplifyLattice l, u64 *cell_key, unsigned *cell_rep,
                                                             unsigned mask, unsigned *__restrict__ vslot, unsigned *header, unsigned *__restrict__ fault)
{
    const unsigned v = blockIdx.x * SP_THREADS + threadIdx.x;
    unsigned steps = 0;
    if (v < V) {
        float g[3], c[3];
        bool ok = sp_cell_of(verts + (size_t)v * 3, l, g, c);
        if (ok) {
            const u64 key = (u64)(unsigned)c[0] | ((u64)(unsigned)c[1] << 21) | ((u64)(unsigned)c[2] << 42);
            unsigned slot = (unsigned)sp_mix(key) & mask;
            ok = false;
            for (u64 i = 0; i <= (u64)mask; ++i) {                    // at most `capacity` slots
                if (steps != SP_EMPTY) ++steps;
                const u64 old = atomicCAS(cell_key + slot, SP_EMPTY_KEY, key);
                if (old == SP_EMPTY_KEY || old == key) {
                    atomicMin(cell_rep + slot, v);
                    vslot[v] = slot;
                    ok = true;
                    break;
                }
                slot = (slot + 1u) & mask;
            }
        }
        if (!ok) {                                                   // outside the lattice, or the table is full (it holds twice the vertices: out of reach)
            header[0] = 1u;
            *fault = 1u;
        }
    }
    sp_note_probe(steps, header);
}

__global__ __launch_bounds__(SP_THREADS) void sp_resolve_kernel(unsigned *__restrict__ vrep, unsigned V, const unsigned *__restrict__ cell_rep, unsigned mask,
                                                                unsigned *header, unsigned *__restrict__ fault)
{
    if (header[0]) return;
    const unsigned v = blockIdx.x * SP_THREADS + threadIdx.x;
    if (v >= V) return;
    const unsigned r = cell_rep[vrep[v] & mask];
    if (r > v) {                                                     // the representative is the cluster's minimum: never above a member
        header[0] = 1u;
        *fault = 1u;
        return;
    }
    vrep[v] = r;
}

// the triple of representatives of triangle f, rotated so that its smallest entry leads; false = a corner outside 0 .. V-1, or two equal representatives
__device__ __forceinline__ bool sp_triple(const int *__restrict__ faces, const unsigned *__restrict__ vrep, unsigned V, unsigned f, unsigned t[3], bool &in_range)
{
    const int *p = faces + (size_t)f * 3;
    const unsigned a = (unsigned)p[0], b = (unsigned)p[1], c = (unsigned)p[2];          // (a negative index is a huge unsigned one)
    in_range = a < V && b < V && c < V;
    if (!in_range) return false;
    const unsigned ra = vrep[a], rb = vrep[b], rc = vrep[c];
    if (ra == rb || rb == rc || ra == rc) return false;
    if (rb < ra && rb < rc) {
        t[0] = rb; t[1] = rc; t[2] = ra;
    } else if (rc < ra && rc < rb) {
        t[0] = rc; t[1] = ra; t[2] = rb;
    } else {
        t[0] = ra; t[1] = rb; t[2] = rc;
    }
    return true;
}

__global__ __launch_bounds__(SP_THREADS) void sp_tri_kernel(const int *__restrict__ faces, unsigned F, unsigned V, const unsigned *__restrict__ vrep, unsigned *tri_slot,
                                                            unsigned mask, unsigned *__restrict__ tslot, unsigned *header, unsigned *__restrict__ fault)
{
    if (header[0]) return;
    const unsigned f = blockIdx.x * SP_THREADS + threadIdx.x;
    unsigned steps = 0;
    if (f < F) {
        unsigned t[3];
        bool in_range;
        if (sp_triple(faces, vrep, V, f, t, in_range)) {
            unsigned slot = (unsigned)sp_mix(((u64)t[0] | ((u64)t[1] << 32)) ^ sp_mix((u64)t[2])) & mask;
            bool ok = false;
            for (u64 i = 0; i <= (u64)mask; ++i) {
                if (steps != SP_EMPTY) ++steps;
                const unsigned old = atomicCAS(tri_slot + slot, SP_EMPTY, f);
                if (old == SP_EMPTY) {
                    ok = true;
                    break;
                }
                unsigned o[3];
                bool o_range;
                if (old < F && sp_triple(faces, vrep, V, old, o, o_range) && o[0] == t[0] && o[1] == t[1] && o[2] == t[2]) {
                    atomicMin(tri_slot + slot, f);
                    ok = true;
                    break;
                }
                slot = (slot + 1u) & mask;
            }
            tslot[f] = slot;
            if (!ok) {
                header[0] = 1u;
                *fault = 1u;
            }
        } else {
            tslot[f] = 0u;                                           // collapsed: in no slot, so tri_slot[0] is never f
            if (!in_range) {
                header[0] = 1u;
                *fault = 1u;
            }
        }
    }
    sp_note_probe(steps, header);
}

__global__ __launch_bounds__(SP_THREADS) void sp_flags_kernel(unsigned F, unsigned V, const unsigned *__restrict__ vrep, const unsigned *__restrict__ tslot,
                                                              const unsigned *__restrict__ tri_slot, unsigned mask, const unsigned *__restrict__ header,
                                                              unsigned char *__restrict__ cnt8, u64 *__restrict__ tile_sum)
{
    __shared__ u64 lds[SP_THREADS / 64];
    const bool bad = header[0] != 0;                                 // bad input: every flag is 0 and the totals are {0, 0}
    u64 mine = 0;
#pragma unroll
    for (int r = 0; r < SP_PER_THREAD; ++r) {
        const unsigned e = blockIdx.x * SP_TILE + r * SP_THREADS + threadIdx.x;           // < n_tiles * SP_TILE: inside cnt8's padded extent
        unsigned byte = 0;
        if (!bad) {
            if (e < V && vrep[e] == e) byte |= 1u;
            if (e < F && tri_slot[tslot[e] & mask] == e) byte |= 8u;
        }
        cnt8[e] = (unsigned char)byte;
        mine += (u64)(byte & 1u) | ((u64)(byte >> 3) << 32);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
#pragma unroll
        for (int w = 0; w < SP_THREADS / 64; ++w) s += lds[w];
        tile_sum[blockIdx.x] = s;
    }
}

hipError_t launch_mesh_simplify_count(const float *verts, long long n_vertices, const int *faces, long long n_triangles, const SimplifyLattice &lat,
                                      const SimplifyScratch &s, long long *counts_dev, unsigned *fault, hipStream_t stream)
{
    const unsigned F = (unsigned)n_triangles, V = (unsigned)n_vertices;
    const unsigned fb = (F + SP_THREADS - 1) / SP_THREADS, vb = (V + SP_THREADS - 1) / SP_THREADS;
    const unsigned mask_v = (unsigned)(s.cap_v - 1), mask_t = (unsigned)(s.cap_t - 1);
    hipError_t e = hipMemsetAsync(s.header, 0, SP_HEADER_BYTES, stream);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync((char *)s.header + s.fill_off, 0xff, s.fill_bytes, stream)) != hipSuccess) return e;
    if (vb) {
        hipLaunchKernelGGL(sp_cell_kernel, dim3(vb), dim3(SP_THREADS), 0, stream, verts, V, lat, s.cell_key, s.cell_rep, mask_v, s.vrep, s.header, fault);
        hipLaunchKernelGGL(sp_resolve_kernel, dim3(vb), dim3(SP_THREADS), 0, stream, s.vrep, V, s.cell_rep, mask_v, s.header, fault);
    }
    if (fb) hipLaunchKernelGGL(sp_tri_kernel, dim3(fb), dim3(SP_THREADS), 0, stream, faces, F, V, s.vrep, s.tri_slot, mask_t, s.tslot, s.header, fault);
    if (s.flags.n_tiles)
        hipLaunchKernelGGL(sp_flags_kernel, dim3(s.flags.n_tiles), dim3(SP_THREADS), 0, stream, F, V, s.vrep, s.tslot, s.tri_slot, mask_t, s.header, s.flags.cnt8,
                           s.flags.tile_base);
    return launch_mesh_scan(s.flags, counts_dev, stream);
}

// ---- emit ------------------------------------------------------------------------------------------------------------------------------------------------------
struct SpEmit {
    float *verts_out;      // [cap_v][3]
    int *faces_out;        // [cap_f][3]
    int *vertex_map;       // [V]
    unsigned cap_v, cap_f; // declared counts = capacities: no store at or beyond them
    unsigned *fault;
};

__device__ __forceinline__ bool sp_refused(const unsigned *__restrict__ header, const u64 *__restrict__ totals, unsigned cap_v, unsigned cap_f)
{
    const u64 tot = totals[0];
    return header[0] != 0 || (unsigned)(tot & 0xffffffffull) != cap_v || (unsigned)(tot >> 32) != cap_f;
}

__global__ __launch_bounds__(SP_THREADS) void sp_accum_kernel(const float *__restrict__ verts, unsigned V, SimplifyLattice l, const unsigned *__restrict__ vrep,
                                                              u64 *sums, const unsigned *__restrict__ header, const u64 *__restrict__ totals, unsigned cap_v,
                                                              unsigned cap_f, unsigned *__restrict__ fault)
{
    if (sp_refused(header, totals, cap_v, cap_f)) return;            // (the emit kernel raises the flag)
    const unsigned v = blockIdx.x * SP_THREADS + threadIdx.x;
    if (v >= V) return;
    float g[3], c[3];
    const unsigned r = vrep[v];
    if (!sp_cell_of(verts + (size_t)v * 3, l, g, c) || r >= V) {     // not the vertices that were counted
        *fault = 1u;
        return;
    }
    u64 *s = sums + (size_t)r * 4;
    atomicAdd(s, 1ull);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float f = g[a] - c[a];                                 // exact, in [0, 1)
        atomicAdd(s + 1 + a, (u64)(unsigned)(f * SP_Q_SCALE));       // truncates; < 2^20
    }
}

__global__ __launch_bounds__(SP_THREADS) void sp_emit_kernel(const float *__restrict__ verts, const int *__restrict__ faces, unsigned F, unsigned V, SimplifyLattice l,
                                                             const unsigned *__restrict__ vrep, const u64 *__restrict__ sums,
                                                             const unsigned char *__restrict__ cnt8, const unsigned *__restrict__ vbase,
                                                             const unsigned *__restrict__ tbase, const unsigned *__restrict__ header, const u64 *__restrict__ totals,
                                                             SpEmit o)
{
    const unsigned e = blockIdx.x * SP_THREADS + threadIdx.x;
    if (sp_refused(header, totals, o.cap_v, o.cap_f)) {              // bad input at count time, or the declared counts are not the counted ones: nothing is written
        if (e == 0) *o.fault = 1u;
        return;
    }
    if (e >= V && e >= F) return;
    const unsigned byte = cnt8[e];
    bool bad = false;
    if (e < V) {
        const unsigned r = vrep[e];
        const unsigned n = r < V && (cnt8[r] & 1u) ? vbase[r] : SP_EMPTY;
        if (n < o.cap_v) {
            o.vertex_map[e] = (int)n;
            if (byte & 1u) {                                         // e is its cluster's representative (then r == e): the cluster's vertex
                float g[3], c[3];
                const u64 *s = sums + (size_t)e * 4;
                const u64 members = s[0];
                if (sp_cell_of(verts + (size_t)e * 3, l, g, c) && members != 0) {
                    float *d = o.verts_out + (size_t)n * 3;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const float frac = (float)((double)s[1 + a] / ((double)members * 1048576.0));
                        const float corner = l.origin[a] + c[a] * l.cell[a];
                        d[a] = corner + frac * l.cell[a];
                    }
                } else {
                    bad = true;
                }
            }
        } else {
            bad = true;
        }
    }
    if (e < F && (byte & 8u)) {
        const unsigned n = tbase[e];
        const int *t = faces + (size_t)e * 3;
        int vi[3];
        bool tri_ok = true;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const unsigned a = (unsigned)t[q];
            unsigned m = SP_EMPTY;
            if (a < V) {                                             // (range checked again: no load outside the scratch whatever `faces` holds now)
                const unsigned r = vrep[a];
                if (r < V && (cnt8[r] & 1u)) m = vbase[r];
            }
            if (m >= o.cap_v) tri_ok = false;
            vi[q] = (int)m;
        }
        if (n < o.cap_f && tri_ok) {
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

hipError_t launch_mesh_simplify_emit(const float *verts, long long n_vertices, const int *faces, long long n_triangles, const SimplifyLattice &lat,
                                     const SimplifyScratch &s, float *verts_out, long long n_vertices_out, int *faces_out, long long n_triangles_out, int *vertex_map,
                                     unsigned *fault, hipStream_t stream)
{
    const unsigned F = (unsigned)n_triangles, V = (unsigned)n_vertices, n = F > V ? F : V;
    SpEmit o;
    o.verts_out = verts_out;
    o.faces_out = faces_out;
    o.vertex_map = vertex_map;
    o.cap_v = (unsigned)n_vertices_out;
    o.cap_f = (unsigned)n_triangles_out;
    o.fault = fault;
    const unsigned vb = (V + SP_THREADS - 1) / SP_THREADS, blocks = (n + SP_THREADS - 1) / SP_THREADS;
    if (s.sums_bytes) {
        hipError_t e = hipMemsetAsync(s.sums, 0, s.sums_bytes, stream);
        if (e != hipSuccess) return e;
    }
    if (vb)
        hipLaunchKernelGGL(sp_accum_kernel, dim3(vb), dim3(SP_THREADS), 0, stream, verts, V, lat, s.vrep, s.sums, s.header, s.flags.totals, o.cap_v, o.cap_f, fault);
    hipLaunchKernelGGL(sp_emit_kernel, dim3(blocks ? blocks : 1), dim3(SP_THREADS), 0, stream, verts, faces, F, V, lat, s.vrep, s.sums, s.flags.cnt8, s.flags.vbase,
                       s.flags.tbase, s.header, s.flags.totals, o);
    return hipGetLastError();
}
