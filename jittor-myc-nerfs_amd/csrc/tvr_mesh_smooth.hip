// tvr_mesh_smooth.hip — vertex adjacency (CSR, with the number of face sides on every edge) of an indexed triangle mesh, and Taubin lambda|mu smoothing over it: what
// smooths an exported mesh (mesh.mesh_adjacency, mesh.smooth_taubin, TensorBase.export_mesh(smooth=)).  include/tvr.h tvr_mesh_adjacency_* / tvr_mesh_smooth hold the
// definitions the kernels match bit for bit; DESIGN.md §4.13.
//
//   count:  degree   per face: its three sides {a,b}, {b,c}, {c,a} (a side with equal ends is skipped); each side adds 1 to the RAW degree of both ends (32-bit atomicAdd).
//                    A corner outside 0 .. V-1 raises the header's `bad` word and the fault flag
//           scan     raw degrees -> raw row starts (reduce / scan / add over tiles of ADJ_TILE entries, 32-bit: tvr_mesh.hip's scheme on plain uint32 arrays)
//           fill     per face: every side writes the other end into both ends' raw rows through a per-row cursor (atomicAdd).  The order inside a raw row depends on
//                    the order the atomics land in; the sort below removes it
//           sort     raw rows of at most ADJ_SHORT entries: ONE THREAD sorts its row by insertion (<= ADJ_SHORT^2 / 2 steps) and run-length encodes it in place;
//                    longer rows are appended to a list and sorted by ONE WORKGROUP each: a bitonic network for any length (every comparator ascending, so the virtual
//                    +infinity padding behind the row never moves), log2(n)(log2(n)+1)/2 passes of n/2 comparators spread over 256 lanes, then a run-length encoding by
//                    two block scans.  After it a row starts with its distinct neighbours, ascending, and the parallel array holds edge_faces
//           scan     degrees -> offsets; the four counts
//   emit:   one thread per half-edge k: its row by binary search in the offsets (<= 32 steps), then a copy from the raw row; one thread per offset
//
//   smooth: check    offsets non-decreasing from 0 to H, every neighbour in 0 .. V-1, else the `bad` word and the fault flag
//           load     positions -> 16-byte rows {x, y, z, pinned} in the scratch (one 16-byte load per gathered neighbour instead of three 4-byte ones)
//           step     one launch per half step: every vertex gathers its neighbours in the row's order from the previous half step's rows, no atomics; the last half
//                    step writes verts_out
//
// No workgroup waits for another; the kernel boundary is the only ordering between workgroups.  Atomics: 32-bit integer atomicAdd / atomicMax only.  Every loop is bounded
// by a count the host checked (< 2^31), every index is compared with its array's extent where it is used, and every kernel after `bad` was raised returns at once.
#include "tvr_kernels.h"

#define ADJ_THREADS 256
#define ADJ_PER_THREAD 4
#define ADJ_TILE (ADJ_THREADS * ADJ_PER_THREAD)
#define ADJ_HEADER_BYTES 256
#define ADJ_LONG_BLOCKS 256                         // workgroups that walk the list of long rows

static_assert(ADJ_SHORT >= 2 && ADJ_SHORT <= 256, "one thread sorts a short row by insertion");

// header words
#define ADJ_H_BAD 0
#define ADJ_H_LONG 1
#define ADJ_H_BOUNDARY 2
#define ADJ_H_NONMANIFOLD 3
#define ADJ_H_MAXDEG 4
#define ADJ_H_TOTAL 5
#define ADJ_H_RAW_TOTAL 6

static inline size_t adj_align(size_t v) { return (v + 255) / 256 * 256; }

AdjScratch adj_carve(long long n_vertices, long long n_triangles, void *scratch)
{
    AdjScratch s;
    const size_t V = (size_t)n_vertices, R = (size_t)n_triangles * 6, tiles = (V + ADJ_TILE - 1) / ADJ_TILE;
    char *b = (char *)scratch;
    size_t off = 0;
    s.raw_cap = (unsigned)R;
    s.n_tiles = (unsigned)tiles;
    s.header = (unsigned *)(b + off);       off += ADJ_HEADER_BYTES;
    s.tile = (unsigned *)(b + off);         off += adj_align(tiles * sizeof(unsigned));
    s.deg = (unsigned *)(b + off);          off += adj_align(V * sizeof(unsigned));
    s.long_rows = (unsigned *)(b + off);    off += adj_align(V * sizeof(unsigned));
    s.raw_off = (unsigned *)(b + off);      off += adj_align((V + 1) * sizeof(unsigned));
    s.off = (unsigned *)(b + off);          off += adj_align((V + 1) * sizeof(unsigned));
    s.raw = (unsigned *)(b + off);          off += adj_align(R * sizeof(unsigned));
    s.cnt = (unsigned *)(b + off);          off += adj_align(R * sizeof(unsigned));
    s.total = off;
    return s;
}

// exclusive scan of x over the 256 threads of the workgroup; `total` = the workgroup's sum.  lds: 4 entries.
__device__ __forceinline__ unsigned adj_block_scan(unsigned x, unsigned *lds, unsigned &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = (unsigned)__shfl_up((int)inc, d, 64);
        if (lane >= d) inc += y;
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    unsigned woff = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < ADJ_THREADS / 64; ++i) {
        const unsigned s = lds[i];
        if (i < w) woff += s;
        tot += s;
    }
    __syncthreads();           // lds may be written again
    total = tot;
    return woff + inc - x;
}

__device__ __forceinline__ void adj_raise(unsigned *header, unsigned *fault)
{
    header[ADJ_H_BAD] = 1u;
    *fault = 1u;
}

// ---- the 32-bit scan: in [n] -> out [n + 1] (exclusive, out[n] = the total, also left in *total_word) ---------------------------------------------------------------
__global__ __launch_bounds__(ADJ_THREADS) void adj_tile_sum_kernel(const unsigned *__restrict__ in, unsigned n, unsigned *__restrict__ tile)
{
    __shared__ unsigned lds[ADJ_THREADS / 64];
    unsigned mine = 0;
#pragma unroll
    for (int r = 0; r < ADJ_PER_THREAD; ++r) {
        const size_t i = (size_t)blockIdx.x * ADJ_TILE + r * ADJ_THREADS + threadIdx.x;
        if (i < n) mine += in[i];
    }
    unsigned total;
    adj_block_scan(mine, lds, total);
    if (threadIdx.x == 0) tile[blockIdx.x] = total;
}

// ONE workgroup: tile sums -> exclusive bases, in place, ADJ_THREADS tiles per step with a running carry
__global__ __launch_bounds__(ADJ_THREADS) void adj_scan_tiles_kernel(unsigned *__restrict__ tile, unsigned n_tiles, unsigned *__restrict__ out, unsigned n,
                                                                     unsigned *__restrict__ total_word)
{
    __shared__ unsigned lds[ADJ_THREADS / 64];
    unsigned carry = 0;
    for (unsigned t0 = 0; t0 < n_tiles; t0 += ADJ_THREADS) {
        const unsigned t = t0 + threadIdx.x;
        const unsigned x = t < n_tiles ? tile[t] : 0;
        unsigned total;
        const unsigned ex = adj_block_scan(x, lds, total);
        if (t < n_tiles) tile[t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        out[n] = carry;
        *total_word = carry;
    }
}

// per tile: thread t takes the 4 consecutive entries tile * ADJ_TILE + 4 t ..
__global__ __launch_bounds__(ADJ_THREADS) void adj_scan_entries_kernel(const unsigned *__restrict__ in, unsigned n, const unsigned *__restrict__ tile,
                                                                       unsigned *__restrict__ out)
{
    __shared__ unsigned lds[ADJ_THREADS / 64];
    const size_t i0 = (size_t)blockIdx.x * ADJ_TILE + ADJ_PER_THREAD * threadIdx.x;
    unsigned c[ADJ_PER_THREAD], mine = 0;
#pragma unroll
    for (int r = 0; r < ADJ_PER_THREAD; ++r) {
        c[r] = i0 + r < n ? in[i0 + r] : 0;
        mine += c[r];
    }
    unsigned total;
    unsigned run = tile[blockIdx.x] + adj_block_scan(mine, lds, total);
#pragma unroll
    for (int r = 0; r < ADJ_PER_THREAD; ++r) {
        if (i0 + r < n) out[i0 + r] = run;
        run += c[r];
    }
}

static void adj_scan(const unsigned *in, unsigned n, unsigned *out, const AdjScratch &s, unsigned *total_word, hipStream_t stream)
{
    if (s.n_tiles) hipLaunchKernelGGL(adj_tile_sum_kernel, dim3(s.n_tiles), dim3(ADJ_THREADS), 0, stream, in, n, s.tile);
    hipLaunchKernelGGL(adj_scan_tiles_kernel, dim3(1), dim3(ADJ_THREADS), 0, stream, s.tile, s.n_tiles, out, n, total_word);
    if (s.n_tiles) hipLaunchKernelGGL(adj_scan_entries_kernel, dim3(s.n_tiles), dim3(ADJ_THREADS), 0, stream, in, n, s.tile, out);
}

// ---- count ---------------------------------------------------------------------------------------------------------------------------------------------------------
// the corners of face f; false = one lies outside 0 .. V-1 (a negative index is a huge unsigned one)
__device__ __forceinline__ bool adj_corners(const int *__restrict__ faces, unsigned f, unsigned V, unsigned c[3])
{
    const int *p = faces + (size_t)f * 3;
    c[0] = (unsigned)p[0];
    c[1] = (unsigned)p[1];
    c[2] = (unsigned)p[2];
    return c[0] < V && c[1] < V && c[2] < V;
}

__global__ __launch_bounds__(ADJ_THREADS) void adj_degree_kernel(const int *__restrict__ faces, unsigned F, unsigned V, unsigned *deg, unsigned *header,
                                                                 unsigned *__restrict__ fault)
{
    const unsigned f = blockIdx.x * ADJ_THREADS + threadIdx.x;
    if (f >= F) return;
    unsigned c[3];
    if (!adj_corners(faces, f, V, c)) {
        adj_raise(header, fault);
        return;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const unsigned a = c[q], b = c[(q + 1) % 3];
        if (a == b) continue;
        atomicAdd(deg + a, 1u);
        atomicAdd(deg + b, 1u);
    }
}

// one end of a side: `other` goes into the raw row of `v` at the row's cursor
__device__ __forceinline__ bool adj_put(unsigned v, unsigned other, unsigned *cursor, const unsigned *__restrict__ raw_off, unsigned *__restrict__ raw, unsigned raw_cap)
{
    const unsigned at = raw_off[v] + atomicAdd(cursor + v, 1u);
    if (at >= raw_off[v + 1] || at >= raw_cap) return false;         // more sides than were counted: not the faces that were counted
    raw[at] = other;
    return true;
}

__global__ __launch_bounds__(ADJ_THREADS) void adj_fill_kernel(const int *__restrict__ faces, unsigned F, unsigned V, unsigned *cursor,
                                                               const unsigned *__restrict__ raw_off, unsigned *__restrict__ raw, unsigned raw_cap, unsigned *header,
                                                               unsigned *__restrict__ fault)
{
    if (header[ADJ_H_BAD]) return;
    const unsigned f = blockIdx.x * ADJ_THREADS + threadIdx.x;
    if (f >= F) return;
    unsigned c[3];
    bool ok = adj_corners(faces, f, V, c);
    if (ok) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const unsigned a = c[q], b = c[(q + 1) % 3];
            if (a == b) continue;
            ok = adj_put(a, b, cursor, raw_off, raw, raw_cap) && ok;
            ok = adj_put(b, a, cursor, raw_off, raw, raw_cap) && ok;
        }
    }
    if (!ok) adj_raise(header, fault);
}

// the sum of x over the workgroup, in every thread.  lds: 4 entries
__device__ __forceinline__ unsigned adj_block_sum(unsigned x, unsigned *lds)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += (unsigned)__shfl_xor((int)x, d, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    unsigned s = 0;
#pragma unroll
    for (int w = 0; w < ADJ_THREADS / 64; ++w) s += lds[w];
    __syncthreads();
    return s;
}

// short rows: one thread each.  Long rows go onto the list.
__global__ __launch_bounds__(ADJ_THREADS) void adj_sort_short_kernel(unsigned V, const unsigned *__restrict__ raw_off, unsigned *__restrict__ raw,
                                                                     unsigned *__restrict__ cnt, unsigned raw_cap, unsigned *__restrict__ deg,
                                                                     unsigned *__restrict__ long_rows, unsigned *header, unsigned *__restrict__ fault)
{
    __shared__ unsigned lds[ADJ_THREADS / 64];
    if (header[ADJ_H_BAD]) return;
    const unsigned v = blockIdx.x * ADJ_THREADS + threadIdx.x;
    unsigned boundary = 0, nonmanifold = 0, d = 0;
    if (v < V) {
        const unsigned s = raw_off[v], e = raw_off[v + 1];
        if (s > e || e > raw_cap) {
            adj_raise(header, fault);
        } else if (e - s > ADJ_SHORT) {
            const unsigned at = atomicAdd(header + ADJ_H_LONG, 1u);
            if (at < V) long_rows[at] = v;
        } else {
            const unsigned n = e - s;
            unsigned *row = raw + s, *rc = cnt + s;
            for (unsigned i = 1; i < n; ++i) {                       // insertion sort, n <= ADJ_SHORT
                const unsigned x = row[i];
                unsigned j = i;
                while (j > 0 && row[j - 1] > x) {
                    row[j] = row[j - 1];
                    --j;
                }
                row[j] = x;
            }
            for (unsigned i = 0; i < n;) {                           // run lengths, in place: d <= i
                const unsigned x = row[i];
                unsigned j = i + 1;
                while (j < n && row[j] == x) ++j;
                row[d] = x;
                rc[d] = j - i;
                if (v < x) {                                         // every undirected edge is counted at its smaller end
                    boundary += j - i == 1 ? 1u : 0u;
                    nonmanifold += j - i > 2 ? 1u : 0u;
                }
                ++d;
                i = j;
            }
            deg[v] = d;
        }
    }
    boundary = adj_block_sum(boundary, lds);
    nonmanifold = adj_block_sum(nonmanifold, lds);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned y = (unsigned)__shfl_xor((int)d, o, 64);
        d = y > d ? y : d;
    }
    if (threadIdx.x == 0) {
        if (boundary) atomicAdd(header + ADJ_H_BOUNDARY, boundary);
        if (nonmanifold) atomicAdd(header + ADJ_H_NONMANIFOLD, nonmanifold);
    }
    if ((threadIdx.x & 63) == 0 && d) atomicMax(header + ADJ_H_MAXDEG, d);
}

__device__ __forceinline__ void adj_compare_exchange(unsigned *row, unsigned i, unsigned j)
{
    const unsigned a = row[i], b = row[j];
    if (a > b) {
        row[i] = b;
        row[j] = a;
    }
}

// long rows: one workgroup each, in place in the scratch (rows of this length are rare and sit in the L2)
__global__ __launch_bounds__(ADJ_THREADS) void adj_sort_long_kernel(unsigned V, const unsigned *__restrict__ raw_off, unsigned *raw, unsigned *cnt, unsigned raw_cap,
                                                                    unsigned *__restrict__ deg, const unsigned *__restrict__ long_rows, unsigned *header,
                                                                    unsigned *__restrict__ fault)
{
    __shared__ unsigned lds[ADJ_THREADS / 64];
    if (header[ADJ_H_BAD]) return;
    unsigned n_long = header[ADJ_H_LONG];
    n_long = n_long < V ? n_long : V;
    for (unsigned li = blockIdx.x; li < n_long; li += gridDim.x) {
        const unsigned v = long_rows[li];
        if (v >= V) continue;                                        // (uniform over the workgroup, like everything that steers a barrier below)
        const unsigned s = raw_off[v], e = raw_off[v + 1];
        if (s > e || e > raw_cap) continue;
        const unsigned n = e - s;
        unsigned *row = raw + s, *rc = cnt + s;
        // bitonic network over n entries: merges of width k = 2, 4, ..; the first pass of a merge pairs i with its mirror image in the block, the others pair i with
        // i + j.  Every comparator puts the smaller value at the smaller index, so entries at or beyond n (+infinity) would never move: those comparators are skipped.
        for (int lk = 1; lk <= 31 && (1u << (lk - 1)) < n; ++lk) {
            const unsigned half = 1u << (lk - 1);
            for (unsigned t = threadIdx.x; ; t += ADJ_THREADS) {
                const unsigned blk = t >> (lk - 1), r = t & (half - 1);
                const unsigned long long i = ((unsigned long long)blk << lk) + r, j = ((unsigned long long)blk << lk) + (2ull * half - 1 - r);
                if (i >= n) break;                                   // i grows with t
                if (j < n) adj_compare_exchange(row, (unsigned)i, (unsigned)j);
            }
            __syncthreads();
            for (int lj = lk - 2; lj >= 0; --lj) {
                const unsigned step = 1u << lj;
                for (unsigned t = threadIdx.x; ; t += ADJ_THREADS) {
                    const unsigned long long i = ((unsigned long long)(t >> lj) << (lj + 1)) + (t & (step - 1)), j = i + step;
                    if (i >= n) break;
                    if (j < n) adj_compare_exchange(row, (unsigned)i, (unsigned)j);
                }
                __syncthreads();
            }
        }
        // run lengths.  First the start of every run, by rank, into the parallel array (rank <= index) ..
        unsigned d = 0;
        for (unsigned c0 = 0; c0 < n; c0 += ADJ_THREADS) {
            const unsigned i = c0 + threadIdx.x;
            const unsigned head = i < n && (i == 0 || row[i] != row[i - 1]) ? 1u : 0u;
            unsigned total;
            const unsigned rank = d + adj_block_scan(head, lds, total);
            if (head) rc[rank] = i;
            d += total;
        }
        __syncthreads();
        // .. then, ADJ_THREADS runs at a time, value and length to the row's front: a store lands at or below every index still to be read
        unsigned boundary = 0, nonmanifold = 0;
        for (unsigned r0 = 0; r0 < d; r0 += ADJ_THREADS) {
            const unsigned r = r0 + threadIdx.x;
            unsigned x = 0, len = 0;
            if (r < d) {
                const unsigned at = rc[r], next = r + 1 < d ? rc[r + 1] : n;
                if (at < n && next <= n && at < next) {
                    x = row[at];
                    len = next - at;
                }
            }
            __syncthreads();
            if (r < d) {
                row[r] = x;
                rc[r] = len;
                if (v < x) {
                    boundary += len == 1 ? 1u : 0u;
                    nonmanifold += len > 2 ? 1u : 0u;
                }
            }
            __syncthreads();
        }
        boundary = adj_block_sum(boundary, lds);
        nonmanifold = adj_block_sum(nonmanifold, lds);
        if (threadIdx.x == 0) {
            deg[v] = d;
            if (boundary) atomicAdd(header + ADJ_H_BOUNDARY, boundary);
            if (nonmanifold) atomicAdd(header + ADJ_H_NONMANIFOLD, nonmanifold);
            atomicMax(header + ADJ_H_MAXDEG, d);
        }
    }
}

__global__ void adj_counts_kernel(const unsigned *__restrict__ header, long long *__restrict__ counts)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool bad = header[ADJ_H_BAD] != 0;
    counts[0] = bad ? 0 : (long long)header[ADJ_H_TOTAL];
    counts[1] = bad ? 0 : (long long)header[ADJ_H_BOUNDARY];
    counts[2] = bad ? 0 : (long long)header[ADJ_H_NONMANIFOLD];
    counts[3] = bad ? 0 : (long long)header[ADJ_H_MAXDEG];
}

hipError_t launch_mesh_adjacency_count(const int *faces, long long n_triangles, long long n_vertices, const AdjScratch &s, long long *counts_dev, unsigned *fault,
                                       hipStream_t stream)
{
    const unsigned F = (unsigned)n_triangles, V = (unsigned)n_vertices;
    const unsigned fb = (F + ADJ_THREADS - 1) / ADJ_THREADS, vb = (V + ADJ_THREADS - 1) / ADJ_THREADS;
    hipError_t e = hipMemsetAsync(s.header, 0, ADJ_HEADER_BYTES, stream);
    if (e != hipSuccess) return e;
    if (V && (e = hipMemsetAsync(s.deg, 0, (size_t)V * sizeof(unsigned), stream)) != hipSuccess) return e;
    if (fb) hipLaunchKernelGGL(adj_degree_kernel, dim3(fb), dim3(ADJ_THREADS), 0, stream, faces, F, V, s.deg, s.header, fault);
    adj_scan(s.deg, V, s.raw_off, s, s.header + ADJ_H_RAW_TOTAL, stream);
    if (V && (e = hipMemsetAsync(s.deg, 0, (size_t)V * sizeof(unsigned), stream)) != hipSuccess) return e;       // now the rows' cursors, then their degrees
    if (fb) hipLaunchKernelGGL(adj_fill_kernel, dim3(fb), dim3(ADJ_THREADS), 0, stream, faces, F, V, s.deg, s.raw_off, s.raw, s.raw_cap, s.header, fault);
    if (V && (e = hipMemsetAsync(s.deg, 0, (size_t)V * sizeof(unsigned), stream)) != hipSuccess) return e;
    if (vb) {
        hipLaunchKernelGGL(adj_sort_short_kernel, dim3(vb), dim3(ADJ_THREADS), 0, stream, V, s.raw_off, s.raw, s.cnt, s.raw_cap, s.deg, s.long_rows, s.header, fault);
        hipLaunchKernelGGL(adj_sort_long_kernel, dim3(vb < ADJ_LONG_BLOCKS ? vb : ADJ_LONG_BLOCKS), dim3(ADJ_THREADS), 0, stream, V, s.raw_off, s.raw, s.cnt, s.raw_cap,
                           s.deg, s.long_rows, s.header, fault);
    }
    adj_scan(s.deg, V, s.off, s, s.header + ADJ_H_TOTAL, stream);
    hipLaunchKernelGGL(adj_counts_kernel, dim3(1), dim3(64), 0, stream, s.header, counts_dev);
    return hipGetLastError();
}

// ---- emit ------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ADJ_THREADS) void adj_emit_kernel(unsigned V, unsigned H, const unsigned *__restrict__ header, const unsigned *__restrict__ off,
                                                               const unsigned *__restrict__ raw_off, const unsigned *__restrict__ raw, const unsigned *__restrict__ cnt,
                                                               unsigned raw_cap, int *__restrict__ offsets, int *__restrict__ neighbours, int *__restrict__ edge_faces,
                                                               unsigned *__restrict__ fault)
{
    const unsigned k = blockIdx.x * ADJ_THREADS + threadIdx.x;
    if (header[ADJ_H_BAD] != 0 || header[ADJ_H_TOTAL] != H) {        // bad input at count time, or the declared H is not the counted one: nothing is written
        if (k == 0) *fault = 1u;
        return;
    }
    bool bad = false;
    if (k <= V) {
        const unsigned o = off[k];
        if (o <= H) offsets[k] = (int)o;
        else bad = true;
    }
    if (k < H && V > 0) {
        unsigned lo = 0, hi = V;                                     // the last row v with off[v] <= k: off[0] = 0 <= k < H = off[V]
        for (int it = 0; it < 32 && hi - lo > 1; ++it) {
            const unsigned mid = lo + (hi - lo) / 2;
            if (off[mid] <= k) lo = mid;
            else hi = mid;
        }
        const unsigned first = off[lo], src = raw_off[lo] + (k - first);
        if (first <= k && src < raw_off[lo + 1] && src < raw_cap && raw[src] < V) {
            neighbours[k] = (int)raw[src];
            edge_faces[k] = (int)cnt[src];
        } else {
            bad = true;
        }
    }
    if (bad) *fault = 1u;
}

hipError_t launch_mesh_adjacency_emit(long long n_vertices, const AdjScratch &s, int *offsets, int *neighbours, int *edge_faces, long long n_half_edges, unsigned *fault,
                                      hipStream_t stream)
{
    const unsigned V = (unsigned)n_vertices, H = (unsigned)n_half_edges;
    const unsigned long long n = (unsigned long long)V + 1 > H ? (unsigned long long)V + 1 : H;
    hipLaunchKernelGGL(adj_emit_kernel, dim3((unsigned)((n + ADJ_THREADS - 1) / ADJ_THREADS)), dim3(ADJ_THREADS), 0, stream, V, H, s.header, s.off, s.raw_off, s.raw, s.cnt,
                       s.raw_cap, offsets, neighbours, edge_faces, fault);
    return hipGetLastError();
}

// ---- Taubin smoothing ------------------------------------------------------------------------------------------------------------------------------------------
SmoothScratch smooth_carve(long long n_vertices, void *scratch)
{
    SmoothScratch s;
    char *b = (char *)scratch;
    size_t off = 0;
    s.header = (unsigned *)(b + off);       off += ADJ_HEADER_BYTES;
    s.rows[0] = (float4 *)(b + off);        off += adj_align((size_t)n_vertices * sizeof(float4));
    s.rows[1] = (float4 *)(b + off);        off += adj_align((size_t)n_vertices * sizeof(float4));
    s.total = off;
    return s;
}

__global__ __launch_bounds__(ADJ_THREADS) void smooth_check_kernel(unsigned V, unsigned H, const int *__restrict__ offsets, const int *__restrict__ neighbours,
                                                                   unsigned *header, unsigned *__restrict__ fault)
{
    const unsigned k = blockIdx.x * ADJ_THREADS + threadIdx.x;
    bool ok = true;
    if (k <= V) {
        const unsigned o = (unsigned)offsets[k];
        ok = o <= H && (k != 0 || o == 0) && (k != V || o == H);
        if (ok && k < V) ok = o <= (unsigned)offsets[k + 1];
    }
    if (k < H) ok = ok && (unsigned)neighbours[k] < V;
    if (!ok) adj_raise(header, fault);
}

// positions -> 16-byte rows; w = 1 (as bits) for a pinned vertex: one whose row holds an edge with a single face side
__global__ __launch_bounds__(ADJ_THREADS) void smooth_load_kernel(const float *__restrict__ verts, unsigned V, unsigned H, const int *__restrict__ offsets,
                                                                  const int *__restrict__ edge_faces, float4 *__restrict__ rows, const unsigned *__restrict__ header)
{
    if (header[ADJ_H_BAD]) return;
    const unsigned v = blockIdx.x * ADJ_THREADS + threadIdx.x;
    if (v >= V) return;
    unsigned pinned = 0;
    if (edge_faces) {
        const unsigned s = (unsigned)offsets[v], e = (unsigned)offsets[v + 1];
        if (s <= e && e <= H)
            for (unsigned k = s; k < e; ++k) pinned |= edge_faces[k] == 1 ? 1u : 0u;
    }
    const float *p = verts + (size_t)v * 3;
    rows[v] = make_float4(p[0], p[1], p[2], __uint_as_float(pinned));
}

// iterations == 0: verts_out = verts, bit for bit
__global__ __launch_bounds__(ADJ_THREADS) void smooth_copy_kernel(const unsigned *__restrict__ verts, unsigned long long n, unsigned *__restrict__ verts_out,
                                                                  const unsigned *__restrict__ header)
{
    if (header[ADJ_H_BAD]) return;
    const unsigned long long i = (unsigned long long)blockIdx.x * ADJ_THREADS + threadIdx.x;
    if (i < n) verts_out[i] = verts[i];
}

// one half step with weight w: rows `in` -> rows `out4`, or -> verts_out (12-byte rows) when out3 is given.  -ffp-contract=off: every operation rounds on its own.
__global__ __launch_bounds__(ADJ_THREADS) void smooth_step_kernel(const float4 *__restrict__ in, float4 *__restrict__ out4, float *__restrict__ out3, unsigned V, unsigned H,
                                                                  const int *__restrict__ offsets, const int *__restrict__ neighbours, float w,
                                                                  const unsigned *__restrict__ header, unsigned *__restrict__ fault)
{
    if (header[ADJ_H_BAD]) return;
    const unsigned v = blockIdx.x * ADJ_THREADS + threadIdx.x;
    if (v >= V) return;
    const float4 p = in[v];
    float4 q = p;
    const unsigned s = (unsigned)offsets[v], e = (unsigned)offsets[v + 1];
    if (s > e || e > H) {                                            // not the adjacency that was checked
        *fault = 1u;
    } else if (s < e && __float_as_uint(p.w) == 0u) {
        unsigned nb = (unsigned)neighbours[s];
        bool ok = nb < V;
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;
        if (ok) {
            const float4 a = in[nb];
            sx = a.x;
            sy = a.y;
            sz = a.z;
        }
        unsigned k = s + 1;
        for (; e - k >= 4 && ok; k += 4) {                           // four gathers in flight; the adds keep the row's order
            const unsigned n0 = (unsigned)neighbours[k], n1 = (unsigned)neighbours[k + 1], n2 = (unsigned)neighbours[k + 2], n3 = (unsigned)neighbours[k + 3];
            ok = n0 < V && n1 < V && n2 < V && n3 < V;
            if (ok) {
                const float4 a = in[n0], b = in[n1], c = in[n2], d = in[n3];
                sx = sx + a.x;
                sy = sy + a.y;
                sz = sz + a.z;
                sx = sx + b.x;
                sy = sy + b.y;
                sz = sz + b.z;
                sx = sx + c.x;
                sy = sy + c.y;
                sz = sz + c.z;
                sx = sx + d.x;
                sy = sy + d.y;
                sz = sz + d.z;
            }
        }
        for (; k < e && ok; ++k) {
            nb = (unsigned)neighbours[k];
            ok = nb < V;
            if (ok) {
                const float4 a = in[nb];
                sx = sx + a.x;
                sy = sy + a.y;
                sz = sz + a.z;
            }
        }
        if (ok) {
            const float n = (float)(e - s);
            const float mx = sx / n, my = sy / n, mz = sz / n;
            const float dx = mx - p.x, dy = my - p.y, dz = mz - p.z;
            const float tx = w * dx, ty = w * dy, tz = w * dz;
            q.x = p.x + tx;
            q.y = p.y + ty;
            q.z = p.z + tz;
        } else {
            *fault = 1u;
        }
    }
    if (out3) {
        float *o = out3 + (size_t)v * 3;
        o[0] = q.x;
        o[1] = q.y;
        o[2] = q.z;
    } else {
        out4[v] = q;
    }
}

hipError_t launch_mesh_smooth(const float *verts, long long n_vertices, const int *offsets, const int *neighbours, const int *edge_faces, long long n_half_edges,
                              int iterations, float lambda, float mu, const SmoothScratch &s, float *verts_out, unsigned *fault, hipStream_t stream)
{
    const unsigned V = (unsigned)n_vertices, H = (unsigned)n_half_edges;
    const unsigned long long n = (unsigned long long)V + 1 > H ? (unsigned long long)V + 1 : H;
    const unsigned vb = (V + ADJ_THREADS - 1) / ADJ_THREADS;
    hipError_t e = hipMemsetAsync(s.header, 0, ADJ_HEADER_BYTES, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(smooth_check_kernel, dim3((unsigned)((n + ADJ_THREADS - 1) / ADJ_THREADS)), dim3(ADJ_THREADS), 0, stream, V, H, offsets, neighbours, s.header, fault);
    if (!vb) return hipGetLastError();
    if (iterations == 0) {
        const unsigned long long words = 3ull * V;
        hipLaunchKernelGGL(smooth_copy_kernel, dim3((unsigned)((words + ADJ_THREADS - 1) / ADJ_THREADS)), dim3(ADJ_THREADS), 0, stream, (const unsigned *)verts, words,
                           (unsigned *)verts_out, s.header);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(smooth_load_kernel, dim3(vb), dim3(ADJ_THREADS), 0, stream, verts, V, H, offsets, edge_faces, s.rows[0], s.header);
    const int steps = 2 * iterations;
    for (int t = 0; t < steps; ++t)
        hipLaunchKernelGGL(smooth_step_kernel, dim3(vb), dim3(ADJ_THREADS), 0, stream, s.rows[t & 1], s.rows[(t + 1) & 1], t == steps - 1 ? verts_out : (float *)nullptr, V,
                           H, offsets, neighbours, (t & 1) ? mu : lambda, s.header, fault);
    return hipGetLastError();
}
