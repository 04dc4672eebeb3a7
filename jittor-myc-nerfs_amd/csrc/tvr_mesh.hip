// tvr_mesh.hip — iso-surface extraction (marching cubes) of a dense fp32 volume [nx][ny][nz], z fastest: the mesh behind `--export_mesh 1`
// (reference tensorf-myc/train.py:41-59 -> utils.py:146-207, which calls skimage.measure.marching_cubes on the CPU).  DESIGN.md §4.10.
//
// All work is indexed by GRID POINT p = (i * ny + j) * nz + k.  A point owns the up-to-three edges that leave it along +x, +y, +z and stay inside the
// volume; a point with i < nx-1, j < ny-1, k < nz-1 is also the cell whose minimum corner it is.  A corner is inside iff value >= level.
//
//   count   per point one byte: bits 0..2 = which owned edges straddle the level (x, y, z), bits 3..5 = triangles of the cell (tvr_mc_table.h);
//           per tile of MESH_TILE points the two sums, packed (vertices | triangles << 32)
//   scan    one workgroup walks the tile sums in chunks of MESH_THREADS and turns them into exclusive bases (the totals go to the scratch header and to
//           the caller's counts); then every tile scans its own bytes from its base: vertex_base[p], tri_base[p]
//   emit    per point: its vertices at vertex_base[p] + rank (axis order x, y, z), its cell's triangles at tri_base[p] + table order; a triangle corner on
//           edge e is vertex_base[owner point of e] + rank of e among the owner's straddling edges
//
// The kernel boundary is the only ordering between workgroups: no workgroup waits for another one.  The output order is a function of the volume alone,
// so the mesh is bit-identical from run to run.  Every store of the emit kernel is bounded by the capacities the caller declared.
#include "tvr_kernels.h"
#include "tvr_mc_table.h"

#define MESH_THREADS 256
#define MESH_PER_THREAD 4
#define MESH_TILE (MESH_THREADS * MESH_PER_THREAD)          // points per tile: 1024
#define MESH_HEADER_BYTES 256                               // scratch header: totals (vertices | triangles << 32)

static_assert(TVR_MESH_TILE == MESH_TILE && TVR_MESH_SCAN_CHUNK == MESH_THREADS, "include/tvr.h states the tile constants");

typedef unsigned long long u64;

static inline size_t mesh_align(size_t v) { return (v + 255) / 256 * 256; }

size_t mesh_scratch_bytes(long long points)
{
    return mesh_carve(points, nullptr).total;
}

MeshScratch mesh_carve(long long points, void *scratch)
{
    MeshScratch s;
    const size_t tiles = (size_t)((points + MESH_TILE - 1) / MESH_TILE), padded = tiles * MESH_TILE;
    char *b = (char *)scratch;
    size_t off = 0;
    s.n_tiles = (unsigned)tiles;
    s.totals = (u64 *)(b + off);          off += MESH_HEADER_BYTES;
    s.tile_base = (u64 *)(b + off);       off += mesh_align(tiles * sizeof(u64));
    s.cnt8 = (unsigned char *)(b + off);  off += mesh_align(padded);
    s.vbase = (unsigned *)(b + off);      off += mesh_align(padded * sizeof(unsigned));
    s.tbase = (unsigned *)(b + off);      off += mesh_align(padded * sizeof(unsigned));
    s.total = off;
    return s;
}

struct MeshDims {
    int nx, ny, nz;
    unsigned n;            // points; 3 n < 2^31 (checked by the host)
};

// exclusive scan of x over the 256 threads of the workgroup (4 waves of 64); `total` = the workgroup's sum.  lds: 4 entries.
__device__ __forceinline__ u64 block_exclusive_scan(u64 x, u64 *lds, u64 &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    u64 inc = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 y = __shfl_up(inc, d, 64);
        if (lane >= d) inc += y;
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    u64 woff = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < MESH_THREADS / 64; ++i) {
        const u64 s = lds[i];
        if (i < w) woff += s;
        tot += s;
    }
    __syncthreads();           // lds may be written again
    total = tot;
    return woff + inc - x;
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_count_kernel(const float *__restrict__ vol, MeshDims d, float level, unsigned char *__restrict__ cnt8,
                                                                  u64 *__restrict__ tile_sum)
{
    __shared__ u64 lds[MESH_THREADS / 64];
    const unsigned sy = (unsigned)d.nz, sx = (unsigned)d.ny * (unsigned)d.nz;
    u64 mine = 0;
#pragma unroll
    for (int r = 0; r < MESH_PER_THREAD; ++r) {
        const unsigned p = blockIdx.x * MESH_TILE + r * MESH_THREADS + threadIdx.x;      // < n_tiles * MESH_TILE: inside cnt8's padded extent
        unsigned byte = 0;
        if (p < d.n) {
            const int k = (int)(p % sy), j = (int)((p / sy) % (unsigned)d.ny), i = (int)(p / sx);
            const bool hx = i < d.nx - 1, hy = j < d.ny - 1, hz = k < d.nz - 1;
            const bool in0 = vol[p] >= level;
            const bool in1 = hx && vol[p + sx] >= level, in2 = hy && vol[p + sy] >= level, in4 = hz && vol[p + 1] >= level;
            unsigned mask = 0;
            if (hx && in1 != in0) mask |= 1;
            if (hy && in2 != in0) mask |= 2;
            if (hz && in4 != in0) mask |= 4;
            unsigned tris = 0;
            if (hx && hy && hz) {
                unsigned c = (in0 ? 1u : 0u) | (in1 ? 2u : 0u) | (in2 ? 4u : 0u) | (in4 ? 16u : 0u);
                c |= vol[p + sx + sy] >= level ? 8u : 0u;
                c |= vol[p + sx + 1] >= level ? 32u : 0u;
                c |= vol[p + sy + 1] >= level ? 64u : 0u;
                c |= vol[p + sx + sy + 1] >= level ? 128u : 0u;
                if (c != 0 && c != 255) tris = TVR_MC_TRI_COUNT[c];
            }
            byte = mask | (tris << 3);
            mine += (u64)__popc(mask) | ((u64)tris << 32);
        }
        cnt8[p] = (unsigned char)byte;
    }
    u64 total;
    block_exclusive_scan(mine, lds, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// ONE workgroup: tile sums -> exclusive bases, in place, MESH_THREADS tiles per step with a running carry; totals to the scratch header and the caller
__global__ __launch_bounds__(MESH_THREADS) void mesh_scan_tiles_kernel(u64 *__restrict__ tile_base, unsigned n_tiles, u64 *__restrict__ totals,
                                                                       long long *__restrict__ counts_out)
{
    __shared__ u64 lds[MESH_THREADS / 64];
    u64 carry = 0;
    for (unsigned t0 = 0; t0 < n_tiles; t0 += MESH_THREADS) {
        const unsigned t = t0 + threadIdx.x;
        const u64 x = t < n_tiles ? tile_base[t] : 0;
        u64 total;
        const u64 ex = block_exclusive_scan(x, lds, total);
        if (t < n_tiles) tile_base[t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        totals[0] = carry;
        counts_out[0] = (long long)(carry & 0xffffffffull);
        counts_out[1] = (long long)(carry >> 32);
    }
}

// per tile: exclusive scan of the points' two counts from the tile's base; thread t takes the 4 consecutive points tile * MESH_TILE + 4 t ..
__global__ __launch_bounds__(MESH_THREADS) void mesh_scan_points_kernel(const unsigned char *__restrict__ cnt8, const u64 *__restrict__ tile_base,
                                                                        unsigned *__restrict__ vbase, unsigned *__restrict__ tbase)
{
    __shared__ u64 lds[MESH_THREADS / 64];
    const size_t p0 = (size_t)blockIdx.x * MESH_TILE + MESH_PER_THREAD * threadIdx.x;       // a multiple of 4, inside the padded extent
    const unsigned four = *(const unsigned *)(cnt8 + p0);
    u64 c[MESH_PER_THREAD], mine = 0;
#pragma unroll
    for (int r = 0; r < MESH_PER_THREAD; ++r) {
        const unsigned b = (four >> (8 * r)) & 0xff;
        c[r] = (u64)__popc(b & 7) | ((u64)(b >> 3) << 32);
        mine += c[r];
    }
    u64 total;
    u64 run = tile_base[blockIdx.x] + block_exclusive_scan(mine, lds, total);
    unsigned v[MESH_PER_THREAD], t[MESH_PER_THREAD];
#pragma unroll
    for (int r = 0; r < MESH_PER_THREAD; ++r) {
        v[r] = (unsigned)(run & 0xffffffffull);
        t[r] = (unsigned)(run >> 32);
        run += c[r];
    }
    *(uint4 *)(vbase + p0) = make_uint4(v[0], v[1], v[2], v[3]);
    *(uint4 *)(tbase + p0) = make_uint4(t[0], t[1], t[2], t[3]);
}

struct MeshEmit {
    float origin[3], spacing[3];
    float *verts;          // [cap_v][3]
    int *faces;            // [cap_t][3]
    unsigned cap_v, cap_t; // declared counts = capacities: no store at or beyond them
    int flip;
    unsigned *fault;
};

__global__ __launch_bounds__(MESH_THREADS) void mesh_emit_kernel(const float *__restrict__ vol, MeshDims d, float level, const unsigned char *__restrict__ cnt8,
                                                                 const unsigned *__restrict__ vbase, const unsigned *__restrict__ tbase,
                                                                 const u64 *__restrict__ totals, MeshEmit e)
{
    const unsigned p = blockIdx.x * MESH_THREADS + threadIdx.x;
    const u64 tot = totals[0];
    if ((unsigned)(tot & 0xffffffffull) != e.cap_v || (unsigned)(tot >> 32) != e.cap_t) {        // the declared counts are not the counted ones: nothing is written
        if (p == 0) *e.fault = 1u;
        return;
    }
    if (p >= d.n) return;
    const unsigned byte = cnt8[p];
    if (byte == 0) return;
    const unsigned sy = (unsigned)d.nz, sx = (unsigned)d.ny * (unsigned)d.nz;
    const int k = (int)(p % sy), j = (int)((p / sy) % (unsigned)d.ny), i = (int)(p / sx);
    // (the bits are re-limited to the edges that exist, so that no load leaves the volume whatever the scratch holds)
    const unsigned mask = byte & ((i < d.nx - 1 ? 1u : 0u) | (j < d.ny - 1 ? 2u : 0u) | (k < d.nz - 1 ? 4u : 0u)), tris = byte >> 3;
    bool bad = false;
    if (mask) {
        const float a = vol[p];
        const unsigned step[3] = {sx, sy, 1u};
        const float base[3] = {(float)i, (float)j, (float)k};
        unsigned idx = vbase[p];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (!(mask & (1u << ax))) continue;
            const float b = vol[p + step[ax]];
            const float t = (level - a) / (b - a);
            float c[3] = {base[0], base[1], base[2]};
            c[ax] = c[ax] + t;
            if (idx < e.cap_v) {
                float *o = e.verts + (size_t)idx * 3;
                o[0] = e.origin[0] + c[0] * e.spacing[0];
                o[1] = e.origin[1] + c[1] * e.spacing[1];
                o[2] = e.origin[2] + c[2] * e.spacing[2];
            } else {
                bad = true;
            }
            ++idx;
        }
    }
    if (tris && i < d.nx - 1 && j < d.ny - 1 && k < d.nz - 1) {
        unsigned c = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) c |= vol[p + (q & 1) * sx + ((q >> 1) & 1) * sy + ((q >> 2) & 1)] >= level ? (1u << q) : 0u;
        unsigned n = TVR_MC_TRI_COUNT[c];
        n = n < tris ? n : tris;                              // both are <= TVR_MC_MAX_TRIS
        const unsigned t0 = tbase[p];
        for (unsigned m = 0; m < n; ++m) {
            int vi[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const unsigned ed = TVR_MC_TRI[c][3 * m + q];           // 0..11 for m < TVR_MC_TRI_COUNT[c]
                const unsigned lo = TVR_MC_EDGE_LO[ed], ax = ed >> 2;
                const unsigned owner = p + (lo & 1) * sx + ((lo >> 1) & 1) * sy + ((lo >> 2) & 1);      // a corner of this cell: inside the volume
                const unsigned om = cnt8[owner] & 7;
                vi[q] = (int)(vbase[owner] + __popc(om & ((1u << ax) - 1u)));
            }
            if (t0 + m < e.cap_t) {
                int *o = e.faces + (size_t)(t0 + m) * 3;
                o[0] = e.flip ? vi[2] : vi[0];
                o[1] = vi[1];
                o[2] = e.flip ? vi[0] : vi[2];
            } else {
                bad = true;
            }
        }
    }
    if (bad) *e.fault = 1u;
}

hipError_t launch_mesh_count(const float *vol, const int dims[3], float level, const MeshScratch &s, long long *counts_dev, hipStream_t stream)
{
    const MeshDims d = {dims[0], dims[1], dims[2], (unsigned)((long long)dims[0] * dims[1] * dims[2])};
    hipLaunchKernelGGL(mesh_count_kernel, dim3(s.n_tiles), dim3(MESH_THREADS), 0, stream, vol, d, level, s.cnt8, s.tile_base);
    return launch_mesh_scan(s, counts_dev, stream);
}

hipError_t launch_mesh_scan(const MeshScratch &s, long long *counts_dev, hipStream_t stream)
{
    hipLaunchKernelGGL(mesh_scan_tiles_kernel, dim3(1), dim3(MESH_THREADS), 0, stream, s.tile_base, s.n_tiles, s.totals, counts_dev);
    if (s.n_tiles)              // (a volume has tiles; the component filter of an empty mesh has none)
        hipLaunchKernelGGL(mesh_scan_points_kernel, dim3(s.n_tiles), dim3(MESH_THREADS), 0, stream, s.cnt8, s.tile_base, s.vbase, s.tbase);
    return hipGetLastError();
}

hipError_t launch_mesh_emit(const float *vol, const int dims[3], float level, const float origin[3], const float spacing[3], const MeshScratch &s, float *verts,
                            long long n_vertices, int *faces, long long n_triangles, int flip, unsigned *fault, hipStream_t stream)
{
    const MeshDims d = {dims[0], dims[1], dims[2], (unsigned)((long long)dims[0] * dims[1] * dims[2])};
    MeshEmit e;
    for (int a = 0; a < 3; ++a) {
        e.origin[a] = origin[a];
        e.spacing[a] = spacing[a];
    }
    e.verts = verts;
    e.faces = faces;
    e.cap_v = (unsigned)n_vertices;
    e.cap_t = (unsigned)n_triangles;
    e.flip = flip ? 1 : 0;
    e.fault = fault;
    hipLaunchKernelGGL(mesh_emit_kernel, dim3((d.n + MESH_THREADS - 1) / MESH_THREADS), dim3(MESH_THREADS), 0, stream, vol, d, level, s.cnt8, s.vbase, s.tbase, s.totals, e);
    return hipGetLastError();
}
