// tvr_mesh_raster.hip — a depth-buffer rasteriser for indexed triangle meshes in the camera conventions of rays.py: what puts an exported mesh into the image space of
// the rendered views (mesh.render_mesh, evaluation.evaluation_mesh, reconstruct --render_mesh).  include/tvr.h tvr_mesh_raster holds the definition (camera, homogeneous
// edge functions, plane depth, box); this file is its one implementation.  DESIGN.md §4.15.
//
//   check    per triangle: an index outside 0 .. V-1 raises the header's `bad` word and the fault flag; every later kernel of the call returns at once on `bad`
//   clear    keys[p] = all ones for the H*W pixels, the four counters = 0
//   small    one lane per triangle: set-up, box; a box of at most large_bbox pixels is walked by the lane, a larger one is appended to the queue (one atomic add
//            per wave: ballot, popcount, the lanes' ranks inside the ballot)
//   large    a fixed grid of workgroups draws queue entries (the count the small kernel left is read on the device); 256 lanes stride over a triangle's box, and
//            when there are fewer entries than workgroups every box is shared by grid / entries of them
//   resolve  per pixel: unpack the key, recompute E_k, b_k and the attributes of the winner by the same expressions, write the four outputs, count the hits
//            (and the queue's entries that covered no pixel)
//
// A claim is one 64-bit atomicMin of (depth bits << 32) | triangle on the pixel's key: depth > near >= 0, so the bit pattern orders as the value, and the minimum over a
// set does not depend on the order its members arrive in — nor on which path (small / large) or launch geometry offered them, because every path evaluates a (triangle,
// pixel) pair with the same inlined code (rs_setup / rs_pixel; fp contraction is off, so equal expressions give equal bits).  Before the atomic a lane reads the key with
// a relaxed agent-scope atomic load (a plain load may be served from a stale line of the XCD's L2) and skips the atomic when its own key is not smaller: keys only
// decrease, so a stale (larger) value can cost a redundant atomic, never a wrong skip.  No workgroup waits for another; the kernel boundary is the only ordering.
// Every pixel index is inside 0 .. H*W-1 by construction of the box (clamped in float before the conversion; H, W <= 2^24, checked by the host, so (float)(W - 1) is exact), every queue slot is checked against the capacity F, every
// triangle and vertex index is checked again where it is used: no load or store leaves the caller's buffers whatever faces and the scratch hold.
#include "tvr_kernels.h"

#define RS_THREADS 256
#define RS_LARGE_BLOCKS 2048

typedef unsigned long long u64;

struct RsHeader {
    unsigned bad;          // a face index outside 0 .. V-1 was seen: nothing else of the call is written
    unsigned n_large;      // entries of the queue
};

struct RsCam {
    float r[9], o[3];      // R row-major, o
    int H, W;
    float fx, fy, cx, cy, near_;
    int cull;
    unsigned large_bbox;
};

struct RsArgs {
    const float *verts;    // [V][3]
    const int *faces;      // [F][3]
    unsigned V, F;
    RsCam cam;
    RsHeader *h;
    u64 *keys;             // [H*W]
    int *queue;            // [F]
    int *counts;           // [4]
    unsigned *fault;
};

struct RsOut {
    const float *attr;     // [V][A] or nullptr
    int n_attr;
    float *depth;          // [H*W]
    int *tri;              // [H*W]
    float *bary;           // [H*W][3]
    float *attr_out;       // [H*W][A] or nullptr
};

enum { RS_OK = 0, RS_SKIPPED = 1, RS_NO_PIXEL = 2 };

struct RsTri {
    float n0x, n0y, n0z, n1x, n1y, n1z, n2x, n2y, n2z;      // q1 x q2, q2 x q0, q0 x q1
    float pnx, pny, pnz, pq;                                 // (q1 - q0) x (q2 - q0) and its product with q0
    float sg;
    int v0, v1, v2;
    unsigned own;                                            // bit k: edge k owns a ray that passes exactly through it
    int i0, i1, j0, j1;                                      // the box, inclusive
    int state;
};

__device__ __forceinline__ bool rs_finite(float x) { return fabsf(x) <= 3.4028234664e38f; }       // false for NaN and +-inf
__device__ __forceinline__ float rs_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

__device__ __forceinline__ void rs_to_camera(const RsCam &c, const float *__restrict__ v, float &x, float &y, float &z)
{
    const float d0 = v[0] - c.o[0], d1 = v[1] - c.o[1], d2 = v[2] - c.o[2];
    x = (d0 * c.r[0] + d1 * c.r[3]) + d2 * c.r[6];
    y = (d0 * c.r[1] + d1 * c.r[4]) + d2 * c.r[7];
    z = (d0 * c.r[2] + d1 * c.r[5]) + d2 * c.r[8];
}

// set-up of triangle t (< F, checked by the caller).  BOX: also the cull and the screen box (the small and large kernels); the resolve kernel needs neither.
template <bool BOX>
__device__ __forceinline__ void rs_setup(const RsArgs &a, unsigned t, RsTri &T)
{
    const RsCam &c = a.cam;
    const int *f = a.faces + (size_t)t * 3;
    T.v0 = f[0]; T.v1 = f[1]; T.v2 = f[2];
    T.state = RS_SKIPPED;
    T.i0 = T.j0 = 0; T.i1 = T.j1 = -1;
    if ((unsigned)T.v0 >= a.V || (unsigned)T.v1 >= a.V || (unsigned)T.v2 >= a.V) return;      // (checked again: this kernel indexes verts with them)
    float q0x, q0y, q0z, q1x, q1y, q1z, q2x, q2y, q2z;
    rs_to_camera(c, a.verts + (size_t)T.v0 * 3, q0x, q0y, q0z);
    rs_to_camera(c, a.verts + (size_t)T.v1 * 3, q1x, q1y, q1z);
    rs_to_camera(c, a.verts + (size_t)T.v2 * 3, q2x, q2y, q2z);
    T.n0x = q1y * q2z - q1z * q2y; T.n0y = q1z * q2x - q1x * q2z; T.n0z = q1x * q2y - q1y * q2x;
    T.n1x = q2y * q0z - q2z * q0y; T.n1y = q2z * q0x - q2x * q0z; T.n1z = q2x * q0y - q2y * q0x;
    T.n2x = q0y * q1z - q0z * q1y; T.n2y = q0z * q1x - q0x * q1z; T.n2z = q0x * q1y - q0y * q1x;
    const float det = rs_dot(q0x, q0y, q0z, T.n0x, T.n0y, T.n0z);
    const bool finite = rs_finite(q0x) && rs_finite(q0y) && rs_finite(q0z) && rs_finite(q1x) && rs_finite(q1y) && rs_finite(q1z) && rs_finite(q2x) && rs_finite(q2y) &&
                        rs_finite(q2z);
    if (!finite || !(det > 0.0f || det < 0.0f)) return;
    T.sg = det > 0.0f ? 1.0f : -1.0f;
    const bool neg = det < 0.0f;
    T.own = ((unsigned)((T.v1 < T.v2) != neg)) | ((unsigned)((T.v2 < T.v0) != neg) << 1) | ((unsigned)((T.v0 < T.v1) != neg) << 2);
    const float ax = q1x - q0x, ay = q1y - q0y, az = q1z - q0z, bx = q2x - q0x, by = q2y - q0y, bz = q2z - q0z;
    T.pnx = ay * bz - az * by; T.pny = az * bx - ax * bz; T.pnz = ax * by - ay * bx;
    T.pq = rs_dot(T.pnx, T.pny, T.pnz, q0x, q0y, q0z);
    T.state = RS_OK;
    if (!BOX) return;
    T.state = RS_NO_PIXEL;
    if (c.cull && det > 0.0f) return;                        // the outward side (right-hand rule) faces away from the camera
    const float z0 = -q0z, z1 = -q1z, z2 = -q2z;            // camera depths
    const bool b0 = !(z0 > 0.0f), b1 = !(z1 > 0.0f), b2 = !(z2 > 0.0f);
    if (b0 && b1 && b2) return;                              // wholly behind the camera
    float il = 0.0f, ih = (float)(c.W - 1), jl = 0.0f, jh = (float)(c.H - 1);
    if (!(b0 || b1 || b2)) {
        const float u0 = c.cx - c.fx * (q0x / z0), u1 = c.cx - c.fx * (q1x / z1), u2 = c.cx - c.fx * (q2x / z2);
        const float w0 = c.cy + c.fy * (q0y / z0), w1 = c.cy + c.fy * (q1y / z1), w2 = c.cy + c.fy * (q2y / z2);
        il = fmaxf(ceilf(fminf(fminf(u0, u1), u2) - 1.5f), il);
        ih = fminf(floorf(fmaxf(fmaxf(u0, u1), u2) + 0.5f), ih);
        jl = fmaxf(ceilf(fminf(fminf(w0, w1), w2) - 1.5f), jl);
        jh = fminf(floorf(fmaxf(fmaxf(w0, w1), w2) + 0.5f), jh);
    }                                                        // else: a corner at or behind the camera plane — the whole image (the price of not clipping)
    if (!(il <= ih && jl <= jh)) return;                     // off screen (the comparison is made in float: il / jl may be +inf, ih / jh -inf)
    T.i0 = (int)il; T.i1 = (int)ih; T.j0 = (int)jl; T.j1 = (int)jh;       // all four inside the image now
    T.state = RS_OK;
}

// pixel (i, j) against triangle T: covered (edge functions, owner rule, depth finite and > near)?  E[] and depth are the definition's values.
__device__ __forceinline__ bool rs_pixel(const RsCam &c, const RsTri &T, int i, int j, float E[3], float &depth)
{
    const float dx = -((((float)i + 0.5f) - c.cx) / c.fx), dy = (((float)j + 0.5f) - c.cy) / c.fy, dz = -1.0f;
    E[0] = T.sg * rs_dot(dx, dy, dz, T.n0x, T.n0y, T.n0z);
    E[1] = T.sg * rs_dot(dx, dy, dz, T.n1x, T.n1y, T.n1z);
    E[2] = T.sg * rs_dot(dx, dy, dz, T.n2x, T.n2y, T.n2z);
    const bool in = (E[0] > 0.0f || (E[0] == 0.0f && (T.own & 1u))) && (E[1] > 0.0f || (E[1] == 0.0f && (T.own & 2u))) && (E[2] > 0.0f || (E[2] == 0.0f && (T.own & 4u)));
    const float s = T.pq / rs_dot(dx, dy, dz, T.pnx, T.pny, T.pnz);
    depth = s * sqrtf(rs_dot(dx, dy, dz, dx, dy, dz));
    return in && rs_finite(depth) && depth > c.near_;
}

__device__ __forceinline__ void rs_claim(u64 *keys, unsigned p, float depth, unsigned t)
{
    const u64 key = ((u64)__float_as_uint(depth) << 32) | (u64)t;
    const u64 cur = __hip_atomic_load(keys + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (key < cur) atomicMin(keys + p, key);
}

__global__ __launch_bounds__(RS_THREADS) void rs_check_kernel(const int *__restrict__ faces, unsigned F, unsigned V, RsHeader *__restrict__ h, unsigned *__restrict__ fault)
{
    const unsigned t = blockIdx.x * RS_THREADS + threadIdx.x;
    if (t >= F) return;
    const int *f = faces + (size_t)t * 3;
    if ((unsigned)f[0] >= V || (unsigned)f[1] >= V || (unsigned)f[2] >= V) {        // (a negative index is a huge unsigned one)
        h->bad = 1u;
        *fault = 1u;
    }
}

__global__ __launch_bounds__(RS_THREADS) void rs_clear_kernel(u64 *__restrict__ keys, unsigned n_pixels, int *__restrict__ counts, const RsHeader *__restrict__ h)
{
    if (h->bad) return;
    const unsigned p = blockIdx.x * RS_THREADS + threadIdx.x;
    if (p < 4) counts[p] = 0;
    if (p < n_pixels) keys[p] = ~0ull;
}

__global__ __launch_bounds__(RS_THREADS) void rs_small_kernel(const RsArgs a)
{
    if (a.h->bad) return;
    const unsigned t = blockIdx.x * RS_THREADS + threadIdx.x;
    bool skipped = false, nopix = false, large = false;
    if (t < a.F) {
        RsTri T;
        rs_setup<true>(a, t, T);
        if (T.state == RS_SKIPPED) skipped = true;
        else if (T.state == RS_NO_PIXEL) nopix = true;
        else {
            const unsigned bw = (unsigned)(T.i1 - T.i0 + 1), area = bw * (unsigned)(T.j1 - T.j0 + 1);      // <= H*W < 2^31
            if (area > a.cam.large_bbox) large = true;
            else {
                bool any = false;
                for (int j = T.j0; j <= T.j1; ++j)
                    for (int i = T.i0; i <= T.i1; ++i) {
                        float E[3], depth;
                        if (rs_pixel(a.cam, T, i, j, E, depth)) {
                            any = true;
                            rs_claim(a.keys, (unsigned)j * (unsigned)a.cam.W + (unsigned)i, depth, t);
                        }
                    }
                nopix = !any;
            }
        }
    }
    // the wave's large triangles go to the queue with one add; the three counters likewise (integer sums do not depend on the order they land in)
    const unsigned lane = threadIdx.x & 63u;
    const u64 ml = __ballot(large), ms = __ballot(skipped), mn = __ballot(nopix);
    unsigned base = 0;
    if (lane == 0) {
        if (ml) {
            base = atomicAdd(&a.h->n_large, (unsigned)__popcll(ml));
            atomicAdd(a.counts + 3, (int)__popcll(ml));
        }
        if (ms) atomicAdd(a.counts + 1, (int)__popcll(ms));
        if (mn) atomicAdd(a.counts + 2, (int)__popcll(mn));
    }
    base = (unsigned)__shfl((int)base, 0, 64);
    if (large) {
        const unsigned slot = base + (unsigned)__popcll(ml & ((1ull << lane) - 1ull));
        if (slot < a.F) a.queue[slot] = (int)t;               // (always: a triangle is appended at most once)
    }
}

// The queue's entries over the grid's G workgroups.  n >= G entries: workgroup b takes entries b, b + G, ... whole.  Fewer: every entry is shared by S = G / n
// workgroups, workgroup b striding from part b % S over the box of entry b / S — one giant triangle is the whole grid's work, not one workgroup's.  A workgroup that
// found a covered pixel sets bit 31 of the entry (triangle indices stay below 2^31); the resolve kernel counts the entries no workgroup marked.
__global__ __launch_bounds__(RS_THREADS) void rs_large_kernel(const RsArgs a)
{
    if (a.h->bad) return;
    const unsigned n = a.h->n_large < a.F ? a.h->n_large : a.F;
    if (n == 0) return;
    const unsigned S = n >= gridDim.x ? 1u : gridDim.x / n, part = blockIdx.x % S;
    for (unsigned q = blockIdx.x / S; q < n; q += gridDim.x / S) {               // q, t and T are the same in every lane: the barrier below is reached by all or none
        const unsigned t = (unsigned)__hip_atomic_load(a.queue + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 0x7fffffffu;
        if (t >= a.F) continue;
        RsTri T;
        rs_setup<true>(a, t, T);
        if (T.state != RS_OK) continue;
        const unsigned bw = (unsigned)(T.i1 - T.i0 + 1), area = bw * (unsigned)(T.j1 - T.j0 + 1);
        bool any = false;
        for (unsigned e = part * RS_THREADS + threadIdx.x; e < area; e += S * RS_THREADS) {
            const int j = T.j0 + (int)(e / bw), i = T.i0 + (int)(e % bw);
            float E[3], depth;
            if (rs_pixel(a.cam, T, i, j, E, depth)) {
                any = true;
                rs_claim(a.keys, (unsigned)j * (unsigned)a.cam.W + (unsigned)i, depth, t);
            }
        }
        const int covered = __syncthreads_or(any ? 1 : 0);
        if (threadIdx.x == 0 && covered) atomicOr((unsigned *)a.queue + q, 0x80000000u);
    }
}

__global__ __launch_bounds__(RS_THREADS) void rs_resolve_kernel(const RsArgs a, const RsOut o, unsigned n_pixels)
{
    if (a.h->bad) return;
    const unsigned p = blockIdx.x * RS_THREADS + threadIdx.x;
    bool hit = false;
    if (p < n_pixels) {
        const u64 key = a.keys[p];
        float depth = __uint_as_float(0x7f800000u), b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
        int tri = -1;
        RsTri T;
        T.v0 = T.v1 = T.v2 = 0;
        const unsigned t = (unsigned)(key & 0xffffffffull);
        if (key != ~0ull && t < a.F) {
            rs_setup<false>(a, t, T);
            if (T.state == RS_OK) {
                float E[3], d;
                rs_pixel(a.cam, T, (int)(p % (unsigned)a.cam.W), (int)(p / (unsigned)a.cam.W), E, d);
                const float sum = (E[0] + E[1]) + E[2];
                b0 = E[0] / sum; b1 = E[1] / sum; b2 = E[2] / sum;
                depth = __uint_as_float((unsigned)(key >> 32));
                tri = (int)t;
                hit = true;
            }
        }
        o.depth[p] = depth;
        o.tri[p] = tri;
        o.bary[(size_t)p * 3 + 0] = b0; o.bary[(size_t)p * 3 + 1] = b1; o.bary[(size_t)p * 3 + 2] = b2;
        for (int k = 0; k < o.n_attr; ++k) {
            float v = 0.0f;
            if (hit)
                v = (b0 * o.attr[(size_t)T.v0 * o.n_attr + k] + b1 * o.attr[(size_t)T.v1 * o.n_attr + k]) + b2 * o.attr[(size_t)T.v2 * o.n_attr + k];
            o.attr_out[(size_t)p * o.n_attr + k] = v;
        }
    }
    const int hits = __syncthreads_count(hit ? 1 : 0);
    if (threadIdx.x == 0 && hits) atomicAdd(a.counts + 0, hits);
    // the large triangles no workgroup found a covered pixel for (n is the same in every lane of the grid: so is the trip count)
    const unsigned n = a.h->n_large < a.F ? a.h->n_large : a.F, stride = gridDim.x * RS_THREADS;
    int missed = 0;
    for (unsigned base = 0; base < n; base += stride) {
        const unsigned q = base + p;
        missed += __syncthreads_count(q < n && !((unsigned)a.queue[q] & 0x80000000u) ? 1 : 0);
    }
    if (threadIdx.x == 0 && missed) atomicAdd(a.counts + 2, missed);
}

static size_t rs_align(size_t v) { return (v + 255) / 256 * 256; }

size_t mesh_raster_scratch_bytes(long long n_triangles, long long n_pixels)
{
    return MESH_RASTER_HEADER_BYTES + rs_align((size_t)n_pixels * sizeof(u64)) + rs_align((size_t)n_triangles * sizeof(int));
}

hipError_t launch_mesh_raster(const float *verts, long long n_vertices, const int *faces, long long n_triangles, const tvr_mesh_camera &cam, const float *attr, int n_attr,
                              float *depth, int *tri, float *bary, float *attr_out, void *scratch, int *counts, unsigned *fault, hipStream_t stream)
{
    const unsigned n_pixels = (unsigned)((long long)cam.H * cam.W);
    RsArgs a;
    a.verts = verts; a.faces = faces; a.V = (unsigned)n_vertices; a.F = (unsigned)n_triangles;
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) a.cam.r[r * 3 + k] = cam.c2w[r * 4 + k];
        a.cam.o[r] = cam.c2w[r * 4 + 3];
    }
    a.cam.H = cam.H; a.cam.W = cam.W; a.cam.fx = cam.fx; a.cam.fy = cam.fy; a.cam.cx = cam.cx; a.cam.cy = cam.cy; a.cam.near_ = cam.near_;
    a.cam.cull = cam.cull;
    a.cam.large_bbox = cam.large_bbox > 0 ? (unsigned)cam.large_bbox : (unsigned)TVR_MESH_RASTER_LARGE_BBOX;
    a.h = (RsHeader *)scratch;
    a.keys = (u64 *)((char *)scratch + MESH_RASTER_HEADER_BYTES);
    a.queue = (int *)((char *)a.keys + rs_align((size_t)n_pixels * sizeof(u64)));
    a.counts = counts; a.fault = fault;
    RsOut o;
    o.attr = attr; o.n_attr = n_attr; o.depth = depth; o.tri = tri; o.bary = bary; o.attr_out = attr_out;
    hipError_t e = hipMemsetAsync(scratch, 0, MESH_RASTER_HEADER_BYTES, stream);
    if (e != hipSuccess) return e;
    const unsigned fb = (a.F + RS_THREADS - 1) / RS_THREADS, pb = (n_pixels + RS_THREADS - 1) / RS_THREADS;
    if (fb) hipLaunchKernelGGL(rs_check_kernel, dim3(fb), dim3(RS_THREADS), 0, stream, faces, a.F, a.V, a.h, fault);
    hipLaunchKernelGGL(rs_clear_kernel, dim3(pb), dim3(RS_THREADS), 0, stream, a.keys, n_pixels, counts, a.h);
    if (fb) {
        hipLaunchKernelGGL(rs_small_kernel, dim3(fb), dim3(RS_THREADS), 0, stream, a);
        hipLaunchKernelGGL(rs_large_kernel, dim3(RS_LARGE_BLOCKS), dim3(RS_THREADS), 0, stream, a);       // a fixed grid; the queue's count is read on the device
    }
    hipLaunchKernelGGL(rs_resolve_kernel, dim3(pb), dim3(RS_THREADS), 0, stream, a, o, n_pixels);
    return hipGetLastError();
}
