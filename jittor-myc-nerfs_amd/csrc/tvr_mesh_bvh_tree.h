// tvr_mesh_bvh_tree.h — what the files that walk the mesh hierarchy share: the blob's header and the carved tree of tvr_mesh_bvh.hip, the lattice of the grid queries,
// the finite test, the dot product in the header's order, the check that a blob belongs to the mesh it is walked with, the (ray, triangle) pair of the casts and a
// wave's 64-bit sum.  Read by tvr_mesh_bvh.hip (build, casts, closest points, signed distance), tvr_mesh_winding.hip (node moments, winding numbers) and
// tvr_mesh_crossings.hip (triangle pairs: the (ray, triangle) pair applied to triangle sides).  include/tvr.h tvr_mesh_bvh_* holds the blob's definition.
#pragma once
#include "tvr_kernels.h"

#define BV_THREADS 256
#define BV_CAST_THREADS 128
#define BV_STACK 64
#define BV_PASSES 62

typedef unsigned long long u64;

struct BvHeader {                       // MESH_BVH_HEADER_BYTES at the blob's start
    unsigned magic, F, bad, height, skipped, reserved[3];
    float lo[3], hi[3];                 // the root's box
};
#define BV_MAGIC 0x48564254u

struct BvTree {
    BvHeader *h;
    float *box;                         // [2F-1][6]: internal nodes 0 .. F-2, then the leaves in key order
    int *child;                         // [F-1][2]
    int *leaf_tri;                      // [F]
    unsigned F, V;
    const float *verts;
    const int *faces;
};

struct BvLattice {                                   // points == nullptr: point i = (ix * ny + iy) * nz + iz sits at origin + index * spacing
    float ox, oy, oz, sx, sy, sz;
    unsigned ny, nz;
};

static size_t bv_align(size_t v) { return (v + 255) / 256 * 256; }

__device__ __forceinline__ bool bv_finite(float x) { return fabsf(x) <= 3.4028234664e38f; }
__device__ __forceinline__ float bv_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

static BvTree bv_tree(const float *verts, long long V, const int *faces, long long F, void *bvh)
{
    MeshBvhCarve L;
    mesh_bvh_bytes(F, &L);
    BvTree T;
    T.h = (BvHeader *)bvh;
    T.box = (float *)((char *)bvh + L.box);
    T.child = (int *)((char *)bvh + L.child);
    T.leaf_tri = (int *)((char *)bvh + L.leaf_tri);
    T.F = (unsigned)F; T.V = (unsigned)V; T.verts = verts; T.faces = faces;
    return T;
}

__device__ __forceinline__ bool bv_blob_ok(const BvTree &T, unsigned *__restrict__ fault)
{
    const bool ok = T.h->magic == BV_MAGIC && T.h->F == T.F && T.h->bad == 0u;
    if (!ok && threadIdx.x == 0) *fault = 1u;
    return ok;
}

#define BV_PAD 3.0517578125e-05f        // 2^-15: the slab test's relative widening

struct BvRay {
    float ox, oy, oz, dx, dy, dz, ix, iy, iz;       // origin, direction, 1 / direction
    float t_min;
    int cull;
};

// (ray, triangle t): the definition of include/tvr.h, i.e. tvr_mesh_raster.hip's rs_setup / rs_pixel with R = identity, o = the ray's origin, dir = the ray's direction
__device__ __forceinline__ bool bv_triangle(const BvTree &T, unsigned t, const BvRay &r, float t_max, float E[3], float &tt, unsigned *__restrict__ fault)
{
    const int *f = T.faces + (size_t)t * 3;
    const int v0 = f[0], v1 = f[1], v2 = f[2];
    if ((unsigned)v0 >= T.V || (unsigned)v1 >= T.V || (unsigned)v2 >= T.V) {
        *fault = 1u;
        return false;
    }
    const float *p0 = T.verts + (size_t)v0 * 3, *p1 = T.verts + (size_t)v1 * 3, *p2 = T.verts + (size_t)v2 * 3;
    const float q0x = p0[0] - r.ox, q0y = p0[1] - r.oy, q0z = p0[2] - r.oz;
    const float q1x = p1[0] - r.ox, q1y = p1[1] - r.oy, q1z = p1[2] - r.oz;
    const float q2x = p2[0] - r.ox, q2y = p2[1] - r.oy, q2z = p2[2] - r.oz;
    const float n0x = q1y * q2z - q1z * q2y, n0y = q1z * q2x - q1x * q2z, n0z = q1x * q2y - q1y * q2x;
    const float n1x = q2y * q0z - q2z * q0y, n1y = q2z * q0x - q2x * q0z, n1z = q2x * q0y - q2y * q0x;
    const float n2x = q0y * q1z - q0z * q1y, n2y = q0z * q1x - q0x * q1z, n2z = q0x * q1y - q0y * q1x;
    const float det = bv_dot(q0x, q0y, q0z, n0x, n0y, n0z);
    const bool finite = bv_finite(q0x) && bv_finite(q0y) && bv_finite(q0z) && bv_finite(q1x) && bv_finite(q1y) && bv_finite(q1z) && bv_finite(q2x) && bv_finite(q2y) &&
                        bv_finite(q2z);
    if (!finite || !(det > 0.0f || det < 0.0f)) return false;
    if (r.cull && det > 0.0f) return false;
    const float sg = det > 0.0f ? 1.0f : -1.0f;
    const bool neg = det < 0.0f;
    const bool own0 = (v1 < v2) != neg, own1 = (v2 < v0) != neg, own2 = (v0 < v1) != neg;
    E[0] = sg * bv_dot(r.dx, r.dy, r.dz, n0x, n0y, n0z);
    E[1] = sg * bv_dot(r.dx, r.dy, r.dz, n1x, n1y, n1z);
    E[2] = sg * bv_dot(r.dx, r.dy, r.dz, n2x, n2y, n2z);
    const bool in = (E[0] > 0.0f || (E[0] == 0.0f && own0)) && (E[1] > 0.0f || (E[1] == 0.0f && own1)) && (E[2] > 0.0f || (E[2] == 0.0f && own2));
    if (!in) return false;
    const float ax = q1x - q0x, ay = q1y - q0y, az = q1z - q0z, bx = q2x - q0x, by = q2y - q0y, bz = q2z - q0z;
    const float pnx = ay * bz - az * by, pny = az * bx - ax * bz, pnz = ax * by - ay * bx;
    const float pq = bv_dot(pnx, pny, pnz, q0x, q0y, q0z);
    tt = pq / bv_dot(r.dx, r.dy, r.dz, pnx, pny, pnz);
    return bv_finite(tt) && tt > r.t_min && tt <= t_max;
}

// false for a ray that never hits: a non-finite component, or d == 0
__device__ __forceinline__ bool bv_ray(BvRay &r, float ox, float oy, float oz, float dx, float dy, float dz, float t_min, int cull)
{
    r.ox = ox; r.oy = oy; r.oz = oz; r.dx = dx; r.dy = dy; r.dz = dz; r.t_min = t_min; r.cull = cull;
    r.ix = 1.0f / dx; r.iy = 1.0f / dy; r.iz = 1.0f / dz;
    const bool fin = bv_finite(ox) && bv_finite(oy) && bv_finite(oz) && bv_finite(dx) && bv_finite(dy) && bv_finite(dz);
    return fin && !(dx == 0.0f && dy == 0.0f && dz == 0.0f);
}

// the wave's sum of a 64-bit counter, in every lane
__device__ __forceinline__ u64 bv_wave_sum(u64 x)
{
    unsigned lo = (unsigned)x, hi = (unsigned)(x >> 32);
    for (int o = 32; o; o >>= 1) {
        const unsigned l2 = (unsigned)__shfl_xor((int)lo, o, 64), h2 = (unsigned)__shfl_xor((int)hi, o, 64);
        const u64 sum = (((u64)hi << 32) | lo) + (((u64)h2 << 32) | l2);
        lo = (unsigned)sum; hi = (unsigned)(sum >> 32);
    }
    return ((u64)hi << 32) | lo;
}
