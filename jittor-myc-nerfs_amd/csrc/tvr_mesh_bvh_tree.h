// tvr_mesh_bvh_tree.h — what the files that walk the mesh hierarchy share: the blob's header and the carved tree of tvr_mesh_bvh.hip, the lattice of the grid queries,
// the finite test, the dot product in the header's order, and the check that a blob belongs to the mesh it is walked with.  Read by tvr_mesh_bvh.hip (build, casts,
// closest points, signed distance) and tvr_mesh_winding.hip (node moments, winding numbers).  include/tvr.h tvr_mesh_bvh_* holds the blob's definition.
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
