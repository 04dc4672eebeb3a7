"""Shared by tests/test_mesh_bvh_host.py and tests/test_gpu_mesh_bvh.py: the two references of the ray queries (include/tvr.h tvr_mesh_bvh_cast / _occlusion) and
the fixtures both are run on.

THE DEFINITION (restated from include/tvr.h; `restate` follows it operation by operation in numpy fp32, every operation rounded on its own, brute force over ALL
triangles — no hierarchy, no box test):
  dot / cross  as in tests/mesh_raster_common.py
  pair         q_k = v_k - o;  n_0 = q1 x q2, n_1 = q2 x q0, n_2 = q0 x q1;  det = q0 . n_0;  sg = sign(det);  det == 0 / NaN or a non-finite q: no hit;
               E_k = sg (d . n_k);  inside iff for every k: E_k > 0, or E_k == 0 and owner_k = (index at the edge's start < index at its end) XOR (sg < 0);
               pn = (q1 - q0) x (q2 - q0);  t = (pn . q0) / (d . pn);  a hit needs t finite and t_min < t <= t_max;  cull drops det > 0
  closest      the smallest t, ties to the smaller triangle index; t (+inf), tri (-1), bary b_k = E_k / ((E_0 + E_1) + E_2) (zeros)
  refused      a ray with a non-finite component or d == 0 never hits
  occlusion    c = dirs_k . n; d' = dirs_k if c >= 0 else -dirs_k; w = d' . n; origin p + bias n; any hit over (0, t_max]; out = sum(w visible) / sum(w) in k order, fp32

THE ORACLE (`oracle`) shares none of that formulation: brute-force Moeller-Trumbore in fp64, nearest hit.  Its ambiguity rule is mesh_raster_common's: a ray is
AMBIGUOUS when some triangle that it hits, or misses by less than MARGIN in barycentric terms, has min |b_k| < MARGIN; such rays are left out of mask and index
comparisons, and nothing else is.

Both references run their ray chunks on a fixed pool of 8 threads (numpy releases the GIL inside its loops)."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from mesh_raster_common import MARGIN, _cross, _dot

F32 = np.float32
INTERIOR = (0.21, -0.13, 0.34)
THREADS = 8


def _chunks(fn, n, chunk):
    """fn(i0, i1) over 0 .. n in pieces of `chunk` on the pool; the pieces write disjoint slices."""
    spans = [(i, min(n, i + chunk)) for i in range(0, n, chunk)]
    with ThreadPoolExecutor(THREADS) as pool:
        list(pool.map(lambda s: fn(*s), spans))


def _chunk_for(n_tri, same_origin=False):
    return max(8, int((3e6 if not same_origin else 6e6) // max(n_tri, 1)))


# ---- (b) the definition in numpy fp32 ---------------------------------------------------------------------------------------------------------------------------------------
def _pairs32(v, f, o, d, t_min, t_max, cull, drop=None):
    """One chunk: o [P or 1, 3], d [P, 3] -> (hit [P,F] bool, t [P,F] f32, E 3 x [P,F] f32).  o with one row is shared by every ray (the set-up is then per triangle)."""
    q = [[v[f[:, c], k][None, :] - o[:, k][:, None] for k in range(3)] for c in range(3)]        # q[c][k]: [P or 1, F]
    q0, q1, q2 = q
    n = [_cross(*q1, *q2), _cross(*q2, *q0), _cross(*q0, *q1)]
    det = _dot(*q0, *n[0])
    fin = np.ones(det.shape, bool)
    for c in range(3):
        for k in range(3):
            fin &= np.isfinite(q[c][k])
    ok = fin & ((det > 0) | (det < 0))
    if cull:
        ok &= ~(det > 0)
    if drop is not None:
        ok = ok & ~drop[None, :]
    sg = np.where(det > 0, F32(1), F32(-1)).astype(np.float32)
    neg = det < 0
    own = [(f[:, 1] < f[:, 2])[None, :] != neg, (f[:, 2] < f[:, 0])[None, :] != neg, (f[:, 0] < f[:, 1])[None, :] != neg]
    dx, dy, dz = d[:, 0][:, None], d[:, 1][:, None], d[:, 2][:, None]
    E = [sg * _dot(dx, dy, dz, *n[k]) for k in range(3)]
    inside = ok
    for k in range(3):
        inside = inside & ((E[k] > 0) | ((E[k] == 0) & own[k]))
    a = [q1[k] - q0[k] for k in range(3)]
    b = [q2[k] - q0[k] for k in range(3)]
    pn = _cross(*a, *b)
    pq = _dot(*pn, *q0)
    t = (pq / _dot(dx, dy, dz, *pn)).astype(np.float32)
    hit = inside & np.isfinite(t) & (t > F32(t_min)) & (t <= F32(t_max))
    return hit, t, E


def refused(o, d):
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    o = np.broadcast_to(o.reshape(-1, 3), d.shape)
    return ~(np.isfinite(o).all(1) & np.isfinite(d).all(1)) | (d == 0).all(1)


def restate(verts, faces, origins, dirs, t_min=0.0, t_max=np.inf, cull=False, drop_triangle=None):
    """The definition, fp32, brute force -> dict(t [N] f32, tri [N] i32, bary [N,3] f32, hit [N] bool).  origins [N,3] or one shared [3].  drop_triangle: an index the
    reference pretends is absent (the host test's proof that the comparison can fail)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    shared = len(o) == 1
    N, F = len(d), len(f)
    t_out, tri_out, bary = np.full(N, np.inf, np.float32), np.full(N, -1, np.int32), np.zeros((N, 3), np.float32)
    bad = refused(o, d)
    drop = None
    if drop_triangle is not None:
        drop = np.zeros(F, bool)
        drop[drop_triangle] = True

    def piece(i0, i1):
        with np.errstate(all="ignore"):
            hit, t, E = _pairs32(v, f, o if shared else o[i0:i1], d[i0:i1], t_min, t_max, cull, drop)
            hit = hit & ~bad[i0:i1, None]
            key = (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(F, dtype=np.uint64)[None, :]
            if F32(t_min) < 0:                                       # negative t: order by value, not by bit pattern
                order = np.where(hit, t, np.inf)
                best = order.min(1)
                k = np.where(hit & (t == best[:, None]), np.arange(F)[None, :], F).min(1)
            else:
                k = np.where(hit, key, np.uint64(0xFFFFFFFFFFFFFFFF)).argmin(1)
            rows = np.arange(i1 - i0)
            any_ = hit.any(1)
            kk = np.where(any_, k, 0)
            t_out[i0:i1] = np.where(any_, t[rows, kk], F32(np.inf))
            tri_out[i0:i1] = np.where(any_, kk, -1)
            e = [np.broadcast_to(E[j], hit.shape)[rows, kk] for j in range(3)]
            tot = (e[0] + e[1]) + e[2]
            for j in range(3):
                bary[i0:i1, j] = np.where(any_, e[j] / tot, F32(0))

    if F:
        _chunks(piece, N, _chunk_for(F, shared))
    return dict(t=t_out, tri=tri_out, bary=bary, hit=tri_out >= 0)


# ---- (a) the fp64 oracle ----------------------------------------------------------------------------------------------------------------------------------------------------
def oracle(verts, faces, origins, dirs, t_min=0.0, t_max=np.inf, cull=False):
    """Moeller-Trumbore, fp64 -> dict(t [N] f64 (+inf), tri [N] (-1), hit [N] bool, ambiguous [N] bool)."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    d = np.asarray(dirs, np.float32).astype(np.float64).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(origins, np.float32).astype(np.float64).reshape(-1, 3), d.shape)
    N, F = len(d), len(f)
    t_out, tri_out, amb = np.full(N, np.inf), np.full(N, -1, np.int64), np.zeros(N, bool)
    bad = refused(o, d)
    if F:
        ok = np.isfinite(v[f]).all((1, 2))
        v0 = np.where(ok[:, None], v[f[:, 0]], 0.0)
        e1 = np.where(ok[:, None], v[f[:, 1]], 0.0) - v0
        e2 = np.where(ok[:, None], v[f[:, 2]], 0.0) - v0

    def piece(i0, i1):
        with np.errstate(all="ignore"):
            D = d[i0:i1][:, None, :]
            pv = np.cross(D, e2[None])
            a = (e1[None] * pv).sum(-1)
            tv = o[i0:i1][:, None, :] - v0[None]
            u = (tv * pv).sum(-1) / a
            qv = np.cross(tv, e1[None])
            w = (D * qv).sum(-1) / a
            t = (e2[None] * qv).sum(-1) / a
            b0 = 1.0 - u - w
            valid = ok[None, :] & np.isfinite(a) & (a != 0) & np.isfinite(t) & (t > t_min) & (t <= t_max) & ~bad[i0:i1, None]
            if cull:
                valid &= a > 0
            bmin = np.minimum(np.minimum(b0, u), w)
            babs = np.minimum(np.minimum(np.abs(b0), np.abs(u)), np.abs(w))
            amb[i0:i1] = (valid & (bmin > -MARGIN) & (babs < MARGIN)).any(1)
            th = np.where(valid & (bmin >= 0), t, np.inf)
            k = th.argmin(1)
            rows = np.arange(i1 - i0)
            t_out[i0:i1] = th[rows, k]
            tri_out[i0:i1] = np.where(np.isfinite(th[rows, k]), k, -1)

    if F:
        _chunks(piece, N, max(4, _chunk_for(F) // 3))
    return dict(t=t_out, tri=tri_out, hit=tri_out >= 0, ambiguous=amb)


def compare(res_t, res_tri, orc):
    """A result (t, tri) against the oracle -> dict(mask_diff, tri_diff: over every ray the oracle does not call ambiguous — nothing else is left out; ambiguous: their
    share of all rays; max_rel_t over the rays both hit with the same triangle; rays)."""
    res_t, res_tri = np.asarray(res_t), np.asarray(res_tri).astype(np.int64)
    clear = ~orc["ambiguous"]
    hit_r = res_tri >= 0
    both = clear & orc["hit"] & hit_r & (orc["tri"] == res_tri)
    rel = np.abs(res_t.astype(np.float64)[both] - orc["t"][both]) / np.abs(orc["t"][both])
    return dict(mask_diff=int(((orc["hit"] != hit_r) & clear).sum()), tri_diff=int(((orc["tri"] != res_tri) & clear).sum()),
                ambiguous=float(orc["ambiguous"].mean()) if len(res_tri) else 0.0, max_rel_t=float(rel.max()) if rel.size else 0.0, rays=int(len(res_tri)))


def equal_to_restate(res_t, res_tri, ref, orc):
    """rays, among those the oracle does not call ambiguous, whose tri or t BITS differ from the restatement's"""
    clear = ~orc["ambiguous"]
    t = np.ascontiguousarray(res_t, np.float32)
    return int((((np.asarray(res_tri).astype(np.int64) != ref["tri"]) | (t.view(np.uint32) != ref["t"].view(np.uint32))) & clear).sum())


# ---- occlusion --------------------------------------------------------------------------------------------------------------------------------------------------------------
def occlusion_rays(points, normals, table, bias):
    """The definition's rays, fp32: (origins [M,3], d' [M,K,3], w [M,K])."""
    p, n, tb = (np.asarray(x, np.float32) for x in (points, normals, table))
    c = _dot(tb[None, :, 0], tb[None, :, 1], tb[None, :, 2], n[:, None, 0], n[:, None, 1], n[:, None, 2])
    flip = ~(c >= 0)
    d = np.where(flip[..., None], -tb[None], tb[None]).astype(np.float32)
    w = np.where(flip, -c, c).astype(np.float32)
    return (p + F32(bias) * n).astype(np.float32), d, w


def occlusion_oracle(verts, faces, points, normals, table, bias, t_max=np.inf):
    """fp64 ambient occlusion over the definition's rays -> (ao [M] f64, ambiguous rays per point [M], max w / sum w per point [M])."""
    o, d, w = occlusion_rays(points, normals, table, bias)
    M, K = w.shape
    r = oracle(verts, faces, np.repeat(o, K, 0), d.reshape(-1, 3), 0.0, t_max)
    vis = ~r["hit"].reshape(M, K)
    w64 = w.astype(np.float64)
    return (w64 * vis).sum(1) / w64.sum(1), r["ambiguous"].reshape(M, K).sum(1), w64.max(1) / w64.sum(1)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def rays_interior(n, seed):
    """n rays from the interior point INTERIOR along seeded Gaussian directions (not unit length): (origin [3], dirs [n,3]) fp32"""
    d = np.random.default_rng(seed).standard_normal((n, 3)).astype(np.float32)
    return np.asarray(INTERIOR, np.float32), d


def rays_exterior(n, seed, radius=4.0, ball=1.3):
    """n rays from seeded origins at `radius`, aimed at seeded points of the ball of radius `ball`: about 10 % miss the unit sphere.  (origins [n,3], dirs [n,3]) fp32"""
    g = np.random.default_rng(seed)
    o = g.standard_normal((n, 3))
    o = (radius * o / np.linalg.norm(o, axis=1, keepdims=True)).astype(np.float32)
    p = g.standard_normal((n, 3))
    p = p / np.linalg.norm(p, axis=1, keepdims=True) * (ball * g.random((n, 1)))                  # the radius uniform in 0 .. ball
    return o, (p.astype(np.float32) - o).astype(np.float32)


def edge_midpoint_rays(verts, faces, origin=INTERIOR):
    """one ray per edge of the mesh from `origin` at the edge's midpoint (v_a + v_b) * 0.5, fp32: (origin [3], dirs [E,3], edges [E,2])"""
    f = np.asarray(faces, np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    e = np.unique(e, axis=0)
    v = np.asarray(verts, np.float32)
    o = np.asarray(origin, np.float32)
    mid = ((v[e[:, 0]] + v[e[:, 1]]) * F32(0.5)).astype(np.float32)
    return o, (mid - o[None]).astype(np.float32), e


def tripled(verts, faces):
    """three stacked copies of the faces: identical centroids and boxes, triangle t + k * F coincides with t"""
    return verts, np.concatenate([faces, faces, faces]).astype(np.int32)


def quad_diagonal_rays(n=13):
    """rays from the origin through points of mesh_raster_common.exact_quad's diagonal x = y at z = -4: every product of the definition is exact"""
    s = (np.arange(n, dtype=np.float32) - (n - 1) / 2) * F32(0.375)
    return np.zeros(3, np.float32), np.stack([s, s, np.full(n, -4.0, np.float32)], -1).astype(np.float32)


def fibonacci_sphere(K):
    """the definition of mesh.fibonacci_sphere, restated"""
    k = np.arange(K, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / K
    phi = 2.0 * math.pi * ((k * 0.6180339887498949) % 1.0)
    s = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    return np.stack((s * np.cos(phi), s * np.sin(phi), z), -1).astype(np.float32)


# ---- reading a blob ---------------------------------------------------------------------------------------------------------------------------------------------------------
def read_tree(blob, lay, F):
    """The tree of a blob (uint8 array) by tvr_mesh_bvh_describe's layout -> dict(header words, boxes [2F-1,6] f32, children [F-1,2] i32, leaf_order [F] i32)."""
    blob = np.ascontiguousarray(blob, np.uint8)
    n_nodes, n_int = (2 * F - 1 if F else 0), max(F - 1, 0)
    assert lay["n_nodes"] == n_nodes and lay["n_internal"] == n_int and lay["total"] == len(blob)
    assert lay["box_stride"] == 24 and lay["child_stride"] == 8 and lay["leaf_stride"] == 4
    words = blob[lay["header"]:lay["header"] + 32].view(np.uint32)
    root = blob[lay["header"] + 32:lay["header"] + 56].view(np.float32)
    return dict(F=int(words[1]), bad=int(words[2]), height=int(words[3]), skipped=int(words[4]), root_box=root.copy(),
                boxes=blob[lay["boxes"]:lay["boxes"] + 24 * n_nodes].view(np.float32).reshape(n_nodes, 6).copy(),
                children=blob[lay["children"]:lay["children"] + 8 * n_int].view(np.int32).reshape(n_int, 2).copy(),
                leaf_order=blob[lay["leaf_order"]:lay["leaf_order"] + 4 * F].view(np.int32).copy())


def check_tree(tree, verts, faces):
    """The structural properties of a tree; returns its height.  Every triangle in exactly one leaf, every node reached exactly once from the root, every internal box
    bit-equal to the union of its children's, leaf boxes the exact min / max of their corners (empty for a non-finite triangle), the root box the finite bounding box."""
    v, f = np.asarray(verts, np.float32), np.asarray(faces, np.int64)
    F = len(f)
    assert tree["F"] == F and tree["bad"] == 0
    if F == 0:
        return 0
    assert sorted(tree["leaf_order"].tolist()) == list(range(F))
    corners = v[f[tree["leaf_order"]]]                                # [F,3,3]
    fin = np.isfinite(corners).all((1, 2))
    lo = np.where(fin[:, None], corners.min(1), np.inf).astype(np.float32)
    hi = np.where(fin[:, None], corners.max(1), -np.inf).astype(np.float32)
    boxes, ch = tree["boxes"], tree["children"]
    assert np.array_equal(boxes[F - 1:, :3], lo) and np.array_equal(boxes[F - 1:, 3:], hi)
    assert tree["skipped"] == int((~fin).sum())
    if F > 1:
        assert ch.min() >= 0 and ch.max() < 2 * F - 1
        assert sorted(ch.reshape(-1).tolist()) == list(range(1, 2 * F - 1))       # every node but the root is the child of exactly one node
        un_lo, un_hi = np.minimum(boxes[ch[:, 0], :3], boxes[ch[:, 1], :3]), np.maximum(boxes[ch[:, 0], 3:], boxes[ch[:, 1], 3:])
        assert np.array_equal(boxes[:F - 1, :3].view(np.uint32), un_lo.view(np.uint32)) and np.array_equal(boxes[:F - 1, 3:].view(np.uint32), un_hi.view(np.uint32))
    depth = np.full(2 * F - 1, -1, np.int64)
    depth[0] = 0
    frontier, height, seen = np.array([0]), 0, 1
    while True:
        frontier = frontier[frontier < F - 1]
        if not len(frontier):
            break
        kids = ch[frontier].reshape(-1)
        assert (depth[kids] == -1).all()
        height += 1
        depth[kids] = height
        seen += len(kids)
        frontier = kids
    assert seen == 2 * F - 1 and tree["height"] == height
    if fin.any():
        pts = corners[fin].reshape(-1, 3)
        assert np.array_equal(boxes[0, :3], pts.min(0)) and np.array_equal(boxes[0, 3:], pts.max(0))
        assert np.array_equal(tree["root_box"], boxes[0])
    return height
