"""Shared by tests/test_mesh_nearest_host.py and tests/test_gpu_mesh_nearest.py: the two references of the closest-point query (include/tvr.h tvr_mesh_bvh_nearest),
the point sets both are run on, and the statistics of mesh.mesh_distance restated in numpy.

THE DEFINITION (restated from include/tvr.h; `restate` follows it operation by operation in numpy fp32, every operation rounded on its own, brute force over ALL
triangles — no hierarchy, no box):
  dot      u . v = (u.x v.x + u.y v.y) + u.z v.z;  cross  u x v = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x)
  pair     a = v0 - p, b = v1 - p, c = v2 - p (a non-finite component: no candidate);  ab = b - a, ac = c - a, bc = c - b;
           d1 = -(ab . a), d2 = -(ac . a), d3 = -(ab . b), d4 = -(ac . b), d5 = -(ab . c), d6 = -(ac . c);
           n = ab x ac;  va = (b x bc) . n, vb = (ac x a) . n, vc = (a x ab) . n
           the first region that holds:
             1 A   d1 <= 0, d2 <= 0                       x = a                                              (1, 0, 0)
             2 B   d3 >= 0, d4 <= d3                      x = b                                              (0, 1, 0)
             3 AB  vc <= 0, d1 >= 0, d3 <= 0              v = d1 / (d1 - d3)           x = a + v ab          (1 - v, v, 0)
             4 C   d6 >= 0, d5 <= d6                      x = c                                              (0, 0, 1)
             5 AC  vb <= 0, d2 >= 0, d6 <= 0              w = d2 / (d2 - d6)           x = a + w ac          (1 - w, 0, w)
             6 BC  va <= 0, d4 - d3 >= 0, d5 - d6 >= 0    w = (d4 - d3) / ((d4 - d3) + (d5 - d6))   x = b + w bc   (0, 1 - w, w)
             7 face  den = (va + vb) + vc, v = vb / den, w = vc / den                  x = (a + v ab) + w ac   ((1 - v) - w, v, w)
           D = x . x; a D that is not finite: no candidate
  result   the smallest D, ties to the smaller triangle index, if D <= max_dist * max_dist (fp32): dist = sqrt(D), tri, bary; else +inf, -1, zeros
  refused  a point with a non-finite component: +inf, -1, zeros

THE ORACLE (`oracle`) shares none of that: fp64, the point projected onto the triangle's plane and tested for lying inside by the signs of three cross products,
else the smallest of the distances to the three edge segments (each a clamped projection).  It measures every triangle whose bounding sphere comes as near to the
point as the nearest centroid does — the others cannot hold the minimum, which is an exact statement in fp64 with the 1e-9 slack it is given.

DIST_BAR is the bar of every fp32-against-fp64 distance comparison, relative to max(distance, longest triangle edge of the mesh): 4 x the largest error of `restate`
against `oracle` over every fixture and point set — measured and asserted by tests/test_mesh_nearest_host.py on the spheres and by tests/test_gpu_mesh_nearest.py on
mc96, whose marching cubes need the device — rounded up to one significant digit.

Both references run their point chunks on a fixed pool of 8 threads (numpy releases the GIL inside its loops)."""
import numpy as np

import mesh_raster_common as RC
from mesh_bvh_common import _chunks

F32 = np.float32
DIST_MEASURED = 1.77e-6    # mc96, `features` (1.7614e-6: points ON the slivers of a marching-cubes mesh; tests/test_gpu_mesh_nearest.py measures it, the marching cubes
#                            need the device); the spheres stay below 2.0e-7 (sphere960 `far`, 1.994e-7)
DIST_BAR = 8e-6            # 4 x 1.77e-6 = 7.08e-6, rounded up to one significant digit
REGIONS = ("vertex A", "vertex B", "edge AB", "vertex C", "edge AC", "edge BC", "face")
MC96_CENTRE = np.asarray([0.03, -0.02, 0.05]) / 0.42        # RC.mc_sphere: the level set's centre after the scaling to radius 1
MC96_VOXEL = (1.0 / 95.0) / 0.42                             # ... and the edge of one of its voxels
MC96_ORIGIN = (-0.5 / 0.42,) * 3                             # ... and the corner of its lattice


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _cross(ax, ay, az, bx, by, bz):
    return ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx


def _weights(r, d1, d2, d3, d4, d5, d6, va, vb, vc):
    """(v, w) of every region and the weights (w0, w1, w2) of region r, fp32, elementwise"""
    one, zero = F32(1), F32(0)
    v3 = d1 / (d1 - d3)
    w5 = d2 / (d2 - d6)
    w6 = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    den = (va + vb) + vc
    v7, w7 = vb / den, vc / den
    w0 = np.select([r == 1, r == 3, r == 5, r == 7], [one, one - v3, one - w5, (one - v7) - w7], zero)
    w1 = np.select([r == 2, r == 3, r == 6, r == 7], [one, v3, one - w6, v7], zero)
    w2 = np.select([r == 4, r == 5, r == 6, r == 7], [one, w5, w6, w7], zero)
    return (v3, w5, w6, v7, w7), (w0.astype(np.float32), w1.astype(np.float32), w2.astype(np.float32))


def _pairs32(c0, c1, c2, p):
    """One chunk: corners c0, c1, c2 [F,3] fp32, points p [P,3] fp32 -> (cand [P,F] bool, D [P,F] f32, region [P,F] int8, the nine d / v values)."""
    a = [c0[:, k][None, :] - p[:, k][:, None] for k in range(3)]
    b = [c1[:, k][None, :] - p[:, k][:, None] for k in range(3)]
    c = [c2[:, k][None, :] - p[:, k][:, None] for k in range(3)]
    fin = np.ones(a[0].shape, bool)
    for q in (a, b, c):
        for k in range(3):
            fin &= np.isfinite(q[k])
    ab = [b[k] - a[k] for k in range(3)]
    ac = [c[k] - a[k] for k in range(3)]
    d1, d2 = -_dot(*ab, *a), -_dot(*ac, *a)
    d3, d4 = -_dot(*ab, *b), -_dot(*ac, *b)
    d5, d6 = -_dot(*ab, *c), -_dot(*ac, *c)
    bc = [c[k] - b[k] for k in range(3)]
    n = _cross(*ab, *ac)
    va, vb, vc = _dot(*_cross(*b, *bc), *n), _dot(*_cross(*ac, *a), *n), _dot(*_cross(*a, *ab), *n)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
             (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    r = np.full(d1.shape, 7, np.int8)
    for i in range(5, -1, -1):                                        # the FIRST region that holds: later ones are overwritten by earlier ones
        r[conds[i]] = i + 1
    dv = (d1, d2, d3, d4, d5, d6, va, vb, vc)
    (v3, w5, w6, v7, w7), _ = _weights(r, *dv)
    x = []
    for k in range(3):
        x.append(np.select([r == 1, r == 2, r == 3, r == 4, r == 5, r == 6], [a[k], b[k], a[k] + v3 * ab[k], c[k], a[k] + w5 * ac[k], b[k] + w6 * bc[k]],
                           (a[k] + v7 * ab[k]) + w7 * ac[k]))
    D = _dot(*x, *x)
    return fin & np.isfinite(D), D, r, dv


def refused(points):
    return ~np.isfinite(np.asarray(points, np.float32).reshape(-1, 3)).all(1)


def restate(verts, faces, points, max_dist=np.inf, drop_triangle=None):
    """The definition, fp32, brute force -> dict(dist [N] f32, tri [N] i32, bary [N,3] f32, D [N] f32 (the winner's squared distance, +inf), region [N] (1 .. 7, 0)).
    drop_triangle: indices the reference pretends are absent (the host test's proof that the comparison can fail)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    N, F = len(p), len(f)
    dist, tri, bary = np.full(N, np.inf, np.float32), np.full(N, -1, np.int32), np.zeros((N, 3), np.float32)
    Dout, region = np.full(N, np.inf, np.float32), np.zeros(N, np.int8)
    bad = refused(p)
    max_sq = F32(max_dist) * F32(max_dist)
    keep = np.ones(F, bool)
    if drop_triangle is not None:
        keep[np.asarray(drop_triangle)] = False
    c0, c1, c2 = (np.ascontiguousarray(v[f[:, k]]) for k in range(3)) if F else (None, None, None)

    def piece(i0, i1):
        with np.errstate(all="ignore"):
            cand, D, r, dv = _pairs32(c0, c1, c2, p[i0:i1])
            cand &= keep[None, :] & ~bad[i0:i1, None]
            Dm = np.where(cand, D, F32(np.inf))
            k = Dm.argmin(1)                                         # the first of the smallest: ties go to the smaller index
            rows = np.arange(i1 - i0)
            ok = cand[rows, k] & (Dm[rows, k] <= max_sq)
            Dk, rk = Dm[rows, k], r[rows, k]
            _, w = _weights(rk, *[x[rows, k] for x in dv])
            dist[i0:i1] = np.where(ok, np.sqrt(Dk), F32(np.inf))
            tri[i0:i1] = np.where(ok, k, -1)
            Dout[i0:i1] = np.where(ok, Dk, F32(np.inf))
            region[i0:i1] = np.where(ok, rk, 0)
            for j in range(3):
                bary[i0:i1, j] = np.where(ok, w[j], F32(0))

    if F and N:
        _chunks(piece, N, max(4, int(1.5e6 // F)))
    return dict(dist=dist, tri=tri, bary=bary, D=Dout, region=region)


# ---- the fp64 oracle ------------------------------------------------------------------------------------------------------------------------------------------------------------
def _segment64(p, a, e, ee):
    """distance^2 from points p [P,1,3] to the segments a + s e, s in [0, 1] ([1,F,3]); ee = e . e"""
    s = np.clip(((p - a) * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0, 1.0)
    q = p - (a + s[..., None] * e)
    return (q * q).sum(-1)


def pair_distance64(points, c0, c1, c2):
    """fp64 distance from points [P,1,3] (or [P,3] with corners [P,3]: one triangle per point) to triangles with corners c0, c1, c2 [1,F,3]: the plane projection if
    it lies inside, else the nearest of the three edge segments."""
    e0, e1, e2 = c1 - c0, c2 - c1, c0 - c2
    n = np.cross(e0, -e2)
    nn = (n * n).sum(-1)
    h = ((points - c0) * n).sum(-1)                                  # (p - c0) . n
    safe = np.where(nn > 0, nn, 1.0)
    q = points - (h / safe)[..., None] * n                          # the foot of the perpendicular
    inside = nn > 0
    for c, e in ((c0, e0), (c1, e1), (c2, e2)):
        inside = inside & ((np.cross(e, q - c) * n).sum(-1) >= 0)
    seg = np.minimum(np.minimum(_segment64(points, c0, e0, (e0 * e0).sum(-1)), _segment64(points, c1, e1, (e1 * e1).sum(-1))),
                     _segment64(points, c2, e2, (e2 * e2).sum(-1)))
    return np.sqrt(np.where(inside, h * h / safe, seg))


def oracle(verts, faces, points):
    """fp64 brute force -> dict(dist [N] f64 (+inf for a refused point or an empty mesh), tri [N] (one triangle at that distance, -1)).  Triangles with a non-finite
    vertex do not count."""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    N = len(p)
    dist, tri = np.full(N, np.inf), np.full(N, -1, np.int64)
    ok = np.isfinite(v[f]).all((1, 2)) if len(f) else np.zeros(0, bool)
    idx = np.flatnonzero(ok)
    bad = refused(p)
    if len(idx) and N:
        c0, c1, c2 = (v[f[idx, k]] for k in range(3))
        mid = (c0 + c1 + c2) / 3.0
        rad = np.sqrt(np.maximum(np.maximum(((c0 - mid) ** 2).sum(-1), ((c1 - mid) ** 2).sum(-1)), ((c2 - mid) ** 2).sum(-1))) * (1.0 + 1e-9) + 1e-300
        mx, my, mz = (np.ascontiguousarray(mid[:, k]) for k in range(3))

        def piece(i0, i1):
            with np.errstate(all="ignore"):
                q = np.where(bad[i0:i1, None], 0.0, p[i0:i1])
                # every triangle is measured whose bounding sphere reaches as near as the nearest centroid (a point of its triangle): the rest cannot hold the minimum
                dc = np.sqrt((q[:, 0, None] - mx[None]) ** 2 + (q[:, 1, None] - my[None]) ** 2 + (q[:, 2, None] - mz[None]) ** 2)
                pi, ti = np.nonzero(dc - rad[None] <= dc.min(1)[:, None] * (1.0 + 1e-9))
                d = pair_distance64(q[pi], c0[ti], c1[ti], c2[ti])
                order = np.lexsort((ti, d, pi))
                first = order[np.concatenate([[True], pi[order][1:] != pi[order][:-1]])]          # per point the smallest distance (then the smallest index)
                dist[i0:i1] = np.where(bad[i0:i1], np.inf, d[first])
                tri[i0:i1] = np.where(bad[i0:i1], -1, idx[ti[first]])

        _chunks(piece, N, max(4, int(1.5e6 // len(idx))))
    return dict(dist=dist, tri=tri)


def longest_edge(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    v = v[np.isfinite(v).all((1, 2))]
    return float(np.sqrt(((v - np.roll(v, 1, 1)) ** 2).sum(-1)).max()) if len(v) else 0.0


def witness(verts, faces, points, res, orc):
    """A result (dict or tuple of dist, tri, bary) against the oracle over every answered point -> dict(dist_err, tri_err, point_err): the largest of
    |dist - dist64|, (fp64 distance to the NAMED triangle) - dist64 and ||p - sum_k bary_k v_k| - dist64|, each / max(dist64, longest edge).  Nothing is exempted."""
    dist, tri, bary = (res["dist"], res["tri"], res["bary"]) if isinstance(res, dict) else res
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    m = np.asarray(tri) >= 0
    if not m.any():
        return dict(dist_err=0.0, tri_err=0.0, point_err=0.0, answered=0)
    t, pm, d64 = np.asarray(tri)[m].astype(np.int64), p[m], orc["dist"][m]
    scale = np.maximum(d64, longest_edge(verts, faces))
    c = v[f[t]]
    named = pair_distance64(pm, c[:, 0], c[:, 1], c[:, 2])
    x = (np.asarray(bary, np.float32).astype(np.float64)[m][:, :, None] * c).sum(1)
    to_x = np.sqrt(((pm - x) ** 2).sum(-1))
    return dict(dist_err=float((np.abs(np.asarray(dist, np.float32).astype(np.float64)[m] - d64) / scale).max()), tri_err=float(((named - d64) / scale).max()),
                point_err=float((np.abs(to_x - d64) / scale).max()), answered=int(m.sum()))


def bits_differ(res, ref):
    """points whose dist, tri or bary BITS differ from the restatement's; res = (dist, tri, bary)"""
    d, t, b = (np.ascontiguousarray(x) for x in res)
    return int(((d.astype(np.float32).view(np.uint32) != ref["dist"].view(np.uint32)) | (t.astype(np.int32) != ref["tri"]) |
                (b.astype(np.float32).view(np.uint32) != ref["bary"].view(np.uint32)).any(1)).sum())


# ---- fixtures and point sets ----------------------------------------------------------------------------------------------------------------------------------------------------
SETS = ("inner", "outer", "far", "verts", "features", "centre")
SHELLS = {"inner": (0.5, 0.98), "outer": (1.02, 1.5), "far": (2.0, 4.0)}


def sphere_mesh(name):
    """sphere960 / sphere6240 / tripled960 -> (verts, faces)"""
    if name == "tripled960":
        v, f = RC.sphere_fixture("sphere960")[:2]
        return v, np.concatenate([f, f, f]).astype(np.int32)
    return RC.sphere_fixture(name)[:2]


def _seed(name, kind):
    return [sum(map(ord, name)), sum(map(ord, kind))]


def vertex_normals(verts, faces):
    """the vertex-averaged (unweighted sum of unit) face normals, fp64, unit length"""
    v, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
    out = np.zeros_like(v)
    for k in range(3):
        np.add.at(out, f[:, k], n)
    return out / np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-300)


def point_set(name, kind, verts, faces, n=4096, centre=(0.0, 0.0, 0.0)):
    """The seeded point set `kind` of the (roughly unit) sphere `name` about `centre`, at most n points, fp32 [.,3]."""
    g = np.random.default_rng(_seed(name, kind))
    v, f = np.asarray(verts, np.float32), np.asarray(faces, np.int64)
    c = np.asarray(centre, np.float64)
    if kind in SHELLS:
        d = g.standard_normal((n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        lo, hi = SHELLS[kind]
        return (c + d * g.uniform(lo, hi, (n, 1))).astype(np.float32)
    if kind == "verts":
        return v if len(v) <= n else v[np.sort(g.choice(len(v), n, replace=False))]
    if kind == "features":
        e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)
        pts = np.concatenate([((v[f[:, 0]] + v[f[:, 1]]) + v[f[:, 2]]) * F32(1 / 3), (v[e[:, 0]] + v[e[:, 1]]) * F32(0.5)]).astype(np.float32)
        return pts if len(pts) <= n else pts[np.sort(g.choice(len(pts), n, replace=False))]
    if kind == "centre":
        return (c + g.uniform(-1e-3, 1e-3, (8, 3)) / np.sqrt(3.0)).astype(np.float32)
    if kind == "displaced":                                          # the vertices moved by +- 0.3 .. 3 voxels along the vertex-averaged face normal
        sel = np.arange(len(v)) if len(v) <= n else np.sort(g.choice(len(v), n, replace=False))
        step = g.uniform(0.3, 3.0, (len(sel), 1)) * g.choice([-1.0, 1.0], (len(sel), 1)) * MC96_VOXEL
        return (v[sel].astype(np.float64) + step * vertex_normals(v, f)[sel]).astype(np.float32)
    raise KeyError(kind)


def fan_smallest(faces, n_vertices):
    """per vertex the smallest index of a triangle that uses it (n_triangles where none does)"""
    f = np.asarray(faces, np.int64)
    out = np.full(n_vertices, len(f), np.int64)
    for k in range(3):
        np.minimum.at(out, f[:, k], np.arange(len(f)))
    return out


# ---- the statistics of mesh.mesh_distance, restated ---------------------------------------------------------------------------------------------------------------------------
def subdivision_weights(n):
    """barycentric weights [n^2, 3] of the sub-triangle centroids in mesh.subdivision_weights' order, from the corners of every sub-triangle"""
    rows = []
    for j in range(n):
        for i in range(n - j):
            rows.append(np.mean([(i, j), (i + 1, j), (i, j + 1)], 0))
    for j in range(n - 1):
        for i in range(n - 1 - j):
            rows.append(np.mean([(i + 1, j), (i + 1, j + 1), (i, j + 1)], 0))
    vw = np.asarray(rows, np.float64) / n
    return np.concatenate([1.0 - vw.sum(1, keepdims=True), vw], 1)


def weighted_quantile(d, w, q):
    """the smallest distance whose cumulative weight, after a sort by distance, reaches q x the total — a plain loop"""
    order = np.argsort(np.asarray(d, np.float64), kind="stable")
    total, run = float(np.asarray(w, np.float64).sum()), 0.0
    for i in order:
        run += float(w[i])
        if run >= q * total:
            return float(d[i])
    return float("nan")


def statistics(dist, weights, unit=1.0):
    """mesh.distance_statistics in numpy fp64 -> dict(max, mean, rms, median, p95, samples, refused)"""
    dist, w = np.asarray(dist, np.float64), np.asarray(weights, np.float64)
    ok = np.isfinite(dist)
    d, w = dist[ok] / unit, w[ok]
    return dict(max=float(d.max()), mean=float((w * d).sum() / w.sum()), rms=float(np.sqrt((w * d * d).sum() / w.sum())), median=weighted_quantile(d, w, 0.5),
                p95=weighted_quantile(d, w, 0.95), samples=int(len(dist)), refused=int((~ok).sum()))
