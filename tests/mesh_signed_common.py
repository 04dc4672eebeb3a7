"""Shared by tests/test_mesh_signed_host.py and tests/test_gpu_mesh_signed.py: the pseudo-normal table and the sign of the signed closest-point query (include/tvr.h
tvr_mesh_pseudonormals_* / tvr_mesh_bvh_signed) restated in numpy, the oracle they are judged by, and the fixtures and point sets both are run on.

THE TABLE (`table`, restated from include/tvr.h operation by operation; dtype float32 gives the definition's own arithmetic, float64 the reference):
  face_n   n = ab x ac, len = sqrt(n . n), n / len per component; (0, 0, 0) and counted degenerate when a vertex is not finite or len is not a finite number > 0
  edge_n   edge k of face f runs from corner (k+1)%3 to (k+2)%3; per undirected edge the sum, from (0, 0, 0), of face_n over its half-edges h = 3 f + k in ascending h,
           written to every one of them; m half-edges: m == 1 open, m > 2 non-manifold, m == 2 leaving the same vertex inconsistent
  vert_n   per vertex the sum, from (0, 0, 0), over its corners in ascending 3 f + k, degenerate faces left out, of atan2(|e1 x e2|, e1 . e2) * face_n
THE SIGN (`signs`): the closest point, its triangle and its region come from mesh_nearest_common.restate — the fp32 definition of the pair arithmetic, brute force over
all triangles; N by region (vert_n of the corner for regions 1, 2, 4; edge_n[tri][2], [1], [0] for 3 (AB), 5 (AC), 6 (BC); face_n for 7), p - c and s = N . (p - c)
in fp64 with c = sum_k bary_k v_k.  mode "face" and "unweighted" are the two shortcuts the fixture must expose: the winning triangle's face normal everywhere, and
vertex normals summed without the angles.
MEASURED on the spiked sphere (tests/test_mesh_signed_host.py asserts the bounds, not the counts): wrong signs of pseudo / face / unweighted on `shell` (4096 points)
0 / 442 / 9, on `near` (1922 points) 0 / 79 / 2; the oracle within 1.4e-14 of 0 or 1 at every point.
THE ORACLE (`winding`) shares none of that: the generalized winding number, fp64, brute force — the sum over all triangles of the solid angle by Van Oosterom &
Strackee's formula, / 4 pi; 1 inside a closed outward-oriented mesh, 0 outside.

VERT_ANGLE_BAR is the bar of the device's vert_n against the fp64 table, as the angle between the two directions in radians: 4 x the largest such angle of the numpy
fp32 table over the three fixtures (the project's convention for DIST_BAR), measured and asserted by tests/test_mesh_signed_host.py."""
import numpy as np

import mesh_nearest_common as NC
import mesh_raster_common as RC

VERT_ANGLE_MEASURED = 1.34e-6  # radians: the thin tetrahedron (1.333e-6); the spiked sphere 1.198e-6, the cube 3.6e-8
VERT_ANGLE_BAR = 5.4e-6        # 4 x 1.34e-6 = 5.36e-6
MARGIN_BAR = 0.05              # the smallest |s| / (|N| dist) the restatement may show on the spiked sphere's two point sets (measured: shell 0.136, near 0.070); the
#                                relative rounding error of an fp32 dot product of three terms is below 1e-6: fp32 cannot flip such a sign
SMALL_MARGIN_BAR = 1e-3        # the same on the cube and the thin tetrahedron (measured: 0.62 / 0.71 and 0.069 / 0.113): still 1000 x the rounding of s
COUNTERS = ("degenerate_faces", "open_edges", "nonmanifold_edges", "inconsistent_edges")


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _cross3(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def table(verts, faces, dtype=np.float32, weighted=True):
    """-> dict(face_n [F,3], edge_n [F,3,3], vert_n [V,3] in `dtype`, counters).  weighted=False: vert_n without the angles (the mutation)."""
    v = np.asarray(verts, np.float32).astype(dtype).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = len(v), len(f)
    with np.errstate(all="ignore"):
        c = v[f] if F else np.zeros((0, 3, 3), dtype)
        n = _cross3(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
        ln = np.sqrt(_dot3(n, n))
        ok = np.isfinite(c).all((1, 2)) & (ln > 0) & np.isfinite(ln)
        face_n = np.where(ok[:, None], n / np.where(ok, ln, 1)[:, None], 0).astype(dtype)
        # half-edges h = 3 f + k, from corner (k+1)%3 to corner (k+2)%3
        h = np.arange(3 * F)
        hf, hk = h // 3, h % 3
        a, b = f[hf, (hk + 1) % 3], f[hf, (hk + 2) % 3]
        key = np.minimum(a, b) * (1 << 32) + np.maximum(a, b)
        order = np.argsort(key, kind="stable")
        edge_n = np.zeros((3 * F, 3), dtype)
        counters = dict(degenerate_faces=int((~ok).sum()), open_edges=0, nonmanifold_edges=0, inconsistent_edges=0)
        starts = np.flatnonzero(np.concatenate([[True], key[order][1:] != key[order][:-1]])) if F else np.zeros(0, np.int64)
        ends = np.concatenate([starts[1:], [3 * F]]) if F else starts
        for s, e in zip(starts, ends):
            run = order[s:e]
            acc = np.zeros(3, dtype)
            for g in run:                                            # ascending h
                acc = acc + face_n[hf[g]]
            edge_n[run] = acc
            m = e - s
            counters["open_edges"] += int(m == 1)
            counters["nonmanifold_edges"] += int(m > 2)
            counters["inconsistent_edges"] += int(m == 2 and a[run[0]] == a[run[1]])
        vert_n = np.zeros((V, 3), dtype)
        for cidx in range(3 * F):                                    # ascending 3 f + k per vertex, because ascending overall
            fi, k = cidx // 3, cidx % 3
            if not ok[fi]:
                continue
            p0, p1, p2 = v[f[fi, k]], v[f[fi, (k + 1) % 3]], v[f[fi, (k + 2) % 3]]
            e1, e2 = (p1 - p0)[None], (p2 - p0)[None]
            cr = _cross3(e1, e2)
            angle = np.arctan2(np.sqrt(_dot3(cr, cr)), _dot3(e1, e2))[0].astype(dtype) if weighted else dtype(1)
            vert_n[f[fi, k]] = vert_n[f[fi, k]] + angle * face_n[fi]
    return dict(face_n=face_n, edge_n=edge_n.reshape(F, 3, 3), vert_n=vert_n, counters=counters)


def direction_angle(a, b):
    """the angle in radians between the directions of the rows of a and b, fp64 (atan2 of |a x b| and a . b: accurate for small angles); rows where both are zero: 0"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ang = np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1))
    return np.where((np.abs(a).sum(1) == 0) & (np.abs(b).sum(1) == 0), 0.0, ang)


# ---- the sign -------------------------------------------------------------------------------------------------------------------------------------------------------------------
EDGE_OF_REGION = {3: 2, 5: 1, 6: 0}
CORNER_OF_REGION = {1: 0, 2: 1, 4: 2}


def region_normals(faces, near, tab, mode="pseudo"):
    """N [P,3] of every answered point by its region (zeros where there is no answer)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    tri, region = near["tri"].astype(np.int64), near["region"]
    N = np.zeros((len(tri), 3), tab["face_n"].dtype)
    ans = tri >= 0
    t = np.where(ans, tri, 0)
    if mode == "face":
        N[ans] = tab["face_n"][t[ans]]
        return N
    m = ans & (region == 7)
    N[m] = tab["face_n"][t[m]]
    for r, k in EDGE_OF_REGION.items():
        m = ans & (region == r)
        N[m] = tab["edge_n"][t[m], k]
    for r, k in CORNER_OF_REGION.items():
        m = ans & (region == r)
        N[m] = tab["vert_n"][f[t[m], k]]
    return N


def signs(verts, faces, points, near, tab, mode="pseudo"):
    """-> dict(s [P] f64 = N . (p - c), margin [P] = |s| / (|N| |p - c|) (inf where the point is on the surface or unanswered), inside [P] bool = s < 0)"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    p = np.asarray(points, np.float32).astype(np.float64)
    t = np.where(near["tri"] >= 0, near["tri"], 0).astype(np.int64)
    c = (near["bary"].astype(np.float64)[:, :, None] * v[f[t]]).sum(1) if len(f) else np.zeros_like(p)
    d = p - c
    N = region_normals(faces, near, tab, mode).astype(np.float64)
    s = (N * d).sum(1)
    den = np.linalg.norm(N, axis=1) * np.linalg.norm(d, axis=1)
    with np.errstate(all="ignore"):
        margin = np.where((near["tri"] >= 0) & (near["dist"] > 0), np.abs(s) / den, np.inf)
    return dict(s=s, margin=margin, inside=s < 0)


def winding(verts, faces, points):
    """generalized winding number [P] f64: sum of 2 atan2(a . (b x c), |a||b||c| + (a . b)|c| + (b . c)|a| + (c . a)|b|) over the triangles, / 4 pi"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    out = np.zeros(len(p))
    for i0 in range(0, len(p), 512):
        q = p[i0:i0 + 512, None, :]
        a, b, c = v[f[:, 0]][None] - q, v[f[:, 1]][None] - q, v[f[:, 2]][None] - q
        la, lb, lc = np.linalg.norm(a, axis=2), np.linalg.norm(b, axis=2), np.linalg.norm(c, axis=2)
        num = (a * np.cross(b, c)).sum(2)
        den = la * lb * lc + (a * b).sum(2) * lc + (b * c).sum(2) * la + (c * a).sum(2) * lb
        out[i0:i0 + 512] = (2.0 * np.arctan2(num, den)).sum(1) / (4.0 * np.pi)
    return out


# ---- fixtures and point sets ----------------------------------------------------------------------------------------------------------------------------------------------------
def _spiked():
    """(verts, faces, shell, near) from ONE generator, numpy.random.default_rng(7), drawn in this order: the vertices' radii, `shell`, `near`"""
    if "spiked" not in _fixture:
        v, f = RC.sphere_fixture("sphere960")[:2]
        g = np.random.default_rng(7)
        r = np.where(g.random(len(v)) < 0.5, 0.55, 1.0) * g.uniform(0.9, 1.1, len(v))
        d = v.astype(np.float64)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        v = (d * r[:, None]).astype(np.float32)
        _fixture["spiked"] = (v, f, shell_points(g, 0.3, 1.4), near_points(v, f, g))
    return _fixture["spiked"]


_fixture = {}


def spiked_sphere():
    """sphere960 with every vertex moved radially to r = (0.55 or 1.0, each with probability 1/2) * U(0.9, 1.1): closed, star-shaped, outward-oriented, full of sharp
    convex and concave edges and vertices"""
    return _spiked()[:2]


def cube():
    """the 12-triangle cube [-0.5, 0.5]^3, outward-oriented"""
    v = np.asarray([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float32)      # index 4 x + 2 y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]                # -x, +x, -y, +y, -z, +z, counter-clockwise from outside
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v, np.asarray(f, np.int32)


def thin_tetrahedron():
    """a unit base triangle in z = 0 and one apex 0.05 above its centroid: three dihedral angles of a few degrees"""
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0.5, np.sqrt(0.75), 0], [0.5, np.sqrt(0.75) / 3, 0.05]], np.float32)
    return v, np.asarray([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)


FIXTURES = {"spiked": spiked_sphere, "cube": cube, "tetra": thin_tetrahedron}


def undirected_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)


def near_points(verts, faces, seed, per_feature=1):
    """per vertex and per edge midpoint `per_feature` points 0.02 .. 0.2 longest-edge lengths away in a uniformly random direction, fp32; seed: a seed or a Generator"""
    v = np.asarray(verts, np.float64)
    e = undirected_edges(faces)
    base = np.repeat(np.concatenate([v, 0.5 * (v[e[:, 0]] + v[e[:, 1]])]), per_feature, 0)
    g = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
    d = g.standard_normal(base.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (base + d * g.uniform(0.02, 0.2, (len(base), 1)) * NC.longest_edge(verts, faces)).astype(np.float32)


def shell_points(seed, lo, hi, n=4096, centre=(0, 0, 0)):
    g = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
    d = g.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (np.asarray(centre) + d * g.uniform(lo, hi, (n, 1))).astype(np.float32)


def point_sets(name, verts, faces):
    """{set name: points} of a fixture: the spiked sphere's `shell` (4096 points at radius 0.3 .. 1.4) and `near` (1922 points by its vertices and edge midpoints);
    the cube's and the tetrahedron's `near` (32 points per vertex and edge midpoint: their vertex and edge regions, inside and outside) and a `shell` about the centroid"""
    if name == "spiked":
        return {"shell": _spiked()[2], "near": _spiked()[3]}
    centre = np.asarray(verts, np.float64).mean(0)
    return {"shell": shell_points(10, 0.01, 1.5, 1024, centre), "near": near_points(verts, faces, 11, 32)}


def measure(name):
    """Everything the host test asserts and the GPU test compares against, of one fixture, computed once: verts, faces, the fp32 and fp64 tables, and per point set the
    points, the nearest restatement, the winding-number oracle and the restated signs (pseudo, face, unweighted)."""
    if name not in _cache:
        v, f = FIXTURES[name]()
        t32, t64, tu = table(v, f, np.float32), table(v, f, np.float64), table(v, f, np.float64, weighted=False)
        sets = {}
        for kind, p in point_sets(name, v, f).items():
            near = NC.restate(v, f, p)
            sets[kind] = dict(points=p, near=near, winding=winding(v, f, p), pseudo=signs(v, f, p, near, t64), face=signs(v, f, p, near, t64, "face"),
                              unweighted=signs(v, f, p, near, tu))
        _cache[name] = dict(verts=v, faces=f, t32=t32, t64=t64, sets=sets)
    return _cache[name]


_cache = {}


# ---- the statistics of mesh.signed_mesh_distance, restated ----------------------------------------------------------------------------------------------------------------
def signed_statistics(sdist, weights, unit=1.0):
    sd, w = np.asarray(sdist, np.float64), np.asarray(weights, np.float64)
    ok = np.isfinite(sd)
    sd, w = sd[ok] / unit, w[ok]
    return dict(signed_mean=float((w * sd).sum() / w.sum()), inside_fraction=float(w[sd < 0].sum() / w.sum()))
