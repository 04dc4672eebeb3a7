"""Shared by tests/test_mesh_crossings_host.py and tests/test_gpu_mesh_crossings.py: the two references of the triangle-pair query (include/tvr.h tvr_mesh_crossings_*)
and the fixtures both are run on.

THE DEFINITION (restated from include/tvr.h; `restate` follows it in numpy fp32, brute force over ALL 3F x F (segment, triangle) tests — no hierarchy, no box test):
  segment   side k of a triangle runs between corners (k+1)%3 and (k+2)%3, from the smaller vertex index u to the larger v: o = verts[u], d = verts[v] - verts[u]
  piercing  mesh_bvh_common._pairs32 — the casts' own restatement — on (o, d) with t_min = 0, t_max = 1, cull off; the point (o + t d) per axis, fp32
  sharing   a segment is not tested against a triangle that has a corner at the position of one of the segment's ends (all three coordinates equal)
  pair      a, b cross iff one of six tests pierces: sides 0, 1, 2 of a against b, then sides 0, 1, 2 of b against a; n_pierce counts them; points are the first two
            piercing points in that order (the second repeats the first when n_pierce == 1); a triangle with a non-finite corner crosses nothing
  self      all i < j;  two meshes: all (q, a), a = q's triangle, b = the tree's.  Rows ascend by (first, second).
THE ORACLE (`oracle_tests`) shares none of that formulation: Moeller-Trumbore in fp64 with u > 0, w > 0, u + w < 1, 0 < t <= 1 and the same sharing rule.  A test is
AMBIGUOUS when the decision flips as every bound is moved by +-MARGIN."""
import numpy as np

import mesh_bvh_common as BC
import mesh_nearest_common as NC
import mesh_signed_common as SC
import mesh_winding_common as WC

F32 = np.float32
MARGIN = 1e-4
PUSH = (0.07, -0.05, 0.03)

# fixture: (pairs, piercings) as the issue states them
EXPECTED = {"union": (164, 328), "pushed": (7, 14), "sphere960": (0, 0), "tripled960": (0, 0), "soup_sphere960": (0, 0), "soup_union": (164, 328),
            "soup_pushed": (7, 14), "bowtie": (1, None), "coplanar": (0, 0), "F0": (0, 0), "F1": (0, 0), "F2": (0, 0)}


# ---- segments and sharing -----------------------------------------------------------------------------------------------------------------------------------------------------
def valid_triangles(verts, faces):
    """[F] bool: every index inside the vertices and every corner finite"""
    v, f = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    inside = ((f >= 0) & (f < len(v))).all(1)
    ok = inside.copy()
    ok[inside] = np.isfinite(v[f[inside]]).all((1, 2))
    return ok


def segments(verts, faces):
    """(o [3F,3], e [3F,3]) fp32: the ends of side k of triangle t at row 3t + k, from the smaller vertex index to the larger (rows of invalid triangles are zeros)"""
    v, f = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    f = np.where(valid_triangles(v, f)[:, None], f, 0)
    a, b = f[:, [1, 2, 0]], f[:, [2, 0, 1]]
    u, w = np.minimum(a, b).reshape(-1), np.maximum(a, b).reshape(-1)
    if len(v) == 0:
        return np.zeros((0, 3), F32), np.zeros((0, 3), F32)
    return v[u], v[w]


def _corners(verts, faces):
    v, f = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_triangles(v, f)
    c = v[np.where(ok[:, None], f, 0)] if len(v) else np.zeros((len(f), 3, 3), F32)
    return c, ok


def _not_tested(o, e, corners, seg_ok, tri_ok):
    """[S, T] bool: the sharing rule, and the triangles that cross nothing"""
    with np.errstate(invalid="ignore"):
        share = np.zeros((len(o), len(corners)), bool)
        for c in range(3):
            for end in (o, e):
                share |= (end[:, None, :] == corners[None, :, c, :]).all(-1)
    return share | ~seg_ok[:, None] | ~tri_ok[None, :]


# ---- (b) the definition in numpy fp32 -----------------------------------------------------------------------------------------------------------------------------------------
def restate_tests(verts_s, faces_s, verts_t, faces_t):
    """every side of mesh s against every triangle of mesh t -> dict(hit [3Fs, Ft] bool, t [3Fs, Ft] f32, o, d [3Fs, 3] f32, tested [3Fs, Ft] bool)"""
    vt, ft = np.asarray(verts_t, F32).reshape(-1, 3), np.asarray(faces_t, np.int64).reshape(-1, 3)
    o, e = segments(verts_s, faces_s)
    d = (e - o).astype(F32)
    corners, tri_ok = _corners(vt, ft)
    seg_ok = np.repeat(valid_triangles(verts_s, faces_s), 3) & ~BC.refused(o, d) if len(o) else np.zeros(0, bool)
    S, T = len(o), len(ft)
    hit, t = np.zeros((S, T), bool), np.zeros((S, T), F32)
    tested = np.zeros((S, T), bool)
    fz = np.where(tri_ok[:, None], ft, 0)

    def piece(i0, i1):
        with np.errstate(all="ignore"):
            h, tt, _ = BC._pairs32(vt, fz, o[i0:i1], d[i0:i1], 0.0, 1.0, False)
            tested[i0:i1] = ~_not_tested(o[i0:i1], e[i0:i1], corners, seg_ok[i0:i1], tri_ok)
            hit[i0:i1] = h & tested[i0:i1]
            t[i0:i1] = tt

    if S and T:
        BC._chunks(piece, S, max(8, int(1.5e6 // T)))
    return dict(hit=hit, t=t, o=o, d=d, tested=tested)


def _assemble(A, B, Fa, Fb, self_query):
    """A: the sides of a against b [3Fa, Fb]; B: the sides of b against a [3Fb, Fa] -> dict(pairs [P,2] i32, n_pierce [P] i32, points [P,2,3] f32)"""
    n = A["hit"].reshape(Fa, 3, Fb).sum(1) + B["hit"].reshape(Fb, 3, Fa).sum(1).T if Fa and Fb else np.zeros((Fa, Fb), np.int64)
    if self_query:
        n = np.triu(n, 1)
    pairs = np.argwhere(n > 0)                                       # row-major: ascending by (first, second)
    points = np.zeros((len(pairs), 2, 3), F32)
    for r, (a, b) in enumerate(pairs):
        got = []
        for X, s, tri in [(A, 3 * a + k, b) for k in range(3)] + [(B, 3 * b + k, a) for k in range(3)]:
            if X["hit"][s, tri]:
                got.append((X["o"][s] + X["t"][s, tri] * X["d"][s]).astype(F32))        # fp32 product, fp32 sum, per axis
        points[r, 0], points[r, 1] = got[0], got[1] if len(got) > 1 else got[0]
    return dict(pairs=pairs.astype(np.int32).reshape(-1, 2), n_pierce=n[n > 0].astype(np.int32), points=points)


def restate(verts, faces, verts_q=None, faces_q=None, tests=None):
    """The definition, fp32, brute force.  Without a query mesh: the self query of (verts, faces); with one: pairs (q, a), q from (verts_q, faces_q), a from (verts, faces).
    tests: restate_tests of the mesh against itself, if at hand (self query)."""
    if verts_q is None:
        H = restate_tests(verts, faces, verts, faces) if tests is None else tests
        return _assemble(H, H, len(faces), len(faces), True)
    return _assemble(restate_tests(verts_q, faces_q, verts, faces), restate_tests(verts, faces, verts_q, faces_q), len(faces_q), len(faces), False)


# ---- (a) the fp64 oracle ------------------------------------------------------------------------------------------------------------------------------------------------------
def oracle_tests(verts_s, faces_s, verts_t, faces_t):
    """Moeller-Trumbore, fp64, every side of s against every triangle of t -> dict(hit [3Fs, Ft] bool, ambiguous [3Fs, Ft] bool)"""
    o32, e32 = segments(verts_s, faces_s)
    corners32, tri_ok = _corners(verts_t, faces_t)
    seg_ok = np.repeat(valid_triangles(verts_s, faces_s), 3) & ~(o32 == e32).all(1) if len(o32) else np.zeros(0, bool)
    o, dd, c = o32.astype(np.float64), e32.astype(np.float64) - o32.astype(np.float64), corners32.astype(np.float64)
    S, T = len(o), len(c)
    hit, amb = np.zeros((S, T), bool), np.zeros((S, T), bool)

    def piece(i0, i1):
        with np.errstate(all="ignore"):
            v0, e1, e2 = c[None, :, 0], c[None, :, 1] - c[None, :, 0], c[None, :, 2] - c[None, :, 0]
            D = dd[i0:i1][:, None, :]
            pv = np.cross(D, e2)
            a = (e1 * pv).sum(-1)
            tv = o[i0:i1][:, None, :] - v0
            u = (tv * pv).sum(-1) / a
            qv = np.cross(tv, e1)
            w = (D * qv).sum(-1) / a
            t = (e2 * qv).sum(-1) / a
            tested = ~_not_tested(o32[i0:i1], e32[i0:i1], corners32, seg_ok[i0:i1], tri_ok)

            def decide(m):
                return tested & (u > m) & (w > m) & (u + w < 1 - m) & (t > m) & (t <= 1 - m)

            hit[i0:i1] = decide(0.0)
            amb[i0:i1] = decide(MARGIN) != decide(-MARGIN)

    if S and T:
        BC._chunks(piece, S, max(4, int(5e5 // T)))
    return dict(hit=hit, ambiguous=amb)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------------------------------------------------
def pushed():
    """sphere960 with vertex 17 pushed through the far side: -1.5 v + PUSH (off the antipodal vertex, so that no edge runs through a vertex)"""
    v, f = NC.sphere_mesh("sphere960")
    v = v.copy()
    v[17] = (F32(-1.5) * v[17] + np.asarray(PUSH, F32)).astype(F32)
    return v, f


def bowtie():
    """two triangles that share vertex 0; the side of the second opposite that vertex runs through the first at (0.55, 0.5, 0)"""
    v = np.asarray([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0.5, 0.5, -1], [0.6, 0.5, 1]], F32)
    return v, np.asarray([[0, 1, 2], [0, 3, 4]], np.int32)


def coplanar():
    """two overlapping triangles in the plane z = 0 without a common vertex: every det is exactly 0"""
    v = np.asarray([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0.5, 0.5, 0], [2.5, 0.5, 0], [0.5, 2.5, 0]], F32)
    return v, np.asarray([[0, 1, 2], [3, 4, 5]], np.int32)


def fixtures():
    """{name: (verts, faces)} in the order of EXPECTED"""
    sv, sf = NC.sphere_mesh("sphere960")
    cv, cf = SC.cube()
    out = {"union": WC.union(), "pushed": pushed(), "sphere960": (sv, sf), "tripled960": NC.sphere_mesh("tripled960"), "soup_sphere960": WC.soup(sv, sf),
           "soup_union": WC.soup(*WC.union()), "soup_pushed": WC.soup(*pushed()), "bowtie": bowtie(), "coplanar": coplanar()}
    for n in (0, 1, 2):
        out[f"F{n}"] = (cv, cf[:n].reshape(-1, 3))
    assert list(out) == list(EXPECTED)
    return out


_cache = {}


def reference(name):
    """dict(verts, faces, tests (restate_tests of the mesh against itself), restate) of a fixture, computed once and left unchanged"""
    if name not in _cache:
        v, f = fixtures()[name]
        tests = restate_tests(v, f, v, f)
        _cache[name] = dict(verts=v, faces=f, tests=tests, restate=restate(v, f, tests=tests))
    return _cache[name]


def bits_differ(res, ref):
    """rows of a result (pairs, n_pierce, points: arrays) that are not the reference's, or -1 when the row counts differ"""
    pairs, n_pierce, points = (np.asarray(x) for x in res)
    if pairs.shape != ref["pairs"].shape:
        return -1
    bad = (pairs != ref["pairs"]).any(1) | (n_pierce != ref["n_pierce"])
    bad |= (np.ascontiguousarray(points, F32).view(np.uint32) != ref["points"].view(np.uint32)).reshape(len(pairs), 6).any(1)
    return int(bad.sum())
