"""Shared by tests/test_mesh_winding_host.py and tests/test_gpu_mesh_winding.py: the table of node moments and the hierarchical winding-number query (include/tvr.h
tvr_mesh_winding_*) restated in numpy over a GIVEN tree, a numpy tree for the host, and the fixtures both are run on.

THE TABLE (`table`, restated from include/tvr.h operation by operation in float32): per leaf A_t = 0.5 (ab x ac), a_t = sqrt(A_t . A_t), m_t = a_t ((v0 + v1) + v2) / 3;
  per internal node, children before parents, (left) + (right); the row {A, c = m / a, r = |farthest corner of the node's box - c|, a}, r = +inf when a is not a finite
  number > 0 or r is not finite.  A tree is dict(children [F-1,2], leaf_order [F], boxes [2F-1,6]) in the blob's numbering: internal nodes 0 .. F-2 (0 the root), node
  F-1+i the leaf of leaf_order[i] — what mesh_bvh_common.read_tree returns for the device's blob and `median_tree` builds on the host.
THE QUERY (`query`): the accept decision d2 > (beta r)(beta r) in float32 exactly as the header writes it, per node over all points at once with
  reached[child] = reached[parent] & ~accept[parent]; the terms in `terms` precision (float64: the reference the device is held to; float32: the header's own expression
  order, which measures what fp32 terms cost), summed in float64, / 4 pi.  beta = inf accepts nothing: the sum over all triangles, mesh_signed_common.winding's.

WINDING_BAR is the bar of the device's w against these references: 4 x E32, E32 the largest |query with float32 terms - reference| over every fixture's point sets at
beta = inf (against the brute-force oracle) and at beta = 2 and 3 (against the float64 query on the same tree), measured and asserted by tests/test_mesh_winding_host.py.
The factor 4 covers the device's atan2f, which is a few ulp from numpy's.
APPROX_MEASURED: max |float64 query - oracle| over the spiked sphere's two point sets on the DEVICE's tree (tests/test_gpu_mesh_winding.py prints it and asserts twice
the value recorded here)."""
import numpy as np

import mesh_nearest_common as NC
import mesh_signed_common as SC

F32 = np.float32
BETAS = (2.0, 3.0, np.inf)
E32_MEASURED = 6.41e-6          # the spiked sphere's `near` set (6.405e-6 at every beta; `shell` 4.7e-6, the union 6.4e-7, the cube 8.8e-7, the tetrahedron 1.7e-6)
WINDING_BAR = 2.6e-5            # 4 x 6.41e-6 = 2.564e-5
APPROX_MEASURED = {2.0: 4.63e-2, 3.0: 7.42e-3}      # 4.621e-2 (`shell`; `near` 3.14e-2) and 7.419e-3 (`shell`; `near` 7.36e-3) on the MI355X's tree


# ---- a tree on the host -----------------------------------------------------------------------------------------------------------------------------------------------------
def median_tree(verts, faces):
    """a valid tree in the blob's numbering by median splits of the centroids along the longest axis of their extent (ties by triangle index)"""
    v, f = np.asarray(verts, F32), np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(f)
    children, leaf_order = np.zeros((max(F - 1, 0), 2), np.int32), np.zeros(F, np.int32)
    boxes = np.zeros((max(2 * F - 1, 0), 6), F32)
    if F == 0:
        return dict(children=children, leaf_order=leaf_order, boxes=boxes)
    cen = v[f].astype(np.float64).mean(1)
    counter = dict(node=0, leaf=0)

    def build(ids):
        if len(ids) == 1:
            node = F - 1 + counter["leaf"]
            leaf_order[counter["leaf"]] = ids[0]
            counter["leaf"] += 1
            c = v[f[ids[0]]]
            boxes[node] = np.concatenate([c.min(0), c.max(0)])
            return node
        node = counter["node"]
        counter["node"] += 1
        axis = int(np.argmax(cen[ids].max(0) - cen[ids].min(0)))
        ids = ids[np.lexsort((ids, cen[ids, axis]))]
        a, b = build(ids[:len(ids) // 2]), build(ids[len(ids) // 2:])
        children[node] = (a, b)
        boxes[node] = np.concatenate([np.minimum(boxes[a, :3], boxes[b, :3]), np.maximum(boxes[a, 3:], boxes[b, 3:])])
        return node

    build(np.arange(F))
    return dict(children=children, leaf_order=leaf_order, boxes=boxes)


def top_down(tree):
    """the internal nodes, every parent before its children"""
    ch, out, frontier = tree["children"], [], [0] if len(tree["children"]) else []
    while frontier:
        out.extend(frontier)
        frontier = [int(c) for n in frontier for c in ch[n] if c < len(ch)]
    assert len(out) == len(ch) == len(set(out))
    return out


# ---- the table --------------------------------------------------------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def leaf_moments(verts, faces):
    """(A [F,3], m [F,3], a [F]) float32 per triangle; zeros for a triangle with a non-finite coordinate"""
    v, f = np.asarray(verts, F32), np.asarray(faces, np.int64).reshape(-1, 3)
    c = v[f] if len(f) else np.zeros((0, 3, 3), F32)
    with np.errstate(all="ignore"):
        A = F32(0.5) * _cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
        a = np.sqrt(_dot(A, A))
        m = a[:, None] * (((c[:, 0] + c[:, 1]) + c[:, 2]) / F32(3.0))
    fin = np.isfinite(c).all((1, 2))
    return np.where(fin[:, None], A, 0).astype(F32), np.where(fin[:, None], m, 0).astype(F32), np.where(fin, a, 0).astype(F32)


def table(tree, verts, faces):
    """rows [F-1,8] float32 {A, c, r, a} of a tree, in the header's expression order"""
    ch, order, boxes = tree["children"], tree["leaf_order"], tree["boxes"]
    n_int = len(ch)
    lA, lm, la = leaf_moments(verts, faces)
    A, m, a = np.zeros((2 * n_int + 1, 3), F32), np.zeros((2 * n_int + 1, 3), F32), np.zeros(2 * n_int + 1, F32)
    if n_int:
        A[n_int:], m[n_int:], a[n_int:] = lA[order], lm[order], la[order]
    rows = np.zeros((n_int, 8), F32)
    with np.errstate(all="ignore"):
        for n in reversed(top_down(tree)):
            l, r_ = ch[n]
            A[n], m[n], a[n] = A[l] + A[r_], m[l] + m[r_], a[l] + a[r_]
            ok = a[n] > 0 and np.isfinite(a[n])
            c = m[n] / a[n] if ok else np.zeros(3, F32)
            e = np.maximum(c - boxes[n, :3], boxes[n, 3:] - c)
            r = np.sqrt(_dot(e, e))
            if not ok or not np.isfinite(r):
                r = F32(np.inf)
            rows[n, :3], rows[n, 3:6], rows[n, 6], rows[n, 7] = A[n], c, r, a[n]
    return rows


# ---- the query --------------------------------------------------------------------------------------------------------------------------------------------------------------
def _solid_angles(c0, c1, c2, q, dtype):
    """[P, T] solid angles of the triangles at the points, in `dtype`, in the header's expression order"""
    a, b, c = c0[None] - q[:, None], c1[None] - q[:, None], c2[None] - q[:, None]
    la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
    num = _dot(a, _cross(b, c))
    den = (((la * lb) * lc + _dot(a, b) * lc) + _dot(b, c) * la) + _dot(c, a) * lb
    return dtype(2.0) * np.arctan2(num, den)


def solid_angles(verts, faces, points, terms=np.float64):
    """[P, F] float64: the solid angle of every triangle at every point, computed in `terms` precision; 0 for a triangle with a non-finite coordinate.  What `query`
    sums over the leaves it reaches: one matrix serves every beta and every tree of a mesh."""
    v, f = np.asarray(verts, F32), np.asarray(faces, np.int64).reshape(-1, 3)
    q = np.asarray(points, F32).reshape(-1, 3).astype(terms)
    c = (v[f] if len(f) else np.zeros((0, 3, 3), F32)).astype(terms)
    out = np.zeros((len(q), len(f)))
    with np.errstate(all="ignore"):
        fin = np.isfinite(c).all((1, 2))
        for i0 in range(0, len(q), 512):
            out[i0:i0 + 512] = np.where(fin[None], _solid_angles(c[:, 0], c[:, 1], c[:, 2], q[i0:i0 + 512], terms), 0)
    return out


def query(tree, rows, verts, faces, points, beta, terms=np.float64, omega=None):
    """-> dict(w [P] float64, node_visits, dipole_terms, triangle_terms) of the hierarchical sum over `tree` with `rows`; omega: solid_angles(...) in `terms`, if at hand"""
    v, f = np.asarray(verts, F32), np.asarray(faces, np.int64).reshape(-1, 3)
    q32 = np.asarray(points, F32).reshape(-1, 3)
    P, F = len(q32), len(f)
    acc = np.zeros(P)
    counts = dict(node_visits=0, dipole_terms=0, triangle_terms=0)
    if F == 0 or P == 0:
        return dict(w=acc, **counts)
    reached = np.zeros((2 * F - 1, P), bool)
    reached[0] = True
    beta32 = F32(beta)
    with np.errstate(all="ignore"):
        for n in top_down(tree):
            R = rows[n]
            d = R[None, 3:6] - q32                                   # float32: the decision exactly as the kernel makes it
            d2 = _dot(d, d)
            br = beta32 * R[6]
            accept = reached[n] & (d2 > br * br)
            l, r_ = tree["children"][n]
            reached[l] = reached[r_] = reached[n] & ~accept
            counts["node_visits"] += int(reached[n].sum())
            counts["dipole_terms"] += int(accept.sum())
            if accept.any():
                if terms is np.float32:
                    t = _dot(d, R[None, :3]) / (d2 * np.sqrt(d2))
                else:
                    d64 = R[None, 3:6].astype(np.float64) - q32.astype(np.float64)
                    dd = _dot(d64, d64)
                    t = _dot(d64, R[None, :3].astype(np.float64)) / (dd * np.sqrt(dd))
                acc += np.where(accept, t.astype(np.float64), 0.0)
    tri = tree["leaf_order"].astype(np.int64)
    leaf_reached = reached[F - 1:].T & np.isfinite(v[f[tri]]).all((1, 2))[None]      # [P, F] in leaf order
    counts["triangle_terms"] = int(leaf_reached.sum())
    om = solid_angles(verts, faces, points, terms) if omega is None else omega
    acc += np.where(leaf_reached, om[:, tri], 0.0).sum(1)
    return dict(w=acc / (4.0 * np.pi), **counts)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------------------------------------------
UNION_OFFSET = (0.8, 0.0, 0.0)


def union():
    """two sphere960, centres 0.8 apart, as ONE mesh of 1920 triangles: every edge has two faces, so the closedness counters are all 0 and strict=True accepts it, yet
    each sphere's cap lies inside the other"""
    v, f = NC.sphere_mesh("sphere960")
    return np.concatenate([v, (v + F32(UNION_OFFSET)).astype(F32)]), np.concatenate([f, f + len(v)]).astype(np.int32)


def union_points():
    return SC.shell_points(5, 0.0, 1.6, 4096, (0.4, 0, 0))


def union_truth(points):
    """inside either sphere: the union of the two shells' own oracles"""
    v, f = NC.sphere_mesh("sphere960")
    return (SC.winding(v, f, points) > 0.5) | (SC.winding(v + F32(UNION_OFFSET), f, points) > 0.5)


def soup(verts, faces):
    """the mesh unwelded: every triangle owns its three vertices"""
    v, f = np.asarray(verts, F32), np.asarray(faces, np.int64)
    return np.ascontiguousarray(v[f].reshape(-1, 3)), np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3)


def defects():
    """sphere960 with face 100 removed / reversed (the signed test's defects)"""
    v, f = NC.sphere_mesh("sphere960")
    rev = f.copy()
    rev[100] = rev[100][::-1]
    return v, {"removed": np.delete(f, 100, 0), "reversed": rev}


def cases():
    """{name: dict(verts, faces, sets {kind: points}, oracle {kind: w float64}, truth {kind: bool} or None)} of every fixture, computed once"""
    if not _cases:
        for name in SC.FIXTURES:
            m = SC.measure(name)
            _cases[name] = dict(verts=m["verts"], faces=m["faces"], sets={k: s["points"] for k, s in m["sets"].items()},
                                oracle={k: s["winding"] for k, s in m["sets"].items()}, truth={k: s["winding"] > 0.5 for k, s in m["sets"].items()})
        sp = _cases["spiked"]
        uv, uf = union()
        up = union_points()
        _cases["union"] = dict(verts=uv, faces=uf, sets={"shell": up}, oracle={"shell": SC.winding(uv, uf, up)}, truth={"shell": union_truth(up)})
        sv, sf = soup(sp["verts"], sp["faces"])
        _cases["soup"] = dict(verts=sv, faces=sf, sets=sp["sets"], oracle={k: SC.winding(sv, sf, p) for k, p in sp["sets"].items()}, truth=sp["truth"])
        probe = SC.shell_points(21, 0.5, 1.5, 1024)
        tv, tf = NC.sphere_mesh("tripled960")
        _cases["tripled"] = dict(verts=tv, faces=tf, sets={"shell": probe}, oracle={"shell": SC.winding(tv, tf, probe)}, truth=None)
        dv, df = defects()
        for kind, f in df.items():
            _cases[kind] = dict(verts=dv, faces=f, sets={"shell": probe}, oracle={"shell": SC.winding(dv, f, probe)}, truth=None)
        cv, cf = SC.cube()
        few = SC.shell_points(10, 0.01, 1.5, 256)
        for n in (1, 2):
            _cases[f"F{n}"] = dict(verts=cv, faces=cf[:n], sets={"shell": few}, oracle={"shell": SC.winding(cv, cf[:n], few)}, truth=None)
    return _cases


_cases = {}


def margin(case):
    """the smallest |w - 0.5| of the oracle over a case's sets"""
    return min(float(np.abs(w - 0.5).min()) for w in case["oracle"].values())
