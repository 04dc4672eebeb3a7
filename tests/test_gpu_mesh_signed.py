"""GPU: the pseudo-normal table and the signed closest-point query (csrc/tvr_mesh_pseudo.hip, csrc/tvr_mesh_bvh.hip bv_signed_kernel; include/tvr.h
tvr_mesh_pseudonormals_* / tvr_mesh_bvh_signed; mesh.build_pseudonormals / signed_distance / contains / signed_distance_grid / signed_mesh_distance, reconstruct
--mesh_compare_signed).  face_n and edge_n bit for bit against the numpy fp32 restatement of tests/mesh_signed_common.py, vert_n as a direction against fp64 within
VERT_ANGLE_BAR, the closedness counters on four defective meshes; |sdist|, tri and bary bit for bit against closest_points and its restatement, feature against the
restatement's region; the SIGN against a winding-number oracle at every point of every set — none excluded, none undecided (tests/test_mesh_signed_host.py shows why
that is possible: the restated sign's margin is far above fp32 rounding, and the same fixture catches face normals and unweighted vertex normals); a reversed mesh,
vertices, refusals, empty inputs, order and chunking, the lattice against the point form, a marching-cubes round trip within a derived bound, and the command line.
The references are computed once per process and shared (mesh_signed_common.measure)."""
import json

import numpy as np
import pytest
import torch

import mesh_nearest_common as NC
import mesh_signed_common as SC

pytestmark = pytest.mark.gpu

_cache = {}


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def build(v, f):
    from jittor_myc_nerfs_amd import mesh
    return mesh.build_bvh(_dev(v), _dev(f, np.int32))


def built(name):
    """(verts, faces, MeshBVH) of a fixture of mesh_signed_common or a sphere of mesh_nearest_common, built once"""
    if name not in _cache:
        v, f = SC.FIXTURES[name]() if name in SC.FIXTURES else NC.sphere_mesh(name)
        _cache[name] = (v, f, build(v, f))
    return _cache[name]


def device_table(bvh, stats=None):
    """the device's table as numpy: dict(face_n, edge_n, vert_n, header [8] uint32, blob)"""
    from jittor_myc_nerfs_amd import mesh
    t = mesh.build_pseudonormals(bvh, stats=stats)
    lay, raw = mesh.pseudonormals_layout(bvh.n_vertices, bvh.n_triangles), _np(t.blob)
    F, V = bvh.n_triangles, bvh.n_vertices
    assert len(raw) == lay["total"]
    part = lambda off, n: raw[off:off + 4 * n].view(np.float32)
    return dict(face_n=part(lay["face_n"], 3 * F).reshape(F, 3), edge_n=part(lay["edge_n"], 9 * F).reshape(F, 3, 3), vert_n=part(lay["vert_n"], 3 * V).reshape(V, 3),
                header=raw[:32].view(np.uint32), blob=raw)


def signed(bvh, p, **kw):
    from jittor_myc_nerfs_amd import mesh
    return tuple(_np(x) for x in mesh.signed_distance(bvh, _dev(p), **kw))


def nearest(bvh, p, **kw):
    from jittor_myc_nerfs_amd import mesh
    return tuple(_np(x) for x in mesh.closest_points(bvh, _dev(p), **kw))


def same_as_nearest(sres, nres):
    """|sdist|, tri and bary of signed_distance against dist, tri, bary of closest_points: the number of points whose bits differ"""
    sd, t, b, _ = sres
    d, t2, b2 = nres
    return int(((_bits(np.abs(sd)) != _bits(d)) | (t != t2) | (_bits(b) != _bits(b2)).any(1)).sum())


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(SC.FIXTURES))
def test_table_equals_the_restatement_and_two_builds_give_the_same_bytes(name):
    from jittor_myc_nerfs_amd import mesh
    v, f, bvh = built(name)
    m = SC.measure(name)
    st = {}
    t = device_table(bvh, stats=st)
    angle = SC.direction_angle(t["vert_n"], m["t64"]["vert_n"]).max()
    face_diff = int((_bits(t["face_n"]) != _bits(m["t32"]["face_n"])).any(1).sum())
    edge_diff = int((_bits(t["edge_n"]).reshape(-1, 3) != _bits(m["t32"]["edge_n"]).reshape(-1, 3)).any(1).sum())
    print(f"    {name}: face_n rows differing {face_diff} of {len(f)}, edge_n rows differing {edge_diff} of {3 * len(f)}; vert_n against fp64 {angle:.4g} rad "
          f"(restatement {SC.direction_angle(m['t32']['vert_n'], m['t64']['vert_n']).max():.4g}, bar {SC.VERT_ANGLE_BAR:g}); counters {st}")
    assert face_diff == 0 and edge_diff == 0                         # bit for bit, +0.0 included
    assert angle <= SC.VERT_ANGLE_BAR
    assert (np.abs(t["vert_n"]).sum(1) > 0).all()                    # every vertex of these fixtures has a fan
    assert st["closed"] and all(st[k] == 0 for k in SC.COUNTERS) and st["table_bytes"] == len(t["blob"])
    assert t["header"].tolist() == [0x4e505654, len(f), len(v), 0, 0, 0, 0, 0]
    assert mesh.build_pseudonormals(bvh) is bvh.pseudonormals        # built once and kept
    again = device_table(build(v, f))
    assert np.array_equal(again["blob"], t["blob"])                  # padding included


def _defects():
    v, f = NC.sphere_mesh("sphere960")
    rev, deg = f.copy(), f.copy()
    rev[100] = rev[100][::-1]
    deg[100, 2] = deg[100, 0]
    return v, {"removed": np.delete(f, 100, 0), "reversed": rev, "tripled": NC.sphere_mesh("tripled960")[1], "repeated": deg}


@pytest.mark.parametrize("kind,counter,count", [("removed", "open_edges", 3), ("reversed", "inconsistent_edges", 3), ("tripled", "nonmanifold_edges", 1440),
                                                ("repeated", "degenerate_faces", 1)])
def test_counters_strictness_and_answers_on_meshes_that_are_not_closed(kind, counter, count):
    from jittor_myc_nerfs_amd import _lib as L, mesh
    v, faces = _defects()
    f = faces[kind]
    bvh = build(v, f)
    st = {}
    t = device_table(bvh, stats=st)
    ref = SC.table(v, f)
    print(f"    sphere960 {kind}: {({k: st[k] for k in SC.COUNTERS})}")
    assert st[counter] == count and not st["closed"] and {k: st[k] for k in SC.COUNTERS} == ref["counters"]
    if kind != "repeated":
        assert sum(st[k] for k in SC.COUNTERS) == count              # and no other counter moved
    assert np.array_equal(_bits(t["face_n"]), _bits(ref["face_n"])) and np.array_equal(_bits(t["edge_n"]), _bits(ref["edge_n"]))
    p = SC.shell_points(21, 0.5, 1.5, 1024)
    with pytest.raises(L.TvrError, match=f"{counter} = {count}"):
        mesh.signed_distance(bvh, _dev(p))
    with pytest.raises(L.TvrError, match="not closed"):
        mesh.contains(bvh, _dev(p))
    with pytest.raises(L.TvrError, match="not closed"):
        mesh.signed_distance_grid(bvh, (4, 4, 4))
    res = signed(bvh, p, strict=False)                               # answers anyway; only the signs are not promised
    assert same_as_nearest(res, nearest(bvh, p)) == 0 and (res[1] >= 0).all() and np.isfinite(res[0]).all()


# ---- the query --------------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(SC.FIXTURES))
def test_distance_triangle_weights_and_feature_on_every_point(name):
    v, f, bvh = built(name)
    for kind, s in SC.measure(name)["sets"].items():
        st = {}
        res = signed(bvh, s["points"], stats=st)
        differ, restated = same_as_nearest(res, nearest(bvh, s["points"])), NC.bits_differ((np.abs(res[0]), res[1], res[2]), s["near"])
        agree = res[1] == s["near"]["tri"]
        feature_diff = int((res[3][agree] != s["near"]["region"][agree] - 1).sum())
        print(f"    {name} {kind}: {len(res[0])} points; bits differing from closest_points {differ}, from the restatement {restated}; tri agrees at {int(agree.sum())}, "
              f"feature differs at {feature_diff}; {st}")
        assert differ == 0 and restated == 0 and agree.all() and feature_diff == 0
        assert st["points_answered"] == len(res[0]) and st["points_refused"] == 0 and st["points_undecided"] == 0
        assert np.isin(res[3], (0, 1, 3)).sum() >= 10 and np.isin(res[3], (2, 4, 5)).sum() >= 10 and (res[3] == 6).sum() >= 10       # vertices, edges and faces all win


@pytest.mark.parametrize("name", tuple(SC.FIXTURES))
def test_sign_equals_the_winding_number_oracle_at_every_point(name):
    from jittor_myc_nerfs_amd import mesh
    v, f, bvh = built(name)
    for kind, s in SC.measure(name)["sets"].items():
        inside = s["winding"] > 0.5
        st = {}
        sd = signed(bvh, s["points"], stats=st)[0]
        wrong = int(((sd < 0) != inside).sum())
        print(f"    {name} {kind}: {len(sd)} points, {int(inside.sum())} inside; wrong signs {wrong}, undecided {st['points_undecided']} "
              f"(the restatement's shortcuts: face normals {int((s['face']['inside'] != inside).sum())}, unweighted {int((s['unweighted']['inside'] != inside).sum())})")
        assert wrong == 0 and st["points_undecided"] == 0            # none excluded, none undecided
        assert np.array_equal(_np(mesh.contains(bvh, _dev(s["points"]))), inside)


def test_a_reversed_mesh_negates_every_sign():
    """Exchanging corners 1 and 2 of every face turns the surface inside out.  The pair arithmetic then sees its corners in another order, so distances may differ in
    their last bits: the answers are held to the reversed mesh's own restatement bit for bit, to the original's within DIST_BAR, and every sign to the negated oracle."""
    v, f, bvh = built("spiked")
    fr = np.ascontiguousarray(f[:, [0, 2, 1]])
    rb = build(v, fr)
    edge = NC.longest_edge(v, f)
    for kind, s in SC.measure("spiked")["sets"].items():
        st = {}
        res, orig = signed(rb, s["points"], stats=st), signed(bvh, s["points"])
        inside = s["winding"] > 0.5
        assert NC.bits_differ((np.abs(res[0]), res[1], res[2]), NC.restate(v, fr, s["points"])) == 0 and st["points_undecided"] == 0
        assert np.array_equal(res[0] < 0, ~inside) and np.array_equal(orig[0] < 0, inside)
        err = np.abs(np.abs(res[0].astype(np.float64)) - np.abs(orig[0].astype(np.float64))) / np.maximum(np.abs(orig[0]), edge)
        print(f"    spiked reversed {kind}: |sdist| against the original's, largest relative difference {err.max():.3g}; same bits at {int((_bits(res[0]) == _bits(-orig[0])).sum())}"
              f" of {len(err)}; same triangle at {int((res[1] == orig[1]).sum())}")
        assert err.max() <= NC.DIST_BAR


def test_vertices_refusals_and_empty_inputs():
    from jittor_myc_nerfs_amd import mesh
    v, f, bvh = built("spiked")
    sd, t, b, ft = signed(bvh, v)                                    # a point that IS a vertex: +0.0, the fan's first triangle, a vertex feature
    assert (_bits(sd) == 0).all() and np.array_equal(t, NC.fan_smallest(f, len(v))) and np.isin(ft, (0, 1, 3)).all()
    q = SC.measure("spiked")["sets"]["shell"]["points"][:64].copy()
    ref = signed(bvh, q)
    q[0, 0], q[1, 2], q[2, 1], q[3] = np.nan, np.inf, -np.inf, np.nan
    st = {}
    res = signed(bvh, q, stats=st)
    assert st["points_refused"] == 4 and st["points_answered"] == 60 and st["points_undecided"] == 0
    assert np.isposinf(res[0][:4]).all() and (res[1][:4] == -1).all() and (res[2][:4] == 0).all() and (res[3][:4] == -1).all()
    assert all(np.array_equal(a[4:], r[4:]) for a, r in zip(res, ref))
    # max_dist: beyond it +inf / -1 / zeros / -1, within it the same bits
    lim = float(np.median(np.abs(ref[0])))
    cut = signed(bvh, SC.measure("spiked")["sets"]["shell"]["points"][:64], max_dist=lim)
    far = np.abs(ref[0]) > np.float32(lim)
    assert 8 < far.sum() < 56 and np.isposinf(cut[0][far]).all() and (cut[3][far] == -1).all() and all(np.array_equal(a[~far], r[~far]) for a, r in zip(cut, ref))
    # no points; no triangles
    none = signed(bvh, np.zeros((0, 3), np.float32))
    assert [x.shape for x in none] == [(0,), (0,), (0, 3), (0,)]
    empty = mesh.build_bvh(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    st, cs = {}, {}
    res = signed(empty, q, stats=st)
    assert mesh.build_pseudonormals(empty, stats=cs).closed and cs["closed"]
    assert np.isposinf(res[0]).all() and (res[1] == -1).all() and (res[2] == 0).all() and (res[3] == -1).all() and st["points_answered"] == 0
    assert not _np(mesh.contains(empty, _dev(q))).any()
    assert tuple(mesh.signed_distance_grid(empty, (2, 3, 4)).shape) == (2, 3, 4) and tuple(mesh.signed_distance_grid(bvh, (0, 3, 4)).shape) == (0, 3, 4)


def test_order_chunking_and_two_runs(monkeypatch):
    from jittor_myc_nerfs_amd import mesh
    v, f, bvh = built("spiked")
    sets = SC.measure("spiked")["sets"]
    p = np.concatenate([sets["shell"]["points"], sets["near"]["points"]])
    base, again = signed(bvh, p), signed(bvh, p)
    assert all(np.array_equal(a, b) for a, b in zip(base, again))
    perm = np.random.default_rng(7).permutation(len(p))
    shuffled = signed(bvh, p[perm])
    assert all(np.array_equal(a, b[perm]) for a, b in zip(shuffled, base))
    monkeypatch.setattr(mesh, "BVH_SIGNED_CHUNK", 1000)
    st = {}
    pieces = signed(bvh, p, stats=st)
    assert all(np.array_equal(a, b) for a, b in zip(pieces, base)) and st["points_answered"] == len(p) and st["points_undecided"] == 0


def test_foreign_tables_are_refused_and_unwanted_outputs_stay_unwritten():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    v, f, bvh = built("spiked")
    p = SC.measure("spiked")["sets"]["shell"]["points"][:300]
    other = built("cube")[2]
    mesh.build_pseudonormals(other)
    mesh.build_pseudonormals(bvh)
    wrong = mesh.MeshBVH(bvh.blob, bvh.verts, bvh.faces, 0, 0)
    wrong.pseudonormals = other.pseudonormals                        # a table of another mesh's size: refused on the host
    with pytest.raises(L.TvrError, match="table holds 1280 B"):
        mesh.signed_distance(wrong, _dev(p))
    wrong.pseudonormals = mesh.MeshPseudonormals(torch.zeros_like(bvh.pseudonormals.blob), bvh.pseudonormals.counters)      # the right size, no header: the flag
    with pytest.raises(L.TvrError, match="fault flag"):
        mesh.signed_distance(wrong, _dev(p))
    # the C call with tri / bary / feature NULL: sdist alone is written, N rows, and the guard rows behind them keep their sentinel
    lib, N, G = L.lib(), len(p), 64
    pd = _dev(p)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    sd = torch.full((N + G,), -7.0, device="cuda")
    table = bvh.pseudonormals.blob
    rc = lib.tvr_mesh_bvh_signed(bvh.verts.data_ptr(), bvh.n_vertices, bvh.faces.data_ptr(), bvh.n_triangles, bvh.blob.data_ptr(), bvh.blob.numel(), table.data_ptr(),
                                 table.numel(), pd.data_ptr(), N, None, float("inf"), sd.data_ptr(), 4 * N, None, 0, None, 0, None, 0, None, flag.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and int(flag.item()) == 0 and bool((sd[N:] == -7).all())
    assert np.array_equal(_np(sd[:N]), signed(bvh, p)[0])


# ---- the lattice ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_lattice_equals_the_point_form_bit_for_bit():
    from jittor_myc_nerfs_amd import mesh
    v, f, bvh = built("spiked")
    dims, origin, spacing = (24, 23, 25), (-1.21, -1.17, -1.3), (0.1051, 0.1063, 0.1049)       # unequal sizes: a transposed layout would show
    st = {}
    vol = mesh.signed_distance_grid(bvh, dims, origin, spacing, stats=st)
    assert tuple(vol.shape) == dims and vol.dtype == torch.float32 and vol.is_contiguous()
    idx = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float32) for n in dims], indexing="ij"), -1).reshape(-1, 3)
    p = np.float32(origin)[None] + idx * np.float32(spacing)[None]                               # fp32: one product, one sum
    st2 = {}
    sd = signed(bvh, p, stats=st2)[0]
    assert np.array_equal(_bits(_np(vol).reshape(-1)), _bits(sd))
    assert st == st2 and st["points_answered"] == len(p) and (sd < 0).sum() > 100 and (sd > 0).sum() > 100


def test_marching_cubes_of_the_field_gives_the_mesh_back():
    """sphere960's field on a 32^3 lattice, its zero level set by marching cubes, and the distance between that and the original.  Derived bound: every point of the
    extracted surface lies in a lattice cell on whose corners the field changes sign; the field is continuous, so the original surface passes through that cell, and
    two points of one cell are at most its diagonal apart.  Conversely a point of the original surface lies in a cell that the surface passes through; where that
    cell has a corner on either side it holds a piece of the extracted surface, and a cell the surface only grazes (all corners on one side) is entered through a
    face from a cell that has — on a sphere of radius 1 with cells of 0.08 such a cap is at most h^2 (3/8) = 0.0024 deep, against a diagonal of 0.14.  So the
    Hausdorff distance is at most one voxel diagonal."""
    from jittor_myc_nerfs_amd import mesh
    v, f, bvh = built("sphere960")
    n, lo, hi = 32, -1.25, 1.25
    h = (hi - lo) / (n - 1)
    vol = mesh.signed_distance_grid(bvh, (n, n, n), (lo, lo, lo), (h, h, h))
    # marching_cubes calls a grid point inside iff value >= level: on the field itself that is the OUTSIDE of the mesh, and flip=True turns the triangles back
    mv, mf = mesh.marching_cubes(vol, 0.0, spacing=(h, h, h), origin=(lo, lo, lo), flip=True)
    got = mesh.signed_mesh_distance(mv, mf, _dev(v), _dev(f, np.int32), bvh_b=bvh)
    diag = np.sqrt(3.0) * h
    print(f"    sphere960 -> 32^3 field -> marching cubes: {mf.shape[0]} triangles; hausdorff {got['hausdorff']:.4f} against a voxel diagonal of {diag:.4f}; "
          f"extracted -> original signed mean {got['a_to_b']['signed_mean']:.5f}")
    assert mf.shape[0] > 500 and 0 < got["hausdorff"] <= diag
    rt = mesh.build_bvh(mv, mf)
    cs = {}
    mesh.build_pseudonormals(rt, stats=cs)
    assert cs["closed"]                                              # a closed field gives a closed, consistently oriented surface,
    probe = _dev([[0.0, 0.0, 0.0], [0.0, 0.0, 2.0]])
    assert _np(mesh.contains(rt, probe)).tolist() == [True, False]   # oriented like the original: the centre is inside
    assert _np(mesh.contains(bvh, probe)).tolist() == [True, False]


# ---- mesh_distance and the command line -----------------------------------------------------------------------------------------------------------------------------------------------
def _chord_depth(v, f):
    """1 - the smallest radius of a point of a mesh whose vertices lie on the unit sphere: a triangle's circumradius is at most longest edge / sqrt(3), so its plane cuts
    the sphere at a depth of at most 1 - sqrt(1 - e^2 / 3)"""
    e = NC.longest_edge(v, f)
    return 1.0 - np.sqrt(1.0 - e * e / 3.0)


@pytest.mark.parametrize("scale", (0.9, 1.1))
def test_signed_distance_of_a_scaled_sphere(scale):
    """A = scale * sphere960 against B = sphere960.  B lies between the spheres of radius rho = 1 - depth and 1, A between scale * rho and scale.  A point at radius
    r < rho is inside B, and its distance to B lies in [rho - r, 1 - r] (it must leave the sphere rho; the radial ray meets B before radius 1); at r > 1 it is
    outside, within [r - 1, r - rho].  So every sample's signed distance, and with it the mean, is within 1.1 * depth of scale - 1."""
    from jittor_myc_nerfs_amd import mesh
    v, f, bvh = built("sphere960")
    assert np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 1).max() < 1e-6
    depth = _chord_depth(v, f)
    va = (v * np.float32(scale)).astype(np.float32)
    plain = mesh.mesh_distance(_dev(va), _dev(f, np.int32), _dev(v), _dev(f, np.int32), bvh_b=bvh)
    st = {}
    got = mesh.signed_mesh_distance(_dev(va), _dev(f, np.int32), _dev(v), _dev(f, np.int32), bvh_b=bvh, stats=st)
    print(f"    {scale} x sphere960 against sphere960 (chord depth {depth:.5f}): a_to_b {got['a_to_b']}")
    assert {k: got["a_to_b"][k] for k in mesh.DISTANCE_STATISTICS} == plain["a_to_b"] and got["hausdorff"] == plain["hausdorff"] and got["chamfer"] == plain["chamfer"]
    assert set(got["a_to_b"]) == set(mesh.DISTANCE_STATISTICS) | set(mesh.SIGNED_STATISTICS)
    assert got["a_to_b"]["inside_fraction"] == (1.0 if scale < 1 else 0.0) and got["b_to_a"]["inside_fraction"] == (0.0 if scale < 1 else 1.0)
    bound = 1.1 * depth + NC.DIST_BAR
    assert abs(got["a_to_b"]["signed_mean"] - (scale - 1.0)) <= bound and abs(got["b_to_a"]["signed_mean"] - (1.0 - scale)) <= bound
    assert abs(abs(got["a_to_b"]["signed_mean"]) - got["a_to_b"]["mean"]) < 1e-12                # one sign throughout: the signed mean is the unsigned one
    assert st["closedness"]["a_to_b"]["closed"] and st["closedness"]["b_to_a"]["closed"] and st["points_undecided"] == 0


def test_command_line_writes_the_signed_keys_and_leaves_the_default_file_alone(tmp_path, capsys):
    from jittor_myc_nerfs_amd import mesh, reconstruct as R
    v, f, _ = built("sphere960")
    a, b, hole = str(tmp_path / "small.ply"), str(tmp_path / "unit.ply"), str(tmp_path / "hole.ply")
    mesh.write_ply(a, (v * np.float32(0.9)).astype(np.float32), f)
    mesh.write_ply(b, v, f)
    mesh.write_ply(hole, v, np.delete(f, 100, 0))
    out = R.main(["--mesh_file", a, "--mesh_compare", b])
    default = open(out, "rb").read()
    va, fa = R._read_mesh_geometry(a)
    vb, fb = R._read_mesh_geometry(b)
    # the report as it was composed before the flag existed
    want = {"mesh_file": a, "reference_file": b, "vertices": len(va), "triangles": len(fa), "reference_vertices": len(vb), "reference_triangles": len(fb),
            "a_is": "mesh_file", "b_is": "reference_file", "subdiv": 2, "world": mesh.mesh_distance(_dev(va), _dev(fa, np.int32), _dev(vb), _dev(fb, np.int32))}
    assert default == json.dumps(want, indent=1).encode()
    assert R.main(["--mesh_file", a, "--mesh_compare", b, "--mesh_compare_signed", "0"]) == out and open(out, "rb").read() == default
    assert R.main(["--mesh_file", a, "--mesh_compare", b, "--mesh_compare_signed", "1"]) == out
    rep = json.loads(open(out).read())
    assert "signed mean" in capsys.readouterr().out
    for side, frac in (("a_to_b", 1.0), ("b_to_a", 0.0)):
        assert {k: rep["world"][side][k] for k in want["world"][side]} == want["world"][side]                 # the unsigned figures are untouched
        assert rep["world"][side]["inside_fraction"] == frac and abs(abs(rep["world"][side]["signed_mean"]) - 0.1) < 0.01
        assert rep["closedness"][side] == dict(dict.fromkeys(SC.COUNTERS, 0), closed=True)
    assert rep["world"]["hausdorff"] == want["world"]["hausdorff"] and {k: rep[k] for k in want if k != "world"} == {k: want[k] for k in want if k != "world"}
    # a target that is not closed: null signed keys with the reason, the unsigned figures still written; the other direction is unaffected
    R.main(["--mesh_file", a, "--mesh_compare", hole, "--mesh_compare_signed", "1"])
    rep = json.loads(open(out).read())
    ab, ba = rep["world"]["a_to_b"], rep["world"]["b_to_a"]
    assert ab["signed_mean"] is None and ab["inside_fraction"] is None and "open_edges = 3" in ab["signed_reason"] and ab["mean"] > 0 and ab["refused"] == 0
    assert rep["closedness"]["a_to_b"]["open_edges"] == 3 and not rep["closedness"]["a_to_b"]["closed"]
    assert ba["inside_fraction"] == 0.0 and "signed_reason" not in ba and rep["closedness"]["b_to_a"]["closed"] and rep["world"]["hausdorff"] > 0
