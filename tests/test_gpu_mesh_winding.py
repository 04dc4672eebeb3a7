"""GPU: the table of node moments and the hierarchical winding-number query (csrc/tvr_mesh_winding.hip; include/tvr.h tvr_mesh_winding_*; mesh.build_winding /
winding_number / winding_contains / winding_number_grid / signed_distance_winding / remesh_watertight, reconstruct --mesh_watertight).  The table bit for bit against
the numpy fp32 restatement of tests/mesh_winding_common.py on the device's own tree; beta = inf within WINDING_BAR of the brute-force fp64 oracle at every point of
every set; beta = 2 and 3 within WINDING_BAR of the fp64 restatement on the device's tree and table, with the same number of node visits, dipoles and triangles; the
approximation error against its recorded value; the classification on the closed fixtures, the union of two overlapping spheres and the unwelded soup, where
mesh.contains is wrong at hundreds of points (tests/test_mesh_winding_host.py shows the same on the CPU); order, chunking, the lattice, refusals; the signed distance;
the watertight remesh within derived bounds; the command line.  The references are computed once per process and shared (mesh_winding_common.cases)."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_bvh_common as MB
import mesh_nearest_common as NC
import mesh_signed_common as SC
import mesh_winding_common as WC

pytestmark = pytest.mark.gpu

CASES = ("spiked", "cube", "tetra", "union", "soup", "tripled", "removed", "reversed", "F1", "F2")
CLASSIFIED = ("spiked", "cube", "tetra", "union", "soup")
_cache = {}


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def build(v, f):
    from jittor_myc_nerfs_amd import mesh
    return mesh.build_bvh(_dev(v).reshape(-1, 3), _dev(f, np.int32).reshape(-1, 3))


def device_rows(bvh):
    """(rows [F-1,8] float32, the whole table as bytes) of a hierarchy's winding table"""
    from jittor_myc_nerfs_amd import mesh
    raw = _np(mesh.build_winding(bvh).blob)
    lay = mesh.winding_layout(bvh.n_triangles)
    assert len(raw) == lay["total"] and lay["row_stride"] == 32
    return raw[lay["rows"]:lay["rows"] + 32 * lay["n_rows"]].view(np.float32).reshape(lay["n_rows"], 8).copy(), raw


def built(name):
    """dict(case, bvh, tree, rows, raw) of a fixture of mesh_winding_common, built once: the device's tree and table read back"""
    if name not in _cache:
        c = WC.cases()[name]
        bvh = build(c["verts"], c["faces"])
        tree = MB.read_tree(_np(bvh.blob), bvh.layout(), bvh.n_triangles)
        rows, raw = device_rows(bvh)
        _cache[name] = dict(case=c, bvh=bvh, tree=tree, rows=rows, raw=raw)
    return _cache[name]


def winding(bvh, p, beta, stats=None):
    from jittor_myc_nerfs_amd import mesh
    return _np(mesh.winding_number(bvh, _dev(p).reshape(-1, 3), beta, stats=stats))


def restated(name, kind, beta):
    """the fp64 restatement on the device's tree and table, once per (fixture, set, beta)"""
    key = (name, kind, beta)
    if key not in _cache:
        b = built(name)
        c = b["case"]
        if ("omega", name, kind) not in _cache:
            _cache[("omega", name, kind)] = WC.solid_angles(c["verts"], c["faces"], c["sets"][kind])
        _cache[key] = WC.query(b["tree"], b["rows"], c["verts"], c["faces"], c["sets"][kind], beta, omega=_cache[("omega", name, kind)])
    return _cache[key]


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_table_equals_the_restatement_bit_for_bit_and_two_builds_give_the_same_bytes(name):
    from jittor_myc_nerfs_amd import mesh
    b = built(name)
    c, bvh = b["case"], b["bvh"]
    F = len(c["faces"])
    MB.check_tree(b["tree"], c["verts"], c["faces"])
    ref = WC.table(b["tree"], c["verts"], c["faces"])
    differ = int((_bits(b["rows"]) != _bits(ref)).any(1).sum()) if F > 1 else 0
    st = {}
    assert mesh.build_winding(bvh, stats=st) is bvh.winding           # built once and kept
    print(f"    {name}: {F} triangles, height {b['tree']['height']}; rows differing from the fp32 restatement {differ} of {max(F - 1, 0)}; {st}")
    assert b["rows"].shape == ref.shape and differ == 0               # A, c, r and a, +0.0 included
    assert st == dict(internal_nodes=max(F - 1, 0), table_bytes=len(b["raw"]))
    assert b["raw"][:32].view(np.uint32).tolist() == [0x4e575654, F, 0, 0, 0, 0, 0, 0]
    if F > 1:
        assert np.isfinite(b["rows"][:, 6]).all() and (b["rows"][:, 7] > 0).all()
    again = build(c["verts"], c["faces"])
    assert np.array_equal(_np(again.blob), _np(bvh.blob))             # the hierarchy's blob is what it was,
    assert np.array_equal(device_rows(again)[1], b["raw"])            # and the table the same bytes, padding included


def test_empty_and_degenerate_meshes():
    from jittor_myc_nerfs_amd import mesh
    empty = mesh.build_bvh(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    rows, raw = device_rows(empty)
    assert rows.shape == (0, 8) and raw[:32].view(np.uint32).tolist() == [0x4e575654, 0, 0, 0, 0, 0, 0, 0] and len(raw) == 256
    q = WC.cases()["F1"]["sets"]["shell"][:64]
    st = {}
    assert (_bits(winding(empty, q, 2.0, stats=st)) == 0).all() and st["points_answered"] == 64 and st["triangle_terms"] == 0      # F == 0: +0.0
    assert not _np(mesh.winding_contains(empty, _dev(q))).any()
    assert tuple(mesh.winding_number_grid(empty, (2, 3, 4)).shape) == (2, 3, 4)
    # zero-area and non-finite triangles: a = 0 below some nodes (r = +inf, never approximated), skipped triangles add nothing
    c = WC.cases()["cube"]
    v = np.concatenate([c["verts"], [[np.nan, 0, 0], [2, 2, 2]]]).astype(np.float32)
    f = np.concatenate([c["faces"], [[8, 0, 1], [9, 9, 9], [9, 9, 9]]]).astype(np.int32)
    bvh = build(v, f)
    tree = MB.read_tree(_np(bvh.blob), bvh.layout(), len(f))
    rows = device_rows(bvh)[0]
    assert np.array_equal(_bits(rows), _bits(WC.table(tree, v, f))) and np.isposinf(rows[:, 6]).any()
    p = c["sets"]["shell"]
    for beta in (2.0, np.inf):
        got = winding(bvh, p, beta)
        ref = WC.query(tree, rows, v, f, p, beta)["w"]
        assert np.isfinite(got).all() and np.abs(got - ref).max() <= WC.WINDING_BAR
    assert np.abs(winding(bvh, p, np.inf) - c["oracle"]["shell"]).max() <= WC.WINDING_BAR      # the additions change nothing


# ---- the query --------------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_exact_mode_is_within_the_bar_of_the_oracle_at_every_point(name):
    b = built(name)
    c = b["case"]
    for kind, p in c["sets"].items():
        st = {}
        w = winding(b["bvh"], p, np.inf, stats=st)
        err = np.abs(w.astype(np.float64) - c["oracle"][kind])
        print(f"    {name} {kind}: {len(p)} points, beta = inf; max |w - oracle| {err.max():.3g} (bar {WC.WINDING_BAR:g}); {st}")
        assert err.max() <= WC.WINDING_BAR                            # none excluded
        assert st == dict(points_answered=len(p), points_refused=0, node_visits=len(p) * (len(c["faces"]) - 1), dipole_terms=0, triangle_terms=len(p) * len(c["faces"]))
    if name == "tripled":
        s = NC.sphere_mesh("sphere960")
        p = c["sets"]["shell"]
        assert np.abs(winding(b["bvh"], p, np.inf) - 3 * SC.winding(s[0], s[1], p)).max() <= 3 * WC.WINDING_BAR       # three coincident shells: 3 x the sphere's


@pytest.mark.parametrize("beta", (2.0, 3.0))
@pytest.mark.parametrize("name", CASES)
def test_approximate_mode_is_within_the_bar_of_the_restatement_at_every_point(name, beta):
    b = built(name)
    c = b["case"]
    for kind, p in c["sets"].items():
        st = {}
        w = winding(b["bvh"], p, beta, stats=st)
        ref = restated(name, kind, beta)
        err = np.abs(w.astype(np.float64) - ref["w"])
        print(f"    {name} {kind}: {len(p)} points, beta = {beta:g}; max |w - restatement| {err.max():.3g} (bar {WC.WINDING_BAR:g}); restatement against the oracle "
              f"{np.abs(ref['w'] - c['oracle'][kind]).max():.3g}; {st}")
        assert err.max() <= WC.WINDING_BAR
        assert {k: st[k] for k in ("node_visits", "dipole_terms", "triangle_terms")} == {k: ref[k] for k in ("node_visits", "dipole_terms", "triangle_terms")}   # every decision
        assert st["points_answered"] == len(p) and st["points_refused"] == 0


@pytest.mark.parametrize("beta", (2.0, 3.0))
def test_approximation_error_against_its_recorded_value(beta):
    c = built("spiked")["case"]
    A = max(float(np.abs(restated("spiked", kind, beta)["w"] - c["oracle"][kind]).max()) for kind in c["sets"])
    dip = sum(restated("spiked", kind, beta)["dipole_terms"] for kind in c["sets"])
    tri = sum(restated("spiked", kind, beta)["triangle_terms"] for kind in c["sets"])
    print(f"    spiked sphere on the device's tree: A({beta:g}) = {A:.4g} (recorded {WC.APPROX_MEASURED[beta]}); {dip} dipoles and {tri} triangles against "
          f"{sum(len(p) for p in c['sets'].values()) * len(c['faces'])} triangles of the exact sum")
    assert A <= 2 * WC.APPROX_MEASURED[beta] and A < 0.25


@pytest.mark.parametrize("name", CLASSIFIED)
def test_classification_equals_the_truth_at_every_point(name):
    from jittor_myc_nerfs_amd import mesh
    b = built(name)
    c = b["case"]
    assert WC.margin(c) > 0.49
    for kind, p in c["sets"].items():
        inside = _np(mesh.winding_contains(b["bvh"], _dev(p)))
        wrong = {beta: int(((winding(b["bvh"], p, beta) > 0.5) != c["truth"][kind]).sum()) for beta in WC.BETAS}
        print(f"    {name} {kind}: {len(p)} points, {int(c['truth'][kind].sum())} inside; wrong at beta 2 / 3 / inf: {wrong}")
        assert np.array_equal(inside, c["truth"][kind]) and all(n == 0 for n in wrong.values())      # none excluded


def test_pseudo_normals_are_wrong_on_the_union_where_the_winding_number_is_right():
    from jittor_myc_nerfs_amd import mesh
    b = built("union")
    c = b["case"]
    p, truth = c["sets"]["shell"], c["truth"]["shell"]
    cs = {}
    mesh.build_pseudonormals(b["bvh"], stats=cs)
    assert cs["closed"]                                              # strict=True accepts it
    pseudo = int((_np(mesh.contains(b["bvh"], _dev(p), strict=True)) != truth).sum())
    wind = int((_np(mesh.winding_contains(b["bvh"], _dev(p))) != truth).sum())
    print(f"    union: mesh.contains wrong at {pseudo} of {len(p)} points, mesh.winding_contains at {wind}")
    assert pseudo > 400 and wind == 0


# ---- invariances and refusals -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_order_chunking_and_two_runs(monkeypatch):
    from jittor_myc_nerfs_amd import mesh
    b = built("spiked")
    sets = b["case"]["sets"]
    p = np.concatenate([sets["shell"], sets["near"]])
    for beta in (2.0, np.inf):
        st0 = {}
        base, again = winding(b["bvh"], p, beta, stats=st0), winding(b["bvh"], p, beta)
        assert np.array_equal(_bits(base), _bits(again))
        perm = np.random.default_rng(7).permutation(len(p))
        assert np.array_equal(_bits(winding(b["bvh"], p[perm], beta)), _bits(base[perm]))
        with monkeypatch.context() as m:
            m.setattr(mesh, "BVH_WINDING_CHUNK", 1000)
            st = {}
            assert np.array_equal(_bits(winding(b["bvh"], p, beta, stats=st)), _bits(base)) and st == st0 and st["points_answered"] == len(p)


def test_lattice_equals_the_point_form_bit_for_bit():
    from jittor_myc_nerfs_amd import mesh
    bvh = built("spiked")["bvh"]
    dims, origin, spacing = (24, 23, 25), (-1.21, -1.17, -1.3), (0.1051, 0.1063, 0.1049)       # unequal sizes: a transposed layout would show
    st = {}
    vol = mesh.winding_number_grid(bvh, dims, origin, spacing, stats=st)
    assert tuple(vol.shape) == dims and vol.dtype == torch.float32 and vol.is_contiguous()
    idx = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float32) for n in dims], indexing="ij"), -1).reshape(-1, 3)
    p = np.float32(origin)[None] + idx * np.float32(spacing)[None]                               # fp32: one product, one sum
    st2 = {}
    w = winding(bvh, p, 2.0, stats=st2)
    assert np.array_equal(_bits(_np(vol).reshape(-1)), _bits(w))
    assert st == st2 and st["points_answered"] == len(p) and (w > 0.5).sum() > 100 and (w < 0.5).sum() > 100
    assert tuple(mesh.winding_number_grid(bvh, (0, 3, 4)).shape) == (0, 3, 4)


def test_refusals_foreign_tables_and_unwanted_counts():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    b = built("spiked")
    bvh = b["bvh"]
    q = b["case"]["sets"]["shell"][:64].copy()
    ref = winding(bvh, q, 2.0)
    q[0, 0], q[1, 2], q[2, 1], q[3] = np.nan, np.inf, -np.inf, np.nan
    st = {}
    w = winding(bvh, q, 2.0, stats=st)
    assert st["points_refused"] == 4 and st["points_answered"] == 60 and np.isnan(w[:4]).all() and np.array_equal(_bits(w[4:]), _bits(ref[4:]))
    assert not _np(mesh.winding_contains(bvh, _dev(q)))[:4].any()
    sd = mesh.signed_distance_winding(bvh, _dev(q))
    assert np.isposinf(_np(sd[0])[:4]).all() and (_np(sd[1])[:4] == -1).all()
    assert winding(bvh, np.zeros((0, 3), np.float32), 2.0).shape == (0,)
    for beta in (0.5, float("nan"), -2.0):
        with pytest.raises(L.TvrError, match="beta"):
            mesh.winding_number(bvh, _dev(q), beta)
    # a vertex of the mesh, an edge midpoint and a face centroid: finite
    v, f = b["case"]["verts"], b["case"]["faces"]
    on = np.concatenate([v[:32], 0.5 * (v[f[:32, 0]] + v[f[:32, 1]]), v[f[:32]].mean(1)]).astype(np.float32)
    assert np.isfinite(winding(bvh, on, 2.0)).all() and np.isfinite(winding(bvh, on, np.inf)).all()
    # a table of another mesh's size is refused on the host; one of the right size without a header raises the flag
    other = built("cube")["bvh"]
    wrong = mesh.MeshBVH(bvh.blob, bvh.verts, bvh.faces, 0, 0)
    wrong.winding = other.winding
    with pytest.raises(L.TvrError, match="table holds 768 B"):
        mesh.winding_number(wrong, _dev(b["case"]["sets"]["shell"][:64]))
    wrong.winding = mesh.MeshWinding(torch.zeros_like(bvh.winding.blob))
    with pytest.raises(L.TvrError, match="fault flag"):
        mesh.winding_number(wrong, _dev(b["case"]["sets"]["shell"][:64]))
    # the C call with counts_dev NULL: w alone is written, N values, and the guard values behind them keep their sentinel
    lib, p = L.lib(), b["case"]["sets"]["shell"][:300]
    N, G = len(p), 64
    pd = _dev(p)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((N + G,), -7.0, device="cuda")
    counts = torch.full((5 + G,), -7, dtype=torch.int64, device="cuda")
    table = bvh.winding.blob
    call = lambda c: lib.tvr_mesh_winding_query(bvh.verts.data_ptr(), bvh.n_vertices, bvh.faces.data_ptr(), bvh.n_triangles, bvh.blob.data_ptr(), bvh.blob.numel(),
                                                table.data_ptr(), table.numel(), pd.data_ptr(), N, None, 2.0, out.data_ptr(), 4 * N, c, flag.data_ptr(), None)
    rc = call(None)
    torch.cuda.synchronize()
    assert rc == 0 and int(flag.item()) == 0 and bool((out[N:] == -7).all()) and np.array_equal(_bits(_np(out[:N])), _bits(winding(bvh, p, 2.0)))
    rc = call(counts.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and bool((counts[5:] == -7).all()) and counts[:2].tolist() == [N, 0] and int(counts[2:5].min()) > 0


# ---- the signed distance ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("union", "soup"))
def test_signed_distance_winding_is_closest_points_with_the_right_sign(name):
    from jittor_myc_nerfs_amd import mesh
    b = built(name)
    c = b["case"]
    for kind, p in c["sets"].items():
        st = {}
        sd, tri, bary = (_np(x) for x in mesh.signed_distance_winding(b["bvh"], _dev(p), stats=st))
        d, t2, b2 = (_np(x) for x in mesh.closest_points(b["bvh"], _dev(p)))
        assert np.array_equal(_bits(np.abs(sd)), _bits(d)) and np.array_equal(tri, t2) and np.array_equal(_bits(bary), _bits(b2))
        assert (d > 0).all() and np.array_equal(sd < 0, c["truth"][kind])                        # right at every point, none excluded
        assert st["points_answered"] == len(p) and st["dipole_terms"] > 0 and st["triangle_tests"] > 0
    lim = float(np.median(d))
    cut = _np(mesh.signed_distance_winding(b["bvh"], _dev(p), max_dist=lim)[0])
    far = d > np.float32(lim)
    assert 0 < far.sum() < len(p) and np.isposinf(cut[far]).all() and np.array_equal(_bits(cut[~far]), _bits(sd[~far]))


# ---- the watertight remesh --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_remesh_of_the_union_is_one_closed_surface_within_a_voxel_of_the_input():
    """Every vertex of the result sits on a lattice edge whose ends lie on either side of the level set; the winding number of a closed shell is piecewise constant and
    jumps only across the surface, and the approximation (a few 1e-2, margin 0.5) cannot move a grid point across the level: the input's OUTER surface crosses that edge,
    so the vertex is within one voxel of it.  A test point farther than the voxel's diagonal from the input surface lies with its whole cell on one side of it, so the
    result classifies it as the input does."""
    from jittor_myc_nerfs_amd import mesh
    b = built("union")
    c = b["case"]
    st = {}
    ov, of = mesh.remesh_watertight(_dev(c["verts"]), _dev(c["faces"], np.int32), resolution=96, stats=st)
    voxel = st["voxel"]
    ext = c["verts"].max(0).astype(np.float64) - c["verts"].min(0)
    assert abs(voxel - ext.max() / 96) < 1e-12 and st["dims"] == [int(np.ceil(e / voxel)) + 5 for e in ext]
    d = _np(mesh.closest_points(b["bvh"], ov)[0])
    p, truth = c["sets"]["shell"], c["truth"]["shell"]
    rb = mesh.build_bvh(ov, of)
    inside = _np(mesh.winding_contains(rb, _dev(p), beta=float("inf")))
    clear = _np(mesh.closest_points(b["bvh"], _dev(p))[0]) > np.sqrt(3.0) * voxel
    print(f"    union -> {st['dims']} lattice, voxel {voxel:.4f} -> {of.shape[0]} triangles, {st['components']} component; input {st['input']}, result {st['result']}; "
          f"vertices at most {d.max() / voxel:.3f} voxels from the input; {int((~clear).sum())} of {len(p)} test points within a diagonal of the surface, wrong among "
          f"the others {int((inside != truth)[clear].sum())}")
    assert of.shape[0] > 5000 and st["input"]["closed"] and st["result"] == dict(dict.fromkeys(SC.COUNTERS, 0), closed=True) and st["components"] == 1
    assert d.max() <= voxel * (1 + 1e-5)
    assert (~clear).sum() <= 0.15 * len(p) and np.array_equal(inside[clear], truth[clear])
    # no internal wall is left: the lens between the centres is inside, and nothing of the result lies in it
    lens = np.asarray([[0.4, 0.0, 0.0]], np.float32)
    assert _np(mesh.closest_points(rb, _dev(lens))[0])[0] > 0.5 and _np(mesh.winding_contains(rb, _dev(lens)))[0]
    # a coarser voxel given outright
    st2 = {}
    mesh.remesh_watertight(_dev(c["verts"]), _dev(c["faces"], np.int32), voxel=0.1, pad=1, stats=st2)
    assert st2["voxel"] == 0.1 and st2["dims"] == [int(np.ceil(e / 0.1)) + 3 for e in ext] and st2["result"]["closed"] and st2["components"] == 1


@pytest.mark.parametrize("name", ("soup", "removed"))
def test_remesh_closes_meshes_that_are_not(name):
    from jittor_myc_nerfs_amd import mesh
    c = built(name)["case"]
    st = {}
    ov, of = mesh.remesh_watertight(_dev(c["verts"]), _dev(c["faces"], np.int32), resolution=64, stats=st)
    print(f"    {name}: input {st['input']} -> {of.shape[0]} triangles, result {st['result']}, {st['components']} component")
    assert not st["input"]["closed"] and st["input"]["open_edges"] > 0
    assert of.shape[0] > 1000 and st["result"] == dict(dict.fromkeys(SC.COUNTERS, 0), closed=True) and st["components"] >= 1
    if name == "removed":
        assert st["components"] == 1                                 # the hole is bridged, nothing floats
    rb = mesh.build_bvh(ov, of)
    assert _np(mesh.contains(rb, _dev([[0.0, 0.0, 0.0], [0.0, 0.0, 2.0]]))).tolist() == [True, False]     # closed and outward: the pseudo-normal sign works again


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_remesh_and_leaves_everything_else_alone(tmp_path, capsys):
    from jittor_myc_nerfs_amd import mesh, reconstruct as R
    c = built("union")["case"]
    s = NC.sphere_mesh("sphere960")
    a, ref = str(tmp_path / "union.ply"), str(tmp_path / "unit.ply")
    mesh.write_ply(a, c["verts"], c["faces"])
    mesh.write_ply(ref, s[0], s[1])
    dist = R.main(["--mesh_file", a, "--mesh_compare", ref])
    before = {n: open(tmp_path / n, "rb").read() for n in sorted(os.listdir(tmp_path))}
    assert R.main(["--mesh_file", a, "--mesh_compare", ref, "--mesh_watertight", "0"]) == dist
    assert {n: open(tmp_path / n, "rb").read() for n in sorted(os.listdir(tmp_path))} == before        # 0: no new file, every byte as it was
    out = R.main(["--mesh_file", a, "--mesh_watertight", "48"])
    assert out == str(tmp_path / "union_watertight.json") and "watertight remesh" in capsys.readouterr().out
    assert sorted(os.listdir(tmp_path)) == sorted(list(before) + ["union_watertight.json", "union_watertight.ply"])
    assert all(open(tmp_path / n, "rb").read() == x for n, x in before.items())
    rep = json.loads(open(out).read())
    ov, of = mesh.read_ply(str(tmp_path / "union_watertight.ply"))[:2]
    assert rep["mesh_file"] == a and rep["watertight_file"] == str(tmp_path / "union_watertight.ply") and rep["resolution"] == 48 and rep["beta"] == 2.0
    assert (rep["vertices"], rep["triangles"], rep["watertight_vertices"], rep["watertight_triangles"]) == (len(c["verts"]), len(c["faces"]), len(ov), len(of))
    ext = float((c["verts"].max(0).astype(np.float64) - c["verts"].min(0)).max())
    assert len(rep["dims"]) == 3 and abs(rep["voxel"] - ext / 48) < 1e-12 and rep["components"] == 1
    assert rep["input"] == rep["result"] == dict(dict.fromkeys(SC.COUNTERS, 0), closed=True)
    # every point of the result lies in a cell that the input's outer surface crosses: within the cell's diagonal of it
    assert set(rep["world"]) == set(rep["voxels"]) and 0 < rep["world"]["a_to_b"]["max"] <= np.sqrt(3.0) * rep["voxel"] * (1 + 1e-5)
    assert abs(rep["voxels"]["a_to_b"]["max"] - rep["world"]["a_to_b"]["max"] / rep["voxel"]) < 1e-6
    assert rep["world"]["b_to_a"]["max"] > 0.3                        # the input's caps inside the other sphere are gone from the result
    # with --mesh_compare the comparison's file is still what it was
    assert R.main(["--mesh_file", a, "--mesh_compare", ref, "--mesh_watertight", "48", "--mesh_watertight_beta", "3"]) == dist
    assert open(dist, "rb").read() == before[os.path.basename(dist)] and json.loads(open(out).read())["beta"] == 3.0
