"""GPU: the triangle-pair query on the mesh hierarchy (csrc/tvr_mesh_crossings.hip; include/tvr.h tvr_mesh_crossings_*; mesh.self_intersections / mesh_intersections /
crossing_faces / mesh_check / write_obj_segments, reconstruct --mesh_check).  Pairs, piercing counts and piercing points bit for bit against the brute-force numpy fp32
restatement of tests/mesh_crossings_common.py on every fixture (tests/test_mesh_crossings_host.py ties that restatement to an fp64 oracle without a device); the
two-mesh query against the union's self query; two runs, a permuted query mesh, points on and off; the counters; the fault flag of a foreign blob; the project's own
marching-cubes and remesh outputs; the command line.  The references are computed once per process and shared (mesh_crossings_common.reference)."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_crossings_common as XC
import mesh_nearest_common as NC
import mesh_winding_common as WC

pytestmark = pytest.mark.gpu

_cache = {}


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def build(v, f):
    from jittor_myc_nerfs_amd import mesh
    return mesh.build_bvh(_dev(v).reshape(-1, 3), _dev(f, np.int32).reshape(-1, 3))


def built(name):
    if name not in _cache:
        r = XC.reference(name)
        _cache[name] = build(r["verts"], r["faces"])
    return _cache[name]


def self_query(bvh, points=True, stats=None):
    from jittor_myc_nerfs_amd import mesh
    return tuple(_np(x) for x in mesh.self_intersections(bvh, points=points, stats=stats))


def two_mesh(bvh, vq, fq, points=True, stats=None):
    from jittor_myc_nerfs_amd import mesh
    return tuple(_np(x) for x in mesh.mesh_intersections(bvh, _dev(vq).reshape(-1, 3), _dev(fq, np.int32).reshape(-1, 3), points=points, stats=stats))


def ascending(pairs):
    key = pairs[:, 0].astype(np.int64) << 32 | pairs[:, 1].astype(np.int64)
    return bool((np.diff(key) > 0).all())


# ---- 1: the self query on every fixture -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(XC.EXPECTED))
def test_self_query_equals_the_restatement_bit_for_bit(name):
    ref = XC.reference(name)["restate"]
    st = {}
    res = self_query(built(name), stats=st)
    pairs, n_pierce, points = res
    print(f"    {name}: {len(XC.reference(name)['faces'])} triangles, {len(pairs)} pairs, {int(n_pierce.sum())} piercings, {st}")
    assert pairs.dtype == np.int32 and pairs.shape == (len(pairs), 2) and n_pierce.dtype == np.int32 and points.dtype == np.float32 and points.shape == (len(pairs), 2, 3)
    assert XC.bits_differ(res, ref) == 0
    assert ascending(pairs) and (pairs[:, 0] < pairs[:, 1]).all()
    want_pairs, want_piercings = XC.EXPECTED[name]
    assert len(pairs) == want_pairs and (want_piercings is None or int(n_pierce.sum()) == want_piercings)
    assert st["pairs"] == len(pairs) and st["triangles_refused"] == 0


def test_a_triangle_with_a_non_finite_corner_crosses_nothing_and_is_counted():
    v, f = XC.pushed()
    v = v.copy()
    hit = np.unique(XC.reference("pushed")["restate"]["pairs"])
    v[f[hit[0], 0], 1] = np.nan                                      # a corner of a triangle that crosses: its whole fan leaves
    ref = XC.restate(v, f)
    st = {}
    res = self_query(build(v, f), stats=st)
    gone = int((~XC.valid_triangles(v, f)).sum())
    assert 0 < len(ref["pairs"]) < 7 and XC.bits_differ(res, ref) == 0 and st["triangles_refused"] == gone > 0


# ---- 2: two meshes --------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_mesh_query_gives_the_unions_pairs_and_the_swap_their_transpose():
    sv, sf = NC.sphere_mesh("sphere960")
    tv = (sv + np.asarray(WC.UNION_OFFSET, np.float32)).astype(np.float32)
    union = XC.reference("union")["restate"]
    want = union["pairs"] - np.asarray([0, len(sf)], np.int32)
    st = {}
    res = two_mesh(build(tv, sf), sv, sf, stats=st)                  # query: the sphere at the origin (the union's first half); tree: the shifted one
    assert np.array_equal(res[0], want) and ascending(res[0]) and st["pairs"] == len(want) == 164
    assert XC.bits_differ(res, dict(union, pairs=want)) == 0         # the same six tests in the same order: the same piercing counts and points
    assert XC.bits_differ(res, XC.restate(tv, sf, sv, sf)) == 0
    back = two_mesh(build(sv, sf), tv, sf)
    order = np.lexsort((want[:, 0], want[:, 1]))
    assert np.array_equal(back[0], want[order][:, ::-1]) and np.array_equal(back[1], res[1][order]) and ascending(back[0])
    assert XC.bits_differ(back, XC.restate(sv, sf, tv, sf)) == 0
    # an empty query mesh and an empty tree
    empty = two_mesh(build(tv, sf), sv, sf[:0])
    assert empty[0].shape == (0, 2) and empty[1].shape == (0,) and empty[2].shape == (0, 2, 3)
    assert two_mesh(build(sv, sf[:0]), tv, sf)[0].shape == (0, 2)


def test_a_query_mesh_that_reuses_the_trees_vertices_shares_by_position():
    """sphere960 against itself as a second mesh: every crossing candidate shares a corner position or is far away, so nothing is reported (an index rule would see
    two meshes without a common index)"""
    sv, sf = NC.sphere_mesh("sphere960")
    assert two_mesh(built("sphere960"), sv.copy(), sf)[0].shape == (0, 2)


# ---- 3: stability ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_a_permuted_query_and_points_off():
    from jittor_myc_nerfs_amd import mesh
    bvh = built("union")
    a, b = self_query(bvh), self_query(build(*XC.fixtures()["union"]))
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    off = self_query(bvh, points=False)
    assert len(off) == 2 and np.array_equal(off[0], a[0]) and np.array_equal(off[1], a[1])
    sv, sf = NC.sphere_mesh("sphere960")
    tv = (sv + np.asarray(WC.UNION_OFFSET, np.float32)).astype(np.float32)
    tree = build(tv, sf)
    plain = two_mesh(tree, sv, sf)
    perm = np.random.default_rng(5).permutation(len(sf))
    mixed = two_mesh(tree, sv, sf[perm])
    assert ascending(mixed[0])
    mapped = np.stack([perm[mixed[0][:, 0]], mixed[0][:, 1]], -1).astype(np.int32)      # query triangle q' of the permuted mesh is triangle perm[q'] of the plain one
    order = np.lexsort((mapped[:, 1], mapped[:, 0]))
    assert XC.bits_differ((mapped[order], mixed[1][order], mixed[2][order]), dict(pairs=plain[0], n_pierce=plain[1], points=plain[2])) == 0
    mask = _np(mesh.crossing_faces(torch.from_numpy(a[0]).cuda(), bvh.n_triangles))
    assert mask.dtype == bool and mask.sum() == 164 and np.array_equal(np.flatnonzero(mask), np.unique(a[0]))
    assert np.array_equal(np.flatnonzero(_np(mesh.crossing_faces(torch.from_numpy(plain[0]).cuda(), len(sf), column=0))), np.unique(plain[0][:, 0]))


# ---- 4: counters ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_counters_and_the_work_the_hierarchy_saves():
    st = {}
    pairs = self_query(built("union"), stats=st)[0]
    F = 1920
    print(f"    union: {st['pair_tests']} triangle-pair tests of {F * (F - 1) // 2} ({st['pair_tests'] / F:.1f} per triangle), {st['node_tests']} node tests "
          f"({st['node_tests'] / F:.1f} per triangle)")
    assert st["pairs"] == len(pairs) == 164 and st["triangles_refused"] == 0
    assert len(pairs) <= st["pair_tests"] < F * (F - 1) // 2 and st["node_tests"] > 0


# ---- 5: the fault flag ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_blob_built_for_another_mesh_raises_the_flag():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    big, small = built("union"), built("sphere960")
    wrong = mesh.MeshBVH(big.blob, small.verts, small.faces, 0, 0)   # large enough for the host's size check; the header names another F
    with pytest.raises(L.TvrError, match="fault flag"):
        mesh.self_intersections(wrong)
    with pytest.raises(L.TvrError, match="fault flag"):
        mesh.mesh_intersections(wrong, small.verts, small.faces)
    with pytest.raises(L.TvrError, match="tvr_mesh_bvh_bytes"):      # too small a blob never reaches the device
        mesh.self_intersections(mesh.MeshBVH(small.blob, big.verts, big.faces, 0, 0))
    with pytest.raises(L.TvrError, match="build_bvh returns"):
        mesh.self_intersections(None)
    with pytest.raises(L.TvrError, match="no CPU fallback|HIP"):
        mesh.mesh_intersections(small, small.verts.cpu(), small.faces.cpu())


# ---- 6: the project's own meshes ------------------------------------------------------------------------------------------------------------------------------------------------
def _restate_checked(v, f):
    tests = XC.restate_tests(v, f, v, f)
    orc = XC.oracle_tests(v, f, v, f)
    clear = ~orc["ambiguous"]
    return XC.restate(v, f, tests=tests), int(((tests["hit"] != orc["hit"]) & clear).sum()), int(orc["ambiguous"].sum()), int(orc["hit"].sum())


def test_marching_cubes_and_the_watertight_remesh():
    from jittor_myc_nerfs_amd import mesh
    n = 24
    g = torch.arange(n, dtype=torch.float32, device="cuda") - 11.37
    vol = 8.3 - torch.sqrt(g[:, None, None] ** 2 + (g[None, :, None] + 0.21) ** 2 + (g[None, None, :] - 0.4) ** 2)
    mv, mf = mesh.marching_cubes(vol.contiguous(), 0.0)
    uv, uf = XC.fixtures()["union"]
    rv, rf = mesh.remesh_watertight(_dev(uv), _dev(uf, np.int32), resolution=20)
    for what, (v, f) in (("marching cubes", (mv, mf)), ("remesh", (rv, rf))):
        assert 500 < f.shape[0] < 3000
        ref, differ, ambiguous, oracle_hits = _restate_checked(_np(v), _np(f))
        res = self_query(mesh.build_bvh(v, f))
        print(f"    {what}: {f.shape[0]} triangles, {len(res[0])} pairs on the device, {len(ref['pairs'])} restated; oracle: {oracle_hits} piercings, {ambiguous} ambiguous "
              f"tests, restatement differs from it on {differ} clear tests")
        assert XC.bits_differ(res, ref) == 0                         # device == restate, whatever the restatement finds
        assert differ == 0                                           # and the restatement is the oracle's wherever the oracle is sure
    assert len(self_query(mesh.build_bvh(mv, mf))[0]) == 0           # a sphere's iso-surface does not cut through itself


# ---- 7: mesh_check and the command line -----------------------------------------------------------------------------------------------------------------------------------------
def test_mesh_check_on_the_union():
    from jittor_myc_nerfs_amd import mesh
    v, f = XC.fixtures()["union"]
    rep = mesh.mesh_check(_dev(v), _dev(f, np.int32))
    ref = XC.reference("union")["restate"]
    length = float(np.linalg.norm(ref["points"][:, 1].astype(np.float64) - ref["points"][:, 0], axis=1).sum())
    assert rep["vertices"] == len(v) and rep["triangles"] == 1920 and rep["closed"] is True and rep["components"] == 2
    assert all(rep[k] == 0 for k in mesh.CLOSEDNESS_COUNTERS)         # the counters call it closed; the crossings say why it is not usable
    assert rep["crossing_pairs"] == 164 and rep["crossing_faces"] == 164 and rep["n_pierce_histogram"] == {2: 164}
    assert abs(rep["crossing_length"] - length) <= 1e-12 * length and length > 1.0
    json.dumps(rep)


def test_command_line_writes_the_check_and_leaves_everything_else_alone(tmp_path, capsys):
    from jittor_myc_nerfs_amd import mesh, reconstruct as R
    v, f = XC.fixtures()["union"]
    s = NC.sphere_mesh("sphere960")
    a, ref = str(tmp_path / "union.ply"), str(tmp_path / "unit.ply")
    mesh.write_ply(a, v, f)
    mesh.write_ply(ref, s[0], s[1])
    dist = R.main(["--mesh_file", a, "--mesh_compare", ref])
    before = {n: open(tmp_path / n, "rb").read() for n in sorted(os.listdir(tmp_path))}
    assert R.main(["--mesh_file", a, "--mesh_compare", ref, "--mesh_check", "0"]) == dist
    assert {n: open(tmp_path / n, "rb").read() for n in sorted(os.listdir(tmp_path))} == before        # 0: no new file, every byte as it was
    out = R.main(["--mesh_file", a, "--mesh_check", "1"])
    assert out == str(tmp_path / "union_check.json") and "crossing pairs" in capsys.readouterr().out
    assert sorted(os.listdir(tmp_path)) == sorted(list(before) + ["union_check.json"])
    rep = json.loads(open(out).read())
    assert rep["mesh_file"] == a and rep["crossing_pairs"] == 164 and rep["crossing_faces"] == 164 and rep["triangles"] == 1920 and rep["components"] == 2
    assert rep["crossing_length_unit"] == "world" and "crossing_length_voxels" not in rep and rep["n_pierce_histogram"] == {"2": 164}
    R.main(["--mesh_file", a, "--mesh_check", "1", "--mesh_check_curves", "1"])
    assert sorted(os.listdir(tmp_path)) == sorted(list(before) + ["union_check.json", "union_crossings.obj"])
    lines = open(tmp_path / "union_crossings.obj").read().split("\n")
    assert sum(x.startswith("v ") for x in lines) == 328 and sum(x.startswith("l ") for x in lines) == 164
    assert all(open(tmp_path / n, "rb").read() == x for n, x in before.items())
    assert R.main(["--mesh_file", a, "--mesh_compare", ref, "--mesh_check", "1"]) == dist and open(dist, "rb").read() == before[os.path.basename(dist)]
