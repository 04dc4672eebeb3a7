"""GPU: the closest-point query and the distance between two meshes (csrc/tvr_mesh_bvh.hip bv_nearest_kernel, include/tvr.h tvr_mesh_bvh_nearest; mesh.closest_points /
surface_samples / mesh_distance, reconstruct --mesh_compare) — dist, tri and bary bit for bit against the numpy fp32 restatement of tests/mesh_nearest_common.py on
every point with no exemption, witness checks against the fp64 oracle within DIST_BAR, vertices at exactly 0, the tie rule, max_dist, refusals, batching, the fault
paths (argument and flag checks: nothing is provoked), the work the hierarchy saves, mesh_distance against derived bounds, and the command line end to end.
The references are computed once per process and shared."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_nearest_common as NC
import mesh_raster_common as RC
from conftest import TINY, make_model
from test_gpu_mesh_bvh import _nan_vertex, _small

pytestmark = pytest.mark.gpu

MESHES = ("sphere960", "sphere6240", "tripled960", "mc96")
_cache = {}


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def built(name):
    """(verts, faces, MeshBVH) of a named mesh, built once"""
    from jittor_myc_nerfs_amd import mesh
    if ("bvh", name) not in _cache:
        if name == "mc96":
            vt, ft = RC.mc_sphere("cuda", n=96)
            v, f = _np(vt), _np(ft)
        else:
            v, f = NC.sphere_mesh(name)
        _cache[("bvh", name)] = (v, f, mesh.build_bvh(_dev(v), _dev(f, np.int32)))
    return _cache[("bvh", name)]


def sets_of(name):
    return NC.SETS + ("displaced",) if name == "mc96" else NC.SETS


def refs(name, kind):
    """(points, restate, oracle) of one fixture and point set: 4 096 points per set on the spheres, 1 024 on mc96"""
    if ("ref", name, kind) not in _cache:
        v, f = built(name)[:2]
        if name == "mc96":
            p = NC.point_set(name, kind, v, f, n=1024, centre=NC.MC96_CENTRE)
        elif name == "tripled960":
            p = refs("sphere960", kind)[0]                           # the single sphere's points: the answers must be the single sphere's
        else:
            p = NC.point_set(name, kind, v, f)
        _cache[("ref", name, kind)] = (p, NC.restate(v, f, p), NC.oracle(v, f, p))
    return _cache[("ref", name, kind)]


def nearest(bvh, p, **kw):
    from jittor_myc_nerfs_amd import mesh
    return tuple(_np(x) for x in mesh.closest_points(bvh, _dev(p), **kw))


def _missed(res, n=None):
    d, t, b = res
    return bool(np.isposinf(d).all() and (t == -1).all() and (b == 0).all() and (n is None or len(d) == n))


# ---- both references ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_bit_equal_to_the_restatement_on_every_point(name):
    v, f, bvh = built(name)
    for kind in sets_of(name):
        p, ref, _ = refs(name, kind)
        st = {}
        res = nearest(bvh, p, stats=st)
        diff = NC.bits_differ(res, ref)
        print(f"    {name} {kind}: {len(p)} points, bits differing from the restatement {diff}; per point {st['node_tests'] / len(p):.1f} node tests, "
              f"{st['triangle_tests'] / len(p):.2f} triangle tests (F = {len(f)})")
        assert diff == 0                                             # dist, tri and bary, every point, no exemption
        assert st["points_answered"] == len(p) and st["points_refused"] == 0 and (res[1] >= 0).all()
        if name == "tripled960":
            assert (res[1] < 960).all()                              # the tie rule: never t + 960 or t + 1920
            assert NC.bits_differ(res, refs("sphere960", kind)[1]) == 0


@pytest.mark.parametrize("name", MESHES)
def test_within_the_bar_of_the_oracle_on_every_point(name):
    v, f, bvh = built(name)
    seen = []
    for kind in sets_of(name):
        p, ref, orc = refs(name, kind)
        res = nearest(bvh, p)
        w, wr = NC.witness(v, f, p, res, orc), NC.witness(v, f, p, ref, orc)
        print(f"    {name} {kind}: kernel {w}; restatement dist_err {wr['dist_err']:.3g} (DIST_MEASURED {NC.DIST_MEASURED:g}, DIST_BAR {NC.DIST_BAR:g})")
        seen.append((kind, len(p), w, wr))
    for kind, n, w, wr in seen:                                      # (every figure is printed before the first assertion)
        assert w["answered"] == n, kind
        assert wr["dist_err"] <= NC.DIST_MEASURED, kind              # the measurement DIST_BAR is 4 x of
        assert w["dist_err"] <= NC.DIST_BAR, kind                    # the distance
        assert w["tri_err"] <= NC.DIST_BAR, kind                     # the NAMED triangle is a witness of the fp64 minimum
        assert w["point_err"] <= NC.DIST_BAR, kind                   # and so is the point that bary reconstructs


@pytest.mark.parametrize("name", MESHES)
def test_a_vertex_is_at_distance_zero_of_its_fans_first_triangle(name):
    v, f, bvh = built(name)
    fan = NC.fan_smallest(f, len(v))
    used = fan < len(f)                                              # (marching cubes leaves no vertex unused; stated, not assumed)
    d, t, b = nearest(bvh, v)
    assert used.all() and (d == 0.0).all() and np.array_equal(t, fan)
    assert (np.sort(b, 1) == np.float32([0, 0, 1])).all()            # a corner's weights


# ---- the small fixtures ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_small_empty_and_nan_meshes_and_refused_points():
    from jittor_myc_nerfs_amd import mesh
    p = NC.point_set("sphere960", "outer", np.zeros((0, 3)), np.zeros((0, 3)), n=512)
    for F in (1, 2, 3):
        v, f = _small(F)
        bvh = mesh.build_bvh(_dev(v), _dev(f, np.int32))
        ref = NC.restate(v, f, p)
        assert NC.bits_differ(nearest(bvh, p), ref) == 0 and (ref["tri"] >= 0).all()
        assert _missed(nearest(bvh, p, max_dist=1e-4), len(p))       # nothing that near: +inf / -1 / 0
    empty = mesh.build_bvh(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    st = {}
    assert _missed(nearest(empty, p, stats=st), len(p)) and st["points_answered"] == 0 and st["triangle_tests"] == 0
    assert _missed(nearest(empty, np.zeros((0, 3), np.float32)), 0)
    # a NaN vertex: its triangles are never named, and the answers are those of the mesh without them
    v, f = _nan_vertex()
    clean = RC.sphere_fixture("sphere960")[0]
    gone = np.flatnonzero((f == 17).any(1))
    q = np.concatenate([p, clean[17][None] * np.float32([[0.9], [1.0], [1.2]])]).astype(np.float32)
    bvh = mesh.build_bvh(_dev(v), _dev(f, np.int32))
    res = nearest(bvh, q)
    assert not np.isin(res[1], gone).any() and (res[1] >= 0).all()
    assert NC.bits_differ(res, NC.restate(v, f, q)) == 0 and NC.bits_differ(res, NC.restate(clean, f, q, drop_triangle=gone)) == 0
    # refused points are counted and answered with +inf / -1 / 0; their neighbours are not disturbed
    v, f, bvh = built("sphere960")
    _, ref, _ = refs("sphere960", "outer")
    q = refs("sphere960", "outer")[0][:64].copy()
    q[0, 0], q[1, 2], q[2, 1], q[3] = np.nan, np.inf, -np.inf, np.nan
    st = {}
    res = nearest(bvh, q, stats=st)
    assert st["points_refused"] == 4 and st["points_answered"] == 60 and _missed(tuple(x[:4] for x in res))
    assert NC.bits_differ(tuple(x[4:] for x in res), {k: ref[k][4:64] for k in ("dist", "tri", "bary")}) == 0


# ---- max_dist, batching, order ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_max_dist():
    v, f, bvh = built("sphere960")
    p = np.concatenate([refs("sphere960", "outer")[0], refs("sphere960", "inner")[0][:1000], v[:100]])
    ref = NC.restate(v, f, p)
    med = np.float32(np.median(ref["dist"]))
    st = {}
    res = nearest(bvh, p, max_dist=float(med), stats=st)
    inside = ref["D"] <= med * med                                   # fp32, as the definition has it
    assert 1000 < inside.sum() < len(p) - 1000 and st["points_answered"] == int(inside.sum())
    assert np.array_equal(res[1] >= 0, inside) and NC.bits_differ(res, NC.restate(v, f, p, max_dist=med)) == 0
    assert NC.bits_differ(tuple(x[inside] for x in res), {k: ref[k][inside] for k in ("dist", "tri", "bary")}) == 0 and _missed(tuple(x[~inside] for x in res))
    # exactly at a point's own distance it is answered; at the float below its square root's square it may not be — ask the restatement
    for i in np.flatnonzero(inside)[:8]:
        one = nearest(bvh, p[i:i + 1], max_dist=float(ref["dist"][i]))
        assert NC.bits_differ(one, NC.restate(v, f, p[i:i + 1], max_dist=ref["dist"][i])) == 0
    zero = nearest(bvh, p, max_dist=0.0)
    assert np.array_equal(zero[1] >= 0, ref["dist"] == 0.0) and (zero[1] >= 0).sum() >= 100 and (zero[0][zero[1] >= 0] == 0).all()
    assert np.array_equal(zero[1][zero[1] >= 0], ref["tri"][ref["dist"] == 0.0])


def test_order_batching_and_two_runs(monkeypatch):
    from jittor_myc_nerfs_amd import mesh
    v, f, bvh = built("sphere6240")
    p = np.concatenate([refs("sphere6240", k)[0] for k in ("outer", "far", "centre", "features")])
    base = nearest(bvh, p)
    again = nearest(bvh, p)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(base, again))
    perm = np.random.default_rng(7).permutation(len(p))
    shuffled = nearest(bvh, p[perm])
    assert all(np.array_equal(a.view(np.uint32), b[perm].view(np.uint32)) for a, b in zip(shuffled, base))
    monkeypatch.setattr(mesh, "BVH_NEAREST_CHUNK", 1000)
    st = {}
    pieces = nearest(bvh, p, stats=st)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(pieces, base)) and st["points_answered"] == len(p)


# ---- fault paths: argument and flag checks only -----------------------------------------------------------------------------------------------------------------------------------
def test_foreign_blob_undersized_outputs_and_guard_bytes():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    v, f, small = built("sphere960")
    big = built("sphere6240")[2]
    p = refs("sphere960", "outer")[0][:300]
    # the blob of another mesh (large enough, so the size check passes): the header says F = 6240, the call F = 960 — the flag is raised and no tree is walked
    foreign = mesh.MeshBVH(big.blob, small.verts, small.faces, 0, 0)
    with pytest.raises(L.TvrError, match="fault flag"):
        mesh.closest_points(foreign, _dev(p))
    # ... and a blob that is too small is refused on the host
    with pytest.raises(L.TvrError, match="bvh"):
        mesh.closest_points(mesh.MeshBVH(small.blob, big.verts, big.faces, 0, 0), _dev(p))
    lib, N, G = L.lib(), len(p), 64
    pd = _dev(p)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    dist = torch.full((N + G,), -7.0, device="cuda")
    tri = torch.full((N + G,), -7, dtype=torch.int32, device="cuda")
    bary = torch.full((N + G, 3), -7.0, device="cuda")

    def call(n, db, tb, bb):
        return lib.tvr_mesh_bvh_nearest(small.verts.data_ptr(), small.n_vertices, small.faces.data_ptr(), small.n_triangles, small.blob.data_ptr(), small.blob.numel(),
                                        pd.data_ptr(), n, float("inf"), dist.data_ptr(), db, tri.data_ptr(), tb, bary.data_ptr(), bb, None, flag.data_ptr(), None)
    for db, tb, bb in ((4 * N - 1, 4 * N, 12 * N), (4 * N, 4 * N - 4, 12 * N), (4 * N, 4 * N, 12 * N - 1)):
        assert call(N, db, tb, bb) == -3                              # TVR_ERR_SCRATCH before any launch
    torch.cuda.synchronize()
    assert bool((dist == -7).all()) and bool((tri == -7).all()) and bool((bary == -7).all())
    # N rows are written, the guard rows behind them keep their sentinel
    assert call(N, 4 * N, 4 * N, 12 * N) == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    assert bool((dist[N:] == -7).all()) and bool((tri[N:] == -7).all()) and bool((bary[N:] == -7).all())
    ref = NC.restate(v, f, p)
    assert NC.bits_differ((_np(dist[:N]), _np(tri[:N]), _np(bary[:N])), ref) == 0


# ---- the hierarchy saves work -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_hierarchy_saves_work():
    """A tree that degenerated into a list would pass every correctness test: mean triangle tests per point must stay below F / 10.  `centre` is left out on purpose:
    from the centre of a sphere every triangle is about equally far, no bound can prune, and the kernel rightly tests nearly all of them."""
    v, f, bvh = built("sphere6240")
    p = np.concatenate([refs("sphere6240", "inner")[0], refs("sphere6240", "outer")[0]])
    st = {}
    nearest(bvh, p, stats=st)
    per_point = st["triangle_tests"] / len(p)
    print(f"    sphere6240 inner + outer: {per_point:.2f} triangle tests and {st['node_tests'] / len(p):.1f} node tests per point (F = {len(f)})")
    assert per_point < len(f) / 10
    st = {}
    nearest(bvh, refs("sphere6240", "centre")[0], stats=st)
    print(f"    sphere6240 centre: {st['triangle_tests'] / 8:.0f} triangle tests per point (not asserted)")


# ---- mesh_distance ------------------------------------------------------------------------------------------------------------------------------------------------------------------
FIGURES = ("max", "mean", "rms", "median", "p95")


def test_distance_of_a_mesh_to_itself_and_to_its_translate():
    from jittor_myc_nerfs_amd import mesh
    v, f, bvh = built("sphere960")
    vd, fd = _dev(v), _dev(f, np.int32)
    st = {}
    same = mesh.mesh_distance(vd, fd, vd, fd, bvh_a=bvh, bvh_b=bvh, stats=st)
    diag = float(np.linalg.norm(v.max(0).astype(np.float64) - v.min(0)))
    print(f"    sphere960 against itself: {same}")
    assert same["hausdorff"] < NC.DIST_BAR * diag and same["a_to_b"] == same["b_to_a"] and same["a_to_b"]["refused"] == 0
    assert same["a_to_b"]["samples"] == 4 * len(f) + len(v) and st["points_answered"] == 2 * same["a_to_b"]["samples"]
    one = mesh.mesh_distance(vd, fd, vd, fd, symmetric=False)
    assert set(one) == {"a_to_b"} and one["a_to_b"] == same["a_to_b"]
    delta = 0.05
    v2 = (v + np.float32([delta, 0, 0])).astype(np.float32)
    got = mesh.mesh_distance(vd, fd, _dev(v2), fd, unit=0.5)
    edge = NC.longest_edge(v, f)
    for side, (va, vb) in (("a_to_b", (v, v2)), ("b_to_a", (v2, v))):
        pts, w = mesh.surface_samples(_dev(va), fd, 2)
        want = NC.statistics(NC.oracle(vb, f, _np(pts))["dist"], _np(w), unit=0.5)
        print(f"    translated by {delta}, {side}: {got[side]}")
        assert got[side]["samples"] == want["samples"] and got[side]["refused"] == 0
        for k in FIGURES:
            assert abs(got[side][k] - want[k]) <= NC.DIST_BAR * max(want[k] * 0.5, edge) / 0.5, (side, k, got[side][k], want[k])
    assert got["hausdorff"] == max(got["a_to_b"]["max"], got["b_to_a"]["max"]) and got["chamfer"] == 0.5 * (got["a_to_b"]["mean"] + got["b_to_a"]["mean"])
    assert 0 < got["hausdorff"] * 0.5 <= delta * (1 + 1e-4)          # every point of one convex copy has its translate in the other


def test_distance_of_a_clustered_mesh_stays_within_a_cell_diagonal():
    """simplify_clustering replaces every vertex by the mean of the vertices of its own cell, which lies within a cell diagonal of it; a point of a surviving triangle
    is the same convex combination of the moved corners, so it too moved by at most a cell diagonal: a derived bound on simplified -> original, not a measured one."""
    from jittor_myc_nerfs_amd import mesh
    v, f, bvh = built("mc96")
    vd, fd = _dev(v), _dev(f, np.int32)
    cell = 2 * NC.MC96_VOXEL
    vs, fs, _ = mesh.simplify_clustering(vd, fd, cell, origin=NC.MC96_ORIGIN)
    got = mesh.mesh_distance(vs, fs, vd, fd, unit=NC.MC96_VOXEL, bvh_b=bvh)
    print(f"    mc96 {len(f)} -> {fs.shape[0]} triangles, in voxels: simplified -> original {got['a_to_b']}; original -> simplified (not asserted) {got['b_to_a']}")
    assert 0 < fs.shape[0] < len(f) // 2
    assert 0 < got["a_to_b"]["max"] <= 2 * np.sqrt(3.0) * (1 + 1e-4) and got["a_to_b"]["refused"] == 0 and got["b_to_a"]["refused"] == 0
    assert got["a_to_b"]["median"] <= got["a_to_b"]["p95"] <= got["a_to_b"]["max"] and got["a_to_b"]["mean"] <= got["a_to_b"]["rms"] <= got["a_to_b"]["max"]


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_command_line_compares_two_exports(tiny_arrays, tmp_path, capsys):
    from jittor_myc_nerfs_amd import reconstruct as R, synthetic
    m = make_model(tiny_arrays, dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=TINY["step_ratio"]))
    alpha = m.getDenseAlpha()[0]
    level = 0.5 * (float(alpha.min()) + float(alpha.max()))
    ckpt = tmp_path / "tiny.th"
    m.save(str(ckpt))
    cmd = ["--export_mesh", "1", "--ckpt", str(ckpt), "--model_name", "TensorVMSplit", "--mesh_level", repr(level)]
    out = R.main(cmd)
    plain = (tmp_path / "tiny.ply").read_bytes()
    m.export_mesh(str(tmp_path / "direct.ply"), level=level)
    assert plain == (tmp_path / "direct.ply").read_bytes()           # without --mesh_compare every byte is what export_mesh writes,
    assert "tiny_distance.json" not in os.listdir(tmp_path)          # and no comparison is written
    (tmp_path / "plain.ply").write_bytes(plain)
    assert R.main(cmd + ["--mesh_simplify", "2", "--mesh_compare", str(tmp_path / "plain.ply")]) == out
    m.export_mesh(str(tmp_path / "direct.ply"), level=level, simplify=2.0)
    assert (tmp_path / "tiny.ply").read_bytes() == (tmp_path / "direct.ply").read_bytes()      # the comparison does not touch the mesh file
    assert "distance of" in capsys.readouterr().out
    rep = json.loads((tmp_path / "tiny_distance.json").read_text())
    assert rep["mesh_file"] == out and rep["reference_file"] == str(tmp_path / "plain.ply")
    vp, fp = R._read_mesh_geometry(str(tmp_path / "plain.ply"))
    vs, fs = R._read_mesh_geometry(out)
    assert (rep["vertices"], rep["triangles"], rep["reference_vertices"], rep["reference_triangles"]) == (len(vs), len(fs), len(vp), len(fp)) and len(fs) < len(fp)
    unit = float(R.mesh_export_voxel(m).min())
    assert rep["voxel_unit"] == unit and len(rep["voxel"]) == 3
    world, vox = rep["world"], rep["voxels"]
    assert np.isfinite(vox["hausdorff"]) and vox["hausdorff"] > 0 and vox["hausdorff"] == pytest.approx(world["hausdorff"] / unit, rel=1e-5)
    cell, _ = m.mesh_simplify_lattice(alpha.shape, "reference", 2.0)
    print(f"    tiny scene, simplify 2, in export voxels: {vox}")
    assert vox["a_to_b"]["max"] <= float(np.linalg.norm(cell)) / unit * (1 + 1e-4)         # simplified -> plain: the cell-diagonal bound
    # without a checkpoint: --mesh_file against the reference, world units only
    os.remove(tmp_path / "tiny_distance.json")
    assert R.main(["--mesh_file", out, "--mesh_compare", str(tmp_path / "plain.ply")]) == str(tmp_path / "tiny_distance.json")
    rep2 = json.loads((tmp_path / "tiny_distance.json").read_text())
    assert rep2["world"] == world and "voxels" not in rep2
