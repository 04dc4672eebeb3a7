"""No GPU: what of the closest-point query (include/tvr.h tvr_mesh_bvh_nearest, mesh.closest_points / surface_samples / mesh_distance, reconstruct --mesh_compare) can
be checked without a device: the declaration, the C call's argument errors (host pointers that are never followed), the signatures and the parser, the restatement of
the definition (tests/mesh_nearest_common.py) against the fp64 oracle on the fixtures the GPU tests use — which is where DIST_BAR comes from — surface_samples and the
weighted quantile."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mesh_nearest_common as NC
import mesh_raster_common as RC
from conftest import ROOT

INVALID, SCRATCH, UNSUPPORTED = -1, -3, -4
MAX_F = 1 << 30
MESHES = ("sphere960", "sphere6240", "tripled960")


def _aligned(n):
    buf = (C.c_uint8 * (n + 256))()
    a = C.addressof(buf)
    return buf, (a + 255) // 256 * 256


def _up(x):
    return (x + 255) // 256 * 256


def _blob_bytes(F):
    return 256 + _up(24 * (2 * F - 1 if F else 0)) + _up(8 * max(F - 1, 0)) + _up(4 * F)


def _call(lib, **kw):
    keep, p = _aligned(1 << 16)
    F, V, N = kw.pop("F", 4), kw.pop("V", 6), kw.pop("N", 5)
    a = dict(verts=p, faces=p, bvh=p, bvh_bytes=_blob_bytes(max(F, 0)) if F <= 1000 else 1 << 16, points=p, max_dist=float("inf"), dist=p, dist_bytes=4 * N, tri=p,
             tri_bytes=4 * N, bary=p, bary_bytes=12 * N, counts=p, flag=p)
    a.update(kw)
    rc = lib.tvr_mesh_bvh_nearest(a["verts"], V, a["faces"], F, a["bvh"], a["bvh_bytes"], a["points"], N, a["max_dist"], a["dist"], a["dist_bytes"], a["tri"],
                                  a["tri_bytes"], a["bary"], a["bary_bytes"], a["counts"], a["flag"], None)
    return rc, lib.tvr_last_error().decode()


# ---- the surface ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_symbol_table_and_package_agree():
    import jittor_myc_nerfs_amd as pkg
    from jittor_myc_nerfs_amd import _lib as L, mesh
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tvr.h")).read(), flags=re.S)
    m = re.search(r"int\s+tvr_mesh_bvh_nearest\s*\(([^;]*)\)\s*;", src)
    assert m, "include/tvr.h does not declare tvr_mesh_bvh_nearest"
    params = [" ".join(x.split()) for x in m.group(1).split(",")]
    assert params == ["const float *verts", "int64_t n_vertices", "const int32_t *faces", "int64_t n_triangles", "const void *bvh", "size_t bvh_bytes",
                      "const float *points", "int64_t n_points", "float max_dist", "float *dist", "size_t dist_bytes", "int32_t *tri", "size_t tri_bytes", "float *bary",
                      "size_t bary_bytes", "int64_t *counts_dev", "uint32_t *fault_flag_dev", "void *stream"]
    res, args = L.SYMBOLS["tvr_mesh_bvh_nearest"]
    assert res is C.c_int and len(args) == 18 and args[8] is C.c_float and args[7] is C.c_int64 and args[5] is C.c_size_t
    assert L.lib().tvr_version() == 141                              # an additive export
    assert hasattr(L.lib(), "tvr_mesh_bvh_nearest")
    for name in ("closest_points", "surface_samples", "mesh_distance"):
        assert getattr(pkg, name) is getattr(mesh, name)


def test_signatures_and_defaults():
    from jittor_myc_nerfs_amd import mesh
    p = inspect.signature(mesh.closest_points).parameters
    assert list(p) == ["bvh", "points", "max_dist", "stats"] and p["max_dist"].default == float("inf") and p["stats"].default is None
    p = inspect.signature(mesh.surface_samples).parameters
    assert list(p) == ["verts", "faces", "subdiv"] and p["subdiv"].default == 2
    p = inspect.signature(mesh.mesh_distance).parameters
    assert list(p) == ["verts_a", "faces_a", "verts_b", "faces_b", "subdiv", "symmetric", "unit", "bvh_a", "bvh_b", "stats"]
    assert [p[k].default for k in ("subdiv", "symmetric", "unit", "bvh_a", "bvh_b", "stats")] == [2, True, 1.0, None, None, None]
    assert mesh.BVH_NEAREST_CHUNK == 1 << 24
    # the signatures this feature must leave alone
    assert list(inspect.signature(mesh.MeshBVH.__init__).parameters) == ["self", "blob", "verts", "faces", "height", "triangles_skipped"]
    assert list(inspect.signature(mesh.build_bvh).parameters) == ["verts", "faces", "stats"]
    assert list(inspect.signature(mesh.cast_rays).parameters) == ["bvh", "rays_or_origins", "dirs", "t_min", "t_max", "any_hit", "cull", "stats"]
    assert list(inspect.signature(mesh.ambient_occlusion).parameters) == ["bvh", "normals", "n_dirs", "bias", "t_max", "points", "dirs", "stats"]


@pytest.mark.parametrize("kw, code, word", [
    (dict(verts=None), INVALID, "verts"),
    (dict(faces=None), INVALID, "faces"),
    (dict(bvh=None), INVALID, "bvh"),
    (dict(points=None), INVALID, "points"),
    (dict(dist=None), INVALID, "dist"),
    (dict(tri=None), INVALID, "tri"),
    (dict(bary=None), INVALID, "bary"),
    (dict(flag=None), INVALID, "fault_flag_dev"),
    (dict(N=-1), INVALID, "n_points"),
    (dict(F=-1), INVALID, "n_triangles"),
    (dict(V=-1), INVALID, "n_vertices"),
    (dict(max_dist=float("nan")), INVALID, "max_dist"),
    (dict(max_dist=-1.0), INVALID, "max_dist"),
    (dict(max_dist=float("-inf")), INVALID, "max_dist"),
    (dict(N=1 << 31), UNSUPPORTED, "n_points"),
    (dict(V=1 << 31), UNSUPPORTED, "n_vertices"),
    (dict(F=MAX_F + 1), UNSUPPORTED, "TVR_MESH_BVH_MAX_TRIANGLES"),
    (dict(bvh_bytes=_blob_bytes(4) - 1), SCRATCH, "bvh"),
    (dict(dist_bytes=19), SCRATCH, "dist [n_points]"),
    (dict(tri_bytes=19), SCRATCH, "tri [n_points]"),
    (dict(bary_bytes=59), SCRATCH, "bary [n_points,3]"),
])
def test_c_argument_errors_come_before_any_launch(kw, code, word):
    from jittor_myc_nerfs_amd import _lib as L
    rc, msg = _call(L.lib(), **kw)
    assert rc == code, (rc, msg)
    assert word in msg and "tvr_mesh_bvh_nearest" in msg, msg


def test_misaligned_blob_is_refused_and_empty_calls_are_accepted():
    from jittor_myc_nerfs_amd import _lib as L
    keep, p = _aligned(1 << 16)
    rc, msg = _call(L.lib(), bvh=p + 4)
    assert rc == INVALID and "aligned" in msg, (rc, msg)
    rc, msg = _call(L.lib(), N=0, points=None, dist=None, tri=None, bary=None, counts=None)       # no point: nothing is launched
    assert rc == 0, msg
    rc, msg = _call(L.lib(), F=0, N=0, verts=None, faces=None, points=None, dist=None, tri=None, bary=None, counts=None, max_dist=0.0)
    assert rc == 0, msg


def test_no_cpu_fallback():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    v, f = RC.latlong_sphere(4, 6)
    bvh = mesh.MeshBVH(torch.zeros(256, dtype=torch.uint8, device="meta"), torch.from_numpy(v), torch.from_numpy(f), 0, 0)
    with pytest.raises(L.TvrError, match="no CPU fallback"):
        mesh.closest_points(bvh, torch.zeros((4, 3)))
    with pytest.raises(L.TvrError, match="MeshBVH"):
        mesh.closest_points(None, torch.zeros((4, 3)))
    with pytest.raises(L.TvrError, match="no CPU fallback"):
        mesh.mesh_distance(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(ValueError, match="unit"):
        mesh.mesh_distance(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(v), torch.from_numpy(f), unit=0.0)


def test_parser():
    from jittor_myc_nerfs_amd import reconstruct
    a = reconstruct.config_parser([])
    assert a.mesh_compare is None
    a = reconstruct.config_parser(["--mesh_compare", "plain.ply", "--mesh_file", "x.obj"])
    assert a.mesh_compare == "plain.ply" and a.mesh_file == "x.obj" and a.export_mesh == 0
    with pytest.raises(SystemExit, match="mesh_file"):
        reconstruct.main(["--mesh_compare", "plain.ply"])             # neither an export nor a --mesh_file: refused before anything runs


# ---- the restatement against the oracle -----------------------------------------------------------------------------------------------------------------------------------------
_cache = {}


def references(name, kind):
    """(verts, faces, points, restate, oracle) of one fixture and point set, computed once per process"""
    if (name, kind) not in _cache:
        v, f = NC.sphere_mesh(name)
        p = NC.point_set(name, kind, v, f)
        _cache[(name, kind)] = (v, f, p, NC.restate(v, f, p), NC.oracle(v, f, p))
    return _cache[(name, kind)]


@pytest.mark.parametrize("name", MESHES)
def test_restatement_is_a_witness_of_the_oracles_minimum(name):
    """Where DIST_BAR comes from: the largest |dist32 - dist64| / max(dist64, longest edge) over every fixture and set is DIST_MEASURED (mc96 needs the marching cubes
    and is measured by the GPU test).  Nothing is exempted: the named triangle and the reconstructed point lie within the bar of the fp64 minimum for every point."""
    worst = 0.0
    for kind in NC.SETS:
        v, f, p, ref, orc = references(name, kind)
        w = NC.witness(v, f, p, ref, orc)
        worst = max(worst, w["dist_err"])
        print(f"    {name} {kind}: {len(p)} points, {w}, triangle named as by the oracle {float((ref['tri'] == orc['tri']).mean()):.3f}")
        assert w["answered"] == len(p) and np.isfinite(orc["dist"]).all()
        assert w["dist_err"] <= NC.DIST_MEASURED and NC.DIST_BAR >= 4 * NC.DIST_MEASURED
        assert w["tri_err"] <= NC.DIST_BAR and w["point_err"] <= NC.DIST_BAR
        b = ref["bary"]
        assert np.abs(b.sum(1) - 1).max() < 1e-6 and b.min() >= -2.0 ** -22         # ((1 - v) - w of the face region may undercut 0 by an ulp or two of 1)
    print(f"    {name}: largest distance error {worst:.3g} (DIST_MEASURED = {NC.DIST_MEASURED:g}, DIST_BAR = {NC.DIST_BAR:g})")


@pytest.mark.parametrize("name", MESHES)
def test_a_vertex_is_at_distance_zero_of_its_fans_first_triangle(name):
    v, f, p, ref, _ = references(name, "verts")
    assert np.array_equal(p, v)
    assert (ref["dist"] == 0.0).all() and np.array_equal(ref["tri"], NC.fan_smallest(f, len(v)))
    assert np.isin(ref["region"], (1, 2, 4)).all()
    if name == "tripled960":
        assert (ref["tri"] < 960).all()


@pytest.mark.parametrize("name", ["sphere960", "sphere6240"])
def test_all_seven_regions_win_somewhere(name):
    r = np.concatenate([references(name, kind)[3]["region"] for kind in ("inner", "outer", "far")])
    counts = np.bincount(r, minlength=8)
    print(f"    {name}: winners per region {dict(zip(NC.REGIONS, counts[1:].tolist()))}")
    assert counts[0] == 0 and (counts[1:] > 0).all()
    inner = references(name, "inner")[3]["region"]
    assert (inner == 7).mean() > 0.99                                # from inside the nearest point lies in a face


def test_the_comparison_can_fail():
    """The power of the bar: a restatement that pretends the winners of a few points are absent names a farther triangle, and the witness check says so."""
    v, f, p, ref, orc = references("sphere960", "outer")
    victims = np.unique(ref["tri"][:8])
    broken = NC.restate(v, f, p, drop_triangle=victims)
    w = NC.witness(v, f, p, broken, orc)
    print(f"    without triangles {victims.tolist()}: {w}")
    assert w["dist_err"] > NC.DIST_BAR and w["tri_err"] > NC.DIST_BAR and NC.bits_differ((broken["dist"], broken["tri"], broken["bary"]), ref) >= 8


def test_max_dist_refusals_and_degenerate_triangles_of_the_restatement():
    v, f, p, ref, _ = references("sphere960", "outer")
    med = np.float32(np.median(ref["dist"]))
    lim = NC.restate(v, f, p, max_dist=med)
    inside = ref["D"] <= med * med
    assert 1000 < inside.sum() < 3100 and np.array_equal(lim["tri"] >= 0, inside)
    assert NC.bits_differ((lim["dist"][inside], lim["tri"][inside], lim["bary"][inside]), {k: ref[k][inside] for k in ("dist", "tri", "bary")}) == 0
    assert np.isinf(lim["dist"][~inside]).all() and (lim["bary"][~inside] == 0).all()
    q = p[:6].copy()
    q[0, 0], q[1, 2], q[2, 1] = np.nan, np.inf, -np.inf
    r = NC.restate(v, f, q)
    assert NC.refused(q).tolist() == [True, True, True, False, False, False] and (r["tri"][:3] == -1).all() and np.array_equal(r["tri"][3:], ref["tri"][3:6])
    # a zero-area triangle never wins through region 7 (0 / 0), but its edges and corners still answer
    dv = np.asarray([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32)
    df = np.asarray([[0, 1, 2], [3, 4, 5]], np.int32)
    r = NC.restate(dv, df, np.asarray([[0.5, 1, 0], [3, 0, 1], [-1, 0, 0]], np.float32))
    assert np.isfinite(r["dist"]).all() and np.allclose(r["dist"], [1.0, np.sqrt(2.0), 1.0])
    # an empty mesh answers nothing
    r = NC.restate(np.zeros((0, 3)), np.zeros((0, 3)), p[:4])
    assert np.isinf(r["dist"]).all() and (r["tri"] == -1).all() and (r["bary"] == 0).all()


# ---- surface_samples and the statistics -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subdiv", [1, 2, 3, 5])
def test_surface_samples(subdiv):
    from jittor_myc_nerfs_amd import mesh
    v, f = RC.sphere_fixture("sphere960")[:2]
    v, f = v.copy(), f.copy()
    f[7] = [5, 5, 9]                                                  # a zero-area triangle
    n2 = subdiv * subdiv
    pts, w = mesh.surface_samples(torch.from_numpy(v), torch.from_numpy(f), subdiv)
    assert pts.dtype == torch.float32 and w.dtype == torch.float32 and tuple(pts.shape) == (len(f) * n2 + len(v), 3) and tuple(w.shape) == (len(f) * n2 + len(v),)
    p2, w2 = mesh.surface_samples(torch.from_numpy(v), torch.from_numpy(f), subdiv)
    assert torch.equal(pts, p2) and torch.equal(w, w2)               # deterministic
    pts, w = pts.numpy().astype(np.float64), w.numpy().astype(np.float64)
    assert np.array_equal(pts[len(f) * n2:], v) and (w[len(f) * n2:] == 0).all()
    c = v.astype(np.float64)[f]
    area = 0.5 * np.linalg.norm(np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]), axis=1)
    assert abs(w.sum() - area.sum()) <= 1e-5 * area.sum()
    assert (w[7 * n2:8 * n2] == 0).all() and (np.delete(w[:len(f) * n2].reshape(len(f), n2), 7, 0) > 0).all()
    assert np.allclose(w[:len(f) * n2].reshape(len(f), n2), area[:, None] / n2, rtol=1e-5, atol=0)
    # the points are the sub-triangle centroids, in order: on their triangles, inside, and their mean is the triangle's centroid
    bw = NC.subdivision_weights(subdiv)
    assert np.allclose(mesh.subdivision_weights(subdiv), bw, atol=1e-15) and bw.min() > 0 and len(bw) == n2 and len(np.unique(bw.round(12), axis=0)) == n2
    want = (bw[None, :, :, None] * c[:, None, :, :]).sum(2)
    assert np.abs(pts[:len(f) * n2].reshape(len(f), n2, 3) - want).max() <= 4e-7
    for t in (0, 7, 500):
        d = NC.pair_distance64(pts[t * n2:(t + 1) * n2], *[np.broadcast_to(c[t, k], (n2, 3)) for k in range(3)])
        assert d.max() <= 4e-7


def test_weighted_quantile_on_a_hand_made_example():
    from jittor_myc_nerfs_amd import mesh
    d = torch.tensor([5.0, 1.0, 3.0, 2.0, 4.0, 9.0])
    w = torch.tensor([1.0, 1.0, 2.0, 4.0, 2.0, 0.0])                  # sorted by distance: 1 (1), 2 (4), 3 (2), 4 (2), 5 (1), 9 (0); cumulative 1, 5, 7, 9, 10, 10
    q = mesh.weighted_quantile(d, w, (0.1, 0.11, 0.5, 0.7, 0.71, 0.95, 1.0)).tolist()
    assert q == [1.0, 2.0, 2.0, 3.0, 4.0, 5.0, 5.0]                  # the weightless 9 never decides, not even at q = 1
    for qq, want in zip((0.1, 0.11, 0.5, 0.7, 0.71, 0.95, 1.0), q):
        assert NC.weighted_quantile(d.numpy(), w.numpy(), qq) == want
    st = dict(zip(mesh.DISTANCE_STATISTICS, mesh.distance_statistics(torch.cat([d, torch.tensor([float("inf")])]), torch.cat([w, torch.tensor([3.0])]), unit=2.0).tolist()))
    assert st["max"] == 4.5 and st["median"] == 1.0 and st["p95"] == 2.5 and st["samples"] == 7 and st["refused"] == 1
    assert st["mean"] == pytest.approx((1 + 8 + 6 + 8 + 5) / 10 / 2) and st["rms"] == pytest.approx(np.sqrt((1 + 16 + 18 + 32 + 25) / 10) / 2)
    ref = NC.statistics(np.append(d.numpy(), np.inf), np.append(w.numpy(), 3.0), unit=2.0)
    assert all(st[k] == pytest.approx(ref[k]) for k in mesh.DISTANCE_STATISTICS)
    assert torch.isnan(mesh.weighted_quantile(d, torch.zeros(6), (0.5,))).all()
