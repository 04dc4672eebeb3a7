"""No GPU: what of the signed distance (include/tvr.h tvr_mesh_pseudonormals_* / tvr_mesh_bvh_signed; mesh.build_pseudonormals / signed_distance / contains /
signed_distance_grid / signed_mesh_distance, reconstruct --mesh_compare_signed) can be checked without a device: the declarations against the ctypes table, the
C calls' argument errors (host pointers that are never followed: every error is raised before a launch), *_bytes against *_describe, the signatures and the parser,
the statistics — and the POWER of the GPU test's fixture: on the spiked sphere the restated sign (tests/mesh_signed_common.py) agrees with a winding-number oracle at
every point, the two shortcuts (face normals, unweighted vertex normals) do not, and the restated sign's margin is far above fp32 rounding, which is what lets the GPU
test compare every point with none excluded.  The measurement behind VERT_ANGLE_BAR is asserted here too."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mesh_nearest_common as NC
import mesh_signed_common as SC
from conftest import ROOT
from test_mesh_nearest_host import _aligned, _blob_bytes, _up

INVALID, SCRATCH, UNSUPPORTED = -1, -3, -4
MAX_F = 1 << 30


def _table_bytes(V, F):
    return 256 + _up(12 * F) + _up(36 * F) + _up(12 * V)


# ---- the surface ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_symbol_table_and_package_agree():
    import jittor_myc_nerfs_amd as pkg
    from jittor_myc_nerfs_amd import _lib as L, mesh
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tvr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tvr_mesh_pseudonormals_[a-z_]+|tvr_mesh_bvh_signed)\s*\(", src))
    assert declared == {"tvr_mesh_pseudonormals_bytes", "tvr_mesh_pseudonormals_scratch_bytes", "tvr_mesh_pseudonormals_describe", "tvr_mesh_pseudonormals_keys",
                        "tvr_mesh_pseudonormals_build", "tvr_mesh_bvh_signed"}
    assert declared <= set(L.SYMBOLS)
    lib = L.lib()
    assert lib.tvr_version() == 141                                   # additive exports: the version stays
    for name in declared:                                            # one ctypes argument per declared parameter
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert len(m.group(1).split(",")) == len(L.SYMBOLS[name][1]), name
    m = re.search(r"int\s+tvr_mesh_bvh_signed\s*\(([^;]*)\)\s*;", src)
    params = [" ".join(x.split()) for x in m.group(1).split(",")]
    assert params == ["const float *verts", "int64_t n_vertices", "const int32_t *faces", "int64_t n_triangles", "const void *bvh", "size_t bvh_bytes", "const void *table",
                      "size_t table_bytes", "const float *points", "int64_t n_points", "const tvr_mesh_lattice *lattice", "float max_dist", "float *sdist",
                      "size_t sdist_bytes", "int32_t *tri", "size_t tri_bytes", "float *bary", "size_t bary_bytes", "int8_t *feature", "size_t feature_bytes",
                      "int64_t *counts_dev", "uint32_t *fault_flag_dev", "void *stream"]
    assert "NOT built: a sign" not in open(os.path.join(ROOT, "include", "tvr.h")).read()
    for name in ("build_pseudonormals", "signed_distance", "contains", "signed_distance_grid", "signed_mesh_distance"):
        assert getattr(pkg, name) is getattr(mesh, name)
    assert mesh.SIGNED_STATISTICS == ("signed_mean", "inside_fraction")
    assert mesh.DISTANCE_STATISTICS == ("max", "mean", "rms", "median", "p95", "samples", "refused")      # unchanged
    assert mesh.CLOSEDNESS_COUNTERS == SC.COUNTERS and len(mesh.FEATURES) == 7 and mesh.FEATURES == NC.REGIONS


def test_signatures_and_defaults():
    from jittor_myc_nerfs_amd import mesh
    assert list(inspect.signature(mesh.MeshBVH.__init__).parameters) == ["self", "blob", "verts", "faces", "height", "triangles_skipped"]       # the constructor stays
    bvh = mesh.MeshBVH(torch.zeros(256, dtype=torch.uint8), torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), 0, 0)
    assert bvh.pseudonormals is None
    p = inspect.signature(mesh.build_pseudonormals).parameters
    assert list(p) == ["bvh", "stats"] and p["stats"].default is None
    p = inspect.signature(mesh.signed_distance).parameters
    assert list(p) == ["bvh", "points", "max_dist", "strict", "stats"] and p["max_dist"].default == float("inf") and p["strict"].default is True
    p = inspect.signature(mesh.contains).parameters
    assert list(p) == ["bvh", "points", "strict"] and p["strict"].default is True
    p = inspect.signature(mesh.signed_distance_grid).parameters
    assert list(p)[:4] == ["bvh", "dims", "origin", "spacing"] and p["strict"].default is True
    assert inspect.signature(mesh.signed_mesh_distance) == inspect.signature(mesh.mesh_distance)      # the same arguments; mesh_distance's own are pinned elsewhere


def test_bytes_and_describe_agree():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    lib = L.lib()
    for V, F in ((0, 0), (3, 1), (4, 4), (482, 960), (1000003, 2000001)):
        lay = mesh.pseudonormals_layout(V, F)
        assert lay["total"] == lib.tvr_mesh_pseudonormals_bytes(V, F) == _table_bytes(V, F)
        assert (lay["header"], lay["face_n"]) == (0, 256) and lay["edge_n"] == 256 + _up(12 * F) and lay["vert_n"] == lay["edge_n"] + _up(36 * F)
        assert (lay["face_stride"], lay["edge_stride"], lay["vert_stride"]) == (12, 36, 12)
        assert all(lay[k] % 256 == 0 for k in ("face_n", "edge_n", "vert_n", "total"))
        assert lib.tvr_mesh_pseudonormals_scratch_bytes(F) == 256 + 2 * _up((3 * F + 31) // 32 * 4)
    assert lib.tvr_mesh_pseudonormals_bytes(4, MAX_F + 1) == 0 and b"n_triangles" in lib.tvr_last_error()
    assert lib.tvr_mesh_pseudonormals_bytes(-1, 4) == 0 and lib.tvr_mesh_pseudonormals_bytes(1 << 31, 4) == 0 and lib.tvr_mesh_pseudonormals_scratch_bytes(-1) == 0
    assert lib.tvr_mesh_pseudonormals_describe(4, 4, None) == INVALID
    assert lib.tvr_mesh_pseudonormals_describe(4, -1, C.byref(L.MeshPseudonormalsLayout())) == INVALID
    assert lib.tvr_mesh_pseudonormals_describe(4, MAX_F + 1, C.byref(L.MeshPseudonormalsLayout())) == UNSUPPORTED


# ---- argument errors: all before any launch (there is no device here: a launch would return TVR_ERR_HIP, not these codes) ------------------------------------------------------
def _signed(lib, **kw):
    from jittor_myc_nerfs_amd import _lib as L
    keep, p = _aligned(1 << 16)
    F, V, N = kw.pop("F", 4), kw.pop("V", 6), kw.pop("N", 5)
    a = dict(verts=p, faces=p, bvh=p, bvh_bytes=_blob_bytes(max(F, 0)) if F <= 1000 else 1 << 16, table=p,
             table_bytes=_table_bytes(max(V, 0), max(F, 0)) if F <= 1000 and V <= 1000 else 1 << 16, points=p, lattice=None, max_dist=float("inf"), sdist=p,
             sdist_bytes=4 * N, tri=p, tri_bytes=4 * N, bary=p, bary_bytes=12 * N, feature=p, feature_bytes=N, counts=p, flag=p)
    a.update(kw)
    lat = a["lattice"]
    if lat is not None:
        s = L.MeshLattice()
        s.origin[:], s.spacing[:], s.dims[:] = lat
        lat = C.byref(s)
    rc = lib.tvr_mesh_bvh_signed(a["verts"], V, a["faces"], F, a["bvh"], a["bvh_bytes"], a["table"], a["table_bytes"], a["points"], N, lat, a["max_dist"], a["sdist"],
                                 a["sdist_bytes"], a["tri"], a["tri_bytes"], a["bary"], a["bary_bytes"], a["feature"], a["feature_bytes"], a["counts"], a["flag"], None)
    return rc, lib.tvr_last_error().decode()


LAT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2, 3, 4])
SIGNED_ERRORS = [
    (dict(F=-1), INVALID, "n_triangles"), (dict(F=MAX_F + 1), UNSUPPORTED, "n_triangles"), (dict(V=-1), INVALID, "n_vertices"), (dict(V=1 << 31), UNSUPPORTED, "n_vertices"),
    (dict(verts=None), INVALID, "verts"), (dict(faces=None), INVALID, "faces"), (dict(flag=None), INVALID, "fault_flag_dev"), (dict(N=-1), INVALID, "n_points"),
    (dict(N=1 << 31, sdist_bytes=1 << 40, tri_bytes=1 << 40, bary_bytes=1 << 40, feature_bytes=1 << 40), UNSUPPORTED, "n_points"),
    (dict(max_dist=float("nan")), INVALID, "max_dist"), (dict(max_dist=-1.0), INVALID, "max_dist"), (dict(bvh=None), INVALID, "bvh"),
    (dict(bvh_bytes=_blob_bytes(4) - 1), SCRATCH, "bvh"), (dict(table=None), INVALID, "table"), (dict(table_bytes=_table_bytes(6, 4) - 1), SCRATCH, "table"),
    (dict(table_bytes=_table_bytes(6, 4) + 256), SCRATCH, "another mesh"), (dict(table_bytes=_table_bytes(100, 50)), SCRATCH, "another mesh"),
    (dict(points=None), INVALID, "points"), (dict(sdist=None), INVALID, "sdist"), (dict(lattice=LAT), INVALID, "both"),
    (dict(sdist_bytes=19), SCRATCH, "sdist"), (dict(tri_bytes=19), SCRATCH, "tri"), (dict(bary_bytes=59), SCRATCH, "bary"), (dict(feature_bytes=4), SCRATCH, "feature"),
    (dict(points=None, lattice=LAT, sdist_bytes=4 * 24 - 1), SCRATCH, "sdist"), (dict(points=None, lattice=LAT, feature_bytes=23, sdist_bytes=96, tri=None, bary=None), SCRATCH, "feature"),
    (dict(points=None, lattice=(LAT[0], LAT[1], [2, -3, 4])), INVALID, "dims"), (dict(points=None, lattice=(LAT[0], [1.0, float("nan"), 1.0], LAT[2])), INVALID, "spacing"),
    (dict(points=None, lattice=([float("inf"), 0.0, 0.0], LAT[1], LAT[2])), INVALID, "origin"),
    (dict(points=None, lattice=(LAT[0], LAT[1], [2048, 2048, 2048])), UNSUPPORTED, "lattice"),
]


@pytest.mark.parametrize("kw,code,word", SIGNED_ERRORS, ids=[f"{i}-{w}" for i, (_, _, w) in enumerate(SIGNED_ERRORS)])
def test_signed_argument_errors_come_before_any_launch(kw, code, word):
    from jittor_myc_nerfs_amd import _lib as L
    rc, msg = _signed(L.lib(), **kw)
    assert rc == code and word in msg, (rc, msg)


def test_table_argument_errors_come_before_any_launch_and_empty_calls_are_accepted():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    keep, p = _aligned(1 << 16)
    F, V = 4, 6
    keys = lambda **kw: lib.tvr_mesh_pseudonormals_keys(kw.get("faces", p), kw.get("V", V), kw.get("F", F), kw.get("ck", p), kw.get("ek", p + 4096), kw.get("kb", 96),
                                                        kw.get("flag", p), None)
    for kw, code in ((dict(F=-1), INVALID), (dict(F=MAX_F + 1), UNSUPPORTED), (dict(V=-1), INVALID), (dict(V=1 << 31), UNSUPPORTED), (dict(faces=None), INVALID),
                     (dict(ck=None), INVALID), (dict(ek=None), INVALID), (dict(ck=p + 4), INVALID), (dict(kb=95), SCRATCH), (dict(flag=None), INVALID)):
        assert keys(**kw) == code, (kw, lib.tvr_last_error())

    def build(**kw):
        a = dict(verts=p, V=V, faces=p, F=F, ck=p, ek=p, eo=p, table=p, tb=_table_bytes(V, F), scratch=p, sb=256 + 2 * 256, counts=p, flag=p)
        a.update(kw)
        return lib.tvr_mesh_pseudonormals_build(a["verts"], a["V"], a["faces"], a["F"], a["ck"], a["ek"], a["eo"], a["table"], a["tb"], a["scratch"], a["sb"], a["counts"],
                                                a["flag"], None)
    for kw, code in ((dict(F=-1), INVALID), (dict(V=-1), INVALID), (dict(verts=None), INVALID), (dict(ck=None), INVALID), (dict(ek=None), INVALID), (dict(eo=None), INVALID),
                     (dict(eo=p + 4), INVALID), (dict(table=None), INVALID), (dict(table=p + 8), INVALID), (dict(tb=_table_bytes(V, F) - 1), SCRATCH),
                     (dict(scratch=None), INVALID), (dict(sb=767), SCRATCH), (dict(flag=None), INVALID)):
        assert build(**kw) == code, (kw, lib.tvr_last_error())
    # nothing to launch: no points (the table and the blob are still checked)
    assert _signed(lib, N=0, points=None, sdist=None, counts=None)[0] == 0
    assert _signed(lib, points=None, lattice=(LAT[0], LAT[1], [0, 3, 4]), sdist=None, counts=None)[0] == 0
    assert _signed(lib, table=p + 4)[0] == INVALID                   # a misaligned table


def test_no_cpu_fallback():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    bvh = mesh.MeshBVH(torch.zeros(256, dtype=torch.uint8), torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.int32), 0, 0)
    bvh.pseudonormals = mesh.MeshPseudonormals(torch.zeros(256, dtype=torch.uint8), dict.fromkeys(SC.COUNTERS, 0))
    with pytest.raises(L.TvrError, match="no CPU fallback"):
        mesh.signed_distance(bvh, torch.zeros(3, 3))
    with pytest.raises(L.TvrError, match="MeshBVH"):
        mesh.contains(None, torch.zeros(3, 3))
    bvh.pseudonormals = mesh.MeshPseudonormals(torch.zeros(256, dtype=torch.uint8), dict(dict.fromkeys(SC.COUNTERS, 0), open_edges=3))
    assert not bvh.pseudonormals.closed
    with pytest.raises(L.TvrError, match="open_edges = 3"):           # strict: refused before any call, naming the counters
        mesh.signed_distance_grid(bvh, (4, 4, 4))


def test_parser_defaults():
    from jittor_myc_nerfs_amd import reconstruct
    a = reconstruct.config_parser([])
    assert a.mesh_compare is None and a.mesh_compare_signed == 0
    a = reconstruct.config_parser(["--mesh_compare", "plain.ply", "--mesh_file", "x.obj", "--mesh_compare_signed", "1"])
    assert a.mesh_compare == "plain.ply" and a.mesh_compare_signed == 1 and a.export_mesh == 0


# ---- the statistics -------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_signed_statistics_match_their_restatement_and_unsigned_ones_are_unchanged():
    from jittor_myc_nerfs_amd import mesh
    g = np.random.default_rng(3)
    sd = g.normal(0.1, 1.0, 500).astype(np.float32)
    w = g.uniform(0.0, 2.0, 500).astype(np.float32)
    w[::7] = 0.0
    sd[5], sd[11] = np.inf, np.inf                                   # unanswered samples count for nothing
    for unit in (1.0, 0.25):
        got = dict(zip(mesh.SIGNED_STATISTICS, mesh.signed_statistics(torch.from_numpy(sd), torch.from_numpy(w), unit).tolist()))
        want = SC.signed_statistics(sd, w, unit)
        assert got["signed_mean"] == pytest.approx(want["signed_mean"], rel=1e-12) and got["inside_fraction"] == pytest.approx(want["inside_fraction"], rel=1e-12)
        assert 0.3 < got["inside_fraction"] < 0.6
        # the unsigned figures of |sdist| are the ones mesh_distance always reported
        un = dict(zip(mesh.DISTANCE_STATISTICS, mesh.distance_statistics(torch.from_numpy(np.abs(sd)), torch.from_numpy(w), unit).tolist()))
        ref = NC.statistics(np.abs(sd), w, unit)
        assert all(un[k] == pytest.approx(ref[k], rel=1e-12) for k in ref)
    assert torch.isnan(mesh.signed_statistics(torch.zeros(3), torch.zeros(3))).all()
    hand = mesh.signed_statistics(torch.tensor([-1.0, 2.0, -3.0, float("inf")]), torch.tensor([1.0, 1.0, 2.0, 5.0]), 2.0).tolist()
    assert hand == [(-1.0 + 2.0 - 6.0) / 4.0 / 2.0, 0.75]


# ---- the power of the fixture -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_spiked_sphere_separates_the_definition_from_both_shortcuts():
    m = SC.measure("spiked")
    assert (len(m["verts"]), len(m["faces"])) == (482, 960) and not any(m["t32"]["counters"].values())
    assert (len(m["sets"]["shell"]["points"]), len(m["sets"]["near"]["points"])) == (4096, 1922)
    worst = np.inf
    for kind, s in m["sets"].items():
        w = s["winding"]
        inside = w > 0.5
        wrong = {mode: int((s[mode]["inside"] != inside).sum()) for mode in ("pseudo", "face", "unweighted")}
        print(f"    spiked {kind}: {len(w)} points, {int(inside.sum())} inside; oracle within {np.abs(w - np.round(w)).max():.1e} of 0 or 1; wrong signs {wrong}; "
              f"smallest margin {s['pseudo']['margin'].min():.4f}; winners per region {np.bincount(s['near']['region'], minlength=8)[1:].tolist()}")
        assert np.abs(w - np.round(w)).max() < 1e-12 and set(np.round(w).astype(int)) == {0, 1}       # the oracle is decided everywhere
        assert (s["near"]["tri"] >= 0).all() and (s["near"]["dist"] > 0).all()
        assert wrong["pseudo"] == 0                                  # the definition: wrong nowhere
        assert wrong["unweighted"] >= 1                              # vertex sums without the angles: wrong in each set
        assert 100 < inside.sum() < len(w) - 100
        worst = min(worst, s["pseudo"]["margin"].min())
        if kind == "shell":
            assert wrong["face"] >= 100                              # the winning triangle's face normal
    assert worst >= SC.MARGIN_BAR                                    # no sign the restatement gives is within fp32 rounding of flipping


@pytest.mark.parametrize("name", ("cube", "tetra"))
def test_small_fixtures_are_decided_in_every_region_inside_and_outside(name):
    m = SC.measure(name)
    assert not any(m["t32"]["counters"].values())
    for kind, s in m["sets"].items():
        inside = s["winding"] > 0.5
        r = s["near"]["region"]
        print(f"    {name} {kind}: {len(r)} points, {int(inside.sum())} inside, smallest margin {s['pseudo']['margin'].min():.4f}, winners per region "
              f"{np.bincount(r, minlength=8)[1:].tolist()}")
        assert np.abs(s["winding"] - np.round(s["winding"])).max() < 1e-12
        assert (s["pseudo"]["inside"] == inside).all() and s["pseudo"]["margin"].min() >= SC.SMALL_MARGIN_BAR
        assert (np.bincount(r, minlength=8)[1:] > 0).all()           # vertex, edge and face regions all win somewhere
        assert inside.sum() >= 10 and (~inside).sum() >= 10
        assert (~inside[np.isin(r, (1, 2, 4))]).sum() >= 10 and (~inside[np.isin(r, (3, 5, 6))]).sum() >= 10
    if name == "tetra":                                              # on a thin solid the face-normal shortcut fails too
        assert (m["sets"]["near"]["face"]["inside"] != (m["sets"]["near"]["winding"] > 0.5)).sum() >= 10


def test_where_the_vertex_normal_bar_comes_from():
    """VERT_ANGLE_BAR: the device's vert_n goes through atan2f and is compared with the fp64 table as a direction.  The bar is 4 x the largest angle between the numpy fp32
    table's vert_n and the fp64 table's over the three fixtures; face_n of the fp32 table (what the device must equal bit for bit) is within fp32 rounding of fp64."""
    worst = 0.0
    for name in SC.FIXTURES:
        m = SC.measure(name)
        a = SC.direction_angle(m["t32"]["vert_n"], m["t64"]["vert_n"]).max()
        print(f"    {name}: fp32 vert_n against fp64, largest angle {a:.4g} rad; face_n max |fp32 - fp64| {np.abs(m['t32']['face_n'] - m['t64']['face_n']).max():.3g}")
        worst = max(worst, a)
        assert np.abs(m["t32"]["face_n"] - m["t64"]["face_n"]).max() < 2e-6 and np.abs(m["t32"]["edge_n"] - m["t64"]["edge_n"]).max() < 4e-6
    assert worst <= SC.VERT_ANGLE_MEASURED and SC.VERT_ANGLE_BAR == pytest.approx(4 * SC.VERT_ANGLE_MEASURED, rel=0.01)
    assert worst >= 0.5 * SC.VERT_ANGLE_MEASURED                      # the recorded figure is the measured one, not a loose cover


def test_the_restated_table_on_defective_meshes():
    """the counters the GPU test expects of the device, by the restatement: one face removed, one reversed, the tripled sphere, a face with a repeated vertex"""
    v, f = NC.sphere_mesh("sphere960")
    E = len(SC.undirected_edges(f))
    assert E == 1440
    assert SC.table(v, np.delete(f, 100, 0))["counters"] == dict(degenerate_faces=0, open_edges=3, nonmanifold_edges=0, inconsistent_edges=0)
    g = f.copy()
    g[100] = g[100][::-1]
    assert SC.table(v, g)["counters"] == dict(degenerate_faces=0, open_edges=0, nonmanifold_edges=0, inconsistent_edges=3)
    assert SC.table(v, NC.sphere_mesh("tripled960")[1])["counters"] == dict(degenerate_faces=0, open_edges=0, nonmanifold_edges=E, inconsistent_edges=0)
    g = f.copy()
    g[100, 2] = g[100, 0]
    c = SC.table(v, g)["counters"]
    assert c["degenerate_faces"] == 1 and c["open_edges"] + c["nonmanifold_edges"] > 0
    # both sides of an edge read the same bits, and a mesh reversed by exchanging corners 1 and 2 negates every face normal exactly (ab x ac becomes ac x ab)
    t, tr = SC.table(v, f), SC.table(v, f[:, [0, 2, 1]])
    e = SC.undirected_edges(f)
    assert np.array_equal(tr["face_n"], -t["face_n"]) and np.array_equal(np.abs(tr["vert_n"]).sum(1) > 0, np.abs(t["vert_n"]).sum(1) > 0)
    h = np.arange(3 * len(f))
    a, b = f[h // 3, (h % 3 + 1) % 3].astype(np.int64), f[h // 3, (h % 3 + 2) % 3].astype(np.int64)
    key = np.minimum(a, b) * (1 << 32) + np.maximum(a, b)
    flat = t["edge_n"].reshape(-1, 3).view(np.uint32)
    for k in np.unique(key)[:200]:
        rows = flat[key == k]
        assert len(rows) == 2 and np.array_equal(rows[0], rows[1])
    assert len(e) == len(np.unique(key))
