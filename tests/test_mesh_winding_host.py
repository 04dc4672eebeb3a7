"""No GPU: what of the winding numbers (include/tvr.h tvr_mesh_winding_*; mesh.build_winding / winding_number / winding_contains / winding_number_grid /
signed_distance_winding / remesh_watertight, reconstruct --mesh_watertight) can be checked without a device: the declarations against the ctypes table, *_bytes
against *_describe, the C calls' argument errors (host pointers that are never followed: every error is raised before a launch), the signatures and the parser — and
the POWER of the GPU test's fixtures: on the union of two overlapping spheres, which every closedness counter calls closed, and on the unwelded spiked sphere the
restated pseudo-normal sign (tests/mesh_signed_common.py) is wrong at hundreds of points where the winding number's is wrong at none.  The restatement of
tests/mesh_winding_common.py is tied to the brute-force oracle here (beta = inf, any tree), and the measurement behind WINDING_BAR is asserted."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mesh_nearest_common as NC
import mesh_signed_common as SC
import mesh_winding_common as WC
from conftest import ROOT
from test_mesh_nearest_host import _aligned, _blob_bytes, _up

INVALID, SCRATCH, UNSUPPORTED = -1, -3, -4
MAX_F = 1 << 30
NAMES = ("tvr_mesh_winding_bytes", "tvr_mesh_winding_scratch_bytes", "tvr_mesh_winding_describe", "tvr_mesh_winding_build", "tvr_mesh_winding_query")
PYTHON = ("build_winding", "winding_number", "winding_contains", "winding_number_grid", "signed_distance_winding", "remesh_watertight")


def _table_bytes(F):
    return 256 + _up(32 * max(F - 1, 0))


# ---- the surface ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_symbol_table_and_package_agree():
    import jittor_myc_nerfs_amd as pkg
    from jittor_myc_nerfs_amd import _lib as L, mesh
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tvr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tvr_mesh_winding_[a-z_]+)\s*\(", src))
    assert declared == set(NAMES) and declared <= set(L.SYMBOLS)
    lib = L.lib()
    assert lib.tvr_version() == 141                                   # additive exports: the version stays
    for name in declared:                                            # one ctypes argument per declared parameter, and the library exports it
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert len(m.group(1).split(",")) == len(L.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    m = re.search(r"int\s+tvr_mesh_winding_query\s*\(([^;]*)\)\s*;", src)
    assert [" ".join(x.split()) for x in m.group(1).split(",")] == [
        "const float *verts", "int64_t n_vertices", "const int32_t *faces", "int64_t n_triangles", "const void *bvh", "size_t bvh_bytes", "const void *table",
        "size_t table_bytes", "const float *points", "int64_t n_points", "const tvr_mesh_lattice *lattice", "float beta", "float *w", "size_t w_bytes", "int64_t *counts_dev",
        "uint32_t *fault_flag_dev", "void *stream"]
    for name in PYTHON:
        assert getattr(pkg, name) is getattr(mesh, name)
    assert mesh.WINDING_COUNTS == ("points_answered", "points_refused", "node_visits", "dipole_terms", "triangle_terms")
    makefile = open(os.path.join(ROOT, "jittor-myc-nerfs_amd", "csrc", "Makefile")).read()
    assert "FLAGS_tvr_mesh_winding := -fhip-fp32-correctly-rounded-divide-sqrt" in makefile and " tvr_mesh_winding.hip" in makefile


def test_signatures_and_defaults():
    from jittor_myc_nerfs_amd import mesh, reconstruct as R
    bvh = mesh.MeshBVH(torch.zeros(256, dtype=torch.uint8), torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), 0, 0)
    assert bvh.winding is None and bvh.pseudonormals is None
    sig = lambda f: inspect.signature(f).parameters
    p = sig(mesh.build_winding)
    assert list(p) == ["bvh", "stats"] and p["stats"].default is None
    p = sig(mesh.winding_number)
    assert list(p) == ["bvh", "points", "beta", "stats"] and p["beta"].default == 2.0 and p["stats"].default is None
    p = sig(mesh.winding_contains)
    assert list(p) == ["bvh", "points", "beta"] and p["beta"].default == 2.0
    p = sig(mesh.winding_number_grid)
    assert list(p) == ["bvh", "dims", "origin", "spacing", "beta", "stats"] and p["origin"].default == (0, 0, 0) and p["spacing"].default == (1, 1, 1) and p["beta"].default == 2.0
    p = sig(mesh.signed_distance_winding)
    assert list(p) == ["bvh", "points", "max_dist", "beta", "stats"] and p["max_dist"].default == float("inf") and p["beta"].default == 2.0
    p = sig(mesh.remesh_watertight)
    assert list(p) == ["verts", "faces", "resolution", "voxel", "pad", "beta", "level", "stats"]
    assert (p["resolution"].default, p["voxel"].default, p["pad"].default, p["beta"].default, p["level"].default) == (256, None, 2, 2.0, 0.5)
    args = R.config_parser(["--mesh_file", "x.ply"])
    assert args.mesh_watertight == 0 and args.mesh_watertight_beta == 2.0 and args.mesh_compare is None and args.mesh_compare_signed == 0
    args = R.config_parser(["--mesh_file", "x.ply", "--mesh_watertight", "48", "--mesh_watertight_beta", "inf"])
    assert args.mesh_watertight == 48 and args.mesh_watertight_beta == float("inf")
    with pytest.raises(SystemExit, match="--mesh_watertight"):
        R.main(["--mesh_watertight", "48"])
    # on a host tensor every entry point says where it runs, before anything else
    from jittor_myc_nerfs_amd import _lib as L
    with pytest.raises(L.TvrError, match="build_bvh returns"):
        mesh.winding_number(None, torch.zeros(1, 3))
    with pytest.raises(L.TvrError, match="MI355X"):
        mesh.remesh_watertight(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))


def test_bytes_and_describe_agree():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    lib = L.lib()
    for F in (0, 1, 2, 4, 960, 2000001):
        lay = mesh.winding_layout(F)
        assert lay["total"] == lib.tvr_mesh_winding_bytes(F) == _table_bytes(F)
        assert (lay["header"], lay["rows"], lay["row_stride"], lay["n_rows"]) == (0, 256, 32, max(F - 1, 0)) and lay["total"] % 256 == 0
        assert lib.tvr_mesh_winding_scratch_bytes(F) == max(_up(4 * max(F - 1, 0)) + _up(16 * max(F - 1, 0)), 256)
        assert mesh.bvh_layout(F)["total"] == _blob_bytes(F)         # the hierarchy's blob keeps its size
    assert lib.tvr_mesh_winding_bytes(MAX_F + 1) == 0 and b"n_triangles" in lib.tvr_last_error()
    assert lib.tvr_mesh_winding_bytes(-1) == 0 and lib.tvr_mesh_winding_scratch_bytes(-1) == 0 and lib.tvr_mesh_winding_scratch_bytes(MAX_F + 1) == 0
    assert lib.tvr_mesh_winding_describe(4, None) == INVALID
    assert lib.tvr_mesh_winding_describe(-1, C.byref(L.MeshWindingLayout())) == INVALID
    assert lib.tvr_mesh_winding_describe(MAX_F + 1, C.byref(L.MeshWindingLayout())) == UNSUPPORTED


# ---- argument errors: all before any launch (there is no device here: a launch would return TVR_ERR_HIP, not these codes) ------------------------------------------------------
def _query(lib, **kw):
    from jittor_myc_nerfs_amd import _lib as L
    keep, p = _aligned(1 << 16)
    F, V, N = kw.pop("F", 4), kw.pop("V", 6), kw.pop("N", 5)
    a = dict(verts=p, faces=p, bvh=p, bvh_bytes=_blob_bytes(max(F, 0)) if F <= 1000 else 1 << 16, table=p, table_bytes=_table_bytes(max(F, 0)) if F <= 1000 else 1 << 16,
             points=p, lattice=None, beta=2.0, w=p, w_bytes=4 * N, counts=p, flag=p)
    a.update(kw)
    lat = a["lattice"]
    if lat is not None:
        s = L.MeshLattice()
        s.origin[:], s.spacing[:], s.dims[:] = lat
        lat = C.byref(s)
    rc = lib.tvr_mesh_winding_query(a["verts"], V, a["faces"], F, a["bvh"], a["bvh_bytes"], a["table"], a["table_bytes"], a["points"], N, lat, a["beta"], a["w"], a["w_bytes"],
                                    a["counts"], a["flag"], None)
    return rc, lib.tvr_last_error().decode()


LAT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2, 3, 4])
QUERY_ERRORS = [
    (dict(beta=0.5), INVALID, "beta"), (dict(beta=float("nan")), INVALID, "beta"), (dict(beta=-2.0), INVALID, "beta"), (dict(beta=float("-inf")), INVALID, "beta"),
    (dict(beta=0.99999994), INVALID, "beta"),
    (dict(F=-1), INVALID, "n_triangles"), (dict(F=MAX_F + 1), UNSUPPORTED, "n_triangles"), (dict(V=-1), INVALID, "n_vertices"), (dict(V=1 << 31), UNSUPPORTED, "n_vertices"),
    (dict(verts=None), INVALID, "verts"), (dict(faces=None), INVALID, "faces"), (dict(flag=None), INVALID, "fault_flag_dev"), (dict(N=-1), INVALID, "n_points"),
    (dict(N=1 << 31, w_bytes=1 << 40), UNSUPPORTED, "n_points"), (dict(bvh=None), INVALID, "bvh"), (dict(bvh_bytes=_blob_bytes(4) - 1), SCRATCH, "bvh"),
    (dict(table=None), INVALID, "table"), (dict(table_bytes=_table_bytes(4) - 1), SCRATCH, "table"), (dict(table_bytes=_table_bytes(4) + 256), SCRATCH, "another mesh"),
    (dict(table_bytes=_table_bytes(50)), SCRATCH, "another mesh"), (dict(points=None), INVALID, "points"), (dict(w=None), INVALID, "w is NULL"),
    (dict(lattice=LAT), INVALID, "both"), (dict(w_bytes=19), SCRATCH, "w [n_points]"), (dict(points=None, lattice=LAT, w_bytes=4 * 24 - 1), SCRATCH, "w [n_points]"),
    (dict(points=None, lattice=(LAT[0], LAT[1], [2, -3, 4])), INVALID, "dims"), (dict(points=None, lattice=(LAT[0], [1.0, float("nan"), 1.0], LAT[2])), INVALID, "spacing"),
    (dict(points=None, lattice=([float("inf"), 0.0, 0.0], LAT[1], LAT[2])), INVALID, "origin"),
    (dict(points=None, lattice=(LAT[0], LAT[1], [2048, 2048, 2048])), UNSUPPORTED, "lattice"),
]


@pytest.mark.parametrize("kw,code,word", QUERY_ERRORS, ids=[f"{i}-{w.split()[0]}" for i, (_, _, w) in enumerate(QUERY_ERRORS)])
def test_query_argument_errors_come_before_any_launch(kw, code, word):
    from jittor_myc_nerfs_amd import _lib as L
    rc, msg = _query(L.lib(), **kw)
    assert rc == code and word in msg, (rc, msg)


def test_build_argument_errors_come_before_any_launch_and_empty_queries_are_accepted():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    lib = L.lib()
    keep, p = _aligned(1 << 16)
    F, V = 4, 6

    def build(**kw):
        a = dict(verts=p, V=V, faces=p, F=F, bvh=p, bb=_blob_bytes(F), table=p, tb=_table_bytes(F), scratch=p, sb=512, flag=p)
        a.update(kw)
        return lib.tvr_mesh_winding_build(a["verts"], a["V"], a["faces"], a["F"], a["bvh"], a["bb"], a["table"], a["tb"], a["scratch"], a["sb"], a["flag"], None)
    for kw, code in ((dict(F=-1), INVALID), (dict(F=MAX_F + 1), UNSUPPORTED), (dict(V=-1), INVALID), (dict(verts=None), INVALID), (dict(faces=None), INVALID),
                     (dict(bvh=None), INVALID), (dict(bvh=p + 8), INVALID), (dict(bb=_blob_bytes(F) - 1), SCRATCH), (dict(table=None), INVALID), (dict(table=p + 8), INVALID),
                     (dict(tb=_table_bytes(F) - 1), SCRATCH), (dict(scratch=None), INVALID), (dict(scratch=p + 4), INVALID), (dict(sb=511), SCRATCH), (dict(flag=None), INVALID)):
        assert build(**kw) == code, (kw, lib.tvr_last_error())
    assert _query(lib, N=0, points=None, w=None, w_bytes=0, counts=None)[0] == 0                                  # no points: nothing is launched
    assert _query(lib, points=None, lattice=(LAT[0], LAT[1], [2, 0, 4]), w=None, w_bytes=0, counts=None)[0] == 0   # an empty lattice
    assert _query(lib, beta=1.0, N=0, counts=None)[0] == 0 and _query(lib, beta=float("inf"), N=0, counts=None)[0] == 0
    # the Python side raises on beta before it asks for a device
    bvh = mesh.MeshBVH(torch.zeros(256, dtype=torch.uint8), torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), 0, 0)
    for beta in (0.5, float("nan"), -1.0):
        with pytest.raises(L.TvrError, match="beta"):
            mesh.signed_distance_winding(bvh, torch.zeros(1, 3), beta=beta)
        with pytest.raises(L.TvrError, match="beta"):
            mesh.winding_number_grid(bvh, (2, 2, 2), beta=beta)


# ---- the power of the fixtures ------------------------------------------------------------------------------------------------------------------------------------------------
def _pseudo_wrong(v, f, p, truth):
    s = SC.signs(v, f, p, NC.restate(v, f, p), SC.table(v, f, np.float64))
    return int((s["inside"] != truth).sum())


def test_pseudo_normals_fail_silently_on_the_union_and_the_winding_number_does_not():
    c = WC.cases()["union"]
    p, truth, w = c["sets"]["shell"], c["truth"]["shell"], c["oracle"]["shell"]
    counters = SC.table(c["verts"], c["faces"])["counters"]
    wrong = _pseudo_wrong(c["verts"], c["faces"], p, truth)
    print(f"    union of two sphere960 ({len(c['faces'])} triangles): counters {counters}; {int(truth.sum())} of {len(p)} points inside; pseudo-normal sign wrong at {wrong}, "
          f"winding > 0.5 wrong at {int(((w > 0.5) != truth).sum())}, min |w - 0.5| {np.abs(w - 0.5).min():.3f}, w up to {w.max():.3f}")
    assert all(counters[k] == 0 for k in SC.COUNTERS)                # strict=True accepts it
    assert wrong == 487 and int(((w > 0.5) != truth).sum()) == 0
    assert WC.margin(c) > 0.49 and w.max() > 1.5                     # 2 in the lens: `> 0.5`, not `== 1`


def test_pseudo_normals_fail_on_the_unwelded_soup_and_the_winding_number_does_not():
    c = WC.cases()["soup"]
    counters = SC.table(c["verts"], c["faces"])["counters"]
    assert counters["open_edges"] == 2880 and len(c["verts"]) == 3 * len(c["faces"])
    wrong = {k: _pseudo_wrong(c["verts"], c["faces"], p, c["truth"][k]) for k, p in c["sets"].items()}
    orc = {k: int(((c["oracle"][k] > 0.5) != c["truth"][k]).sum()) for k in c["sets"]}
    print(f"    unwelded spiked sphere: counters {counters}; pseudo-normal sign wrong at {wrong}, winding > 0.5 wrong at {orc}")
    assert wrong == {"shell": 442, "near": 79} and orc == {"shell": 0, "near": 0} and WC.margin(c) > 0.49


def test_margins_of_every_classified_fixture():
    for name, c in WC.cases().items():
        if c["truth"] is not None:
            assert WC.margin(c) > 0.49, name                         # the oracle's margin is 0.5: no approximation of a few 1e-2 flips a sign
            assert all(np.array_equal(c["oracle"][k] > 0.5, c["truth"][k]) for k in c["sets"])
    t, s = WC.cases()["tripled"], NC.sphere_mesh("sphere960")
    assert np.abs(t["oracle"]["shell"] - 3 * SC.winding(s[0], s[1], t["sets"]["shell"])).max() < 1e-12


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_median_tree_is_a_tree_and_the_table_sums_what_lies_below():
    for name in ("spiked", "cube", "F1", "F2"):
        c = WC.cases()[name]
        v, f = c["verts"], c["faces"]
        tree = WC.median_tree(v, f)
        F = len(f)
        assert sorted(tree["leaf_order"].tolist()) == list(range(F))
        if F > 1:
            assert sorted(tree["children"].reshape(-1).tolist()) == list(range(1, 2 * F - 1))
        rows = WC.table(tree, v, f)
        assert rows.shape == (F - 1, 8) and rows.dtype == np.float32
        if F > 1:
            A, m, a = (x.astype(np.float64) for x in WC.leaf_moments(v, f))
            assert np.abs(rows[0, :3] - A.sum(0)).max() < 1e-5 and abs(rows[0, 7] - a.sum()) < 1e-4 * a.sum()
            assert np.abs(rows[0, 3:6] - m.sum(0) / a.sum()).max() < 1e-5
            lo, hi = v[f].reshape(-1, 3).min(0), v[f].reshape(-1, 3).max(0)
            corners = np.stack(np.meshgrid(*zip(lo, hi), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
            assert abs(rows[0, 6] - np.linalg.norm(corners - rows[0, 3:6].astype(np.float64), axis=1).max()) < 1e-5
            assert (rows[:, 6] > 0).all() and (rows[:, 7] > 0).all()
    closed = WC.table(WC.median_tree(*SC.cube()), *SC.cube())
    assert np.abs(closed[0, :3]).max() < 1e-7                        # a closed surface's area vectors cancel: its far field has no dipole
    # a degenerate soup: zero area everywhere -> never approximated
    v = np.zeros((4, 3), np.float32)
    f = np.asarray([[0, 1, 2], [1, 2, 3], [0, 2, 3]], np.int32)
    rows = WC.table(WC.median_tree(v, f), v, f)
    assert np.isposinf(rows[:, 6]).all() and (rows[:, 7] == 0).all() and (rows[:, 3:6] == 0).all()


def test_restatement_equals_the_oracle_and_e32_stands_behind_the_bar():
    """beta = inf with fp64 terms is the brute-force sum on any tree (1e-12); E32 = what fp32 terms cost at beta = inf, 2, 3; WINDING_BAR >= 4 x E32."""
    e32, exact, approx = {}, 0.0, {}
    for name, c in WC.cases().items():
        v, f = c["verts"], c["faces"]
        tree = WC.median_tree(v, f)
        rows = WC.table(tree, v, f)
        for kind, p in c["sets"].items():
            om64, om32 = WC.solid_angles(v, f, p), WC.solid_angles(v, f, p, np.float32)
            for beta in WC.BETAS:
                r64, r32 = WC.query(tree, rows, v, f, p, beta, omega=om64), WC.query(tree, rows, v, f, p, beta, np.float32, omega=om32)
                assert {k: r64[k] for k in ("node_visits", "dipole_terms", "triangle_terms")} == {k: r32[k] for k in ("node_visits", "dipole_terms", "triangle_terms")}
                if beta == np.inf:
                    exact = max(exact, float(np.abs(r64["w"] - c["oracle"][kind]).max()))
                    assert r64["dipole_terms"] == 0 and r64["triangle_terms"] == len(p) * len(f)
                    ref = c["oracle"][kind]
                else:
                    ref = r64["w"]
                    approx[(name, kind, beta)] = float(np.abs(r64["w"] - c["oracle"][kind]).max())
                    if c["truth"] is not None:
                        assert np.array_equal(r64["w"] > 0.5, c["truth"][kind])
                e32[(name, kind, beta)] = float(np.abs(r32["w"] - ref).max())
    worst = max(e32, key=e32.get)
    print(f"    E32 = {e32[worst]:.4g} at {worst}; beta = inf against the oracle {exact:.3g}; WINDING_BAR = {WC.WINDING_BAR:g}")
    print("    median-split tree, spiked sphere, max |restatement - oracle|: " + ", ".join(f"beta {b:g}: {max(approx[('spiked', k, b)] for k in ('shell', 'near')):.3g}"
                                                                                                 for b in (2.0, 3.0)))
    assert exact < 1e-12
    assert WC.WINDING_BAR >= 4 * e32[worst] and WC.E32_MEASURED >= e32[worst] and WC.WINDING_BAR <= 4.1 * WC.E32_MEASURED       # the bar is the measurement's, not wider
    assert approx[("spiked", "shell", 3.0)] < approx[("spiked", "shell", 2.0)] < 0.1                                              # beta buys accuracy
