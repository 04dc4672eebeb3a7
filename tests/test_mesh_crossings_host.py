"""No GPU: what of the triangle-pair query (include/tvr.h tvr_mesh_crossings_*; mesh.self_intersections / mesh_intersections / crossing_faces / mesh_check /
write_obj_segments, reconstruct --mesh_check) can be checked without a device: the declarations against the ctypes table, the C calls' argument errors (host pointers
that are never followed: every error is raised before a launch), the signatures, the parser, write_obj_segments, the keys of mesh_check's report — and the POWER of
the GPU test's fixtures: on every one of them the brute-force fp32 restatement of tests/mesh_crossings_common.py decides every (segment, triangle) test as the fp64
Moeller-Trumbore oracle does, no test is ambiguous, and the pair and piercing counts are the ones the issue states."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mesh_crossings_common as XC
from conftest import ROOT
from test_mesh_nearest_host import _aligned, _blob_bytes

INVALID, SCRATCH, UNSUPPORTED = -1, -3, -4
MAX_F = 1 << 30
NAMES = ("tvr_mesh_crossings_count", "tvr_mesh_crossings_emit")
PYTHON = ("self_intersections", "mesh_intersections", "crossing_faces", "mesh_check", "write_obj_segments")
CHECK_KEYS = ("vertices", "triangles", "degenerate_faces", "open_edges", "nonmanifold_edges", "inconsistent_edges", "closed", "components", "crossing_pairs",
              "crossing_faces", "crossing_length", "n_pierce_histogram")


# ---- the surface ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_symbol_table_and_package_agree():
    import jittor_myc_nerfs_amd as pkg
    from jittor_myc_nerfs_amd import _lib as L, mesh
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tvr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tvr_mesh_crossings_[a-z_]+)\s*\(", src))
    assert declared == set(NAMES) and declared <= set(L.SYMBOLS)
    lib = L.lib()
    assert lib.tvr_version() == 141                                   # additive exports: the version stays
    for name in declared:                                            # one ctypes argument per declared parameter, and the library exports it
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert len(m.group(1).split(",")) == len(L.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    m = re.search(r"int\s+tvr_mesh_crossings_emit\s*\(([^;]*)\)\s*;", src)
    assert [" ".join(x.split()) for x in m.group(1).split(",")] == [
        "const float *verts", "int64_t n_vertices", "const int32_t *faces", "int64_t n_triangles", "const void *bvh", "size_t bvh_bytes", "int32_t mode",
        "const float *verts_q", "int64_t n_vertices_q", "const int32_t *faces_q", "int64_t n_triangles_q", "const int64_t *offsets", "size_t offsets_bytes", "int64_t n_pairs",
        "int32_t *pairs", "size_t pairs_bytes", "int32_t *n_pierce", "size_t n_pierce_bytes", "float *points", "size_t points_bytes", "uint32_t *fault_flag_dev", "void *stream"]
    for name in PYTHON:
        assert getattr(pkg, name) is getattr(mesh, name)
    assert mesh.CROSSINGS_COUNTS == ("pairs", "triangles_refused", "node_tests", "pair_tests")
    makefile = open(os.path.join(ROOT, "jittor-myc-nerfs_amd", "csrc", "Makefile")).read()
    assert "FLAGS_tvr_mesh_crossings := -fhip-fp32-correctly-rounded-divide-sqrt" in makefile and " tvr_mesh_crossings.hip" in makefile


def test_signatures_defaults_and_the_parser():
    from jittor_myc_nerfs_amd import _lib as L, mesh, reconstruct as R
    sig = lambda f: inspect.signature(f).parameters
    p = sig(mesh.self_intersections)
    assert list(p) == ["bvh", "points", "stats"] and p["points"].default is False and p["stats"].default is None
    p = sig(mesh.mesh_intersections)
    assert list(p) == ["bvh", "verts_q", "faces_q", "points", "stats"] and p["points"].default is False and p["stats"].default is None
    p = sig(mesh.crossing_faces)
    assert list(p) == ["pairs", "n_faces", "column"] and p["column"].default is None
    p = sig(mesh.mesh_check)
    assert list(p) == ["verts", "faces", "bvh"] and p["bvh"].default is None
    assert list(sig(mesh.write_obj_segments)) == ["path", "points"]
    # --mesh_check 0 is the default, and naming it leaves every other value of the option set as it was
    plain, off, on = (vars(R.config_parser(["--mesh_file", "x.ply"] + extra)) for extra in ([], ["--mesh_check", "0"], ["--mesh_check", "1", "--mesh_check_curves", "1"]))
    assert plain["mesh_check"] == 0 and plain["mesh_check_curves"] == 0 and off == plain
    assert (on["mesh_check"], on["mesh_check_curves"]) == (1, 1) and {k: v for k, v in on.items() if not k.startswith("mesh_check")} == \
        {k: v for k, v in plain.items() if not k.startswith("mesh_check")}
    with pytest.raises(SystemExit, match="--mesh_check"):
        R.main(["--mesh_check", "1"])
    # on a host tensor every entry point says where it runs, before anything else
    with pytest.raises(L.TvrError, match="build_bvh returns"):
        mesh.self_intersections(None)
    bvh = mesh.MeshBVH(torch.zeros(256, dtype=torch.uint8), torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), 0, 0)
    with pytest.raises(L.TvrError, match="no CPU fallback"):
        mesh.mesh_intersections(bvh, torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(L.TvrError, match="no CPU fallback"):
        mesh.mesh_check(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
    # crossing_faces is plain tensor work: it runs where the pairs are
    pairs = torch.tensor([[0, 4], [2, 4], [2, 5]], dtype=torch.int32)
    assert mesh.crossing_faces(pairs, 7).tolist() == [True, False, True, False, True, True, False]
    assert mesh.crossing_faces(pairs, 7, column=0).tolist() == [True, False, True, False, False, False, False]
    assert mesh.crossing_faces(pairs, 7, column=1).tolist() == [False, False, False, False, True, True, False]
    assert mesh.crossing_faces(pairs[:0], 3).tolist() == [False] * 3


def test_mesh_check_report_keys(monkeypatch):
    """the report's keys and plain JSON types, with the device calls stood in for (the GPU test checks the values)"""
    import json
    from jittor_myc_nerfs_amd import mesh
    bvh = mesh.MeshBVH(torch.zeros(256, dtype=torch.uint8), torch.zeros(5, 3), torch.tensor([[0, 1, 2], [0, 3, 4]], dtype=torch.int32), 0, 0)
    pts = torch.tensor([[[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]]])

    def pseudonormals(b, stats=None):
        stats.update(dict.fromkeys(mesh.CLOSEDNESS_COUNTERS, 0), open_edges=6, closed=False)
    monkeypatch.setattr(mesh, "build_pseudonormals", pseudonormals)
    monkeypatch.setattr(mesh, "self_intersections", lambda b, points=False, stats=None: (torch.tensor([[0, 1]], dtype=torch.int32), torch.tensor([1], dtype=torch.int32), pts))
    monkeypatch.setattr(mesh, "mesh_components", lambda f, V, stats=None: (None, None, 1))
    rep = mesh.mesh_check(None, None, bvh=bvh)
    assert tuple(rep) == CHECK_KEYS
    assert rep == dict(vertices=5, triangles=2, degenerate_faces=0, open_edges=6, nonmanifold_edges=0, inconsistent_edges=0, closed=False, components=1, crossing_pairs=1,
                       crossing_faces=2, crossing_length=5.0, n_pierce_histogram={1: 1})
    assert json.loads(json.dumps(rep))["n_pierce_histogram"] == {"1": 1}


def test_write_obj_segments_round_trip(tmp_path):
    from jittor_myc_nerfs_amd import mesh
    pts = np.random.default_rng(3).standard_normal((17, 2, 3)).astype(np.float32)
    pts[0, 0] = (1e-30, -3.4e38, 0.1)
    path = str(tmp_path / "curves.obj")
    mesh.write_obj_segments(path, torch.from_numpy(pts))
    lines = [x.split() for x in open(path).read().splitlines()]
    assert {x[0] for x in lines} == {"v", "l"}                       # nothing but vertices and lines
    v = np.asarray([[np.float32(c) for c in x[1:]] for x in lines if x[0] == "v"], np.float32)
    l = np.asarray([[int(c) for c in x[1:]] for x in lines if x[0] == "l"])
    assert np.array_equal(v.view(np.uint32), pts.reshape(-1, 3).view(np.uint32))
    assert np.array_equal(l, np.stack([2 * np.arange(17) + 1, 2 * np.arange(17) + 2], -1))
    mesh.write_obj_segments(path, np.zeros((0, 2, 3), np.float32))
    assert open(path).read() == ""


# ---- argument errors: all before any launch (there is no device here: a launch would return TVR_ERR_HIP, not these codes) ------------------------------------------------------
def _call(lib, emit, **kw):
    keep, p = _aligned(1 << 16)
    F, V, Fq, Vq, P = kw.pop("F", 4), kw.pop("V", 6), kw.pop("Fq", 3), kw.pop("Vq", 5), kw.pop("P", 7)
    a = dict(verts=p, faces=p, bvh=p, bvh_bytes=_blob_bytes(max(F, 0)) if F <= 1000 else 1 << 16, mode=1, verts_q=p, faces_q=p, count=p, count_bytes=None, total=p, counts=p,
             offsets=p, offsets_bytes=None, pairs=p, pairs_bytes=8 * max(P, 0), n_pierce=p, n_pierce_bytes=4 * max(P, 0), points=p, points_bytes=24 * max(P, 0), flag=p)
    a.update(kw)
    nq = max(F if a["mode"] == 0 else Fq, 0)
    if a["count_bytes"] is None:
        a["count_bytes"] = 4 * nq
    if a["offsets_bytes"] is None:
        a["offsets_bytes"] = 8 * (nq + 1)
    head = (a["verts"], V, a["faces"], F, a["bvh"], a["bvh_bytes"], a["mode"], a["verts_q"], Vq, a["faces_q"], Fq)
    if emit:
        rc = lib.tvr_mesh_crossings_emit(*head, a["offsets"], a["offsets_bytes"], P, a["pairs"], a["pairs_bytes"], a["n_pierce"], a["n_pierce_bytes"], a["points"],
                                         a["points_bytes"], a["flag"], None)
    else:
        rc = lib.tvr_mesh_crossings_count(*head, a["count"], a["count_bytes"], a["total"], a["counts"], a["flag"], None)
    return rc, lib.tvr_last_error().decode()


BOTH = [
    (dict(F=-1), INVALID, "n_triangles"), (dict(F=MAX_F + 1), UNSUPPORTED, "n_triangles"), (dict(V=-1), INVALID, "n_vertices"), (dict(V=1 << 31), UNSUPPORTED, "n_vertices"),
    (dict(verts=None), INVALID, "verts"), (dict(faces=None), INVALID, "faces"), (dict(flag=None), INVALID, "fault_flag_dev"), (dict(mode=2), INVALID, "mode"),
    (dict(mode=-1), INVALID, "mode"), (dict(Fq=-1), INVALID, "n_triangles_q"), (dict(Vq=-1), INVALID, "n_vertices_q"), (dict(Fq=MAX_F + 1), UNSUPPORTED, "n_triangles_q"),
    (dict(Vq=1 << 31), UNSUPPORTED, "n_vertices_q"), (dict(verts_q=None), INVALID, "verts_q"), (dict(faces_q=None), INVALID, "faces_q"), (dict(bvh=None), INVALID, "bvh"),
    (dict(bvh_bytes=_blob_bytes(4) - 1), SCRATCH, "bvh"),
]
COUNT = BOTH + [(dict(total=None), INVALID, "total_dev"), (dict(count=None), INVALID, "count_out"), (dict(count_bytes=11), SCRATCH, "count_out"),
                (dict(mode=0, count_bytes=15), SCRATCH, "count_out")]
EMIT = BOTH + [(dict(P=-1), INVALID, "n_pairs"), (dict(P=1 << 31), UNSUPPORTED, "n_pairs"), (dict(offsets=None), INVALID, "offsets"), (dict(offsets_bytes=31), SCRATCH, "offsets"),
               (dict(mode=0, offsets_bytes=39), SCRATCH, "offsets"), (dict(pairs=None), INVALID, "pairs"), (dict(n_pierce=None), INVALID, "n_pierce"),
               (dict(pairs_bytes=55), SCRATCH, "pairs [n_pairs,2]"), (dict(n_pierce_bytes=27), SCRATCH, "n_pierce [n_pairs]"), (dict(points_bytes=167), SCRATCH, "points [n_pairs,2,3]")]


@pytest.mark.parametrize("kw,code,word", COUNT, ids=[f"{i}-{w.split()[0]}" for i, (_, _, w) in enumerate(COUNT)])
def test_count_argument_errors_come_before_any_launch(kw, code, word):
    from jittor_myc_nerfs_amd import _lib as L
    rc, msg = _call(L.lib(), False, **kw)
    assert rc == code and word in msg and "tvr_mesh_crossings_count" in msg, (rc, msg)


@pytest.mark.parametrize("kw,code,word", EMIT, ids=[f"{i}-{w.split()[0]}" for i, (_, _, w) in enumerate(EMIT)])
def test_emit_argument_errors_come_before_any_launch(kw, code, word):
    from jittor_myc_nerfs_amd import _lib as L
    rc, msg = _call(L.lib(), True, **kw)
    assert rc == code and word in msg and "tvr_mesh_crossings_emit" in msg, (rc, msg)


def test_misaligned_buffers_and_what_a_self_query_does_not_read():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    keep, p = _aligned(1 << 16)
    assert _call(lib, False, bvh=p + 8)[0] == INVALID and _call(lib, True, bvh=p + 8)[0] == INVALID
    rc, msg = _call(lib, True, offsets=p + 4)
    assert rc == INVALID and "8-byte aligned" in msg
    # a self query ignores the query mesh's arguments: with them NULL or negative the call gets past every check (and then fails to launch: there is no device)
    rc, msg = _call(lib, True, mode=0, verts_q=None, faces_q=None, Fq=-5, Vq=-5)
    assert rc not in (INVALID, SCRATCH, UNSUPPORTED), (rc, msg)
    # an empty query mesh launches nothing in the second pass: valid without a device, its pointers never followed
    assert _call(lib, True, Fq=0, P=0, offsets=None, offsets_bytes=0, pairs=None, n_pierce=None, points=None, verts_q=None, faces_q=None)[0] == 0
    assert _call(lib, True, mode=0, F=0, V=0, P=0, verts=None, faces=None, offsets=None, offsets_bytes=0, pairs=None, n_pierce=None, points=None)[0] == 0


# ---- the power of the fixtures --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(XC.EXPECTED))
def test_restatement_equals_the_oracle_and_gives_the_stated_counts(name):
    r = XC.reference(name)
    v, f, res = r["verts"], r["faces"], r["restate"]
    orc = XC.oracle_tests(v, f, v, f)
    differ, ambiguous = int((r["tests"]["hit"] != orc["hit"]).sum()), int(orc["ambiguous"].sum())
    hist = dict(zip(*(x.tolist() for x in np.unique(res["n_pierce"], return_counts=True))))
    print(f"    {name}: {len(f)} triangles, {len(res['pairs'])} pairs, {int(res['n_pierce'].sum())} piercings {hist}, {len(np.unique(res['pairs']))} triangles involved; "
          f"{int(r['tests']['tested'].sum())} of {3 * len(f) * len(f)} tests made, {differ} differ from the oracle, {ambiguous} ambiguous")
    assert differ == 0 and ambiguous == 0                            # the condition is "no test excluded"
    pairs, piercings = XC.EXPECTED[name]
    assert len(res["pairs"]) == pairs and (piercings is None or int(res["n_pierce"].sum()) == piercings)
    assert (res["pairs"][:, 0] < res["pairs"][:, 1]).all() and res["points"].shape == (pairs, 2, 3)
    if name in ("union", "soup_union"):
        assert hist == {2: 164} and len(np.unique(res["pairs"])) == 164
    if name == "bowtie":
        assert res["pairs"].tolist() == [[0, 1]] and res["n_pierce"].tolist() in ([1], [2])
        assert np.array_equal(res["points"][0, 0], res["points"][0, 1]) and np.abs(res["points"][0, 0] - np.asarray([0.55, 0.5, 0.0], np.float32)).max() < 1e-6


def test_soups_report_what_their_welded_meshes_do_and_an_index_rule_would_not():
    """position, not index: a soup's pairs are its welded mesh's pairs — and judged by index the unwelded sphere reports rounding noise between neighbours"""
    for name in ("union", "pushed"):
        a, b = XC.reference(name)["restate"], XC.reference("soup_" + name)["restate"]
        assert np.array_equal(a["pairs"], b["pairs"]) and np.array_equal(a["n_pierce"], b["n_pierce"])
    v, f = XC.fixtures()["soup_sphere960"]
    with np.errstate(all="ignore"):
        import mesh_bvh_common as BC
        o, e = XC.segments(v, f)
        hit = np.concatenate([BC._pairs32(v, f.astype(np.int64), o[i:i + 480], (e - o)[i:i + 480], 0.0, 1.0, False)[0] for i in range(0, len(o), 480)])
    hit[np.arange(len(o)), np.arange(len(o)) // 3] = False           # an index rule: a side is not tested against its own triangle — all that indices can tell in a soup
    n = hit.reshape(len(f), 3, len(f)).sum(1)
    noise = int(((n + n.T) > 0).sum() // 2)
    print(f"    soup(sphere960) by an index rule: {noise} pairs; by position: 0")
    assert noise > 1000
