"""No GPU: the oracle of tests/mesh_simplify_common.py against a brute-force grouping and against hand-worked cases of the definition in include/tvr.h (boundary rule,
duplicates, reversed triangles, unused vertices), the argument errors of tvr_mesh_simplify_* (reported before any launch), the symbol list, the ValueErrors, the
no-CPU-fallback rule, the command line, and that export_mesh(simplify=0) never reaches the simplifier."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import mesh_simplify_common as SC

INVALID, UNSUPPORTED = -1, -4


def _same(got, want):
    gv, gf, gm = got
    wv, wf, wm = want
    assert np.array_equal(gm, wm) and np.array_equal(gf, wf)
    assert gv.dtype == np.float32 and wv.dtype == np.float32 and gv.shape == wv.shape
    assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32))


@pytest.mark.parametrize("seed", range(6))
def test_oracle_equals_brute_force_on_random_meshes(seed):
    rng = np.random.default_rng(seed)
    v, f = SC.random_mesh(rng, int(rng.integers(20, 60)), int(rng.integers(10, 80)))
    for cell, origin in ((1.0, (0, 0, 0)), (0.5, (0, 0, 0)), ((1.3, 0.7, 2.0), (-0.25, -0.5, -0.125)), (0.01, (0, 0, 0)), (100.0, (-1, -1, -1))):
        _same(SC.simplify_oracle(v, f, cell, origin), SC.brute_force(v, f, cell, origin))


def test_boundary_belongs_to_the_upper_cell():
    # x = 2.0 with cell 2 lies ON the boundary between cells 0 and 1: it goes with x = 2.5 (cell 1), not with x = 1.5 (cell 0)
    v = np.array([[1.5, 0.5, 0.5], [2.0, 0.5, 0.5], [2.5, 0.5, 0.5], [0.0, 0.0, 0.0]], np.float32)
    pos, faces, vmap = SC.simplify_oracle(v, np.array([[0, 1, 2]]), 2.0)
    assert vmap.tolist() == [0, 1, 1, 0] and len(faces) == 0
    # cell 0 holds vertices 0 and 3: fractions (0.75, 0.25, 0.25) and 0 -> means 0.375, 0.125, 0.125 of a cell of 2
    assert pos.tolist() == [[0.75, 0.25, 0.25], [2.25, 0.5, 0.5]]
    # a vertex exactly at the origin is inside (cell 0); just below it is outside the lattice, and so is NaN
    for bad in ([-1e-6, 0, 0], [0, np.nan, 0], [0, 0, np.inf], [0, 2.0 * 2 ** 21, 0]):
        with pytest.raises(SC.OutsideLattice):
            SC.simplify_oracle(np.array([bad], np.float32), np.zeros((0, 3), np.int64), 2.0)
    SC.simplify_oracle(np.array([[0, 2.0 * (2 ** 21 - 1), 0]], np.float32), np.zeros((0, 3), np.int64), 2.0)
    with pytest.raises(IndexError):
        SC.simplify_oracle(v, np.array([[0, 1, 4]]), 2.0)


def test_duplicates_rotations_and_reversals():
    # vertices 0..2 in three cells, 3..5 their twins in the same cells (cell 1.0)
    base = np.array([[0.25, 0.25, 0.25], [1.25, 0.25, 0.25], [0.25, 1.25, 0.25]], np.float32)      # dyadic: the quantisation is exact
    v = np.concatenate((base, base + np.float32(0.5)))
    faces = np.array([[4, 5, 3], [0, 1, 2], [2, 0, 1], [2, 1, 0], [3, 5, 4], [0, 3, 1], [1, 2, 2]])
    pos, out, vmap = SC.simplify_oracle(v, faces, 1.0)
    assert vmap.tolist() == [0, 1, 2, 0, 1, 2]
    # face 0 maps to (1, 2, 0): it survives in ITS corner order; faces 1 and 2 are rotations of it and go; face 3 is the reversal and stays, face 4 is its
    # rotation and goes; faces 5 and 6 collapse
    assert out.tolist() == [[1, 2, 0], [2, 1, 0]]
    assert np.array_equal(pos, (base + np.float32(0.25)))
    # unused vertices are clustered like any other and every cluster keeps its vertex
    pos, out, vmap = SC.simplify_oracle(np.concatenate((v, np.array([[3.5, 3.5, 3.5]], np.float32))), faces[:2], 1.0)
    assert vmap.tolist() == [0, 1, 2, 0, 1, 2, 3] and len(pos) == 4 and out.tolist() == [[1, 2, 0]]
    # one cell for everything: one vertex, no faces; an empty mesh
    pos, out, vmap = SC.simplify_oracle(v, faces, 8.0)
    assert len(pos) == 1 and len(out) == 0 and vmap.tolist() == [0] * 6
    pos, out, vmap = SC.simplify_oracle(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), 1.0)
    assert pos.shape == (0, 3) and out.shape == (0, 3) and vmap.shape == (0,)


def test_symbols_are_listed_and_exported():
    from jittor_myc_nerfs_amd import _lib as L
    for name in ("tvr_mesh_simplify_scratch_bytes", "tvr_mesh_simplify_count", "tvr_mesh_simplify_emit"):
        assert name in L.SYMBOLS
        assert hasattr(L.lib(), name)
    assert L.lib().tvr_version() == 141


def test_argument_errors_without_gpu():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    lib = L.lib()
    dummy = C.c_void_p(1 << 20)                                      # 256-byte aligned, never dereferenced: every check precedes the launches
    off = C.c_void_p((1 << 20) + 16)
    big = 1 << 40
    V, F = 1000, 3000
    top = 2 ** 31 - 1
    f3 = lambda *x: (C.c_float * 3)(*x)
    org, cell, inv = f3(0, 0, 0), f3(2, 2, 2), f3(.5, .5, .5)

    def refused(rc, code, what):
        assert rc == code, (what, rc, lib.tvr_last_error())
        assert what.encode() in lib.tvr_last_error(), (what, lib.tvr_last_error())

    def count(verts=dummy, nv=V, faces=dummy, nf=F, origin=org, cell=cell, inv_cell=inv, scratch=dummy, scratch_bytes=big, counts=dummy, flag=dummy):
        return lib.tvr_mesh_simplify_count(verts, nv, faces, nf, origin, cell, inv_cell, scratch, scratch_bytes, counts, flag, None)

    def emit(verts=dummy, nv=V, faces=dummy, nf=F, origin=org, cell=cell, inv_cell=inv, scratch=dummy, scratch_bytes=big, vo=dummy, vo_bytes=big, nvo=10, fo=dummy,
             fo_bytes=big, nfo=10, vmap=dummy, vmap_bytes=big, flag=dummy):
        return lib.tvr_mesh_simplify_emit(verts, nv, faces, nf, origin, cell, inv_cell, scratch, scratch_bytes, vo, vo_bytes, nvo, fo, fo_bytes, nfo, vmap, vmap_bytes, flag,
                                          None)

    # scratch: a multiple of 256, linear in the counts (the tables are powers of two: between 2 and 4 slots an element), 0 for counts that are refused
    fn = lib.tvr_mesh_simplify_scratch_bytes
    need = fn(V, F)
    cap_v, cap_t = mesh.simplify_table_capacities(V, F)
    assert (cap_v, cap_t) == (2048, 8192) and mesh.simplify_table_capacities(0, 0) == (256, 256) and mesh.simplify_table_capacities(1024, 1025) == (2048, 4096)
    assert need % 256 == 0 and need >= 256 + 9 * F + 36 * V + 4 * F + 12 * cap_v + 4 * cap_t
    assert fn(0, 0) > 0
    for n in (10 ** 5, 10 ** 6, 10 ** 7):
        assert fn(n, 2 * n) <= 256 * 16 + 1024 * 9 + (84 + 2 * 20 + 2 * 9 + 1) * n, n            # at most 84 B a vertex + 20 B a triangle + 9 B an element
    assert 0 < fn(top, top) < 200 * top
    assert fn(-1, 5) == 0 and b"negative" in lib.tvr_last_error()
    assert fn(5, -1) == 0 and b"negative" in lib.tvr_last_error()
    assert fn(top + 1, 5) == 0 and b"2^31" in lib.tvr_last_error()
    assert fn(5, top + 1) == 0 and b"2^31" in lib.tvr_last_error()
    for call in (count, emit):
        refused(call(nv=-1), INVALID, "negative")
        refused(call(nf=-1), INVALID, "negative")
        refused(call(nv=top + 1), UNSUPPORTED, "2^31")
        refused(call(nf=top + 1), UNSUPPORTED, "2^31")
        for kw in ("verts", "faces", "origin", "cell", "inv_cell", "flag"):
            refused(call(**{kw: None}), INVALID, "NULL")
        refused(call(scratch=None), INVALID, "scratch is NULL")
        refused(call(scratch=off), INVALID, "aligned")
        refused(call(scratch_bytes=need - 1), INVALID, "scratch holds")
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refused(call(cell=f3(2, bad, 2)), INVALID, "positive and finite")
            refused(call(inv_cell=f3(.5, .5, bad)), INVALID, "positive and finite")
        assert call(nv=0, nf=0, verts=None, faces=None, scratch=None) == INVALID                # empty meshes still need their (header) scratch
    refused(count(counts=None), INVALID, "counts_dev is NULL")
    for kw in ("vo", "fo", "vmap"):
        refused(emit(**{kw: None}), INVALID, "NULL")
    refused(emit(vo_bytes=10 * 12 - 1), INVALID, "verts_out holds")
    refused(emit(fo_bytes=10 * 12 - 1), INVALID, "faces_out holds")
    refused(emit(vmap_bytes=V * 4 - 1), INVALID, "vertex_map holds")
    for kw in (dict(nvo=V + 1), dict(nfo=F + 1), dict(nvo=-1), dict(nfo=-1)):
        refused(emit(**kw), INVALID, "outside")


def test_value_errors_and_no_cpu_fallback(tiny_arrays, hyper_tiny, tmp_path):
    from conftest import make_model
    from jittor_myc_nerfs_amd import _lib as L, mesh
    v, f = torch.zeros(4, 3), torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)
    for cell in (0, -1.0, float("nan"), float("inf"), (1.0, 0.0, 1.0), (1.0, 2.0), 1e-46, 1e39):
        with pytest.raises(ValueError, match="cell"):
            mesh.simplify_clustering(v, f, cell)
    with pytest.raises(ValueError, match="origin"):
        mesh.simplify_clustering(v, f, 1.0, origin=(0, 0))
    with pytest.raises(L.TvrError, match="no CPU fallback"):
        mesh.simplify_clustering(v, f, 1.0)
    m = make_model(tiny_arrays, hyper_tiny, device="cpu")
    for s in (0.5, 0.999, -1.0, -0.0001, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="simplify"):
            m.export_mesh(str(tmp_path / "x.ply"), simplify=s)
        with pytest.raises(ValueError, match="simplify"):
            m.mesh_simplify_lattice([16, 20, 24], "reference", s)
    assert not (tmp_path / "x.ply").exists()
    cell, origin = m.mesh_simplify_lattice([16, 20, 24], "reference", 2.0)
    aabb = np.asarray(m.aabb.cpu(), np.float32)
    assert origin == aabb[0].tolist()
    assert cell == [2.0 * float(x) for x in ((aabb[1] - aabb[0]) / np.array([16, 20, 24], np.float32))]
    cell, _ = m.mesh_simplify_lattice([16, 20, 24], "samples", 1.0)
    assert cell == [float(x) for x in ((aabb[1] - aabb[0]) / np.array([15, 19, 23], np.float32))]


def test_export_mesh_reaches_the_simplifier_only_when_asked(tiny_arrays, hyper_tiny, tmp_path, monkeypatch):
    """Marching cubes and the simplifier are replaced by recorders (there is no device here): simplify = 0 writes the file of a call without the keyword and never
    calls the simplifier; simplify = 2 calls it once, after the component filter, with the export's lattice, and writes what it returns."""
    from conftest import make_model
    from jittor_myc_nerfs_amd import mesh, read_ply
    m = make_model(tiny_arrays, hyper_tiny, device="cpu")
    verts = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32)
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    calls = []
    monkeypatch.setattr(m, "getDenseAlpha", lambda gridSize=None: (torch.zeros(16, 20, 24), None))
    monkeypatch.setattr(mesh, "marching_cubes", lambda *a, **k: (verts, faces))

    def recorder(v, f, cell, origin=(0, 0, 0), stats=None):
        calls.append((v, f, cell, origin))
        stats.update(vertices_in=4, vertices_out=3, triangles_in=2, triangles_out=1, max_probe=1, table_capacity=256)
        return v[:3], f[:1], torch.tensor([0, 1, 2, 2], dtype=torch.int32)

    monkeypatch.setattr(mesh, "simplify_clustering", recorder)
    p0, p1, p2 = (str(tmp_path / f"{i}.ply") for i in range(3))
    m.export_mesh(p0)
    m.export_mesh(p1, simplify=0.0)
    assert calls == [] and m.mesh_export_stats == {}
    assert open(p0, "rb").read() == open(p1, "rb").read()
    v2, f2 = m.export_mesh(p2, simplify=2.0)
    assert len(calls) == 1 and calls[0][0] is verts and calls[0][1] is faces
    assert (calls[0][2], calls[0][3]) == tuple(m.mesh_simplify_lattice([16, 20, 24], "reference", 2.0))
    assert m.mesh_export_stats["triangles_out"] == 1 and m.mesh_export_stats["vertices_out"] == 3
    rv, rf = read_ply(p2)
    assert np.array_equal(rv, verts[:3].numpy()) and np.array_equal(rf, faces[:1].numpy()) and torch.equal(v2, verts[:3]) and torch.equal(f2, faces[:1])
    assert inspect.signature(type(m).export_mesh).parameters["simplify"].default == 0.0


def test_command_line_option(tmp_path):
    from jittor_myc_nerfs_amd import reconstruct as R
    assert R.config_parser([]).mesh_simplify == 0.0
    a = R.config_parser(["--export_mesh", "1", "--mesh_simplify", "2.5"])
    assert a.export_mesh == 1 and a.mesh_simplify == 2.5 and isinstance(a.mesh_simplify, float)
    cfg = tmp_path / "c.txt"
    cfg.write_text("export_mesh = 1\nmesh_simplify = 3\nmesh_keep_largest = 1\n")
    a = R.config_parser(["--config", str(cfg)])
    assert a.mesh_simplify == 3.0 and a.mesh_keep_largest == 1
