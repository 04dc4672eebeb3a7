"""CPU: the marching-cubes case table (scripts/gen_mc_table.py -> csrc/tvr_mc_table.h), the PLY reader / writer, the argument errors of the tvr_mesh_* entry
points (reported before any launch, so reachable with no GPU) and the `--export_mesh` command line.  The table is checked against the face rule restated HERE
(marching squares per face; four cut edges: every inside corner cut off on its own), not against the generator's own construction."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mesh_common as MC
from conftest import ROOT


@pytest.fixture(scope="module")
def gen():
    return MC.load_generator()


@pytest.fixture(scope="module")
def table(gen):
    tri, cnt = gen.build_table()
    return tri, cnt, [lo for lo, _ in gen.EDGE_CORNERS]


def test_committed_header_is_the_generators_output(gen):
    with open(os.path.join(ROOT, "jittor-myc-nerfs_amd", "csrc", "tvr_mc_table.h")) as f:
        assert f.read() == gen.header_text()


def _edge(a, b):
    return (min(a, b), max(a, b))


# the cell's geometry restated: corner c at (c & 1, (c >> 1) & 1, (c >> 2) & 1); an edge joins two corners that differ in one bit; a face fixes one coordinate
CELL_EDGES = sorted(_edge(a, a ^ (1 << bit)) for a in range(8) for bit in range(3) if not a & (1 << bit))
FACES = [[c for c in range(8) if ((c >> axis) & 1) == side] for axis in range(3) for side in (0, 1)]


def _expected_face_segments(case, corners):
    """Undirected marching-squares segments of one face, as pairs of cell edges (each a corner pair)."""
    inside = lambda c: (case >> c) & 1
    edges = [e for e in CELL_EDGES if e[0] in corners and e[1] in corners]
    assert len(edges) == 4
    cut = [e for e in edges if inside(e[0]) != inside(e[1])]
    if len(cut) == 0:
        return []
    if len(cut) == 2:
        return [frozenset(cut)]
    assert len(cut) == 4
    return [frozenset(e for e in cut if c in e) for c in corners if inside(c)]


def test_table_properties_of_every_case(gen, table):
    tri, cnt, _ = table
    assert len(gen.EDGE_CORNERS) == 12 and sorted(_edge(a, b) for a, b in gen.EDGE_CORNERS) == CELL_EDGES
    assert all(lo < hi and hi == lo | (1 << (e >> 2)) for e, (lo, hi) in enumerate(gen.EDGE_CORNERS))          # edge e runs along axis e >> 2 from its owner corner
    assert cnt[0] == 0 and cnt[255] == 0 and (tri[0] == -1).all() and (tri[255] == -1).all()
    assert int(cnt.max()) <= gen.MAX_TRIS
    for case in range(256):
        tris = [tuple(int(x) for x in t) for t in tri[case][:cnt[case]]]
        assert (tri[case][cnt[case]:] == -1).all()
        cut = {e for e, (a, b) in enumerate(gen.EDGE_CORNERS) if ((case >> a) & 1) != ((case >> b) & 1)}
        used = {e for t in tris for e in t}
        assert used == cut, (case, used, cut)                                        # only cut edges, and every cut edge
        assert all(len(set(t)) == 3 for t in tris)
        directed = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
        assert len(set(directed)) == len(directed), case                              # no directed edge twice inside a cell
        # every triangle side that lies in a face of the cell is a marching-squares segment of that face, and each such segment is there once:
        # in particular no diagonal of a fan lies in a face, where the neighbouring cell could lay one of its own on the same two edges
        boundary = [d for d in directed if (d[1], d[0]) not in directed]
        interior = [d for d in directed if (d[1], d[0]) in directed]
        for corners in FACES:
            in_face = lambda e: set(gen.EDGE_CORNERS[e]) <= set(corners)
            got = sorted(sorted(_edge(*gen.EDGE_CORNERS[e]) for e in d) for d in boundary if in_face(d[0]) and in_face(d[1]))
            want = sorted(sorted(s) for s in _expected_face_segments(case, corners))
            assert got == want, (case, corners, got, want)
            assert not any(in_face(a) and in_face(b) for a, b in interior), (case, corners)
        # the boundary is a set of closed directed loops: one side arrives at and one leaves every cut edge
        assert sorted(a for a, _ in boundary) == sorted(cut) and sorted(b for _, b in boundary) == sorted(cut), case
    print(f"    {int(cnt.sum())} triangles over the 256 cases, at most {int(cnt.max())} per case")


def test_table_on_whole_volumes_on_the_cpu(table):
    """The table applied by numpy (mesh_common.numpy_marching_cubes): closed and consistently oriented on noise that holds all 256 cases, the right Euler
    characteristics, outward orientation — the checks tests/test_gpu_mesh.py makes on the kernels' output, made here on the table alone."""
    tri, cnt, lo = table
    vol = MC.noise_volume((24, 20, 18))
    hist = MC.all_cases_occur(vol, 0.5)
    assert (hist > 0).all()
    print(f"    rarest case occurs {int(hist.min())} times")
    v, f = MC.numpy_marching_cubes(vol, 0.5, tri, cnt, lo)
    assert len(v) == int(MC.straddle_masks(vol, 0.5).sum())
    MC.assert_closed_and_oriented(f, len(v))
    for vol, chi in ((MC.sphere_volume(), 2), (MC.torus_volume(), 0), (MC.two_spheres_volume(), 4)):
        v, f = MC.numpy_marching_cubes(vol, 0.0, tri, cnt, lo)
        MC.assert_closed_and_oriented(f, len(v))
        assert MC.euler_characteristic(len(v), f) == chi
    vol = MC.sphere_volume()
    v, f = MC.numpy_marching_cubes(vol, 0.0, tri, cnt, lo)
    lo_cells, hi_cells = MC.cell_count_bounds(vol, 0.0)
    sv = MC.signed_volume(v, f)
    print(f"    sphere: {lo_cells} <= {sv:.1f} <= {hi_cells}")
    assert 0 < lo_cells <= sv <= hi_cells


# ---- PLY ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_ply_header_bytes_and_round_trip(tmp_path):
    from jittor_myc_nerfs_amd import mesh
    verts = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, -2.25], [0.0, 3.0e-7, 1.0], [-1.0e9, 2.0, 0.1]], np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    path = tmp_path / "m.ply"
    mesh.write_ply(path, torch.tensor(verts), torch.tensor(faces))
    data = path.read_bytes()
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
              b"element face 2\nproperty list uchar int vertex_indices\nend_header\n")
    assert data[:len(header)] == header
    body = data[len(header):]
    assert body[:48] == verts.astype("<f4").tobytes()
    assert body[48:] == b"".join(b"\x03" + row.astype("<i4").tobytes() for row in faces) and len(body) == 48 + 2 * 13
    v, f = mesh.read_ply(path)
    assert v.dtype == np.float32 and f.dtype == np.int32 and np.array_equal(v, verts) and np.array_equal(f, faces)
    mesh.write_ply(path, verts[:0], faces[:0])                                   # an empty mesh is a valid file
    v, f = mesh.read_ply(path)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    path.write_bytes(header.replace(b"float x", b"double x") + body)
    with pytest.raises(ValueError):
        mesh.read_ply(path)
    path.write_bytes(header + body[:-1])
    with pytest.raises(ValueError):
        mesh.read_ply(path)


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------------------------------
INVALID, UNSUPPORTED = -1, -4


def test_mesh_argument_errors_without_gpu():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    dims = lambda *d: (C.c_int32 * 3)(*d)
    dummy = C.c_void_p(1 << 20)                                      # 256-byte aligned, never dereferenced: every check precedes the launches
    org, sp = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    big = 1 << 40
    d = dims(24, 20, 18)
    points = 24 * 20 * 18
    need = lib.tvr_mesh_scratch_bytes(d)
    tiles = -(-points // 1024)
    assert need >= 256 + tiles * 8 + tiles * 1024 * 9 and need % 256 == 0                 # header, tile bases, one byte and two words per point of whole tiles
    assert lib.tvr_mesh_scratch_bytes(dims(2, 2, 2)) > 0

    def count(volume=dummy, dd=d, scratch=dummy, scratch_bytes=big, counts=dummy):
        return lib.tvr_mesh_count(volume, dd, 0.5, scratch, scratch_bytes, counts, None)

    def emit(volume=dummy, dd=d, origin=org, spacing=sp, scratch=dummy, scratch_bytes=big, verts=dummy, verts_bytes=big, nv=10, faces=dummy, faces_bytes=big,
             nt=10, flag=dummy):
        return lib.tvr_mesh_emit(volume, dd, 0.5, origin, spacing, scratch, scratch_bytes, verts, verts_bytes, nv, faces, faces_bytes, nt, 0, flag, None)

    def refused(rc, code, what):
        assert rc == code, (what, rc, lib.tvr_last_error())
        assert what.encode() in lib.tvr_last_error(), (what, lib.tvr_last_error())

    # NULL pointers
    assert lib.tvr_mesh_scratch_bytes(None) == 0 and b"dims" in lib.tvr_last_error()
    refused(count(dd=None), INVALID, "dims")
    refused(count(volume=None), INVALID, "NULL")
    refused(count(counts=None), INVALID, "NULL")
    refused(count(scratch=None), INVALID, "scratch is NULL")
    refused(emit(dd=None), INVALID, "dims")
    for kw in ("volume", "origin", "spacing", "flag"):
        refused(emit(**{kw: None}), INVALID, "NULL")
    refused(emit(scratch=None), INVALID, "scratch is NULL")
    refused(emit(verts=None), INVALID, "verts / faces is NULL")
    refused(emit(faces=None), INVALID, "verts / faces is NULL")
    # a dimension below 2
    for bad in (dims(1, 20, 18), dims(24, 0, 18), dims(24, 20, -3)):
        assert lib.tvr_mesh_scratch_bytes(bad) == 0 and b"at least 2" in lib.tvr_last_error()
        refused(count(dd=bad), INVALID, "at least 2")
        refused(emit(dd=bad), INVALID, "at least 2")
    # undersized or misaligned buffers
    refused(count(scratch_bytes=need - 1), INVALID, "scratch holds")
    refused(emit(scratch_bytes=need - 1), INVALID, "scratch holds")
    refused(count(scratch=C.c_void_p((1 << 20) + 16)), INVALID, "aligned")
    refused(emit(verts_bytes=10 * 12 - 1), INVALID, "verts holds")
    refused(emit(faces_bytes=10 * 12 - 1), INVALID, "faces holds")
    refused(emit(nv=-1), INVALID, "outside")
    refused(emit(nv=3 * points + 1), INVALID, "outside")
    refused(emit(nt=5 * points + 1), INVALID, "outside")
    # int32 indices: 3 * points must stay below 2^31
    huge = dims(895, 895, 894)                                       # 716 127 350 points: 3 x that is 2 148 382 050 >= 2^31
    assert 3 * 895 * 895 * 894 >= 2 ** 31 > 3 * 894 * 894 * 894
    assert lib.tvr_mesh_scratch_bytes(huge) == 0 and b"2^31" in lib.tvr_last_error()
    refused(count(dd=huge), UNSUPPORTED, "2^31")
    refused(emit(dd=huge), UNSUPPORTED, "2^31")
    assert lib.tvr_mesh_scratch_bytes(dims(894, 894, 894)) > 9 * 894 ** 3


def test_tile_constants_agree_with_the_header():
    from jittor_myc_nerfs_amd import mesh
    src = open(os.path.join(ROOT, "include", "tvr.h")).read()
    assert int(re.search(r"#define TVR_MESH_TILE (\d+)", src).group(1)) == mesh.MESH_TILE
    assert int(re.search(r"#define TVR_MESH_SCAN_CHUNK (\d+)", src).group(1)) == mesh.MESH_SCAN_CHUNK


def test_marching_cubes_has_no_cpu_fallback():
    import jittor_myc_nerfs_amd as J
    from jittor_myc_nerfs_amd import _lib as L
    assert J.marching_cubes is J.mesh.marching_cubes and J.write_ply is J.mesh.write_ply and J.read_ply is J.mesh.read_ply
    with pytest.raises(L.TvrError, match="no CPU fallback"):
        J.marching_cubes(torch.zeros(4, 4, 4), 0.5)
    assert hasattr(J.TensorBase, "export_mesh")


# ---- command line ---------------------------------------------------------------------------------------------------------------------------------------------
def test_export_mesh_command_line(tmp_path):
    from jittor_myc_nerfs_amd import reconstruct as R
    a = R.config_parser([])
    assert a.mesh_level == 0.0005 and a.mesh_grid is None and a.export_mesh == 0
    cfg = tmp_path / "c.txt"
    cfg.write_text("export_mesh = 1\nmesh_level = 0.005\nmesh_grid = [64, 48, 32]\n")
    a = R.config_parser(["--config", str(cfg)])
    assert a.export_mesh == 1 and a.mesh_level == 0.005 and a.mesh_grid == [64, 48, 32]
    # a missing checkpoint: the command says so; it is no longer refused as not implemented, and it starts no training run
    with pytest.raises(FileNotFoundError, match="checkpoint"):
        R.main(["--export_mesh", "1", "--ckpt", str(tmp_path / "missing.th")])
    with pytest.raises(FileNotFoundError, match="checkpoint"):
        R.main(["--export_mesh", "1"])
