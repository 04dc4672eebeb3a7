"""CPU: the PLY vertex attributes (mesh.write_ply / read_ply_attributes), the new command-line options, and the argument checks of tvr_density_gradient that come
before any launch (so they can be reached with no GPU) — plus: none of the new entry points has a CPU fallback."""
import ctypes as C

import numpy as np
import pytest
import torch


BASE = b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
NORMALS = b"property float nx\nproperty float ny\nproperty float nz\n"
COLORS = b"property uchar red\nproperty uchar green\nproperty uchar blue\n"
TAIL = b"element face 1\nproperty list uchar int vertex_indices\nend_header\n"

VERTS = np.array([[0.0, 0.25, -1.5], [1.0, 2.0, 3.0], [-4.0, 5.5, 6.0]], np.float32)
FACES = np.array([[0, 1, 2]], np.int32)
NRM = np.array([[0.0, 0.0, 1.0], [0.6, 0.8, 0.0], [-1.0, 0.0, 0.0]], np.float32)
COL = np.array([[0, 128, 255], [1, 2, 3], [250, 251, 252]], np.uint8)


def _plain_bytes():
    """today's file, restated: header, 12 B per vertex, 13 B per face"""
    return BASE + TAIL + VERTS.tobytes() + b"\x03" + FACES.tobytes()


@pytest.mark.parametrize("with_n,with_c", [(False, False), (True, False), (False, True), (True, True)])
def test_header_bytes_body_layout_and_round_trip(tmp_path, with_n, with_c):
    from jittor_myc_nerfs_amd import mesh, read_ply, read_ply_attributes
    path = str(tmp_path / "m.ply")
    mesh.write_ply(path, VERTS, FACES, normals=NRM if with_n else None, colors=COL if with_c else None)
    data = open(path, "rb").read()
    header = BASE + (NORMALS if with_n else b"") + (COLORS if with_c else b"") + TAIL
    assert data.startswith(header) and mesh.ply_header(3, 1, with_n, with_c) == header
    body = b""
    for i in range(3):                                   # one vertex after the other: x y z [nx ny nz] [r g b], little endian, no padding
        body += VERTS[i].tobytes() + (NRM[i].tobytes() if with_n else b"") + (COL[i].tobytes() if with_c else b"")
    assert data == header + body + b"\x03" + FACES.tobytes()
    v, f, attrs = read_ply_attributes(path)
    assert np.array_equal(v, VERTS) and np.array_equal(f, FACES) and v.dtype == np.float32 and f.dtype == np.int32
    assert sorted(attrs) == sorted((["normals"] if with_n else []) + (["colors"] if with_c else []))
    if with_n:
        assert np.array_equal(attrs["normals"], NRM) and attrs["normals"].dtype == np.float32
    if with_c:
        assert np.array_equal(attrs["colors"], COL) and attrs["colors"].dtype == np.uint8
    if with_n or with_c:
        with pytest.raises(ValueError):                  # read_ply stays the reader of the reference's subset
            read_ply(path)
    else:
        assert data == _plain_bytes()
        v0, f0 = read_ply(path)
        assert np.array_equal(v0, VERTS) and np.array_equal(f0, FACES)


def test_write_ply_without_attributes_is_unchanged(tmp_path):
    from jittor_myc_nerfs_amd import mesh
    a, b, c = (str(tmp_path / n) for n in ("a.ply", "b.ply", "c.ply"))
    mesh.write_ply(a, VERTS, FACES)
    mesh.write_ply(b, VERTS, FACES, None, None)
    mesh.write_ply(c, torch.as_tensor(VERTS), torch.as_tensor(FACES), normals=None, colors=None)
    assert open(a, "rb").read() == _plain_bytes() == open(b, "rb").read() == open(c, "rb").read()
    assert mesh.ply_header(3, 1) == BASE + TAIL
    # tensors and arrays write the same attribute bytes; an empty mesh keeps its header
    mesh.write_ply(a, VERTS, FACES, normals=NRM, colors=COL)
    mesh.write_ply(b, torch.as_tensor(VERTS), torch.as_tensor(FACES), normals=torch.as_tensor(NRM), colors=torch.as_tensor(COL))
    assert open(a, "rb").read() == open(b, "rb").read()
    mesh.write_ply(a, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), normals=np.zeros((0, 3), np.float32), colors=np.zeros((0, 3), np.uint8))
    v, f, attrs = mesh.read_ply_attributes(a)
    assert v.shape == (0, 3) and f.shape == (0, 3) and attrs["normals"].shape == (0, 3) and attrs["colors"].shape == (0, 3)
    with pytest.raises(ValueError):
        mesh.write_ply(a, VERTS, FACES, normals=NRM[:2])
    with pytest.raises(ValueError):
        mesh.write_ply(a, VERTS, FACES, colors=COL.astype(np.float32) / 255.0)          # colours are bytes, not unit floats


def test_read_ply_attributes_refuses_everything_else(tmp_path):
    from jittor_myc_nerfs_amd import mesh, read_ply_attributes
    path = str(tmp_path / "m.ply")
    mesh.write_ply(path, VERTS, FACES, normals=NRM, colors=COL)
    data = open(path, "rb").read()
    bad = str(tmp_path / "bad.ply")

    def refused(blob):
        open(bad, "wb").write(blob)
        with pytest.raises(ValueError):
            read_ply_attributes(bad)

    refused(data[:-1])                                                       # truncated body
    refused(data[:-13])                                                      # a whole face short
    refused(data + b"\x00")                                                  # trailing bytes
    refused(data[:60])                                                       # no end_header
    refused(b"plx" + data[3:])
    refused(data.replace(b"property uchar blue\n", b"property uchar blue\nproperty uchar alpha\n"))       # an unknown property
    refused(data.replace(b"property float nx", b"property float s"))
    refused(data.replace(COLORS + TAIL, TAIL).replace(NORMALS, COLORS + NORMALS))      # known properties in another order
    refused(data.replace(b"binary_little_endian", b"binary_big_endian"))
    refused(data.replace(b"property float nz\n", b""))                       # two of three normal components
    refused(data.replace(b"element face 1", b"element face 1\nelement edge 0"))
    quad = bytearray(data)
    quad[len(data) - 13] = 4                                                 # the face's count byte
    refused(bytes(quad))


def test_new_options_default_to_off(tmp_path):
    from jittor_myc_nerfs_amd import reconstruct as R
    a = R.config_parser([])
    assert a.mesh_normals == 0 and a.mesh_colors == 0
    a = R.config_parser(["--mesh_normals", "1"])
    assert a.mesh_normals == 1 and a.mesh_colors == 0
    cfg = tmp_path / "mesh.txt"
    cfg.write_text("export_mesh = 1\nmesh_normals = 1\nmesh_colors = 1\n")
    a = R.config_parser(["--config", str(cfg)])
    assert a.export_mesh == 1 and a.mesh_normals == 1 and a.mesh_colors == 1


def test_density_gradient_argument_errors_without_gpu():
    """As test_abi_refuses_undersized_output_buffers_without_gpu does for its siblings: the byte counts are checked first, so a buffer one float short is
    TVR_ERR_SCRATCH (-3) even with no scene; with the sizes right the next check (no scene) answers with TVR_ERR_INVALID (-1)."""
    from jittor_myc_nerfs_amd import _lib as L
    lib, m = L.lib(), 1000
    dummy = C.c_void_p(4096)                                                 # never dereferenced
    h = (C.c_float * 3)(0.1, 0.1, 0.1)
    assert lib.tvr_density_gradient(None, dummy, m, C.byref(h), dummy, m * 4, dummy, m * 12 - 4, None) == -3
    assert b"grad [m,3]" in lib.tvr_last_error() and b"tvr_density_gradient" in lib.tvr_last_error()
    assert lib.tvr_density_gradient(None, dummy, m, C.byref(h), dummy, m * 4 - 4, dummy, m * 12, None) == -3
    assert b"sigma_feature [m]" in lib.tvr_last_error()
    assert lib.tvr_density_gradient(None, dummy, m, C.byref(h), None, 0, dummy, m * 4, None) == -3          # [m] where [m,3] is written
    assert lib.tvr_density_gradient(None, dummy, m, C.byref(h), None, 0, dummy, m * 12, None) == -1         # sigma_feature may be NULL: its size is not looked at
    assert b"scene" in lib.tvr_last_error()
    assert lib.tvr_density_gradient(None, dummy, m, C.byref(h), dummy, m * 4, dummy, m * 12, None) == -1
    assert lib.tvr_density_gradient(None, None, 0, None, None, 0, None, 0, None) == -1                       # m == 0 still needs a scene


def test_new_entry_points_have_no_cpu_fallback(tiny_arrays, hyper_tiny, tmp_path):
    import jittor_myc_nerfs_amd as J
    from conftest import make_model
    from jittor_myc_nerfs_amd._lib import TvrError
    assert hasattr(J, "read_ply_attributes")
    m = make_model(tiny_arrays, hyper_tiny, device="cpu")
    pts = torch.zeros((4, 3))
    for call in (lambda: m.compute_density_gradient(pts), lambda: m.compute_density_gradient(pts, half_width=0.1), lambda: m.surface_normals(pts),
                 lambda: m.mesh_vertex_attributes(pts), lambda: m.mesh_vertex_attributes(pts[:0]),
                 lambda: m.export_mesh(str(tmp_path / "x.ply"), normals=True, colors=True)):
        with pytest.raises(TvrError):
            call()
    assert not (tmp_path / "x.ply").exists()
