"""No GPU: the oracle of tests/mesh_components_common.py against the anchored fixture values, the size policy (mesh.component_keep_mask on CPU tensors), the argument
errors of tvr_mesh_components / tvr_mesh_filter_* (reported before any launch), the pass-through and no-CPU-fallback rules, the command line."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_components_common as CM

INVALID, UNSUPPORTED = -1, -4


def _sizes(name):
    v, f = CM.cpu_mesh(name)
    label, sizes, n = CM.components_oracle(f, len(v))
    return len(v), len(f), label, sizes, n


def test_fixtures_agree_with_the_oracle():
    V, F, label, sizes, n = _sizes("two_spheres")
    assert (V, F, n) == (290, 572, 2) and sorted(sizes[sizes > 0].tolist()) == [272, 300]
    V, F, label, sizes, n = _sizes("noise")
    s = sizes[label == np.arange(V)]
    assert F == 20868 and n == 87 and s.max() == 19888 and int((s == 8).sum()) == 68 and int((s == 32).sum()) == 2 and s.sum() == F
    V, F, label, sizes, n = _sizes("integer")
    s = sizes[label == np.arange(V)]
    assert n == 16 and int((s == 32).sum()) == 2 and s.max() == 3072
    for name in CM.VOLUMES:                                               # what the definitions say of every labelling
        V, F, label, sizes, n = _sizes(name)
        f = CM.cpu_mesh(name)[1]
        assert (label <= np.arange(V)).all() and (label[label] == label).all()
        assert (label[f[:, 0]] == label[f[:, 1]]).all() and (label[f[:, 1]] == label[f[:, 2]]).all()
        assert sizes.sum() == F and (sizes[label != np.arange(V)] == 0).all()


@pytest.mark.parametrize("name", ["two_spheres", "noise", "integer"])
def test_policy_on_cpu_tensors_equals_the_oracle(name):
    from jittor_myc_nerfs_amd import mesh
    V, F, label, sizes, n = _sizes(name)
    tl, ts = torch.as_tensor(label, dtype=torch.int32), torch.as_tensor(sizes, dtype=torch.int32)
    for m, k in [(0, 0)] + CM.POLICY_GRID:
        got = mesh.component_keep_mask(tl, ts, min_faces=m, keep_largest=k)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (V,)
        assert np.array_equal(got.numpy(), CM.keep_oracle(label, sizes, m, k)), (name, m, k)
    assert int(mesh.component_keep_mask(tl, ts).sum()) == n               # both options off: every component


def test_policy_ties_go_to_the_smaller_label():
    from jittor_myc_nerfs_amd import mesh
    V, F, label, sizes, n = _sizes("integer")
    tl, ts = torch.as_tensor(label, dtype=torch.int32), torch.as_tensor(sizes, dtype=torch.int32)
    tied = np.nonzero(sizes == 32)[0]
    big = int(np.nonzero(sizes == 3072)[0][0])
    assert len(tied) == 2
    k3 = np.nonzero(mesh.component_keep_mask(tl, ts, keep_largest=3).numpy())[0]
    assert sorted(k3.tolist()) == sorted([big, int(tied[0]), int(tied[1])])
    k2 = np.nonzero(mesh.component_keep_mask(tl, ts, keep_largest=2).numpy())[0]
    assert sorted(k2.tolist()) == sorted([big, int(tied.min())])
    # unused vertices are components of zero faces: kept only with both options off
    lab = torch.arange(5, dtype=torch.int32)
    siz = torch.tensor([0, 2, 0, 2, 0], dtype=torch.int32)
    assert mesh.component_keep_mask(lab, siz).tolist() == [1, 1, 1, 1, 1]
    assert mesh.component_keep_mask(lab, siz, min_faces=1).tolist() == [0, 1, 0, 1, 0]
    assert mesh.component_keep_mask(lab, siz, keep_largest=4).tolist() == [0, 1, 0, 1, 0]
    assert mesh.component_keep_mask(lab, siz, keep_largest=1).tolist() == [0, 1, 0, 0, 0]
    for kw in (dict(min_faces=-1), dict(keep_largest=-1)):
        with pytest.raises(ValueError, match="negative"):
            mesh.component_keep_mask(lab, siz, **kw)
        with pytest.raises(ValueError, match="negative"):
            mesh.filter_components(torch.zeros(5, 3), torch.zeros(0, 3, dtype=torch.int32), **kw)


def test_argument_errors_without_gpu():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    dummy = C.c_void_p(1 << 20)                                      # 256-byte aligned, never dereferenced: every check precedes the launches
    big = 1 << 40
    V, F = 1000, 3000
    top = 2 ** 31 - 1

    def refused(rc, code, what):
        assert rc == code, (what, rc, lib.tvr_last_error())
        assert what.encode() in lib.tvr_last_error(), (what, lib.tvr_last_error())

    def comp(faces=dummy, nf=F, nv=V, label=dummy, label_bytes=big, sizes=dummy, sizes_bytes=big, ncomp=dummy, scratch=dummy, scratch_bytes=big, flag=dummy):
        return lib.tvr_mesh_components(faces, nf, nv, label, label_bytes, sizes, sizes_bytes, ncomp, scratch, scratch_bytes, flag, None)

    def count(faces=dummy, nf=F, nv=V, label=dummy, keep=dummy, scratch=dummy, scratch_bytes=big, counts=dummy, flag=dummy):
        return lib.tvr_mesh_filter_count(faces, nf, nv, label, keep, scratch, scratch_bytes, counts, flag, None)

    def emit(verts=dummy, faces=dummy, nf=F, nv=V, scratch=dummy, scratch_bytes=big, vo=dummy, vo_bytes=big, nvo=10, fo=dummy, fo_bytes=big, nfo=10, kept=dummy,
             kept_bytes=big, flag=dummy):
        return lib.tvr_mesh_filter_emit(verts, faces, nf, nv, scratch, scratch_bytes, vo, vo_bytes, nvo, fo, fo_bytes, nfo, kept, kept_bytes, flag, None)

    # scratch sizes; 0 for counts that are refused
    need_c, need_f = lib.tvr_mesh_components_scratch_bytes(V, F), lib.tvr_mesh_filter_scratch_bytes(V, F)
    tiles = -(-F // 1024)
    assert need_c >= 8 and need_c % 256 == 0
    assert need_f >= 256 + tiles * 8 + tiles * 1024 * 9 and need_f % 256 == 0
    assert lib.tvr_mesh_components_scratch_bytes(0, 0) > 0 and lib.tvr_mesh_filter_scratch_bytes(0, 0) > 0
    assert lib.tvr_mesh_filter_scratch_bytes(top, top) > 9 * top
    for fn in (lib.tvr_mesh_components_scratch_bytes, lib.tvr_mesh_filter_scratch_bytes):
        assert fn(-1, 5) == 0 and b"negative" in lib.tvr_last_error()
        assert fn(5, -1) == 0 and b"negative" in lib.tvr_last_error()
        assert fn(top + 1, 5) == 0 and b"2^31" in lib.tvr_last_error()
        assert fn(5, top + 1) == 0 and b"2^31" in lib.tvr_last_error()
    # negative counts, int32 indices
    for call in (comp, count, emit):
        refused(call(nv=-1), INVALID, "negative")
        refused(call(nf=-1), INVALID, "negative")
        refused(call(nv=top + 1), UNSUPPORTED, "2^31")
        refused(call(nf=top + 1), UNSUPPORTED, "2^31")
    # NULL pointers
    for kw in ("faces", "label", "sizes", "ncomp", "flag"):
        refused(comp(**{kw: None}), INVALID, "NULL")
    refused(comp(scratch=None), INVALID, "scratch is NULL")
    for kw in ("faces", "label", "keep", "counts", "flag"):
        refused(count(**{kw: None}), INVALID, "NULL")
    refused(count(scratch=None), INVALID, "scratch is NULL")
    for kw in ("faces", "vo", "fo", "kept", "flag"):
        refused(emit(**{kw: None}), INVALID, "NULL")
    refused(emit(scratch=None), INVALID, "scratch is NULL")
    # undersized or misaligned buffers
    off = C.c_void_p((1 << 20) + 16)
    refused(comp(label_bytes=V * 4 - 1), INVALID, "vertex_label holds")
    refused(comp(sizes_bytes=V * 4 - 1), INVALID, "vertex_label holds")
    refused(comp(scratch_bytes=need_c - 1), INVALID, "scratch holds")
    refused(comp(scratch=off), INVALID, "aligned")
    refused(count(scratch_bytes=need_f - 1), INVALID, "scratch holds")
    refused(count(scratch=off), INVALID, "aligned")
    refused(emit(scratch_bytes=need_f - 1), INVALID, "scratch holds")
    refused(emit(scratch=off), INVALID, "aligned")
    refused(emit(vo_bytes=10 * 12 - 1), INVALID, "verts_out holds")
    refused(emit(fo_bytes=10 * 12 - 1), INVALID, "faces_out holds")
    refused(emit(kept_bytes=10 * 4 - 1), INVALID, "kept_vertex holds")
    # declared counts above V / F
    refused(emit(nvo=V + 1), INVALID, "outside")
    refused(emit(nfo=F + 1), INVALID, "outside")
    refused(emit(nvo=-1), INVALID, "outside")
    refused(emit(nfo=-1), INVALID, "outside")


def test_defaults_pass_the_inputs_through():
    from jittor_myc_nerfs_amd import mesh
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    v2, f2, kept = mesh.filter_components(v, f)
    assert v2 is v and f2 is f and kept is None
    v2, f2, kept = mesh.filter_components(v, f, min_faces=0, keep_largest=0)
    assert v2 is v and f2 is f and kept is None


def test_no_cpu_fallback():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    v, f = torch.zeros(4, 3), torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)
    for call in (lambda: mesh.filter_components(v, f, min_faces=1), lambda: mesh.filter_components(v, f, keep_largest=1), lambda: mesh.mesh_components(f, 4)):
        with pytest.raises(L.TvrError, match="no CPU fallback"):
            call()


def test_command_line_options(tmp_path):
    import inspect
    from jittor_myc_nerfs_amd import TensorBase, reconstruct as R
    a = R.config_parser([])
    assert a.mesh_min_faces == 0 and a.mesh_keep_largest == 0
    a = R.config_parser(["--mesh_min_faces", "50", "--mesh_keep_largest", "2"])
    assert a.mesh_min_faces == 50 and a.mesh_keep_largest == 2
    cfg = tmp_path / "c.txt"
    cfg.write_text("export_mesh = 1\nmesh_min_faces = 7\nmesh_keep_largest = 1\n")
    a = R.config_parser(["--config", str(cfg)])
    assert a.export_mesh == 1 and a.mesh_min_faces == 7 and a.mesh_keep_largest == 1
    sig = inspect.signature(TensorBase.export_mesh).parameters
    assert sig["min_component_faces"].default == 0 and sig["keep_largest"].default == 0
