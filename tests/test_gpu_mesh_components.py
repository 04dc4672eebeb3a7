"""GPU (-m gpu): connected components of a mesh and the component filter (csrc/tvr_mesh_cc.hip through mesh.mesh_components / mesh.filter_components) and the export
paths built on them.  The oracle is tests/mesh_components_common.py (numpy, restated from the definitions); every comparison is np.array_equal / torch.equal —
labels, sizes and indices are integers and the surviving coordinates are copies."""
import functools

import numpy as np
import pytest
import torch

import mesh_common as MC
import mesh_components_common as CM
from conftest import TINY, make_model

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def _verts_for(n):
    """distinct, exactly representable coordinates for index-only meshes (n < 2^24 / 3)"""
    return torch.arange(3 * n, dtype=torch.float32, device="cuda").view(n, 3)


def _check_components(faces_t, V, stats=None):
    """labels, sizes and the count against the oracle; -> (label, sizes) as numpy"""
    from jittor_myc_nerfs_amd import mesh
    label, sizes, n = mesh.mesh_components(faces_t, V, stats=stats)
    assert label.is_cuda and label.dtype == torch.int32 and sizes.dtype == torch.int32 and tuple(label.shape) == (V,) and tuple(sizes.shape) == (V,)
    wl, ws, wn = CM.components_oracle(_np(faces_t), V)
    assert np.array_equal(_np(label), wl) and np.array_equal(_np(sizes), ws) and n == wn
    return wl, ws


def _check_filter(verts_t, faces_t, label, sizes, m, k):
    """filter_components against the oracle's filtered mesh -> (verts', faces') tensors"""
    from jittor_myc_nerfs_amd import mesh
    st = {}
    v2, f2, kept = mesh.filter_components(verts_t, faces_t, min_faces=m, keep_largest=k, stats=st)
    keep = CM.keep_oracle(label, sizes, m, k)
    wv, wf, wk = CM.filter_oracle(_np(verts_t), _np(faces_t), label, keep)
    assert v2.dtype == torch.float32 and f2.dtype == torch.int32 and kept.dtype == torch.int32
    assert tuple(v2.shape) == (len(wk), 3) and tuple(f2.shape) == (len(wf), 3), (m, k, tuple(v2.shape), tuple(f2.shape), len(wk), len(wf))
    assert np.array_equal(_np(kept), wk) and np.array_equal(_np(f2), wf), (m, k)
    assert bool((kept[1:] > kept[:-1]).all())                                            # ascending
    assert torch.equal(v2, verts_t[kept.long()]) and np.array_equal(_np(v2).view(np.uint32), wv.view(np.uint32))      # bit-equal to the input's rows
    assert st["components"] == int((label == np.arange(len(label))).sum()) and st["components_kept"] == int(keep.sum())
    assert st["triangles_dropped"] == faces_t.shape[0] - len(wf)
    return v2, f2


@functools.lru_cache(maxsize=None)
def _gpu_mesh(name):
    """(verts, faces) tensors of a fixture volume from the HIP marching cubes — extracted once, shared, never written to"""
    from jittor_myc_nerfs_amd import marching_cubes
    make, level = CM.VOLUMES[name]
    return marching_cubes(torch.as_tensor(make()).cuda(), level)


# ---- marching-cubes meshes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CM.VOLUMES))
def test_marching_cubes_meshes(name):
    v, f = _gpu_mesh(name)
    assert np.array_equal(_np(f), CM.cpu_mesh(name)[1])                                   # the fixture the host tests anchor
    label, sizes = _check_components(f, v.shape[0])
    for m, k in CM.POLICY_GRID:
        v2, f2 = _check_filter(v, f, label, sizes, m, k)
        if name in CM.CLOSED and f2.shape[0]:
            MC.assert_closed_and_oriented(_np(f2), v2.shape[0])
    if name == "noise":
        v2, f2 = _check_filter(v, f, label, sizes, 0, 1)
        assert f2.shape[0] == 19888 and f.shape[0] == 20868
    if name == "two_spheres":
        assert sorted(sizes[sizes > 0].tolist()) == [272, 300]


# ---- synthetic index buffers ---------------------------------------------------------------------------------------------------------------------------------
STRIP_V = 300_000


@functools.lru_cache(maxsize=None)
def _strip(order):
    from jittor_myc_nerfs_amd import mesh
    assert STRIP_V > mesh.MESH_TILE * mesh.MESH_SCAN_CHUNK                                # the scan carry crosses a chunk boundary
    f = CM.strip_faces(STRIP_V)
    rng = np.random.default_rng(11)
    if order == "descending":
        f = f[::-1]
    elif order == "permuted":
        f = f[rng.permutation(len(f))]
    elif order == "relabelled":
        f = rng.permutation(STRIP_V)[f]
    return _dev(f, torch.int32)


@pytest.mark.parametrize("order", ["ascending", "descending", "permuted", "relabelled"])
def test_deep_chain_strip(order):
    """One component of 300 000 vertices: the deepest chain hooking and flattening can be handed.  mesh_components raises on the fault flag, so returning at all says
    no walk gave up; the most steps any walk took are printed next to the bound."""
    f = _strip(order)
    st = {}
    label, sizes = _check_components(f, STRIP_V, stats=st)
    print(f"    {order}: longest walk {st['max_walk_steps']} steps, bound {st['walk_step_bound']}")
    assert (label == 0).all() and sizes[0] == STRIP_V - 2
    assert 0 <= st["max_walk_steps"] < st["walk_step_bound"]
    verts = _verts_for(STRIP_V)
    v2, f2 = _check_filter(verts, f, label, sizes, 0, 1)                                  # everything survives: identity through a scan of 300 000 elements
    assert torch.equal(v2, verts) and torch.equal(f2, f)
    v2, f2 = _check_filter(verts, f, label, sizes, STRIP_V, 0)                            # nothing does
    assert v2.shape[0] == 0 and f2.shape[0] == 0


def test_many_tied_roots_and_unused_vertices():
    n = 100_000
    f = _dev(CM.disjoint_triangles(n), torch.int32)
    label, sizes = _check_components(f, 3 * n)
    assert int((sizes == 1).sum()) == n
    verts = _verts_for(3 * n)
    v2, f2 = _check_filter(verts, f, label, sizes, 0, 5)
    assert np.array_equal(_np(f2), np.arange(15).reshape(5, 3))                           # all tied: the five smallest labels
    _check_filter(verts, f, label, sizes, 1, 0)
    # unused vertices in front, in the middle and at the end
    front, mid, end = 1500, 2049, 777
    half = n // 2
    faces = np.concatenate((CM.disjoint_triangles(half, front), CM.disjoint_triangles(n - half, front + 3 * half + mid)))
    V = front + 3 * n + mid + end
    f = _dev(faces, torch.int32)
    label, sizes = _check_components(f, V)
    assert int((label == np.arange(V)).sum()) == n + front + mid + end
    verts = _verts_for(V)
    for m, k in ((0, 5), (1, 0), (0, n + 10), (2, 0)):
        v2, f2 = _check_filter(verts, f, label, sizes, m, k)
    assert v2.shape[0] == 0 and f2.shape[0] == 0                                          # (2, 0): no component has two faces
    v2, f2 = _check_filter(verts, f, label, sizes, 1, 0)
    assert v2.shape[0] == 3 * n and f2.shape[0] == n                                      # the unused vertices go with the first active option


def test_degenerate_duplicated_and_empty():
    from jittor_myc_nerfs_amd import mesh
    faces = np.array([[4, 4, 7], [7, 2, 2], [9, 8, 6], [9, 8, 6], [6, 8, 9], [1, 1, 1], [3, 5, 3]], np.int64)      # (a, a, b), duplicates, a point, a needle
    V = 11
    f = _dev(faces, torch.int32)
    label, sizes = _check_components(f, V)
    assert label.tolist() == [0, 1, 2, 3, 2, 3, 6, 2, 6, 6, 10]
    verts = _verts_for(V)
    for m, k in ((0, 1), (0, 2), (2, 0), (1, 0), (3, 1), (4, 0)):
        _check_filter(verts, f, label, sizes, m, k)
    # F = 0 with V > 0: every vertex its own component; V = 0
    none = torch.zeros(0, 3, dtype=torch.int32, device="cuda")
    label, sizes = _check_components(none, 5)
    assert label.tolist() == [0, 1, 2, 3, 4] and sizes.tolist() == [0] * 5
    v2, f2 = _check_filter(_verts_for(5), none, label, sizes, 0, 1)
    assert v2.shape[0] == 0 and f2.shape[0] == 0
    label, sizes = _check_components(none, 0)
    v2, f2, kept = mesh.filter_components(torch.zeros(0, 3, device="cuda"), none, keep_largest=1)
    assert tuple(v2.shape) == (0, 3) and tuple(f2.shape) == (0, 3) and tuple(kept.shape) == (0,)
    torch.cuda.synchronize()


def test_two_runs_agree():
    from jittor_myc_nerfs_amd import mesh
    for verts, f in ((_gpu_mesh("noise")), (_verts_for(STRIP_V), _strip("permuted"))):
        runs = []
        for _ in range(2):
            label, sizes, n = mesh.mesh_components(f, verts.shape[0])
            runs.append((label, sizes, n) + mesh.filter_components(verts, f, keep_largest=1))
        assert runs[0][2] == runs[1][2]
        for a, b in zip(runs[0][:2] + runs[0][3:], runs[1][:2] + runs[1][3:]):
            assert torch.equal(a, b)


# ---- guards -----------------------------------------------------------------------------------------------------------------------------------------------------
class _Guards:
    """4 KB of 0xA5 behind every buffer allocated inside (tests/test_gpu_canaries.py's mechanism); under the TVR_GUARDS=1 sweep the guards are already there"""

    def __enter__(self):
        from jittor_myc_nerfs_amd import _lib as L
        self.keep = L.GUARD_BYTES
        self.own = self.keep <= 0
        if self.own:
            L._guarded.clear()
            L.GUARD_BYTES = 4096
        return L

    def __exit__(self, *exc):
        from jittor_myc_nerfs_amd import _lib as L
        if self.own:
            L.GUARD_BYTES = self.keep
            L._guarded.clear()


@pytest.mark.parametrize("bad", ["V", "-1"])
def test_bad_face_index_raises_the_flag_and_writes_nothing(bad):
    from jittor_myc_nerfs_amd import mesh
    v, f = _gpu_mesh("two_spheres")
    V, F = v.shape[0], f.shape[0]
    good_label, good_sizes, _ = mesh.mesh_components(f, V)
    keep = mesh.component_keep_mask(good_label, good_sizes, keep_largest=1)
    fb = f.clone()
    fb[F // 2, 1] = V if bad == "V" else -1
    with _Guards() as L:
        lib = L.lib()
        label = L.dev_empty((V,), torch.int32, "cuda", what="test labels").fill_(-7)
        sizes = L.dev_empty((V,), torch.int32, "cuda", what="test sizes").fill_(-7)
        ncomp = L.dev_empty((1,), torch.int64, "cuda", what="test count").fill_(-7)
        scratch = L.dev_bytes(lib.tvr_mesh_components_scratch_bytes(V, F), "cuda", what="test scratch")
        flag = L.dev_bytes(4, "cuda", zero=True, what="test flag").view(torch.int32)
        L.check(lib.tvr_mesh_components(fb.data_ptr(), F, V, label.data_ptr(), L.nbytes(label), sizes.data_ptr(), L.nbytes(sizes), ncomp.data_ptr(), scratch.data_ptr(),
                                        L.nbytes(scratch), flag.data_ptr(), None), "tvr_mesh_components")
        torch.cuda.synchronize()
        assert int(flag.item()) == 1
        assert bool((label == -7).all()) and bool((sizes == -7).all()) and int(ncomp.item()) == -7
        assert L.check_guards() == []
        # the filter with labels of the sound mesh and the damaged faces: the count raises the flag, and the emit that follows writes nothing
        scratch, n_v, n_f, flag = mesh.filter_count(fb, V, good_label, keep)
        assert int(flag.item()) == 1
        flag.zero_()
        vo = L.dev_empty((n_v, 3), torch.float32, "cuda", what="test verts").fill_(-7.0)
        fo = L.dev_empty((n_f, 3), torch.int32, "cuda", what="test faces").fill_(-7)
        kept = L.dev_empty((n_v,), torch.int32, "cuda", what="test kept").fill_(-7)
        L.check(lib.tvr_mesh_filter_emit(v.data_ptr(), fb.data_ptr(), F, V, scratch.data_ptr(), L.nbytes(scratch), vo.data_ptr(), L.nbytes(vo), n_v, fo.data_ptr(),
                                         L.nbytes(fo), n_f, kept.data_ptr(), L.nbytes(kept), flag.data_ptr(), None), "tvr_mesh_filter_emit")
        torch.cuda.synchronize()
        assert int(flag.item()) == 1
        assert bool((vo == -7.0).all()) and bool((fo == -7).all()) and bool((kept == -7).all())
        assert L.check_guards() == []
    for call in (lambda: mesh.mesh_components(fb, V), lambda: mesh.filter_components(v, fb, keep_largest=1)):
        with pytest.raises(L.TvrError, match="fault flag"):
            call()


def test_wrong_capacities_raise_the_flag_and_write_nothing():
    from jittor_myc_nerfs_amd import mesh
    v, f = _gpu_mesh("noise")
    V, F = v.shape[0], f.shape[0]
    label, sizes, _ = mesh.mesh_components(f, V)
    keep = mesh.component_keep_mask(label, sizes, keep_largest=1)
    with _Guards() as L:
        lib = L.lib()
        scratch, n_v, n_f, flag = mesh.filter_count(f, V, label, keep)
        assert int(flag.item()) == 0 and n_f == 19888 and 100 < n_v < V

        def emit(decl_v, decl_f):
            vo = L.dev_empty((decl_v, 3), torch.float32, "cuda", what="test verts").fill_(-7.0)
            fo = L.dev_empty((decl_f, 3), torch.int32, "cuda", what="test faces").fill_(-7)
            kept = L.dev_empty((decl_v,), torch.int32, "cuda", what="test kept").fill_(-7)
            fl = L.dev_bytes(4, "cuda", zero=True, what="test flag").view(torch.int32)
            L.check(lib.tvr_mesh_filter_emit(v.data_ptr(), f.data_ptr(), F, V, scratch.data_ptr(), L.nbytes(scratch), vo.data_ptr() if decl_v else None, L.nbytes(vo),
                                             decl_v, fo.data_ptr() if decl_f else None, L.nbytes(fo), decl_f, kept.data_ptr() if decl_v else None, L.nbytes(kept),
                                             fl.data_ptr(), None), "tvr_mesh_filter_emit")
            torch.cuda.synchronize()
            return vo, fo, kept, int(fl.item())

        for decl_v, decl_f in ((n_v - 1, n_f), (n_v, n_f - 1), (n_v + 1, n_f), (n_v, n_f + 1), (n_v // 2, n_f // 2), (0, 0), (V, F)):
            vo, fo, kept, fl = emit(decl_v, decl_f)
            assert fl == 1, (decl_v, decl_f)
            assert bool((vo == -7.0).all()) and bool((fo == -7).all()) and bool((kept == -7).all())
            assert L.check_guards() == []
        vo, fo, kept, fl = emit(n_v, n_f)                                                 # the true counts: no flag, everything written
        assert fl == 0 and L.check_guards() == []
        assert int((fo < 0).sum()) == 0 and int(fo.max()) < n_v and int((kept < 0).sum()) == 0 and torch.equal(vo, v[kept.long()])


# ---- through the model ------------------------------------------------------------------------------------------------------------------------------------------
def _hyper():
    from jittor_myc_nerfs_amd import synthetic
    return dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=TINY["step_ratio"])


def test_model_export_mesh_drops_components(tiny_arrays, tmp_path):
    """The tiny scene's own mesh at its mid level has THREE components (278 vertices, 548 triangles; printed below), so keep_largest = 1 really drops two of
    them through the model.  A fourth is planted as well — a small blob added to the scene's alpha volume, away from the surface — and filtered through mesh.py."""
    from jittor_myc_nerfs_amd import marching_cubes, mesh, read_ply, read_ply_attributes
    m = make_model(tiny_arrays, _hyper())
    alpha = m.getDenseAlpha()[0]
    level = 0.5 * (float(alpha.min()) + float(alpha.max()))
    p0, p1, p2, p3 = (str(tmp_path / f"{i}.ply") for i in range(4))
    v1, f1 = m.export_mesh(p1, level=level)
    assert m.mesh_export_stats == {}
    m.export_mesh(p0, level=level, min_component_faces=0, keep_largest=0)
    assert open(p0, "rb").read() == open(p1, "rb").read()                                 # both options 0: the file of a call without the keywords
    label, sizes = _check_components(f1, v1.shape[0])
    n = int((label == np.arange(len(label))).sum())
    print(f"    tiny scene at level {level:g}: {v1.shape[0]} vertices, {f1.shape[0]} triangles, {n} component(s)")
    v2, f2 = m.export_mesh(p2, level=level, keep_largest=1)
    wv, wf, kept = mesh.filter_components(v1, f1, keep_largest=1)
    assert torch.equal(v2, wv) and torch.equal(f2, wf)
    assert m.mesh_export_stats["components"] == n and m.mesh_export_stats["components_kept"] == 1
    assert n >= 2 and 0 < f2.shape[0] < f1.shape[0] and m.mesh_export_stats["triangles_dropped"] == f1.shape[0] - f2.shape[0]
    rv, rf = read_ply(p2)
    assert np.array_equal(rv, _np(v2)) and np.array_equal(rf, _np(f2))
    # attributes are computed for the survivors only and equal the unfiltered export's rows kept_vertex
    m.export_mesh(p3, level=level, normals=True, colors=True)
    _, _, full = read_ply_attributes(p3)
    m.export_mesh(p3, level=level, normals=True, colors=True, keep_largest=1)
    rv, rf, part = read_ply_attributes(p3)
    k = _np(kept).astype(np.int64)
    assert np.array_equal(rv, _np(v2)) and np.array_equal(rf, _np(f2))
    assert np.array_equal(part["normals"].view(np.uint32), full["normals"][k].view(np.uint32)) and np.array_equal(part["colors"], full["colors"][k])
    with pytest.raises(ValueError, match="negative"):
        m.export_mesh(p3, level=level, keep_largest=-1)
    # a planted blob: 2 x 2 x 2 grid points above the level where the 5 x 5 x 5 neighbourhood lies below it
    pooled = torch.nn.functional.max_pool3d(alpha[None, None], 5, stride=1, padding=2)[0, 0]
    free = pooled < level
    free[:3], free[-3:], free[:, :3], free[:, -3:], free[:, :, :3], free[:, :, -3:] = False, False, False, False, False, False
    spots = free.nonzero()
    assert spots.shape[0] > 0, "no free spot for a blob in the tiny scene's alpha volume"
    i, j, kk = (int(x) for x in spots[0])
    planted = alpha.clone()
    planted[i:i + 2, j:j + 2, kk:kk + 2] = float(alpha.max())
    vb, fb = marching_cubes(planted, level)
    lb, sb = _check_components(fb, vb.shape[0])
    assert int((lb == np.arange(len(lb))).sum()) == n + 1
    assert fb.shape[0] > f1.shape[0]
    for mm, k in ((0, 1), (0, n), (0, n + 1), (9, 0), (int(sb.max()), 0)):
        _check_filter(vb, fb, lb, sb, mm, k)
