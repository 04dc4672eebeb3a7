"""GPU (-m gpu): vertex-clustering simplification (csrc/tvr_mesh_simplify.hip through mesh.simplify_clustering) and the export path built on it.  The oracle is
tests/mesh_simplify_common.py (numpy, restated from the definition in include/tvr.h); every comparison is exact — np.array_equal / torch.equal on indices, maps and
counts, the uint32 view on positions.  There is no tolerance in this file."""
import functools

import numpy as np
import pytest
import torch

import mesh_components_common as CM
import mesh_simplify_common as SC
from conftest import TINY, make_model

pytestmark = pytest.mark.gpu

CELLS = (2.0, 1.5, 3.7)                                     # in voxels; the fixture meshes have unit spacing
ORIGINS = ((0.0, 0.0, 0.0), (-0.37, -0.11, -0.23))          # the first puts nearly every vertex's two lattice-aligned coordinates exactly on cell boundaries


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


@functools.lru_cache(maxsize=None)
def _gpu_mesh(name):
    """(verts, faces) tensors of a fixture volume from the HIP marching cubes — extracted once, shared, never written to"""
    from jittor_myc_nerfs_amd import marching_cubes
    make, level = CM.VOLUMES[name]
    return marching_cubes(torch.as_tensor(make()).cuda(), level)


def _check(verts_t, faces_t, cell, origin=(0, 0, 0)):
    """simplify_clustering against the oracle, everything exact -> (verts', faces', vertex_map, stats)"""
    from jittor_myc_nerfs_amd import mesh
    st = {}
    v2, f2, vmap = mesh.simplify_clustering(verts_t, faces_t, cell, origin=origin, stats=st)
    wv, wf, wm = SC.simplify_oracle(_np(verts_t), _np(faces_t), cell, origin)
    assert v2.is_cuda and v2.dtype == torch.float32 and f2.dtype == torch.int32 and vmap.dtype == torch.int32
    assert tuple(v2.shape) == (len(wv), 3) and tuple(f2.shape) == (len(wf), 3) and tuple(vmap.shape) == (verts_t.shape[0],), (cell, origin, tuple(v2.shape), wv.shape)
    assert np.array_equal(_np(vmap), wm), (cell, origin)
    assert np.array_equal(_np(f2), wf), (cell, origin)
    assert np.array_equal(_np(v2).view(np.uint32), wv.view(np.uint32)), (cell, origin)
    assert (st["vertices_in"], st["vertices_out"], st["triangles_in"], st["triangles_out"]) == (verts_t.shape[0], len(wv), faces_t.shape[0], len(wf))
    assert 0 <= st["max_probe"] <= st["table_capacity"]
    assert st["table_capacity"] == max(mesh.simplify_table_capacities(verts_t.shape[0], faces_t.shape[0]))
    return v2, f2, vmap, st


# ---- marching-cubes meshes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CM.VOLUMES))
def test_marching_cubes_meshes(name):
    v, f = _gpu_mesh(name)
    on_boundary = float(((v / 2.0) == torch.floor(v / 2.0)).float().mean())
    for origin in ORIGINS:
        for cell in CELLS:
            v2, f2, vmap, st = _check(v, f, cell, origin)
            assert 0 < f2.shape[0] < f.shape[0] and 0 < v2.shape[0] < v.shape[0]
            print(f"    {name} cell {cell} origin {origin}: {v.shape[0]} -> {v2.shape[0]} vertices, {f.shape[0]} -> {f2.shape[0]} triangles, "
                  f"longest probe {st['max_probe']} of {st['table_capacity']} slots")
    # two of a marching-cubes vertex's three coordinates are integers and about half of those are even: a third of all coordinates lie exactly on a boundary of the
    # cell-2 lattice at origin 0 — the common case, not a corner case
    assert on_boundary > 0.25
    if name == "noise":
        assert f.shape[0] == 20868
        wv, wf, wm = SC.simplify_oracle(_np(v), _np(f), 3.7)
        m = wm[_np(f).astype(np.int64)]
        alive = (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])
        assert int(alive.sum()) - len(wf) > 100             # the case with many duplicate triangles


# ---- hand-made meshes ----------------------------------------------------------------------------------------------------------------------------------------
def test_hand_made_meshes():
    from jittor_myc_nerfs_amd import mesh
    tet_v = _dev([[0.25, 0.25, 0.25], [1.25, 0.5, 0.75], [0.5, 1.75, 0.25], [0.75, 0.5, 1.5]], torch.float32)
    tet_f = _dev([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], torch.int32)
    # all vertices in one cell: one vertex, no faces
    v2, f2, vmap, _ = _check(tet_v, tet_f, 4.0)
    assert tuple(v2.shape) == (1, 3) and f2.shape[0] == 0 and vmap.tolist() == [0, 0, 0, 0]
    assert v2.tolist() == [[0.6875, 0.75, 0.6875]]          # the mean of dyadic coordinates is exact
    # a cell below every vertex distance: faces unchanged, the map is the identity, positions are the oracle's (quantised to 2^-20 of a cell)
    v2, f2, vmap, _ = _check(tet_v, tet_f, 0.2)
    assert torch.equal(f2, tet_f) and vmap.tolist() == [0, 1, 2, 3] and tuple(v2.shape) == (4, 3)
    # two triangles collapsing onto one triple: the lower index stays, in ITS corner order; the reversed one is another triangle and stays
    base = np.array([[0.25, 0.25, 0.25], [1.25, 0.25, 0.25], [0.25, 1.25, 0.25]], np.float32)
    twins = _dev(np.concatenate((base, base + np.float32(0.5))), torch.float32)
    v2, f2, vmap, _ = _check(twins, _dev([[4, 5, 3], [0, 1, 2]], torch.int32), 1.0)
    assert f2.tolist() == [[1, 2, 0]] and vmap.tolist() == [0, 1, 2, 0, 1, 2] and np.array_equal(_np(v2), base + np.float32(0.25))
    v2, f2, vmap, _ = _check(twins, _dev([[5, 3, 4], [0, 1, 2], [2, 1, 0], [3, 5, 4]], torch.int32), 1.0)
    assert f2.tolist() == [[2, 0, 1], [2, 1, 0]]
    # vertices no face uses: clustered like any other, every cluster keeps its vertex
    lone = torch.cat((twins, _dev([[3.5, 3.5, 3.5], [3.75, 3.5, 3.5], [0.5, 0.5, 0.5]], torch.float32)))
    v2, f2, vmap, _ = _check(lone, _dev([[0, 1, 2]], torch.int32), 1.0)
    assert vmap.tolist() == [0, 1, 2, 0, 1, 2, 3, 3, 0] and tuple(v2.shape) == (4, 3) and f2.tolist() == [[0, 1, 2]]
    # no faces; nothing at all
    none = torch.zeros(0, 3, dtype=torch.int32, device="cuda")
    v2, f2, vmap, _ = _check(lone, none, 1.0)
    assert tuple(v2.shape) == (4, 3) and tuple(f2.shape) == (0, 3)
    st = {}
    v2, f2, vmap = mesh.simplify_clustering(torch.zeros(0, 3, device="cuda"), none, 1.0, stats=st)
    assert tuple(v2.shape) == (0, 3) and tuple(f2.shape) == (0, 3) and tuple(vmap.shape) == (0,)
    assert (st["vertices_out"], st["triangles_out"], st["max_probe"]) == (0, 0, 0)
    torch.cuda.synchronize()


# ---- past one chunk of the scan ----------------------------------------------------------------------------------------------------------------------------------
STRIP_NX, STRIP_NY = 70_000, 4


@functools.lru_cache(maxsize=None)
def _lattice_strip():
    """A planar strip of STRIP_NX x STRIP_NY lattice points at spacing 1 (vertex i * NY + j at (i, j, 0)), two triangles per quad, built on the device:
    (verts, faces, i of each quad, j of each quad)"""
    i, j = torch.meshgrid(torch.arange(STRIP_NX, device="cuda"), torch.arange(STRIP_NY, device="cuda"), indexing="ij")
    verts = torch.stack((i, j, torch.zeros_like(i)), -1).view(-1, 3).to(torch.float32)
    qi, qj = i[:-1, :-1].reshape(-1), j[:-1, :-1].reshape(-1)
    v00 = qi * STRIP_NY + qj
    v10, v01, v11 = v00 + STRIP_NY, v00 + 1, v00 + STRIP_NY + 1
    faces = torch.stack((torch.stack((v00, v10, v11), -1), torch.stack((v00, v11, v01), -1)), 1).view(-1, 3).to(torch.int32)
    return verts, faces, qi, qj


def test_lattice_strip_past_one_scan_chunk():
    """More than TVR_MESH_TILE * TVR_MESH_SCAN_CHUNK vertices and triangles, checked against a closed form (the numpy oracle would be slow here).
    Cell 0.5, origin 0: every vertex alone in its cell (2 i, 2 j, 0) with fraction 0 — the identity, bit for bit.
    Cell 2, origin -0.5: g = (i + 0.5) / 2, so vertex (i, j) falls into cell (i // 2, j // 2, 0) and no coordinate lies on a boundary.  A cluster's smallest index is
    (2 a) NY + 2 b, ascending in (a, b): vertex_map = (i // 2) (NY / 2) + j // 2.  Of a quad's corners A = cell(i, j), B = cell(i + 1, j), C = cell(i + 1, j + 1),
    D = cell(i, j + 1): i even gives A = B and C = D, j even gives A = D and B = C — both triangles (A, B, C) and (A, C, D) collapse unless i and j are both odd, and
    those quads map onto distinct coarse quads, so nothing is a duplicate: 2 (NX / 2 - 1) (NY / 2 - 1) triangles survive, in order.  In-cell fractions are 0.25 and
    0.75 on x and y (mean 0.5, exact) and 0.25 on z: position (2 a + 0.5, 2 b + 0.5, 0)."""
    from jittor_myc_nerfs_amd import mesh
    verts, faces, qi, qj = _lattice_strip()
    V, F = verts.shape[0], faces.shape[0]
    assert V > mesh.MESH_TILE * mesh.MESH_SCAN_CHUNK and F > mesh.MESH_TILE * mesh.MESH_SCAN_CHUNK and STRIP_NX % 2 == 0 and STRIP_NY % 2 == 0
    st = {}
    v2, f2, vmap = mesh.simplify_clustering(verts, faces, 0.5, stats=st)
    assert torch.equal(v2, verts) and torch.equal(f2, faces) and torch.equal(vmap, torch.arange(V, dtype=torch.int32, device="cuda"))
    assert st["max_probe"] <= st["table_capacity"]
    v2, f2, vmap = mesh.simplify_clustering(verts, faces, 2.0, origin=(-0.5, -0.5, -0.5), stats=st)
    half = STRIP_NY // 2
    idx = torch.arange(V, device="cuda")
    want_map = ((idx // STRIP_NY) // 2) * half + (idx % STRIP_NY) // 2
    assert v2.shape[0] == (STRIP_NX // 2) * half and f2.shape[0] == 2 * (STRIP_NX // 2 - 1) * (half - 1)
    assert torch.equal(vmap.long(), want_map)
    odd = ((qi % 2 == 1) & (qj % 2 == 1)).repeat_interleave(2)
    assert torch.equal(f2.long(), want_map[faces[odd].long()])
    n = torch.arange(v2.shape[0], device="cuda")
    want_pos = torch.stack((2.0 * (n // half) + 0.5, 2.0 * (n % half) + 0.5, torch.zeros_like(n, dtype=torch.float32)), -1).to(torch.float32)
    assert torch.equal(v2, want_pos)
    assert st["max_probe"] <= st["table_capacity"]


def test_two_runs_agree():
    from jittor_myc_nerfs_amd import mesh
    strip_v, strip_f, _, _ = _lattice_strip()
    for verts, faces, cell, origin in (_gpu_mesh("noise") + (3.7, ORIGINS[1]), _gpu_mesh("noise") + (2.0, ORIGINS[0]), (strip_v, strip_f, 3.0, (-0.25, -0.25, -0.25))):
        a = mesh.simplify_clustering(verts, faces, cell, origin=origin)
        b = mesh.simplify_clustering(verts, faces, cell, origin=origin)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ---- the fault flag ----------------------------------------------------------------------------------------------------------------------------------------------
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


def _raw_emit(L, v, f, lat, scratch, decl_v, decl_f):
    """tvr_mesh_simplify_emit into sentinel-filled, guarded buffers of the declared sizes -> (verts_out, faces_out, vertex_map, flag value)"""
    from jittor_myc_nerfs_amd import mesh
    lib = L.lib()
    V, F = v.shape[0], f.shape[0]
    vo = L.dev_empty((decl_v, 3), torch.float32, "cuda", what="test verts").fill_(-7.0)
    fo = L.dev_empty((decl_f, 3), torch.int32, "cuda", what="test faces").fill_(-7)
    vm = L.dev_empty((V,), torch.int32, "cuda", what="test map").fill_(-7)
    fl = L.dev_bytes(4, "cuda", zero=True, what="test flag").view(torch.int32)
    o, c, inv = (mesh._c3(x) for x in lat)
    L.check(lib.tvr_mesh_simplify_emit(v.data_ptr(), V, f.data_ptr(), F, o, c, inv, scratch.data_ptr(), L.nbytes(scratch), vo.data_ptr() if decl_v else None, L.nbytes(vo),
                                       decl_v, fo.data_ptr() if decl_f else None, L.nbytes(fo), decl_f, vm.data_ptr(), L.nbytes(vm), fl.data_ptr(), None),
            "tvr_mesh_simplify_emit")
    torch.cuda.synchronize()
    return vo, fo, vm, int(fl.item())


def _untouched(vo, fo, vm):
    return bool((vo == -7.0).all()) and bool((fo == -7).all()) and bool((vm == -7).all())


@pytest.mark.parametrize("bad", ["face index V", "face index -1", "NaN vertex", "vertex below origin", "vertex beyond the lattice"])
def test_bad_input_raises_the_flag_and_writes_nothing(bad):
    """Reported conditions, not device faults: the damaged value is range-checked before it is used, so no access leaves a buffer."""
    from jittor_myc_nerfs_amd import mesh
    v, f = _gpu_mesh("two_spheres")
    V, F = v.shape[0], f.shape[0]
    lat = mesh._lattice(2.0, (0, 0, 0))
    good = mesh.simplify_count(v, f, *lat)
    assert int(good[3].item()) == 0 and 0 < good[1] < V and 0 < good[2] < F
    vb, fb = v.clone(), f.clone()
    if bad.startswith("face index"):
        fb[F // 2, 1] = V if bad.endswith("V") else -1
    else:
        vb[V // 2, 1] = {"NaN vertex": float("nan"), "vertex below origin": -0.001, "vertex beyond the lattice": 2.0 * 2 ** 21}[bad]
    with _Guards() as L:
        scratch, n_v, n_f, flag = mesh.simplify_count(vb, fb, *lat)
        torch.cuda.synchronize()
        assert int(flag.item()) == 1 and L.check_guards() == []
        # whatever sizes the caller goes on with — the ones just counted, or those of the sound mesh — the emit raises the flag again and writes nothing
        for decl_v, decl_f in ((n_v, n_f), (good[1], good[2])):
            vo, fo, vm, fl = _raw_emit(L, vb, fb, lat, scratch, decl_v, decl_f)
            assert fl == 1 and _untouched(vo, fo, vm) and L.check_guards() == []
    with pytest.raises(L.TvrError, match="fault flag"):
        mesh.simplify_clustering(vb, fb, 2.0)


def test_wrong_capacities_raise_the_flag_and_write_nothing():
    from jittor_myc_nerfs_amd import mesh
    v, f = _gpu_mesh("noise")
    V, F = v.shape[0], f.shape[0]
    lat = mesh._lattice(2.0, ORIGINS[1])
    want = mesh.simplify_clustering(v, f, 2.0, origin=ORIGINS[1])
    with _Guards() as L:
        scratch, n_v, n_f, flag = mesh.simplify_count(v, f, *lat)
        assert int(flag.item()) == 0 and (n_v, n_f) == (want[0].shape[0], want[1].shape[0]) and L.check_guards() == []
        for decl_v, decl_f in ((n_v - 1, n_f), (n_v, n_f - 1), (n_v + 1, n_f), (n_v, n_f + 1), (0, 0), (V, F)):
            vo, fo, vm, fl = _raw_emit(L, v, f, lat, scratch, decl_v, decl_f)
            assert fl == 1 and _untouched(vo, fo, vm), (decl_v, decl_f)
            assert L.check_guards() == []
        vo, fo, vm, fl = _raw_emit(L, v, f, lat, scratch, n_v, n_f)                        # the true counts: no flag, everything written; the scratch serves again
        assert fl == 0 and L.check_guards() == []
        assert torch.equal(vo, want[0]) and torch.equal(fo, want[1]) and torch.equal(vm, want[2])


# ---- through the model ------------------------------------------------------------------------------------------------------------------------------------------
def _hyper():
    from jittor_myc_nerfs_amd import synthetic
    return dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=TINY["step_ratio"])


def test_model_export_mesh_simplifies(tiny_arrays, tmp_path, monkeypatch):
    from jittor_myc_nerfs_amd import mesh, read_ply, read_ply_attributes
    m = make_model(tiny_arrays, _hyper())
    alpha = m.getDenseAlpha()[0]
    level = 0.5 * (float(alpha.min()) + float(alpha.max()))
    p0, p1, p2, p3 = (str(tmp_path / f"{i}.ply") for i in range(4))
    v1, f1 = m.export_mesh(p1, level=level)
    m.export_mesh(p0, level=level, simplify=0.0)
    assert open(p0, "rb").read() == open(p1, "rb").read() and m.mesh_export_stats == {}    # 0: the file of a call without the keyword
    v2, f2 = m.export_mesh(p2, level=level, simplify=2.0)
    cell, origin = m.mesh_simplify_lattice(alpha.shape, "reference", 2.0)
    wv, wf, _ = mesh.simplify_clustering(v1, f1, cell, origin=origin)
    assert torch.equal(v2, wv) and torch.equal(f2, wf) and 0 < f2.shape[0] < f1.shape[0] and v2.shape[0] < v1.shape[0]
    ov, of, _ = SC.simplify_oracle(_np(v1), _np(f1), cell, origin)
    assert np.array_equal(_np(v2).view(np.uint32), ov.view(np.uint32)) and np.array_equal(_np(f2), of)
    rv, rf = read_ply(p2)
    assert np.array_equal(rv.view(np.uint32), _np(wv).view(np.uint32)) and np.array_equal(rf, _np(wf))
    st = m.mesh_export_stats
    assert (st["vertices_in"], st["vertices_out"], st["triangles_in"], st["triangles_out"]) == (v1.shape[0], v2.shape[0], f1.shape[0], f2.shape[0])
    assert st["max_probe"] <= st["table_capacity"]
    print(f"    tiny scene, simplify 2: {v1.shape[0]} -> {v2.shape[0]} vertices, {f1.shape[0]} -> {f2.shape[0]} triangles")
    # attributes are evaluated at the NEW vertices, one row each
    m.export_mesh(p3, level=level, normals=True, colors=True, simplify=2.0)
    rv, rf, attrs = read_ply_attributes(p3)
    assert np.array_equal(rv.view(np.uint32), _np(wv).view(np.uint32)) and np.array_equal(rf, _np(wf))
    assert attrs["normals"].shape == (wv.shape[0], 3) and attrs["colors"].shape == (wv.shape[0], 3)
    want_n = m.surface_normals(m.mesh_sample_positions(wv, alpha.shape, "reference"))
    assert np.array_equal(attrs["normals"].view(np.uint32), _np(want_n).view(np.uint32))
    for s in (0.5, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="simplify"):
            m.export_mesh(p3, level=level, simplify=s)
    # with the component filter, on the two-spheres volume in place of the scene's: one sphere survives and is simplified, the floater is not welded to it
    make, lvl = CM.VOLUMES["two_spheres"]
    vol = torch.as_tensor(make()).cuda()
    monkeypatch.setattr(m, "getDenseAlpha", lambda gridSize=None: (vol, None))
    va, fa = m.export_mesh(p3, level=lvl)
    vk, fk = m.export_mesh(p3, level=lvl, keep_largest=1)
    assert fa.shape[0] == 572 and fk.shape[0] == 300
    vs, fs = m.export_mesh(p3, level=lvl, keep_largest=1, simplify=2.0)
    st = dict(m.mesh_export_stats)
    cell, origin = m.mesh_simplify_lattice(vol.shape, "reference", 2.0)
    wv, wf, _ = mesh.simplify_clustering(vk, fk, cell, origin=origin)
    assert torch.equal(vs, wv) and torch.equal(fs, wf) and 0 < fs.shape[0] < 300
    assert st["components"] == 2 and st["components_kept"] == 1 and st["triangles_dropped"] == 272 and st["triangles_in"] == 300 and st["triangles_out"] == fs.shape[0]
    _, sizes, _ = mesh.mesh_components(fs, vs.shape[0])
    assert int((sizes > 0).sum()) == 1                                                     # one component carries every triangle
    rv, rf = read_ply(p3)
    assert np.array_equal(rv.view(np.uint32), _np(vs).view(np.uint32)) and np.array_equal(rf, _np(fs))


def test_command_line_writes_a_smaller_file(tiny_arrays, tmp_path, capsys):
    """`--export_mesh 1 --mesh_simplify 2` on a checkpoint of the tiny scene: the file of export_mesh(simplify=2.0), smaller than the one without the option."""
    from jittor_myc_nerfs_amd import read_ply, reconstruct as R
    m = make_model(tiny_arrays, _hyper())
    alpha = m.getDenseAlpha()[0]
    level = 0.5 * (float(alpha.min()) + float(alpha.max()))
    ckpt = tmp_path / "tiny.th"
    m.save(str(ckpt))
    cmd = ["--export_mesh", "1", "--ckpt", str(ckpt), "--model_name", "TensorVMSplit", "--mesh_level", repr(level)]
    out = R.main(cmd)
    plain = (tmp_path / "tiny.ply").read_bytes()
    assert R.main(cmd + ["--mesh_simplify", "0"]) == out and (tmp_path / "tiny.ply").read_bytes() == plain
    assert R.main(cmd + ["--mesh_simplify", "2"]) == out
    small = (tmp_path / "tiny.ply").read_bytes()
    assert "simplified from" in capsys.readouterr().out
    m.export_mesh(str(tmp_path / "direct.ply"), level=level, simplify=2.0)
    assert small == (tmp_path / "direct.ply").read_bytes() and len(small) < len(plain)
    v, f = read_ply(str(tmp_path / "tiny.ply"))
    assert 0 < f.shape[0] and int(f.max()) < v.shape[0]
    with pytest.raises(ValueError, match="simplify"):
        R.main(cmd + ["--mesh_simplify", "0.5"])
