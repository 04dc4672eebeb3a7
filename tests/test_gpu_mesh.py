"""GPU (-m gpu): the HIP marching cubes (csrc/tvr_mesh.hip through mesh.marching_cubes) and the export paths built on it.  The checks are vectorised numpy over
the OUTPUT (mesh_common.py): vertex count and positions against numpy's crossing points in the specified order, index ranges, every directed edge exactly
once with its reverse exactly once (closed, consistently oriented), Euler characteristics, signed volumes.  They do not restate the case table.

Vertex positions: the bar is 2 ulp of the coordinate; bit equality is expected (hipcc rounds fp32 division correctly by default, and the kernel's operations
are separately rounded like numpy's) and the observed maximum is printed."""
import functools

import numpy as np
import pytest
import torch

import cp_common as CC
import mesh_common as MC
from conftest import TINY, make_model

pytestmark = pytest.mark.gpu

POSITION_ULP = 2.0


def _np(t):
    return t.detach().cpu().numpy()


def _mc(vol, level, **kw):
    from jittor_myc_nerfs_amd import marching_cubes
    v, f = marching_cubes(torch.as_tensor(vol).cuda(), level, **kw)
    assert v.is_cuda and f.is_cuda and v.dtype == torch.float32 and f.dtype == torch.int32
    assert v.dim() == 2 and v.shape[1] == 3 and f.dim() == 2 and f.shape[1] == 3
    return v, f


@functools.lru_cache(maxsize=None)
def _sphere():
    """(volume, verts, faces) of the off-centre sphere on 16^3 — extracted once, shared, never written to."""
    vol = MC.sphere_volume()
    v, f = _mc(vol, 0.0)
    return vol, _np(v), _np(f)


def _check_vertices(vol, level, v, spacing=(1, 1, 1), origin=(0, 0, 0)):
    want = MC.reference_vertices(vol, level, spacing, origin)
    assert v.shape == want.shape, (v.shape, want.shape)                     # V = number of straddling grid edges
    assert v.shape[0] == int(MC.straddle_masks(vol, level).sum())
    worst = float(MC.ulp_distance(v, want).max(initial=0.0))
    print(f"    {v.shape[0]} vertices, max position difference {worst:g} ulp (bit-equal: {np.array_equal(v, want)})")
    assert worst <= POSITION_ULP
    return worst


def _noise_checks(shape, seed):
    vol = MC.noise_volume(shape, seed)
    v, f = _mc(vol, 0.5)
    _check_vertices(vol, 0.5, _np(v))
    MC.assert_closed_and_oriented(_np(f), v.shape[0])
    v2, f2 = _mc(vol, 0.5)
    assert torch.equal(v, v2) and torch.equal(f, f2)                         # the order is a function of the volume alone
    return vol, v, f


def test_noise_volume_with_all_256_cases():
    shape = (24, 20, 18)                                                     # three different lengths: an axis mix-up shows
    hist = MC.all_cases_occur(MC.noise_volume(shape, 0), 0.5)
    assert (hist > 0).all(), "the test volume must hold every case"
    print(f"    rarest case occurs {int(hist.min())} times")
    vol, v, f = _noise_checks(shape, 0)
    assert f.shape[0] > 0
    # a world transform: one multiply and one add per coordinate, separately rounded
    sp, org = (0.25, 0.1, 3.0), (-1.5, 0.7, 100.0)
    vw, fw = _mc(vol, 0.5, spacing=sp, origin=org)
    _check_vertices(vol, 0.5, _np(vw), sp, org)
    assert torch.equal(fw, f)


def test_topology_and_orientation():
    vol, v, f = _sphere()
    MC.assert_closed_and_oriented(f, len(v))
    assert MC.euler_characteristic(len(v), f) == 2
    tv, tf = (_np(t) for t in _mc(MC.torus_volume(), 0.0))
    MC.assert_closed_and_oriented(tf, len(tv))
    assert MC.euler_characteristic(len(tv), tf) == 0
    sv, sf = (_np(t) for t in _mc(MC.two_spheres_volume(), 0.0))
    MC.assert_closed_and_oriented(sf, len(sv))
    assert MC.euler_characteristic(len(sv), sf) == 4
    # outward orientation: the signed volume is positive, and it lies between the cells wholly inside and the cells with any corner inside (the surface
    # separates inside from outside corners and stays within the cells it cuts; unit spacing) — a derived bound, not a tuned one
    vol_signed = MC.signed_volume(v, f)
    lo, hi = MC.cell_count_bounds(vol, 0.0)
    print(f"    sphere: {lo} <= signed volume {vol_signed:.2f} <= {hi}")
    assert vol_signed > 0 and 0 < lo <= vol_signed <= hi
    fv, ff = (_np(t) for t in _mc(vol, 0.0, flip=True))
    assert np.array_equal(fv, v) and np.array_equal(ff, f[:, ::-1])
    assert MC.signed_volume(fv, ff) == pytest.approx(-vol_signed, rel=1e-12)             # the same fp64 products, summed in another order


def test_open_surface_leaves_through_the_boundary_only():
    vol = MC.slab_volume()
    v, f = (_np(t) for t in _mc(vol, 0.0))
    _check_vertices(vol, 0.0, v)
    assert f.max() < len(v)
    _, counts, has_rev, edges = MC.edge_usage(f, len(v))
    assert (counts == 1).all()
    single = edges[~has_rev]
    assert len(single) > 0, "the slab must leave the volume"
    hi = np.array(vol.shape, np.float32) - 1
    a, b = v[single[:, 0]], v[single[:, 1]]
    on_face = ((a == 0) & (b == 0)) | ((a == hi) & (b == hi))              # both ends on the same boundary plane of the volume
    assert on_face.any(axis=1).all()


def test_level_equal_to_attained_values():
    vol = MC.integer_volume()
    v, f = (_np(t) for t in _mc(vol, 2.0))
    _check_vertices(vol, 2.0, v)
    MC.assert_closed_and_oriented(f, len(v))
    assert len(np.unique(v, axis=0)) < len(v)                                # positions coincide (t = 0 or 1); the indices stay distinct


def test_edges_of_the_domain():
    one = np.zeros((2, 2, 2), np.float32)
    one[0, 0, 0] = 1.0                                                       # a single cell with one inside corner: three vertices, one triangle
    v, f = (_np(t) for t in _mc(one, 0.25))
    assert np.array_equal(v, np.array([[0.75, 0, 0], [0, 0.75, 0], [0, 0, 0.75]], np.float32)) and f.shape == (1, 3) and sorted(f[0]) == [0, 1, 2]
    assert MC.signed_volume(v, f) > 0                                        # the normal points away from the inside corner: the tetrahedron with the origin is positive
    for fill in (0.0, 1.0):                                                  # all below / all above
        v, f = _mc(np.full((7, 5, 3), fill, np.float32), 0.5)
        assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)
    torch.cuda.synchronize()


def test_understated_capacities_raise_the_fault_flag_and_write_nothing():
    """tvr_mesh_emit with declared counts below the counted totals: the flag is raised, the output buffers keep their fill, and the guard bytes behind every
    buffer (scratch, counts, outputs, flag) are intact."""
    import ctypes as C
    from jittor_myc_nerfs_amd import _lib as L, mesh
    lib = L.lib()
    vol = torch.as_tensor(MC.noise_volume((24, 20, 18), 0)).cuda()
    dims = (C.c_int32 * 3)(*vol.shape)
    org, sp = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    keep = L.GUARD_BYTES
    own_guards = keep <= 0                                                   # (under the TVR_GUARDS=1 sweep the guards are already there)
    if own_guards:
        L._guarded.clear()
        L.GUARD_BYTES = 4096
    try:
        vol_c, scratch, nv, nt = mesh.mesh_count(vol, 0.5)
        assert nv > 100 and nt > 100

        def emit(decl_v, decl_t):
            verts = L.dev_empty((decl_v, 3), torch.float32, "cuda", what="test verts").fill_(-7.0)
            faces = L.dev_empty((decl_t, 3), torch.int32, "cuda", what="test faces").fill_(-7)
            flag = L.dev_bytes(4, "cuda", zero=True, what="test flag").view(torch.int32)
            L.check(lib.tvr_mesh_emit(vol_c.data_ptr(), dims, 0.5, org, sp, scratch.data_ptr(), L.nbytes(scratch), verts.data_ptr() if decl_v else None, L.nbytes(verts),
                                      decl_v, faces.data_ptr() if decl_t else None, L.nbytes(faces), decl_t, 0, flag.data_ptr(), None), "tvr_mesh_emit")
            torch.cuda.synchronize()
            return verts, faces, int(flag.item())

        for decl_v, decl_t in ((nv - 1, nt), (nv, nt - 1), (nv // 2, nt // 2), (0, 0)):
            verts, faces, flag = emit(decl_v, decl_t)
            assert flag == 1, (decl_v, decl_t)
            assert bool((verts == -7.0).all()) and bool((faces == -7).all())
            assert L.check_guards() == []
        verts, faces, flag = emit(nv, nt)                                    # the true counts: no flag, everything written
        assert flag == 0 and L.check_guards() == []
        assert int((faces < 0).sum()) == 0 and int(faces.max()) < nv and not bool((verts == -7.0).all(dim=1).any())
    finally:
        if own_guards:
            L.GUARD_BYTES = keep
            L._guarded.clear()


def test_past_one_scan_block():
    """The scan is reduce / scan / add: tiles of MESH_TILE points, and ONE workgroup that walks the tile sums MESH_SCAN_CHUNK at a time with a carry.  Every level
    is exercised once there are more than two chunks of tiles (a carry that is itself carried) and the last tile is ragged:
    130 x 70 x 66 = 600 600 points = 586 full tiles + 536 points = 2 chunks of 256 tiles + 75 tiles."""
    from jittor_myc_nerfs_amd import mesh
    shape = (130, 70, 66)
    points = shape[0] * shape[1] * shape[2]
    tiles = -(-points // mesh.MESH_TILE)
    assert tiles > 2 * mesh.MESH_SCAN_CHUNK and tiles % mesh.MESH_SCAN_CHUNK != 0 and points % mesh.MESH_TILE != 0
    _noise_checks(shape, 1)


# ---- model level ------------------------------------------------------------------------------------------------------------------------------------------------
def _hyper():
    from jittor_myc_nerfs_amd import synthetic
    return dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=TINY["step_ratio"])


def _models(tiny_arrays):
    return {"TensorVMSplit": make_model(tiny_arrays, _hyper()), "TensorCP": CC.make_cp_model(CC.cp_arrays(16, 48), _hyper())}


@pytest.mark.parametrize("name", ["TensorVMSplit", "TensorCP"])
def test_model_export_mesh(tiny_arrays, tmp_path, name):
    from jittor_myc_nerfs_amd import marching_cubes, read_ply, reconstruct as R
    m = _models(tiny_arrays)[name]
    alpha = m.getDenseAlpha()[0]
    level = 0.5 * (float(alpha.min()) + float(alpha.max()))
    aabb = m.aabb.float().cpu()
    n = torch.tensor([float(s) for s in alpha.shape])
    lo, hi = aabb[0].numpy(), aabb[1].numpy()
    for spacing, voxel in (("reference", (aabb[1] - aabb[0]) / n), ("samples", (aabb[1] - aabb[0]) / (n - 1))):
        path = tmp_path / f"{name}_{spacing}.ply"
        m.export_mesh(str(path), level=level, spacing=spacing)
        v, f = read_ply(str(path))
        wv, wf = marching_cubes(alpha, level, spacing=voxel.tolist(), origin=aabb[0].tolist())
        assert f.shape[0] >= 1
        assert np.array_equal(v, _np(wv)) and np.array_equal(f, _np(wf))                      # bit for bit
        assert (v >= lo).all() and (v <= hi).all()
        print(f"    {name} / {spacing}: {v.shape[0]} vertices, {f.shape[0]} triangles at level {level:g}")
    # the command line on a checkpoint of this model
    ckpt = tmp_path / f"{name}.th"
    m.save(str(ckpt))
    args = R.config_parser(["--export_mesh", "1", "--ckpt", str(ckpt), "--model_name", name, "--mesh_level", repr(level)])
    out = R.main(["--export_mesh", "1", "--ckpt", str(ckpt), "--model_name", name, "--mesh_level", repr(level)])
    assert out == str(tmp_path / f"{name}.ply") and R.export_mesh(args) == out
    assert (tmp_path / f"{name}.ply").read_bytes() == (tmp_path / f"{name}_reference.ply").read_bytes()
