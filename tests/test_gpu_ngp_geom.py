"""GPU: the density gradient and the density lattice of an Instant-NGP field (csrc/tvr_ngp_geom.hip, include/tvr_ngp.h "geometry") and the mesh export built on
them (ngp_mesh.py), against the references of tests/ngp_geom_common.py.

Bars.  Values: bit-equal to tvr_ngp_density.  Gradient: per point the error divided by S = sum_k |g_enc,k| |d enc_k / d p|_1 is held to 4 x the worst such error
of the fp32 restatement on the same points (the project's rule for fp32-class kernels; the yardstick is computed here, on the CPU, and is about 1.1e-7 on the
shared scenes), points failing the ReLU margin excluded, at most 1 % of them.  Lattice: bit-equal where evaluated, exactly the empty value elsewhere.  Sphere:
bounds derived in the tests' docstrings."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import ngp_geom_common as K
from conftest import NGP_AABB_SCALE

pytestmark = pytest.mark.gpu
F, U32 = np.float32, np.uint32
NAN = float("nan")


def _model(arrs, aabb_scale, dev, with_sampler=False):
    from jittor_myc_nerfs_amd import ngp
    model = ngp.NGPNetworks(aabb_scale).to(dev)
    sampler = ngp.DensityGridSampler(model, aabb_scale, rng=ngp.Pcg32(1337)).to(dev) if with_sampler else None
    ngp.load_scene_arrays(model, sampler, arrs)
    return model, sampler


@pytest.fixture(scope="module")
def setup(ngp_scene):
    levels, arrs = ngp_scene
    dev = torch.device("cuda:0")
    model, sampler = _model(arrs, NGP_AABB_SCALE, dev, with_sampler=True)
    pos = K.sample_positions(4099)
    return dict(levels=levels, arrs=arrs, dev=dev, model=model, sampler=sampler, pos=pos, pos_dev=torch.from_numpy(pos).to(dev))


def _bits(t):
    return t.detach().cpu().numpy().view(U32)


def _gradient_call(model, p, n, n_dev=None, raw=True):
    """tvr_ngp_density_gradient on rows p (a possibly row-strided [m,>=3] view) into NaN-filled outputs of m rows -> (raw [m], grad [m,3])."""
    from jittor_myc_nerfs_amd import _lib as L, ngp
    dev = p.device
    m = p.shape[0]
    raw_out, grad_out = torch.full((m,), NAN, device=dev), torch.full((m, 3), NAN, device=dev)
    grid = model.pos_encoder.m_grid
    L.check(L.lib().tvr_ngp_density_gradient(C.byref(model.pos_encoder.cfg), grid.data_ptr(), model.packed().data_ptr(), p.data_ptr(), p.stride(0), n,
                                             None if n_dev is None else n_dev.data_ptr(), raw_out.data_ptr() if raw else None, grad_out.data_ptr(),
                                             ngp._stream(dev)), "tvr_ngp_density_gradient")
    torch.cuda.synchronize()
    return raw_out, grad_out


# ------------------------------------------------------------------------------------------------------------------ 1. value bit-equality
def test_value_bit_equal_to_density(setup):
    model, p = setup["model"], setup["pos_dev"]
    n = p.shape[0]
    assert n % 32 != 0 and n % 256 != 0
    want = model.density_raw(p)
    wide = torch.full((n, 7), NAN, device=p.device)
    wide[:, :3] = p
    results = {}
    for name, rows in (("contiguous", p), ("stride 7", wide[:, :3])):
        raw, grad = _gradient_call(model, rows, n)
        assert np.array_equal(_bits(raw), _bits(want)), name
        assert torch.isfinite(grad).all(), name
        results[name] = grad
        raw2, grad2 = model.density_gradient(rows)
        assert np.array_equal(_bits(raw2), _bits(want)) and np.array_equal(_bits(grad2), _bits(grad)), name
        _, grad3 = _gradient_call(model, rows, n, raw=False)                  # raw_out may be NULL
        assert np.array_equal(_bits(grad3), _bits(grad)), name
        for cut in (33, 0):
            n_dev = torch.tensor([cut], dtype=torch.int32, device=p.device)
            raw_c, grad_c = _gradient_call(model, rows, n, n_dev=n_dev)
            assert np.array_equal(_bits(raw_c[:cut]), _bits(want[:cut])) and np.array_equal(_bits(grad_c[:cut]), _bits(grad[:cut])), (name, cut)
            assert torch.isnan(raw_c[cut:]).all() and torch.isnan(grad_c[cut:]).all(), (name, cut)      # rows past n are untouched
        raw_s, grad_s = _gradient_call(model, rows, 100)                      # n_max below the buffer: the same
        assert np.array_equal(_bits(raw_s[:100]), _bits(want[:100])) and torch.isnan(raw_s[100:]).all() and torch.isnan(grad_s[100:]).all()
    assert np.array_equal(_bits(results["contiguous"]), _bits(results["stride 7"]))


# ------------------------------------------------------------------------------------------------------------------ 2. gradient against fp64
def _check_gradient(model, levels, arrs, pos, dev, what):
    ref = K.density_gradient_ref(arrs, levels, pos, torch.float64)
    keep = K.relu_margin_ok(ref)
    excluded = 1.0 - keep.mean()
    yard = K.scaled_error(K.density_gradient_ref(arrs, levels, pos, torch.float32)["grad"], ref, keep)
    raw, grad = model.density_gradient(torch.from_numpy(pos).to(dev))
    got = K.scaled_error(grad.cpu().numpy(), ref, keep)
    tangent = float(np.abs(ref["J"]).max())
    print(f"{what}: {len(pos)} points, excluded {excluded:.4%}, kernel scaled error {got:.3e}, fp32 yardstick {yard:.3e}, bar {4 * yard:.3e}, largest tangent {tangent:.0f}")
    assert excluded <= K.MARGIN_CAP
    assert yard > 0
    assert np.abs(raw.cpu().numpy().astype(np.float64) - ref["raw"]).max() <= 2e-4 * max(1.0, np.abs(ref["raw"]).max())
    assert got <= 4 * yard, f"{what}: scaled error {got:.3e} above 4 x the fp32 yardstick {yard:.3e}"


def test_gradient_against_fp64(setup):
    """Measured on an MI355X: kernel 1.86e-7; the fp32 yardstick on these points is 1.06e-7, the bar 4.22e-7."""
    _check_gradient(setup["model"], setup["levels"], setup["arrs"], setup["pos"], setup["dev"], "aabb_scale 4")


@pytest.mark.parametrize("gain", [1.0, 4.0])
def test_gradient_large_scale_levels(ngp_scene, gain):
    """aabb_scale 16: grid_levels(16) ends at scale 32767 (2048 * 16 - 1; the library refuses scales above 65000), tangents up to 5.9e4 on the U(-1, 1) table.
    gain 4 multiplies the table by 4: tangents up to 2.4e5, more than 98 % of the points hold one above the fp16 split's 65504 — the per-column power of two
    (include/tvr_ngp.h, RANGE) is what keeps them exact."""
    aabb_scale, n, _ = K.GRADIENT_CASES[1]
    levels, arrs = K.gradient_scene(ngp_scene, aabb_scale, gain)
    dev = torch.device("cuda:0")
    model, _ = _model(arrs, aabb_scale, dev)
    _check_gradient(model, levels, arrs, K.sample_positions(n), dev, f"aabb_scale {aabb_scale} gain {gain}")


# ------------------------------------------------------------------------------------------------------------------ 3. lattice
DIMS = (37, 33, 35)                               # odd, no multiple of the 2 x 4 x 4 brick
EMPTY = -123.5
# "cube": the first and the last plane of every axis lie outside [0, 1]; 65 of its points sit in occupied cells of the shared scene (checked on the CPU).
# "dense": the same dims drawn around the scene's occupied shell, all inside the cube: 13 470 occupied points against 29 265 empty ones.
LATTICES = {"cube": ((-0.01, -0.01, -0.01), (1.03 / 36, 1.03 / 32, 1.03 / 34)), "dense": ((0.41, 0.415, 0.42), (0.005, 0.0052, 0.0049))}
MIN_OCCUPIED = {"cube": 50, "dense": 10000}


@pytest.fixture(scope="module", params=sorted(LATTICES))
def lattice(request, setup):
    from jittor_myc_nerfs_amd import ngp
    origin, spacing = LATTICES[request.param]
    pts = K.lattice_points(DIMS, origin, spacing)
    inside = K.in_cube(pts)
    if request.param == "cube":
        assert not inside[0].any() and not inside[-1].any() and not inside[:, -1].any() and not inside[:, :, -1].any() and inside.sum() > 30000
    want = setup["model"].density_raw(torch.from_numpy(pts.reshape(-1, 3)).to(setup["dev"])).reshape(DIMS)
    plain = ngp.density_volume(setup["model"], None, dims=DIMS, origin=origin, spacing=spacing, empty_value=EMPTY)
    torch.cuda.synchronize()
    return dict(name=request.param, origin=origin, spacing=spacing, pts=pts, inside=inside, want=_bits(want), plain=plain)


def _with_bitfield(setup, lattice, bitfield):
    from jittor_myc_nerfs_amd import ngp
    s = ngp.DensityGridSampler(setup["model"], NGP_AABB_SCALE, rng=ngp.Pcg32(1337)).to(setup["dev"])
    s.density_grid_bitfield.copy_(torch.as_tensor(bitfield))
    v = ngp.density_volume(setup["model"], s, dims=DIMS, origin=lattice["origin"], spacing=lattice["spacing"], empty_value=EMPTY)
    torch.cuda.synchronize()
    return v


def test_lattice_without_bitfield(setup, lattice):
    got = _bits(lattice["plain"])
    assert lattice["plain"].shape == DIMS and lattice["plain"].is_contiguous()
    empty = np.array(EMPTY, F).view(U32)
    assert np.array_equal(got[lattice["inside"]], lattice["want"][lattice["inside"]])
    assert (got[~lattice["inside"]] == empty).all()


def test_lattice_with_the_scenes_bitfield(setup, lattice):
    bits = setup["arrs"]["density_grid_bitfield"]
    lo, hi = setup["sampler"].aabb_range
    occ = K.occupied_np(lattice["pts"], bits, lo, hi) & lattice["inside"]
    assert occ.sum() >= MIN_OCCUPIED[lattice["name"]] and (lattice["inside"] & ~occ).sum() > 10000, (int(occ.sum()), int(lattice["inside"].sum()))
    got = _bits(_with_bitfield(setup, lattice, bits))
    assert np.array_equal(got[occ], lattice["want"][occ])
    assert (got[~occ] == np.array(EMPTY, F).view(U32)).all()


def test_lattice_all_zero_and_all_one_bitfields(setup, lattice):
    n = setup["sampler"].density_grid_bitfield.numel()
    assert (_bits(_with_bitfield(setup, lattice, np.zeros(n, np.uint8))) == np.array(EMPTY, F).view(U32)).all()
    assert np.array_equal(_bits(_with_bitfield(setup, lattice, np.full(n, 255, np.uint8))), _bits(lattice["plain"]))


def test_lattice_default_empty_value_and_resolution(setup):
    from jittor_myc_nerfs_amd import ngp
    v = ngp.density_volume(setup["model"], None, resolution=5)
    pts = K.lattice_points((5, 5, 5), (0, 0, 0), [ngp.unit_spacing(5)] * 3)
    assert K.in_cube(pts).all()
    want = setup["model"].density_raw(torch.from_numpy(pts.reshape(-1, 3)).to(setup["dev"])).reshape(5, 5, 5)
    assert np.array_equal(_bits(v), _bits(want))
    v = ngp.density_volume(setup["model"], None, dims=(3, 2, 2), origin=(-1, 0, 0), spacing=(1, 1, 1))
    assert (v[0] == ngp.DENSITY_FLOOR).all() and math.isfinite(ngp.DENSITY_FLOOR)
    from jittor_myc_nerfs_amd import _lib as L
    cpu_model = ngp.NGPNetworks(1)                                            # no CPU fallback: a model that was not moved to the device raises
    with pytest.raises(L.TvrError):
        cpu_model.density_gradient(torch.zeros(4, 3))
    with pytest.raises(L.TvrError):
        ngp.density_volume(cpu_model, None, resolution=4)


# ------------------------------------------------------------------------------------------------------------------ 4. determinism
def test_same_bytes_on_two_runs(setup, lattice):
    from jittor_myc_nerfs_amd import ngp
    a = setup["model"].density_gradient(setup["pos_dev"])
    b = setup["model"].density_gradient(setup["pos_dev"])
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    again = ngp.density_volume(setup["model"], None, dims=DIMS, origin=lattice["origin"], spacing=lattice["spacing"], empty_value=EMPTY)
    assert np.array_equal(_bits(again), _bits(lattice["plain"]))
    bits = setup["arrs"]["density_grid_bitfield"]
    assert np.array_equal(_bits(_with_bitfield(setup, lattice, bits)), _bits(_with_bitfield(setup, lattice, bits)))


# ------------------------------------------------------------------------------------------------------------------ 5. a sphere, end to end
R_SPHERE, K_SPHERE, RES = 0.2, 40.0, 96
UNIT_BOX = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


@pytest.fixture(scope="module")
def sphere(tmp_path_factory):
    from jittor_myc_nerfs_amd import mesh, ngp, ngp_mesh
    from oracle import ngp_oracle as N
    levels = N.grid_levels(NGP_AABB_SCALE)
    arrs = K.sphere_scene(levels, R_SPHERE, K_SPHERE)
    dev = torch.device("cuda:0")
    model, sampler = _model(arrs, NGP_AABB_SCALE, dev, with_sampler=True)
    dims, origin, spacing = ngp_mesh.export_lattice(sampler, RES, UNIT_BOX)
    vol = ngp.density_volume(model, sampler, dims=dims, origin=origin, spacing=spacing)
    verts, faces = mesh.marching_cubes(vol, math.log(1.0), spacing=spacing, origin=origin)
    torch.cuda.synchronize()
    return dict(levels=levels, arrs=arrs, dev=dev, model=model, sampler=sampler, dims=dims, spacing=spacing, vol=vol, verts=verts, faces=faces,
                dir=tmp_path_factory.mktemp("ngp_sphere"))


def test_sphere_mesh_geometry(sphere):
    """Every vertex lies within sqrt(3) / scale + voxel of the sphere: the field is k times a convex combination of values of the 1-Lipschitz R - |p - c| over a cell
    of diagonal sqrt(3) / scale, so its zeros are within that of the sphere, and a marching-cubes vertex is within one voxel of a zero on its edge.  The empty value
    appears outside the surface only (sphere_scene's occupancy is a solid ball), so the mesh is one closed component, oriented outwards."""
    from jittor_myc_nerfs_amd import mesh
    verts, faces = sphere["verts"], sphere["faces"]
    V = verts.shape[0]
    assert sphere["dims"] == [RES] * 3 and V > 1000 and faces.shape[0] > 2000
    assert (sphere["vol"] == -1.0e4).any() and (sphere["vol"] > 0).any()     # space was skipped, and the ball is there
    _, _, n_comp = mesh.mesh_components(faces, V)
    assert int(n_comp) == 1
    st = {}
    mesh.mesh_adjacency(faces, V, stats=st)
    assert st["boundary_edges"] == 0 and st["nonmanifold_edges"] == 0
    _, scale, _ = K.sphere_level(sphere["levels"])
    v = verts.double().cpu().numpy() - 0.5
    dist = np.abs(np.linalg.norm(v, axis=1) - R_SPHERE)
    assert dist.max() <= math.sqrt(3.0) / scale + sphere["spacing"][0], float(dist.max())
    f = faces.cpu().numpy().astype(np.int64)
    volume = float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)
    exact = 4.0 / 3.0 * math.pi * R_SPHERE ** 3
    print(f"sphere: {V} vertices, {f.shape[0]} triangles, worst |r - R| {dist.max():.5f}, signed volume {volume:.6f} vs {exact:.6f} ({volume / exact - 1:+.3%})")
    assert volume > 0 and abs(volume / exact - 1.0) <= 0.05


def test_sphere_normals(sphere):
    """The kernel's normals at the mesh vertices against the fp64 reference's.  The gradient bar (error <= 4 y S per component, y the fp32 restatement's own scaled
    error on these vertices) bounds the angle: |g' - g| <= sqrt(3) * 4 y S, and the angle between g' and g is at most asin(|g' - g| / |g|); the fp32 normalisation
    adds a few 2^-24.  Vertices failing the ReLU margin are excluded, at most 5 % of them (none here: the two live units are +-enc, so the relative margin
    never fails; what protects these vertices, where |raw| / k goes down to 1e-11, is the kernel's rescaled hidden layer for the mask, csrc/tvr_ngp_field.h)."""
    verts = sphere["verts"]
    pos = verts.cpu().numpy()
    ref = K.density_gradient_ref(sphere["arrs"], sphere["levels"], pos, torch.float64)
    keep = K.relu_margin_ok(ref)
    excluded = 1.0 - keep.mean()
    # the yardstick's own ReLU pattern must be the reference's where it is measured: marching cubes puts many vertices where the field is linear along the edge, at
    # |raw| / k ~ 1e-9, and at a few of them (symmetry planes) the fp32 restatement's two live units are exactly 0 — its gradient is then 0, an error of S / 2
    r32 = K.density_gradient_ref(sphere["arrs"], sphere["levels"], pos, torch.float32)
    same = ((r32["h"] > 0) == (ref["h"] > 0)).all(1)
    assert (keep & same).mean() >= 0.9
    yard = K.scaled_error(r32["grad"], ref, keep & same)
    n = sphere["model"].surface_normals(verts).double().cpu().numpy()
    g = ref["grad"]
    gn = np.linalg.norm(g, axis=1)
    assert (gn[keep] > 0).all()
    want = -g / np.maximum(gn, 1e-300)[:, None]
    sin_angle = np.linalg.norm(np.cross(n, want), axis=1)
    bound = np.minimum(1.0, math.sqrt(3.0) * 4 * yard * ref["S"] / np.maximum(gn, 1e-300)) + 8 * 2.0 ** -24
    radial = pos.astype(np.float64) - 0.5
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    mean_deg = float(np.degrees(np.arccos(np.clip((n * radial).sum(1), -1, 1)))[keep].mean())
    print(f"sphere normals: excluded {excluded:.3%}, fp32 yardstick {yard:.3e}, worst sin(angle) {sin_angle[keep].max():.3e} (worst bound ratio "
          f"{(sin_angle[keep] / bound[keep]).max():.3f}), mean angle to the radial direction {mean_deg:.3f} deg")
    norms = np.linalg.norm(n, axis=1)
    print(f"sphere normals: zero normals {(norms == 0).sum()} (kept: {(norms[keep] == 0).sum()}), antiparallel {((n * want).sum(1) < 0).sum()} (kept: "
          f"{((n * want).sum(1)[keep] < 0).sum()}), |raw| / k at zero normals up to {np.abs(ref['raw'][norms == 0]).max(initial=0) / K_SPHERE:.3e}, "
          f"smallest kept |raw| / k {np.abs(ref['raw'][keep]).min() / K_SPHERE:.3e}")
    assert excluded <= 0.05
    assert (sin_angle[keep] <= bound[keep]).all()
    assert (np.abs(np.linalg.norm(n[keep], axis=1) - 1.0) <= 1e-6).all() and ((n * want).sum(1)[keep] > 0).all()
    assert ((n * radial).sum(1)[keep] > 0.9).all()                            # outwards


def test_sphere_export_and_command_line(sphere):
    from jittor_myc_nerfs_amd import mesh, ngp, ngp_mesh
    from jittor_myc_nerfs_amd.ngp_train import save_jnerf_checkpoint
    model, sampler, verts, faces = sphere["model"], sphere["sampler"], sphere["verts"], sphere["faces"]
    path = os.path.join(str(sphere["dir"]), "sphere.ply")
    world, f2 = ngp_mesh.export_mesh(model, sampler, path, density_level=1.0, resolution=RES, bbox=UNIT_BOX, normals=True, colors=True)
    assert torch.equal(f2, faces) and world.shape == verts.shape
    v, f, attrs = mesh.read_ply_attributes(path)
    assert v.shape == (verts.shape[0], 3) and f.shape == (faces.shape[0], 3) and attrs["normals"].shape == v.shape and attrs["colors"].shape == v.shape
    assert attrs["colors"].dtype == np.uint8 and np.array_equal(f, faces.cpu().numpy())
    # world coordinates, the documented mapping by hand for one vertex: x_ngp = u * 4 - 1.5, world = (uncycle(x_ngp) - 0.5) / 0.33
    i = verts.shape[0] // 2
    u = verts[i].double().cpu().numpy()
    x = u * 4.0 - 1.5
    want = (np.array([x[2], x[0], x[1]]) - 0.5) / ngp.NERF_SCALE
    assert np.abs(v[i] - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    back = ngp_mesh.world_to_unit(torch.from_numpy(v[i:i + 1]), sampler.aabb_range).numpy()[0]
    assert np.abs(back - u).max() <= 1e-6
    # the normals are the kernel's at the unit-cube vertices, carried to world axes by the same cycle
    n = model.surface_normals(verts)[:, [2, 0, 1]].cpu().numpy()
    assert np.array_equal(attrs["normals"].view(U32), n.view(U32))
    # the command line, in-process, on a checkpoint of this scene.  Its default box is the occupied cells of cascade 0, the unit cube's [0.375, 0.625]^3 here, so the
    # level is raised to e^4: raw = k (R - r) = 4 at r = R - 4 / k = 0.1, a sphere inside that box.
    ckpt, out = os.path.join(str(sphere["dir"]), "params.pkl"), os.path.join(str(sphere["dir"]), "cli.ply")
    save_jnerf_checkpoint(ckpt, model, sampler, 7)
    assert ngp_mesh.main(["--ckpt", ckpt, "--out", out, "--resolution", "48", "--density_level", repr(math.exp(4.0)), "--normals", "1", "--min_faces", "4",
                          "--keep_largest", "1"]) == 0
    v2, f2, a2 = mesh.read_ply_attributes(out)
    assert len(v2) > 100 and len(f2) > 100 and "normals" in a2 and "colors" not in a2
    u2 = ngp_mesh.world_to_unit(torch.from_numpy(v2), sampler.aabb_range).double().numpy() - 0.5
    _, scale, _ = K.sphere_level(sphere["levels"])
    voxel = (0.25 + 2 * 0.25 / 47) / 47 * 1.01                                # the padded box's lattice is no coarser than the unpadded one's voxel
    assert np.abs(np.linalg.norm(u2, axis=1) - (R_SPHERE - 4.0 / K_SPHERE)).max() <= math.sqrt(3.0) / scale + voxel
