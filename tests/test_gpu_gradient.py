"""GPU: tvr_density_gradient (csrc/tvr_march.hip density_gradient_kernel, csrc/tvr_cp.hip cp_density_gradient_kernel) and what stands on it — surface normals,
head-on vertex colours and the PLY attributes of export_mesh.

The oracle is the tests' own fp64 restatement (tests/gradient_common.py).  The allowance is cp_common.allowance(g32, g64, relative=True): four times the error the
same restatement makes in fp32 on the CPU against fp64 on the same inputs, never below the default floor of 1e-6 of max |g64|; it is computed from the two
restatements alone, never from what the kernel returns.  Beyond the oracle the header promises bit-equalities, which are asserted as such: the centre value against
tvr_density_feature, and the gradient against the same quotient of tvr_density_feature at the shifted points."""
import ctypes as C

import numpy as np
import pytest
import torch

import cp_common as CC
import gradient_common as GC
from conftest import TINY, make_model

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 1029)


def _hyper():
    from jittor_myc_nerfs_amd import synthetic
    return dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=TINY["step_ratio"])


def _np(t):
    return t.detach().cpu().numpy()


def _check_gradient(m, density, label):
    """density(dtype) -> f.  Every half width on the whole point set, then the sizes 1 / 63 / 1029 (one lane's quad alone, a ragged wave, more than one block
    with a ragged last one: 1029 points are 4116 lanes = 16 blocks of 256 + 20 lanes; the CP kernel's 1029 lanes = 4 blocks + 5)."""
    from jittor_myc_nerfs_amd import _lib as L
    pts = GC.point_set(TINY["gridSize"])
    assert pts.shape[0] > max(SIZES)
    x = pts.cuda()
    sf_ref = m.compute_densityfeature(x)
    f64, f32 = density(torch.float64), density(torch.float32)
    for name, h in GC.half_widths(TINY["gridSize"]).items():
        g64, g32 = GC.gradient_restatement(f64, pts, h, torch.float64), GC.gradient_restatement(f32, pts, h, torch.float32)
        tol = CC.allowance(g32, g64, relative=True)
        sf, g = m.compute_density_gradient(x, half_width=None if name == "cell" else h.tolist())
        torch.cuda.synchronize()
        err = float((g.cpu().double() - g64).abs().max())
        print(f"    {label} / h = {name}: max |g64| = {float(g64.abs().max()):.4g}, fp32 restatement error = {float((g32.double() - g64).abs().max()):.3g}, "
              f"kernel error = {err:.3g}, allowance = {tol:.3g}")
        assert g.shape == (pts.shape[0], 3) and sf.shape == (pts.shape[0],)
        assert bool(torch.isfinite(g).all())
        assert err <= tol
        assert torch.equal(sf, sf_ref)                                             # the centre: bit-equal to tvr_density_feature
        # the gradient: bit-equal to the quotient of tvr_density_feature at the shifted points (shift, difference and product separately rounded fp32)
        hd = h.cuda()
        comp = torch.stack([(m.compute_densityfeature(GC.shifted(x, hd, k, +1)) - m.compute_densityfeature(GC.shifted(x, hd, k, -1))) *
                            (torch.tensor(0.5) / h[k]).cuda() for k in range(3)], -1)
        nd = int((g != comp).sum())
        print(f"      elements that differ from the composition of seven tvr_density_feature calls: {nd}")
        assert torch.equal(g, comp)
        # sigma_feature = NULL: the same gradient
        sc = m._ensure_scene()
        hw = (C.c_float * 3)(*h.tolist())
        g2 = torch.full_like(g, float("nan"))
        L.check(L.lib().tvr_density_gradient(sc, x.data_ptr(), x.shape[0], C.byref(hw), None, 0, g2.data_ptr(), L.nbytes(g2), None), "tvr_density_gradient")
        torch.cuda.synchronize()
        assert torch.equal(g2, g)
        for n in SIZES:
            sfn, gn = m.compute_density_gradient(x[:n].contiguous(), half_width=h.tolist())
            assert torch.equal(gn, g[:n]) and torch.equal(sfn, sf[:n]), (name, n)


@pytest.mark.parametrize("comps", ["16x3", "5-8-3"])
def test_vm_gradient(tiny_arrays, comps):
    from jittor_myc_nerfs_amd import synthetic
    hyper = _hyper()
    if comps == "16x3":
        arrs, m = tiny_arrays, make_model(tiny_arrays, hyper)
    else:                                                                          # unequal, smaller component counts: zero-padded channels in every texel
        dc, ac = [5, 8, 3], [7, 12, 5]
        arrs = synthetic.make_scene_arrays(TINY["gridSize"], TINY["aabb"], seed=5, density_n_comp=dc, appearance_n_comp=ac)
        m = GC.make_vm_model(arrs, hyper, dc, ac)
    _check_gradient(m, lambda dt: GC.vm_density(arrs, hyper, dt), f"VM {comps}")


@pytest.mark.parametrize("r_sigma,r_app", [r for r in CC.RANKS if r[0] in (96, 5, 1)])
def test_cp_gradient(r_sigma, r_app):
    arrs = CC.cp_arrays(r_sigma, r_app)
    m = CC.make_cp_model(arrs, _hyper())
    _check_gradient(m, lambda dt: GC.cp_density_fn(arrs, dt), f"CP R_sigma = {r_sigma}")


def test_argument_checks_come_before_any_launch(tiny_arrays):
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    for m in (make_model(tiny_arrays, _hyper()), CC.make_cp_model(CC.cp_arrays(5, 50), _hyper())):
        sc = m._ensure_scene()
        n = 100
        x = (torch.rand((n, 3), device="cuda") * 2 - 1).contiguous()
        grad = torch.full((n, 3), -7.0, device="cuda")
        sigma = torch.full((n,), -7.0, device="cuda")
        good = (C.c_float * 3)(0.1, 0.1, 0.1)

        def call(hw, grad_bytes=None, sigma_bytes=None, count=n, xp=x.data_ptr(), gp=grad.data_ptr()):
            return lib.tvr_density_gradient(sc, xp, count, hw, sigma.data_ptr(), L.nbytes(sigma) if sigma_bytes is None else sigma_bytes, gp,
                                            L.nbytes(grad) if grad_bytes is None else grad_bytes, None)

        for bad in (0.0, -0.1, float("nan"), float("inf")):
            for k in range(3):
                hw = (C.c_float * 3)(0.1, 0.1, 0.1)
                hw[k] = bad
                assert call(C.byref(hw)) == -1 and b"half_width" in lib.tvr_last_error(), (bad, k)
        assert call(None) == -1
        assert call(C.byref(good), grad_bytes=n * 12 - 4) == -3 and b"grad [m,3]" in lib.tvr_last_error()
        assert call(C.byref(good), sigma_bytes=n * 4 - 4) == -3 and b"sigma_feature [m]" in lib.tvr_last_error()
        assert call(C.byref(good), count=-1) == -1
        assert call(C.byref(good), xp=None) == -1 and call(C.byref(good), gp=None) == -1
        torch.cuda.synchronize()
        assert bool((grad == -7.0).all()) and bool((sigma == -7.0).all())           # nothing was launched
        assert call(C.byref(good), count=0) == 0
        assert lib.tvr_density_gradient(sc, None, 0, C.byref(good), None, 0, None, 0, None) == 0
        torch.cuda.synchronize()
        assert bool((grad == -7.0).all()) and bool((sigma == -7.0).all())
        assert call(C.byref(good)) == 0                                             # and the same call with everything right runs
        torch.cuda.synchronize()
        assert not bool((grad == -7.0).any()) and not bool((sigma == -7.0).any())
        sf, g = m.compute_density_gradient(x, half_width=0.1)
        assert torch.equal(g, grad) and torch.equal(sf, sigma)
        with pytest.raises(ValueError):
            m.compute_density_gradient(x, half_width=[0.1, 0.1])
        with pytest.raises(L.TvrError):
            m.compute_density_gradient(x, half_width=0.0)
        e_sf, e_g = m.compute_density_gradient(x[:0])
        assert e_sf.shape == (0,) and e_g.shape == (0, 3)


def test_normals_of_a_gaussian_blob(tmp_path):
    """A rank-1 CP scene whose density lines are positive Gaussians centred on a grid node c: unimodal and symmetric about c along every axis, so each component of
    -grad (symmetric difference) has the sign of x_k - c_k or is zero — by the definition, not by measurement — and every normal points away from c."""
    arrs = GC.gaussian_cp_arrays()
    m = CC.make_cp_model(arrs, _hyper())
    alpha = m.getDenseAlpha()[0]
    level = 0.5 * (float(alpha.min()) + float(alpha.max()))
    verts, faces = m.export_mesh(str(tmp_path / "blob.ply"), level=level, spacing="samples")
    assert verts.shape[0] >= 30 and faces.shape[0] >= 30
    n = m.surface_normals(verts)
    torch.cuda.synchronize()
    assert n.shape == verts.shape and n.dtype == torch.float32
    length = n.double().norm(dim=-1)
    assert float((length - 1.0).abs().max()) <= 1e-5
    c = torch.as_tensor(GC.gaussian_centre_world())
    out = (n.cpu().double() * (verts.cpu().double() - c)).sum(-1)
    assert float(out.min()) > 0.0, f"{int((out <= 0).sum())} of {len(out)} normals do not point away from the blob's centre"
    # against the fp64 restatement, with the normalised fp32 coordinates the library was given as the input of both restatements
    xn = m.normalize_coord(verts).cpu()
    h = GC.cell(TINY["gridSize"])
    n64 = GC.normals_restatement(GC.gradient_restatement(GC.cp_density_fn(arrs, torch.float64), xn, h, torch.float64), TINY["aabb"], torch.float64)
    n32 = GC.normals_restatement(GC.gradient_restatement(GC.cp_density_fn(arrs, torch.float32), xn, h, torch.float32), TINY["aabb"], torch.float32)
    a32, a = float(GC.angles(n32, n64).max()), float(GC.angles(n.cpu(), n64).max())
    tol = max(4.0 * a32, 1e-6)                                                     # cp_common.allowance's rule on the angle (radians)
    print(f"    {verts.shape[0]} vertices: largest angle to the fp64 normals {a:.3g} rad, fp32 restatement {a32:.3g} rad, allowance {tol:.3g} rad")
    assert a <= tol
    # a zero gradient (far outside the box every tap is padding) gives a zero vector, not NaN
    far = torch.tensor([[50.0, 50.0, 50.0]], device="cuda")
    assert torch.equal(m.surface_normals(far), torch.zeros((1, 3), device="cuda"))


# ---- colours --------------------------------------------------------------------------------------------------------------------------------------------------------
def _surface(m):
    from jittor_myc_nerfs_amd import marching_cubes
    alpha = m.getDenseAlpha()[0]
    level = 0.5 * (float(alpha.min()) + float(alpha.max()))
    aabb = m.aabb.float()
    n = torch.tensor([float(s) for s in alpha.shape])
    verts, faces = marching_cubes(alpha, level, spacing=((aabb[1] - aabb[0]) / (n - 1)).tolist(), origin=aabb[0].tolist())
    assert verts.shape[0] >= 30
    return verts, faces, level


@pytest.mark.parametrize("name", ["TensorVMSplit", "TensorCP", "NerfPlusPlus"])
def test_vertex_colours(tiny_arrays, tiny_npp_arrays, name):
    from oracle import tensorf_oracle as TO
    hyper = _hyper()
    if name == "TensorCP":
        arrs = CC.cp_arrays(16, 48)
        m = CC.make_cp_model(arrs, hyper)
    else:
        arrs = tiny_arrays if name == "TensorVMSplit" else tiny_npp_arrays
        m = make_model(arrs, hyper)
    assert type(m).__name__ == name
    verts, _, _ = _surface(m)
    attrs = m.mesh_vertex_attributes(verts)
    torch.cuda.synchronize()
    assert sorted(attrs) == ["colors", "normals"]
    nrm, col = attrs["normals"], attrs["colors"]
    assert col.dtype == torch.uint8 and col.shape == verts.shape and col.device.type == "cuda" and nrm.dtype == torch.float32
    assert torch.equal(nrm, m.surface_normals(verts))
    # byte for byte the public calls composed by hand
    with torch.no_grad():
        xn = m.normalize_coord(verts)
        rgb = m.renderModule(None, -nrm, m.compute_appfeature(xn))
        by_hand = torch.round(255.0 * rgb.clamp(0, 1)).to(torch.uint8)
    assert torch.equal(col, by_hand)
    assert int(col.max()) > int(col.min())                                         # not one flat colour
    # against the fp64 network on the same normals: the project's RGB bar (1e-3) in levels plus one rounding step
    xc, vd = xn.cpu(), (-nrm).cpu().double()
    if name == "TensorCP":
        sc64 = CC.oracle_scene(arrs, hyper, torch.float64)
        f64 = CC.cp_app(arrs, xc, torch.float64)
    else:
        sc64 = GC.vm_oracle(arrs, hyper, torch.float64)
        f64 = TO.compute_appfeature(sc64, xc.double())
    rgb64 = TO.mlp_render_fea(sc64, vd, f64)
    err = float((col.cpu().double() - 255.0 * rgb64.clamp(0, 1)).abs().max())
    print(f"    {name}: {verts.shape[0]} vertices, largest |colour - 255 rgb64| = {err:.3f} levels")
    assert err <= 1e-3 * 255 + 1
    only_n = m.mesh_vertex_attributes(verts, colors=False)
    only_c = m.mesh_vertex_attributes(verts, normals=False)
    assert sorted(only_n) == ["normals"] and sorted(only_c) == ["colors"] and torch.equal(only_c["colors"], col) and torch.equal(only_n["normals"], nrm)
    empty = m.mesh_vertex_attributes(verts[:0])
    assert empty["normals"].shape == (0, 3) and empty["colors"].shape == (0, 3) and empty["colors"].dtype == torch.uint8


def test_reftensorf_gives_normals_and_refuses_colours(tiny_ref_arrays):
    m = make_model(tiny_ref_arrays, _hyper())
    assert type(m).__name__ == "REFTensoRF"
    verts, _, _ = _surface(m)
    attrs = m.mesh_vertex_attributes(verts, colors=False)
    assert sorted(attrs) == ["normals"] and torch.equal(attrs["normals"], m.surface_normals(verts))
    assert float((attrs["normals"].double().norm(dim=-1) - 1.0).abs().max()) <= 1e-5
    with pytest.raises(NotImplementedError, match="REFTensoRF"):
        m.mesh_vertex_attributes(verts)
    with pytest.raises(NotImplementedError, match="REFTensoRF"):
        m.mesh_vertex_attributes(verts, normals=False, colors=True)


# ---- export_mesh end to end ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["TensorVMSplit", "TensorCP"])
def test_export_mesh_with_attributes(tiny_arrays, tmp_path, name):
    from jittor_myc_nerfs_amd import read_ply, read_ply_attributes, reconstruct as R
    m = make_model(tiny_arrays, _hyper()) if name == "TensorVMSplit" else CC.make_cp_model(CC.cp_arrays(16, 48), _hyper())
    alpha = m.getDenseAlpha()[0]
    level = 0.5 * (float(alpha.min()) + float(alpha.max()))
    aabb = m.aabb.float().cuda()
    n = torch.tensor([float(s) for s in alpha.shape], device="cuda")
    for spacing in ("reference", "samples"):
        plain, off, on, again = [str(tmp_path / f"{name}_{spacing}_{k}.ply") for k in ("plain", "off", "on", "again")]
        pv, pf = m.export_mesh(plain, level=level, spacing=spacing)
        ov, of = m.export_mesh(off, level=level, spacing=spacing, normals=False, colors=False)
        assert open(plain, "rb").read() == open(off, "rb").read() and torch.equal(pv, ov) and torch.equal(pf, of)
        av, af = m.export_mesh(on, level=level, spacing=spacing, normals=True, colors=True)
        assert torch.equal(av, pv) and torch.equal(af, pf)
        v, f, attrs = read_ply_attributes(on)
        v0, f0 = read_ply(plain)
        assert f.shape[0] >= 1 and np.array_equal(v, v0) and np.array_equal(f, f0)      # the vertices written stay as they are, bit for bit
        at = pv if spacing == "samples" else aabb[0] + (pv - aabb[0]) * (n / (n - 1))    # where the field was sampled
        want = m.mesh_vertex_attributes(at)
        assert np.array_equal(attrs["normals"], _np(want["normals"])) and np.array_equal(attrs["colors"], _np(want["colors"]))
        assert attrs["normals"].dtype == np.float32 and attrs["colors"].dtype == np.uint8
        with pytest.raises(ValueError):
            read_ply(on)
        m.export_mesh(again, level=level, spacing=spacing, normals=True, colors=True)
        assert open(again, "rb").read() == open(on, "rb").read()
        # one attribute alone
        m.export_mesh(again, level=level, spacing=spacing, normals=True)
        v1, f1, a1 = read_ply_attributes(again)
        assert sorted(a1) == ["normals"] and np.array_equal(a1["normals"], attrs["normals"]) and np.array_equal(v1, v0) and np.array_equal(f1, f0)
        # flip reverses the triangles only: the normals follow the field
        m.export_mesh(again, level=level, spacing=spacing, flip=True, normals=True, colors=True)
        v2, f2, a2 = read_ply_attributes(again)
        assert np.array_equal(v2, v0) and np.array_equal(np.sort(f2, axis=1), np.sort(f0, axis=1)) and not np.array_equal(f2, f0)
        assert np.array_equal(a2["normals"], attrs["normals"]) and np.array_equal(a2["colors"], attrs["colors"])
        print(f"    {name} / {spacing}: {v.shape[0]} vertices, {f.shape[0]} triangles with normals and colours")
    # the command line on a checkpoint of this model (spacing "reference", the checkpoint's grid)
    ckpt = tmp_path / f"{name}.th"
    m.save(str(ckpt))
    out = R.main(["--export_mesh", "1", "--ckpt", str(ckpt), "--model_name", name, "--mesh_level", repr(level), "--mesh_normals", "1", "--mesh_colors", "1"])
    assert out == str(tmp_path / f"{name}.ply")
    assert open(out, "rb").read() == open(str(tmp_path / f"{name}_reference_on.ply"), "rb").read()
    out = R.main(["--export_mesh", "1", "--ckpt", str(ckpt), "--model_name", name, "--mesh_level", repr(level)])
    assert open(out, "rb").read() == open(str(tmp_path / f"{name}_reference_plain.ply"), "rb").read()
