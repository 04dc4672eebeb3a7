"""CPU: TensorCP's C-ABI argument checks and host logic (constructor, parameter shapes, optimizer groups, checkpoints, grid maintenance, regularisers, refusals), and a
check of the tests' OWN CP restatement (cp_common.py) against a dense trilinear lookup — every GPU test of tests/test_gpu_cp.py leans on that restatement."""
import ctypes as C
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cp_common as CC
from conftest import TINY


def _desc(L, r_sigma=96, r_app=288, grid=(300, 300, 300), view_pe=2, fea_pe=2, variant=0):
    d = L.SceneDesc()
    d.grid[:] = list(grid)
    d.aabb[:] = [-1.5] * 3 + [1.5] * 3
    d.density_n_comp[:] = [r_sigma, 0, 0]                    # entries [1], [2] are ignored
    d.app_n_comp[:] = [r_app, 0, 0]
    d.app_dim, d.featureC, d.view_pe, d.fea_pe, d.step_size, d.variant = 27, 128, view_pe, fea_pe, 0.005, variant
    return d


def test_cp_abi_argument_errors_without_gpu():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    for kw, field in ((dict(r_sigma=97), b"density_n_comp[0]"), (dict(r_app=289), b"app_n_comp[0]"), (dict(variant=1), b"variant"), (dict(view_pe=7), b"view_pe")):
        d = _desc(L, **kw)
        assert lib.tvr_cp_scene_packed_bytes(C.byref(d)) == 0, kw
        assert field in lib.tvr_last_error(), (kw, lib.tvr_last_error())
        h = C.c_void_p()
        assert lib.tvr_cp_scene_create(C.byref(d), None, 0, C.byref(h)) == -4 and field in lib.tvr_last_error()      # TVR_ERR_UNSUPPORTED
    d = _desc(L)
    n = lib.tvr_cp_scene_packed_bytes(C.byref(d))
    assert 1.3e6 < n < 4e6, n                                # lines (3 x 301 x (96 + 288) x 4 B) and the network; no planes (the VM scene: 96 MB)
    assert lib.tvr_cp_scene_packed_bytes(C.byref(_desc(L, 1, 1))) < n
    assert lib.tvr_cp_scene_packed_bytes(C.byref(_desc(L, view_pe=6, fea_pe=6))) == n + 26 * 8192       # + the streamed layer-1 image of the lockstep form
    h = C.c_void_p()
    assert lib.tvr_cp_scene_create(C.byref(d), None, 0, C.byref(h)) == -3                                # TVR_ERR_SCRATCH
    assert lib.tvr_scene_packed_bytes(C.byref(d)) == 0       # the same descriptor is no TensorVMSplit scene (96 > 16 components per plane)


def _cpu_model(r=(96, 288), **kw):
    from jittor_myc_nerfs_amd import synthetic
    hyper = dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=TINY["step_ratio"])
    arrs = CC.cp_arrays(*r)
    return CC.make_cp_model(arrs, hyper, device="cpu", **kw), arrs


def test_cp_constructor_shapes_groups_and_kwargs_round_trip():
    from jittor_myc_nerfs_amd import TensorCP
    m, arrs = _cpu_model()
    g = TINY["gridSize"]
    for i in range(3):
        assert tuple(m.density_line[i].shape) == (1, 96, g[2 - i], 1) and tuple(m.app_line[i].shape) == (1, 288, g[2 - i], 1)
    assert tuple(m.basis_mat.weight.shape) == (27, 288)
    groups = m.get_optparam_groups(0.02, 0.001)
    assert len(groups) == 4 and [gr["lr"] for gr in groups] == [0.02, 0.02, 0.001, 0.001]
    assert sum(len(list(gr["params"])) for gr in groups) == len(list(m.parameters())) == 3 + 3 + 1 + 6
    keys = set(m.state_dict().keys())
    assert keys == ({f"density_line.{i}" for i in range(3)} | {f"app_line.{i}" for i in range(3)} | {"basis_mat.weight"}
                    | {f"renderModule.mlp.{j}.{p}" for j in (0, 2, 4) for p in ("weight", "bias")})
    assert not hasattr(m, "density_plane") and not hasattr(m, "app_plane")
    # the reference's initialisation: scale 0.2 (tensoRF.py:323-324)
    torch.manual_seed(0)
    fresh = TensorCP(TINY["aabb"], [64, 64, 64], "cpu", density_n_comp=[96], appearance_n_comp=[288], shadingMode="MLP_Fea", view_pe=2, fea_pe=2)
    assert abs(float(torch.cat([p.detach().reshape(-1) for p in fresh.density_line]).std()) - 0.2) < 0.01
    kw = m.get_kwargs()
    assert kw["density_n_comp"] == [96] and kw["appearance_n_comp"] == [288] and kw["gridSize"] == g
    m2 = TensorCP(device="cpu", **kw)
    assert {k: tuple(v.shape) for k, v in m2.state_dict().items()} == {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert m2.nSamples == m.nSamples and float(m2.stepSize) == float(m.stepSize)


def test_cp_save_load_bit_equal(tmp_path):
    from jittor_myc_nerfs_amd import TensorCP, AlphaGridMask, load_checkpoint
    m, _ = _cpu_model((5, 50))
    vol = (torch.rand(6, 5, 4) > 0.5).float()
    m.alphaMask = AlphaGridMask("cpu", m.aabb, vol)
    path = str(tmp_path / "cp.th")
    m.save(path)
    ckpt = load_checkpoint(path)
    m2 = TensorCP(device="cpu", **ckpt["kwargs"])
    m2.load(ckpt)
    for (k, a), (k2, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
    assert torch.equal(m2.alphaMask.alpha_volume.view(6, 5, 4), vol)
    # a reference `.th` dict: numpy arrays, plus non-parameter entries a Jittor state_dict lists
    sd = {k: v.numpy() for k, v in m.state_dict().items()}
    sd["aabb"] = np.zeros((2, 3), np.float32)
    m3 = TensorCP(device="cpu", **ckpt["kwargs"])
    m3.load({"kwargs": ckpt["kwargs"], "state_dict": sd})
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m3.state_dict().values()))


def test_cp_upsample_shrink_and_regularisers_match_the_reference_lines():
    from jittor_myc_nerfs_amd import AlphaGridMask
    m, arrs = _cpu_model((16, 48))
    dl = [p.detach().clone() for p in m.density_line]
    al = [p.detach().clone() for p in m.app_line]
    # density_L1 (tensoRF.py:431-435), TV terms with weight 1e-3 (:437-447)
    assert torch.equal(m.density_L1(), sum(torch.mean(torch.abs(x)) for x in dl))
    reg = lambda x: ((x[:, :, 1:] - x[:, :, :-1]) ** 2).sum()
    assert torch.equal(m.TV_loss_density(reg), sum(reg(x) * 1e-3 for x in dl))
    assert torch.equal(m.TV_loss_app(reg), sum(reg(x) * 1e-3 for x in al))
    # upsample_volume_grid (:380-398): each line to res_target[vecMode[i]] points, bilinear, align_corners=True
    target = [21, 33, 40]
    m.upsample_volume_grid(target)
    for i in range(3):
        want = F.interpolate(dl[i], size=(target[2 - i], 1), mode="bilinear", align_corners=True)
        assert torch.equal(m.density_line[i].data, want) and tuple(m.app_line[i].shape) == (1, 48, target[2 - i], 1)
        assert torch.equal(m.app_line[i].data, F.interpolate(al[i], size=(target[2 - i], 1), mode="bilinear", align_corners=True))
    assert m.gridSize.tolist() == target and len(m.get_optparam_groups()) == 4
    # shrink (:401-429) with an alpha mask of another resolution: index arithmetic and the corrected box
    dl = [p.detach().clone() for p in m.density_line]
    aabb0, units, grid = m.aabb.clone(), m.units.clone(), m.gridSize.clone()
    m.alphaMask = AlphaGridMask("cpu", m.aabb, torch.ones(8, 8, 8))
    new_aabb = torch.tensor([[-0.9, -0.5, -0.7], [0.8, 0.9, 0.4]])
    m.shrink(new_aabb)
    t_l, b_r = (new_aabb[0] - aabb0[0]) / units, (new_aabb[1] - aabb0[0]) / units
    t_l, b_r = torch.round(torch.round(t_l)).long(), torch.round(b_r).long() + 1
    b_r = torch.stack([b_r, grid.long()]).amin(0)
    for i in range(3):
        ax = 2 - i
        assert torch.equal(m.density_line[i].data, dl[i][..., int(t_l[ax]):int(b_r[ax]), :])
    t_l_r, b_r_r = t_l / (grid - 1), (b_r - 1) / (grid - 1)
    assert torch.equal(m.aabb[0], (1 - t_l_r) * aabb0[0] + t_l_r * aabb0[1]) and torch.equal(m.aabb[1], (1 - b_r_r) * aabb0[0] + b_r_r * aabb0[1])
    assert m.gridSize.tolist() == (b_r - t_l).tolist()


def test_cp_has_no_cpu_fallback_and_no_training():
    from jittor_myc_nerfs_amd import _lib as L
    m, _ = _cpu_model((5, 50))
    pts = torch.zeros(4, 3)
    rays = torch.tensor([[0.0, 0.0, -4.0, 0.0, 0.0, 1.0]])
    for call in (lambda: m.compute_densityfeature(pts), lambda: m.compute_appfeature(pts), lambda: m.compute_alpha(pts), lambda: m.render_rays(rays),
                 lambda: m(rays, is_train=False), lambda: m.renderModule._owner()._mlp_render(pts, torch.zeros(4, 27))):
        with pytest.raises(L.TvrError):
            with torch.no_grad():
                call()
    with pytest.raises(NotImplementedError, match="CP training is not built"):
        m(rays, is_train=True)
    with pytest.raises(NotImplementedError, match="CP training is not built"):
        m.render_rays_autograd(rays)


def test_reconstruct_lists_cp_and_refuses_to_train_it():
    from jittor_myc_nerfs_amd import TensorCP, reconstruct
    assert "TensorCP" in reconstruct.MODELS and reconstruct.MODELS["TensorCP"] is TensorCP
    args = types.SimpleNamespace(model_name="TensorCP", dataset_name="blender", datadir="/nonexistent/never/opened", ndc_ray=0)
    with pytest.raises(NotImplementedError, match="CP training is not built"):
        reconstruct.reconstruction(args, device="cpu")


@pytest.mark.parametrize("r", [(5, 50), (1, 1)])
def test_the_restatement_equals_a_dense_trilinear_lookup(r):
    """A trilinear interpolation of a separable product is the product of the linear interpolations: the restatement of tensoRF.py:345-360 every GPU test leans on must
    agree with a 3-D grid_sample of the dense tensor sum_r L2[r][x] L1[r][y] L0[r][z] on the tiny grid (three different axis lengths: a vecMode mix-up shows)."""
    arrs = CC.cp_arrays(*r)
    L0, L1, L2 = [torch.as_tensor(arrs[f"density_line.{i}"]).double()[0, :, :, 0] for i in range(3)]      # [R, gz], [R, gy], [R, gx]
    gx, gy, gz = TINY["gridSize"]
    assert L0.shape[1] == gz and L1.shape[1] == gy and L2.shape[1] == gx
    dense = torch.einsum("rz,ry,rx->zyx", L0, L1, L2)[None, None]                                      # (1, 1, D = z, H = y, W = x)
    pts = torch.tensor(np.random.default_rng(3).uniform(-1, 1, (500, 3)))                              # (x, y, z) in [-1, 1]
    want = F.grid_sample(dense, pts.view(1, -1, 1, 1, 3), align_corners=True).view(-1)
    got = CC.cp_density(arrs, pts, torch.float64)
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
    got32 = CC.cp_density(arrs, pts.float(), torch.float32)
    assert float((got32.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    # the appearance restatement the same way, component by component through an identity basis
    a = dict(arrs, basis_mat=np.eye(27, r[1], dtype=np.float32))
    A0, A1, A2 = [torch.as_tensor(arrs[f"app_line.{i}"]).double()[0, :, :, 0] for i in range(3)]
    k = min(27, r[1])
    dense_a = torch.einsum("rz,ry,rx->rzyx", A0[:k], A1[:k], A2[:k])[None]
    want_a = F.grid_sample(dense_a, pts.view(1, -1, 1, 1, 3), align_corners=True).view(k, -1).T
    got_a = CC.cp_app(a, pts, torch.float64)[:, :k]
    assert float((got_a - want_a).abs().max()) <= 1e-5 * float(want_a.abs().max())
