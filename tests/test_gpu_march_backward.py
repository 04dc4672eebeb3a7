"""GPU (-m gpu): march_backward_kernel and app_h_backward_kernel (csrc/tvr_train.hip) beyond the one configuration the other gradient tests run them in (48 samples =
one chunk, eps_T = 0, grid 16x20x24 = the LDS form of both): more than one 64-sample chunk, early exit on, a chunk skipped in the middle of a ray, a chunk behind the
box, the explicit-depth form with its lam6 gradient, and grids on either side of the two kernels' LDS limits.

Reference: tests/march_backward_common.py (float64, from the formulas; vetted on the CPU by tests/test_march_backward_host.py, which also shows that a dropped carry
or an off-by-one chunk would miss the bar by a wide margin on exactly these inputs).  Bars: the training step's own — 5e-4 of a tensor's largest gradient entry, 2e-4
on forward outputs (tests/test_gpu_training.py::test_gradients_match_oracle_autograd).

Which path a test drives is in its id:
  * S64 / S65 / S130 / S192 / S256: 1, 2 (one lane, dist 0), 3, 3, 4 chunks; eps0: no exit; eps0.0001: the `T < eps_T` break after chunk 0 and after a later chunk;
  * hollow-*: the `mv == 0 -> continue` with the tap windows carried over it, and the `mb == 0 && seen` break; bits / float: the two alpha-mask lookups;
  * zform-*: tvr_march_backward_z with d lam6;
  * 997x12x12: march_backward_kernel<LINE_LDS = true> at the last size that fits; 998x12x12: <false>; both: app_h_backward_kernel<false>;
    500x260x140: both kernels' LDS forms with long lines."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import march_backward_common as MB
from conftest import make_model

pytestmark = pytest.mark.gpu


def _dev(x, dtype=torch.float32):
    return None if x is None else torch.as_tensor(x).to("cuda", dtype).contiguous()


def _float_alpha_lookup(m):
    """hand the scene its alpha volume WITHOUT the bit volume the model builds beside it: the kernels then take alpha_lookup(...) > 0 (include/tvr.h,
    tvr_scene_set_alpha with bits = NULL)"""
    from jittor_myc_nerfs_amd import _lib as L
    sc = m._ensure_scene(settle=False)
    am = m.alphaMask
    ag, ab, inv = am._c_args()
    L.check(L.lib().tvr_scene_set_alpha(sc, am.alpha_volume.data_ptr(), C.byref(ag), C.byref(ab), C.byref(inv), None, 0, None), "tvr_scene_set_alpha")
    m._alpha_bits = None


def _march(m, c):
    """the case's loss through _MarchFn on the device -> (queue sorted ray-major / along the ray: w, xyz, ray; acc; lam; six density gradients)"""
    from jittor_myc_nerfs_amd.autograd_ops import _MarchFn
    rays = _dev(c.rays)
    params = list(m.density_plane) + list(m.density_line)
    w, acc, xyz, ray_id, _, lam = _MarchFn.apply(m, rays, _dev(c.jitter), c.S, c.eps_T, _dev(c.z_vals), *params)
    loss = (MB.g_of(xyz) * w).sum() + (_dev(c.a) * acc).sum()                  # grad_w = g at the queue's own positions
    if c.z_form:
        loss = loss + (_dev(c.b) * lam).sum()
    grads = torch.autograd.grad(loss, params)
    # the queue's order across rays is the kernels' business: sort by ray, then along the ray
    along = (xyz.detach() * (rays[ray_id, 3:6] * _dev(c.sc.invaabbSize))).sum(-1).cpu().numpy()
    order = torch.as_tensor(np.lexsort((along, ray_id.cpu().numpy())))
    return dict(w=w.detach().cpu()[order], xyz=xyz.detach().cpu()[order], ray=ray_id.cpu()[order], acc=acc.detach().cpu(), lam=lam.detach().cpu(),
                grads=[g.cpu() for g in grads], xyz_dev=xyz.detach())


def _check_march(name, c, got):
    r = c.ref()
    app = r["app"]
    ray_ref = torch.nonzero(app)[:, 0]
    assert got["ray"].shape == ray_ref.shape and torch.equal(got["ray"], ray_ref), f"{name}: the queue holds {got['ray'].shape[0]} samples, the reference {int(app.sum())}"
    worst_f = {"w": float((got["w"].double() - r["w"][app]).abs().max()), "acc": float((got["acc"].double() - r["acc"]).abs().max()),
               "xyz": float((got["xyz"].double() - r["xyz"][app]).abs().max())}
    if c.z_form:
        worst_f["lam"] = float((got["lam"].double() - r["lam6"]).abs().max())
    worst = 0.0
    for k, g, gr in zip(MB.DENSITY_NAMES, got["grads"], r["grads"]):
        err = MB.rel_err(g, gr)
        worst = max(worst, err)
        print(f"MEASURED {name} grad {k:16s} rel-max-err {err:.2e}  (max |g_ref| {float(gr.abs().max()):.2e})")
    print(f"MEASURED {name} forward " + " ".join(f"{k} {v:.2e}" for k, v in worst_f.items()) + f"  WORST-GRAD {worst:.2e}  (n {c.n}, S {c.S}, eps_T {c.eps_T:g}, "
          f"grid {list(c.sc.gridSize)}, ends per chunk {c.stats()['ends_in']})")
    assert worst_f["xyz"] < 1e-5, worst_f
    for k in ("w", "acc", "lam"):
        assert worst_f.get(k, 0.0) < MB.BAR_FWD, (k, worst_f)
    for k, g, gr in zip(MB.DENSITY_NAMES, got["grads"], r["grads"]):
        assert float(gr.abs().max()) > 0, f"{k}: the reference gradient is identically zero"
        assert MB.rel_err(g, gr) < MB.BAR_GRAD, f"{name} {k}: max |grad diff| / max |grad| = {MB.rel_err(g, gr):.2e}"


@pytest.mark.parametrize("name", list(MB.KERNEL_CASES))
def test_march_matches_float64_reference(name):
    """w (queue), acc, lam6 and the six density-factor gradients of tvr_march_forward / _backward (and the _z forms) against the float64 reference"""
    c = MB.KERNEL_CASES[name]()
    assert c.n_dropped <= MB.MAX_DROPPED * c.n_before
    m = make_model(c.arrs, c.hyper)
    if name.startswith("hollow-float"):
        _float_alpha_lookup(m)
    _check_march(name, c, _march(m, c))


# ---- the LDS limits ------------------------------------------------------------------------------------------------------------------------------
GRIDS = {"997x12x12-sum1021-march_LINE_LDS_true-app_h_LINE_LDS_false": ([997, 12, 12], True, False),
         "998x12x12-sum1022-march_LINE_LDS_false-app_h_LINE_LDS_false": ([998, 12, 12], False, False),
         "500x260x140-sum900-march_LINE_LDS_true-app_h_LINE_LDS_true": ([500, 260, 140], True, True)}


@functools.lru_cache(maxsize=None)
def _on_grid(name):
    """(model, case, the march's results) with the tiny field upsampled to a big ragged grid; the reference gets the upsampled arrays back from the model"""
    grid, march_lds, app_lds = GRIDS[name]
    # the launchers' choices, restated (launch_march_backward: 16 waves x 6 KB of staging + 64 B per line texel in 160 KB; launch_app_h_backward: 192 B per texel of
    # the longest line in 150 KB)
    assert (16 * 6144 + (sum(grid) + 3) * 64 <= 160 * 1024) == march_lds and ((max(grid) + 1) * 192 <= 150 * 1024) == app_lds
    arrs = MB.tiny_arrays()
    m = make_model(arrs, MB.hyper(MB.step_ratio_for(grid)))
    m.upsample_volume_grid(grid)
    up = dict(arrs)
    for i in range(3):
        for k in ("density_plane", "density_line", "app_plane", "app_line"):
            up[f"{k}.{i}"] = getattr(m, k)[i].detach().cpu().numpy()
    c = MB.grid_case(up, grid)
    assert float(c.sc.stepSize) == float(m.stepSize) and c.n_dropped <= MB.MAX_DROPPED * c.n_before
    return m, c, _march(m, c)


@pytest.mark.parametrize("name", list(GRIDS))
def test_march_on_either_side_of_the_lds_limit(name):
    """S = 130, eps_T = 1e-4 on grids whose three line images just fit / no longer fit the LDS beside the per-wave staging"""
    m, c, got = _on_grid(name)
    _check_march(name, c, got)


@pytest.mark.parametrize("name", list(GRIDS))
def test_app_h_on_either_side_of_the_lds_limit(name):
    """tvr_app_h_forward / _backward at the queue positions of the same marches against float64 h = bilinear(plane) * linear(line) and its autograd, seeded dh"""
    from jittor_myc_nerfs_amd.autograd_ops import _AppHFn
    m, c, got = _on_grid(name)
    xyz = got["xyz_dev"]
    M = xyz.shape[0]
    assert M > 4096
    params = list(m.app_plane) + list(m.app_line)
    h = _AppHFn.apply(m, xyz, *params)
    dh = torch.tensor(np.random.default_rng(5).standard_normal((M, 144)))
    grads = torch.autograd.grad((h * _dev(dh)).sum(), params)
    leaves = [torch.tensor(c.arrs[k], dtype=torch.float64).requires_grad_(True) for k in MB.APP_NAMES]
    h_ref = MB.app_h64(leaves[:3], leaves[3:], xyz.cpu().double())
    ref = torch.autograd.grad((h_ref * dh).sum(), leaves)
    err_h = float((h.detach().cpu().double() - h_ref.detach()).abs().max())
    worst = 0.0
    for k, g, gr in zip(MB.APP_NAMES, grads, ref):
        err = MB.rel_err(g, gr)
        worst = max(worst, err)
        print(f"MEASURED app_h {name} grad {k:12s} rel-max-err {err:.2e}  (max |g_ref| {float(gr.abs().max()):.2e})")
    print(f"MEASURED app_h {name} forward h {err_h:.2e} (max |h| {float(h_ref.abs().max()):.2e})  WORST-GRAD {worst:.2e}  (M {M}, grid {list(c.sc.gridSize)})")
    assert err_h < MB.BAR_FWD
    for k, g, gr in zip(MB.APP_NAMES, grads, ref):
        assert float(gr.abs().max()) > 0, f"{k}: the reference gradient is identically zero"
        assert MB.rel_err(g, gr) < MB.BAR_GRAD, f"{name} {k}: {MB.rel_err(g, gr):.2e}"


# ---- the whole step ------------------------------------------------------------------------------------------------------------------------------
def _step_case():
    return MB.KERNEL_CASES["S192-eps0.0001-nojitter"]()


def _cw(c):
    return torch.tensor(np.random.default_rng(12).standard_normal((c.n, 3)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _oracle_step(white_bg):
    """every leaf's gradient through oracle.tensorf_oracle.execute with the reference's keep mask standing for the early exit"""
    from oracle import tensorf_oracle as TO
    c = _step_case()
    sc = TO.scene_from_arrays(c.arrs, **c.hyper)
    leaves = {f"{name}.{i}": t for name in ("density_plane", "density_line", "app_plane", "app_line") for i, t in enumerate(getattr(sc, name))}
    leaves["basis_mat"] = sc.basis_mat
    leaves.update(sc.mlp)
    for t in leaves.values():
        t.requires_grad_(True)
    rgb, _ = TO.execute(sc, torch.tensor(c.rays), white_bg=white_bg, N_samples=c.S, sample_keep=c.keep_mask())
    (rgb * _cw(c)).sum().backward()
    return rgb.detach(), {k: t.grad.clone() for k, t in leaves.items()}


@functools.lru_cache(maxsize=None)
def _hip_step(white_bg, static):
    c = _step_case()
    m = make_model(c.arrs, c.hyper)
    assert m.eps_T is None and abs(float(m.rayMarch_weight_thres) - 1e-4) < 1e-10            # the default: early exit at the appearance threshold, as training runs
    m.static_training = static
    rgb, _ = m.render_rays_autograd(_dev(c.rays), white_bg=white_bg, N_samples=c.S)
    assert (getattr(m, "_train_buf", None) is not None) == static
    (rgb * _cw(c).cuda()).sum().backward()
    mlp = m.renderModule.mlp
    got = {"basis_mat": m.basis_mat.weight.grad, "W1": mlp[0].weight.grad, "b1": mlp[0].bias.grad, "W2": mlp[2].weight.grad, "b2": mlp[2].bias.grad,
           "W3": mlp[4].weight.grad, "b3": mlp[4].bias.grad}
    for i in range(3):
        got[f"density_plane.{i}"], got[f"density_line.{i}"] = m.density_plane[i].grad, m.density_line[i].grad
        got[f"app_plane.{i}"], got[f"app_line.{i}"] = m.app_plane[i].grad, m.app_line[i].grad
    return rgb.detach().cpu(), {k: v.detach().cpu() for k, v in got.items()}


@pytest.mark.parametrize("static", [True, False], ids=["fused", "eager"])
@pytest.mark.parametrize("white_bg", [True, False], ids=["white", "black"])
def test_whole_step_with_early_exit_matches_oracle_autograd(white_bg, static):
    """render_rays_autograd at the default eps_T (1e-4) on the long-ray case (S = 192: three chunks, rays ending after chunk 0, after chunk 1, never): every leaf
    against autograd through the oracle"""
    rgb_o, ref = _oracle_step(white_bg)
    rgb, got = _hip_step(white_bg, static)
    err_rgb = float((rgb - rgb_o).abs().max())
    worst = 0.0
    for k, r in ref.items():
        err = MB.rel_err(got[k], r)
        worst = max(worst, err)
        print(f"MEASURED step static={static} white_bg={white_bg} grad {k:18s} rel-max-err {err:.2e}  (max |g_ref| {float(r.abs().max()):.2e})")
    print(f"MEASURED step static={static} white_bg={white_bg} forward rgb {err_rgb:.2e}  WORST-GRAD {worst:.2e}")
    assert err_rgb < MB.BAR_FWD
    for k, r in ref.items():
        assert float(r.abs().max()) > 0, f"{k}: oracle gradient is identically zero"
        assert MB.rel_err(got[k], r) < MB.BAR_GRAD, f"{k}: {MB.rel_err(got[k], r):.2e}"


@pytest.mark.parametrize("white_bg", [True, False], ids=["white", "black"])
def test_fused_and_eager_step_agree_with_early_exit(white_bg):
    rgb_f, fused = _hip_step(white_bg, True)
    rgb_e, eager = _hip_step(white_bg, False)
    assert float((rgb_f - rgb_e).abs().max()) < MB.BAR_FWD
    for k, e in eager.items():
        err = MB.rel_err(fused[k], e)
        print(f"MEASURED fused-vs-eager white_bg={white_bg} grad {k:18s} rel-max-err {err:.2e}")
        assert err < MB.BAR_GRAD, f"{k}: {err:.2e}"
