"""GPU (-m gpu): REFTensoRF's training kernels against float64, stage by stage — the REF instantiation of mlp_train_backward_kernel (the extra -dot row),
ref_heads_backward_kernel (normalisation, reflection, the tint gate, the penalty gradient arriving through -dot), heads_scale_kernel / basis_backward_kernel<3> (the
heads' k-step at its own power-of-two scale) and the penalty / clamp branches of the compositing kernels.

Reference: tests/ref_shade_common.py (float64, from the formulas; vetted on the CPU by tests/test_ref_shade_host.py, which also shows that each of nine plausible
defects of the backward would miss the bar by a wide margin on exactly these inputs).  Bars: 2e-5 on forward values, 2e-4 of a tensor's largest gradient entry
(tests/test_gpu_training.py::test_fused_mlp_training_kernels_match_float64_autograd); the whole step's 2e-4 / 5e-4 (tests/march_backward_common.py).

Which path a test drives is in its id:
  * M37: below one 128-row group, a ragged 32-tile, the weight gradients as torch products; M4099: just past the switch to tvr_gemm_tn (dg8^T h with Ka = lda = 8
    included); M10007: many groups, ragged for 32, 128 and 256;
  * in0 / noin0: with and without the penalty-like term on the -dot output (grad_in0 given / NULL);
  * fused / eager, white / black: the whole step (tvr_train_forward / _backward, or the chain of autograd Functions) on the long-ray case (S = 192: three chunks,
    early exit on) with pixels that leave [0, 1] on both sides before the clamp."""
import functools

import pytest
import torch

import march_backward_common as MB
import ref_shade_common as RS
from conftest import make_model

pytestmark = pytest.mark.gpu


def _dev(x, dtype=torch.float32):
    return torch.as_tensor(x).to("cuda", dtype).contiguous()


def _hyper():
    return MB.hyper(step_ratio=0.5)


def _params(m):
    mlp = m.renderModule.mlp
    return [m.basis_mat.weight, m.normal_linear.weight, m.normal_linear.bias, m.diffuse_linear.weight, m.diffuse_linear.bias, m.specular_linear.weight,
            m.specular_linear.bias, m.rho_linear.weight, m.rho_linear.bias, mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias, mlp[4].weight, mlp[4].bias]


@functools.lru_cache(maxsize=None)
def _run(M, with_in0, target=64.0, spike_row=None):
    """_RefMlpTrainFn forward + backward on the vetted batch -> dict(rgb, in0, grads {RS.GRAD_NAMES}, sat), on the CPU"""
    from jittor_myc_nerfs_amd.autograd_ops import _RefMlpTrainFn
    I = RS.inputs(M, spike_row)
    m = make_model(I.arrs, _hyper())
    m.grad_scale_target = float(target)
    m._ensure_scene(force=True)
    h = _dev(I.h).requires_grad_(True)
    params = _params(m)
    rgb, in0 = _RefMlpTrainFn.apply(m, h, _dev(I.view), *params)
    loss = (rgb * _dev(I.cw)).sum()
    if with_in0:
        loss = loss + (_dev(I.a) * torch.relu(in0) ** 2).sum()
    grads = torch.autograd.grad(loss, [h] + params)
    torch.cuda.synchronize()
    return dict(rgb=rgb.detach().cpu(), in0=in0.detach().cpu(), grads={k: g.detach().cpu() for k, g in zip(RS.GRAD_NAMES, grads)}, sat=int(m._get_sat_flag().item()))


def _check_grads(tag, got, ref):
    worst = 0.0
    for k in RS.GRAD_NAMES:
        g, r = got[k], ref[k]
        assert tuple(g.shape) == tuple(r.shape), k
        if k.startswith("rho"):
            continue
        err = RS.rel_err(g, r)
        worst = max(worst, err)
        print(f"MEASURED {tag} grad {k:10s} rel-max-err {err:.2e}  (max |g_ref| {float(r.abs().max()):.2e})")
    print(f"MEASURED {tag} WORST-GRAD {worst:.2e}")
    for k in RS.GRAD_NAMES:
        if k.startswith("rho"):
            assert float(got[k].abs().max()) == 0.0, f"{k}: k = 1 / rho is unused by MLPRender_Fea_Ref, its gradient is exactly zero"
        else:
            assert RS.rel_err(got[k], ref[k]) < RS.BAR_GRAD, f"{tag} {k}: max |grad diff| / max |grad| = {RS.rel_err(got[k], ref[k]):.2e}"


@pytest.mark.parametrize("with_in0", [True, False], ids=["in0", "noin0"])
@pytest.mark.parametrize("M", RS.MS, ids=[f"M{M}" for M in RS.MS])
def test_ref_mlp_train_fn_matches_float64_reference(M, with_in0):
    """(a) rgb, in0 = -dot, dh and the seventeen parameter gradients of _RefMlpTrainFn against the float64 reference"""
    got, ref = _run(M, with_in0), RS.inputs(M).run(with_in0)
    tag = f"ref-mlp M={M} in0={with_in0}"
    e_rgb, e_in0 = float((got["rgb"].double() - ref["rgb"]).abs().max()), float((got["in0"].double() - ref["in0"]).abs().max())
    print(f"MEASURED {tag} forward rgb {e_rgb:.2e} in0 {e_in0:.2e}")
    assert got["rgb"].shape == (M, 3) and got["in0"].shape == (M,)
    _check_grads(tag, got["grads"], ref["grads"])
    assert e_rgb < RS.BAR_FWD and e_in0 < RS.BAR_FWD
    assert got["sat"] == 0


@pytest.mark.parametrize("M", RS.MS, ids=[f"M{M}" for M in RS.MS])
def test_training_forward_is_the_inference_kernel_and_saves_what_the_backward_reads(M):
    """(b) tvr_mlp_train_forward_ref called directly: feats32[:, 27:31] (reflection, -dot), g8 (the raw heads) and rgb_s against the reference; rgb of (a) against the
    inference entry point (tvr_mlp_render_ref through renderModule) on the saved features, reflection and -dot, mixed with the saved heads"""
    from jittor_myc_nerfs_amd import _lib as L
    from jittor_myc_nerfs_amd.autograd_ops import _stream_ptr
    I = RS.inputs(M)
    ref = I.run()
    m = make_model(I.arrs, _hyper())
    sc = m._ensure_scene(force=True)
    h, vd = _dev(I.h), _dev(I.view)
    new = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    rgb, rgb_s, feats, g8, h1, h2 = new(M, 3), new(M, 3), new(M, 32), new(M, 8), new(M, 128), new(M, 128)
    L.check(L.lib().tvr_mlp_train_forward_ref(sc, h.data_ptr(), vd.data_ptr(), M, rgb.data_ptr(), L.nbytes(rgb), feats.data_ptr(), L.nbytes(feats), h1.data_ptr(),
                                              L.nbytes(h1), h2.data_ptr(), L.nbytes(h2), g8.data_ptr(), L.nbytes(g8), rgb_s.data_ptr(), L.nbytes(rgb_s),
                                              _stream_ptr(h.device)), "tvr_mlp_train_forward_ref")
    torch.cuda.synchronize()
    assert torch.equal(rgb.cpu(), _run(M, True)["rgb"])                                      # the autograd function's forward is this call
    want_g8 = torch.cat([ref["n"], ref["tint_raw"], ref["rgb_d"], ref["rho_raw"]], dim=1)    # {normal 3 (not normalised), tint, rgb_d 3, rho}
    errs = {"refl": float((feats[:, 27:30].cpu().double() - ref["refl"]).abs().max()), "in0": float((feats[:, 30].cpu().double() - ref["in0"]).abs().max()),
            "rgb_s": float((rgb_s.cpu().double() - ref["rgb_s"]).abs().max()),
            # the heads are large on these h (|n| ~ 130): relative to max(1, max |ref|), as tests/test_gpu_ref.py::test_ref_feature_and_mlp_entry_points measures them
            "g8": float((g8.cpu().double() - want_g8).abs().max()) / max(1.0, float(want_g8.abs().max())),
            "f": float((feats[:, :27].cpu().double() - ref["f"]).abs().max()) / max(1.0, float(ref["f"].abs().max()))}
    assert float(feats[:, 31].abs().max()) == 0.0
    with torch.no_grad():
        net = m.renderModule(None, feats[:, 27:30].contiguous(), feats[:, :27].contiguous(), feats[:, 30].contiguous(), None)
        mixed = torch.relu(g8[:, 3:4]) * net + g8[:, 4:7]
    errs["inference-rgb_s"] = float((net - rgb_s).abs().max())
    errs["inference-rgb"] = float((mixed - rgb).abs().max())
    print(f"MEASURED ref-forward M={M} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < RS.BAR_FWD, (k, v)


def test_backward_does_not_depend_on_the_gradient_scale():
    """(c) grad_scale_target 64 and 4: the same gradients within the bar, no saturation"""
    M = RS.MS[-1]
    a, b = _run(M, True), _run(M, True, 4.0)
    assert a["sat"] == 0 and b["sat"] == 0
    _check_grads(f"ref-mlp M={M} target 4 vs 64", b["grads"], a["grads"])
    _check_grads(f"ref-mlp M={M} target 4", b["grads"], RS.inputs(M).run(True)["grads"])


def test_one_large_colour_gradient_sets_the_heads_scale():
    """(c) one row's colour gradient 1e3 times the others': the heads' k-step takes its scale from that row (d rgb_d IS the colour gradient), the network's chain
    from tint * gradient; dh and every parameter gradient still meet the bar"""
    got, ref = _run(RS.SPIKE[0], True, 64.0, RS.SPIKE[1]), RS.inputs(*RS.SPIKE).run(True)
    assert got["sat"] == 0
    _check_grads(f"ref-mlp M={RS.SPIKE[0]} spike row {RS.SPIKE[1]}", got["grads"], ref["grads"])
    rest = torch.ones(RS.SPIKE[0], dtype=torch.bool)
    rest[RS.SPIKE[1]] = False
    print(f"MEASURED ref-mlp spike: dh of the other rows, rel-max-err against their own largest entry {RS.rel_err(got['grads']['dh'][rest], ref['grads']['dh'][rest]):.2e}")


# ---- (d) the whole step past one chunk, with early exit and the clamp ----------------------------------------------------------------------------
def _leaf_grads(m):
    mlp = m.renderModule.mlp
    got = {"basis_mat": m.basis_mat.weight.grad, "W1": mlp[0].weight.grad, "b1": mlp[0].bias.grad, "W2": mlp[2].weight.grad, "b2": mlp[2].bias.grad,
           "W3": mlp[4].weight.grad, "b3": mlp[4].bias.grad, "normal_W": m.normal_linear.weight.grad, "normal_b": m.normal_linear.bias.grad,
           "diffuse_W": m.diffuse_linear.weight.grad, "diffuse_b": m.diffuse_linear.bias.grad, "specular_W": m.specular_linear.weight.grad,
           "specular_b": m.specular_linear.bias.grad}
    for i in range(3):
        got[f"density_plane.{i}"], got[f"density_line.{i}"] = m.density_plane[i].grad, m.density_line[i].grad
        got[f"app_plane.{i}"], got[f"app_line.{i}"] = m.app_plane[i].grad, m.app_line[i].grad
    return got


@functools.lru_cache(maxsize=None)
def _hip_step(white_bg, static, which="free", penalty=True):
    c = RS.step_case()
    m = make_model(RS.step_arrays(), c.hyper)
    assert type(m).__name__ == "REFTensoRF" and m.eps_T is None and abs(float(m.rayMarch_weight_thres) - 1e-4) < 1e-10
    m.static_training = static
    rgb, _ = m.render_rays_autograd(_dev(c.rays), white_bg=white_bg, N_samples=c.S)
    assert (getattr(m, "_train_buf", None) is not None) == static
    loss = (rgb * RS.step_cw(white_bg, which).cuda()).sum()
    if penalty:
        loss = loss + 0.5 * m.penalty
    loss.backward()
    torch.cuda.synchronize()
    got = _leaf_grads(m)
    assert all(g is not None for g in got.values())
    return rgb.detach().cpu(), float(m.penalty.detach()), {k: v.detach().cpu() for k, v in got.items()}, int(m._get_sat_flag().item())


@pytest.mark.parametrize("static", [True, False], ids=["fused", "eager"])
@pytest.mark.parametrize("white_bg", [True, False], ids=["white", "black"])
def test_ref_whole_step_with_early_exit_and_clamp_matches_oracle_autograd(white_bg, static):
    """sum(rgb_map * cw) + 0.5 * penalty at the default eps_T on the long-ray case: every leaf against autograd through the oracle"""
    rgb_o, pen_o, ref = RS.oracle_step(white_bg)
    rgb, pen, got, sat = _hip_step(white_bg, static)
    tag = f"ref-step static={static} white_bg={white_bg}"
    err_rgb = float((rgb - rgb_o).abs().max())
    worst = 0.0
    for k, r in ref.items():
        err = MB.rel_err(got[k], r)
        worst = max(worst, err)
        print(f"MEASURED {tag} grad {k:18s} rel-max-err {err:.2e}  (max |g_ref| {float(r.abs().max()):.2e})")
    print(f"MEASURED {tag} forward rgb {err_rgb:.2e} penalty {pen:.6e} (oracle {pen_o:.6e})  WORST-GRAD {worst:.2e}")
    assert err_rgb < MB.BAR_FWD and sat == 0
    assert abs(pen - pen_o) < MB.BAR_FWD * max(1.0, abs(pen_o))
    # a channel the oracle clamps by more than the margin comes out at the clamp's edge, exactly
    pre = RS.step_forward(white_bg)["pre"]
    assert bool((rgb[pre < -RS.CLAMP_MARGIN] == 0.0).all()) and bool((rgb[pre > 1.0 + RS.CLAMP_MARGIN] == 1.0).all())
    for k, r in ref.items():
        assert float(r.abs().max()) > 0, f"{k}: oracle gradient is identically zero"
        assert MB.rel_err(got[k], r) < MB.BAR_GRAD, f"{tag} {k}: {MB.rel_err(got[k], r):.2e}"


@pytest.mark.parametrize("white_bg", [True, False], ids=["white", "black"])
def test_ref_fused_and_eager_step_agree(white_bg):
    rgb_f, pen_f, fused, _ = _hip_step(white_bg, True)
    rgb_e, pen_e, eager, _ = _hip_step(white_bg, False)
    assert float((rgb_f - rgb_e).abs().max()) < MB.BAR_FWD and abs(pen_f - pen_e) < MB.BAR_FWD * max(1.0, abs(pen_e))
    for k, e in eager.items():
        err = MB.rel_err(fused[k], e)
        print(f"MEASURED ref fused-vs-eager white_bg={white_bg} grad {k:18s} rel-max-err {err:.2e}")
        assert err < MB.BAR_GRAD, f"{k}: {err:.2e}"


@pytest.mark.parametrize("static", [True, False], ids=["fused", "eager"])
@pytest.mark.parametrize("white_bg", [True, False], ids=["white", "black"])
def test_clamped_pixel_channels_pass_no_gradient(white_bg, static):
    """a cw that is non-zero only on channels the oracle clamps (by more than the margin a forward within the bar may be off by): every leaf gradient is zero"""
    assert float((RS.step_cw(white_bg, "clamped") != 0).float().mean()) >= 0.10
    _, _, got, _ = _hip_step(white_bg, static, "clamped", False)
    for k, g in got.items():
        assert float(g.abs().max()) == 0.0, f"{k}: a clamped channel passed a gradient of {float(g.abs().max()):.2e}"
