"""CPU only: the float64 reference of REFTensoRF's appearance branch (tests/ref_shade_common.py) and the inputs tests/test_gpu_ref_kernels.py runs the kernels on.
  * the reference evaluated in float32 agrees with itself in float64 within the forward bar: the inputs are not ill-conditioned at the bar;
  * the conditions that keep the inputs from being vacuous (the tint gate closed / open, -dot of both signs, |n| away from its clamp, no gradient identically zero);
  * every mutation of the reference's gradient moves a compared tensor by more than the gradient bar: a kernel with that defect would fail;
  * the whole-step case leaves [0, 1] on both sides before the clamp, ends rays early and fills more than 4096 appearance rows."""
import pytest
import torch

import ref_shade_common as RS


def _all_inputs():
    return [RS.inputs(M) for M in RS.MS] + [RS.inputs(*RS.SPIKE)]


@pytest.mark.parametrize("M", RS.MS)
def test_reference_in_float32_agrees_with_itself_in_float64(M):
    I = RS.inputs(M)
    r64, r32 = I.run(), I.run(dtype=torch.float32)
    errs = {k: float((r32[k].double() - r64[k]).abs().max()) for k in ("rgb", "in0", "refl", "rgb_s", "tint_raw", "rgb_d")}
    # f and n are large on these h (|f| ~ 120): relative to max(1, max |ref|), as tests/test_gpu_ref.py::test_ref_feature_and_mlp_entry_points measures the heads
    for k in ("f", "n"):
        errs[k] = float((r32[k].double() - r64[k]).abs().max()) / max(1.0, float(r64[k].abs().max()))
    print(f"MEASURED reference fp32-vs-fp64 M={M} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < 0.5 * RS.BAR_FWD, (k, v)            # half the bar: the kernel's own rounding needs the other half
    for k in RS.GRAD_NAMES:
        if float(r64["grads"][k].abs().max()) > 0:
            assert RS.rel_err(r32["grads"][k], r64["grads"][k]) < 0.5 * RS.BAR_GRAD, k


def test_conditions_hold_at_every_batch_size():
    for I in _all_inputs():
        s = I.stats()
        print("MEASURED inputs", s)
        assert 0.25 <= s["tint_closed"] <= 0.75 and 0.25 <= s["in0_pos"] <= 0.75, s
        assert s["n_min"] >= 1e-3 * s["n_median"], s
        assert s["tint_margin"] > RS.TINT_MARGIN and s["skipped"] <= 0.01 * I.M + 2, s
        assert float((I.view.norm(dim=-1) - 1.0).abs().max()) < 1e-6 and float(I.a.min()) >= 0.0
        for with_in0 in (True, False):
            g = I.run(with_in0)["grads"]
            for k in RS.GRAD_NAMES:
                if k.startswith("rho"):
                    assert float(g[k].abs().max()) == 0.0          # k = 1 / rho is unused by MLPRender_Fea_Ref
                else:
                    assert float(g[k].abs().max()) > 0.0, k
    I = RS.inputs(*RS.SPIKE)
    cw = I.cw.abs().max(1).values
    assert float(cw[RS.SPIKE[1]]) > 100 * float(torch.cat((cw[:RS.SPIKE[1]], cw[RS.SPIKE[1] + 1:])).max())
    # the tint gate is closed on that row: its gradient reaches the heads' k-step (d rgb_d) and not the network, so the heads' scale and the network's differ by
    # the spike's factor and the accumulators' rescale between the two is not by one
    assert float(I.run()["tint_raw"][RS.SPIKE[1]]) < 0.0
    assert float(I.run()["grads"]["dh"].abs().max()) > 10 * float(RS.inputs(RS.SPIKE[0]).run()["grads"]["dh"].abs().max())


@pytest.mark.parametrize("mutation", RS.MUTATIONS)
def test_the_bar_sees_every_mutation(mutation):
    for M in RS.MS:
        I = RS.inputs(M)
        for with_in0 in (True, False):
            if mutation == "grad_in0_not_added" and not with_in0:
                continue                                            # nothing arrives through the -dot output in this form
            k, move = RS.worst_move(I.run(with_in0, mutation), I.run(with_in0))
            print(f"MEASURED mutation {mutation} M={M} with_in0={with_in0}: {k} moves by {move:.2e}")
            assert move > 10 * RS.BAR_GRAD, (mutation, M, with_in0, k, move)
            ref, mut = I.run(with_in0), I.run(with_in0, mutation)
            assert torch.equal(ref["rgb"], mut["rgb"]) and torch.equal(ref["in0"], mut["in0"])       # a defect of the gradient alone


@pytest.mark.parametrize("white_bg", [True, False], ids=["white", "black"])
def test_whole_step_inputs_leave_the_unit_interval_and_end_early(white_bg):
    """Pixel channels before the clamp, through oracle.tensorf_oracle.execute with the REFTensoRF arrays.  Over a black background 53.6 % of the channels are exactly
    0 whatever the diffuse bias is (the rays of the long-ray case without an appearance sample: no colour reaches them), so 40 % strictly inside, 5 % below and 5 %
    above cannot hold together there; inside is then counted among the channels of rays that carry colour.  Over white every figure is of all channels."""
    s = RS.step_stats(white_bg)
    pre = RS.step_forward(white_bg)["pre"]
    coloured = float((pre != (1.0 if white_bg else 0.0)).any(1).float().mean())
    print(f"MEASURED step inputs white_bg={white_bg} {s} rays-with-colour {coloured:.3f}")
    assert s["below"] >= 0.05 and s["above"] >= 0.05, s
    if white_bg:
        assert s["inside"] >= 0.40, s
    else:
        assert coloured < 0.5 and s["inside"] >= 0.40 * coloured, s
    assert s["ends_early"] >= 0.10 and s["M"] > 4096, s
    for which in ("free", "clamped"):
        cw = RS.step_cw(white_bg, which)
        assert float((cw != 0).float().mean()) >= (0.25 if which == "free" else 0.10)
    clamped = RS.step_cw(white_bg, "clamped") != 0
    assert bool(((pre[clamped] < 0) | (pre[clamped] > 1)).all())


def test_oracle_gives_clamped_channels_no_gradient():
    _, _, grads = RS.oracle_step(True, "clamped", False)
    assert all(float(g.abs().max()) == 0.0 for g in grads.values())
    _, pen, grads = RS.oracle_step(True, "free", True)
    assert pen > 0 and all(float(g.abs().max()) > 0.0 for g in grads.values())
