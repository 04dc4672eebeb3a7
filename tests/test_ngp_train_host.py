"""Host-side checks of Instant-NGP training (no GPU): the references of tests/ngp_train_common.py against the project's CPU oracle and against finite
differences, and the plain-torch pieces of jittor_myc_nerfs_amd.ngp_train (Huber, ExpDecay, EMA, the ray-count update, the data's rays, the checkpoint).
Also the compositor tests' inputs with a step size per row: that they meet the conditions the GPU tests lean on, that the constant-dt inputs cannot see a
kernel reading the wrong row's dt, and that on the new inputs each of six restated defects exceeds a GPU bar at least tenfold."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ngp_frame_common as F  # noqa: E402
import ngp_train_common as K  # noqa: E402
from conftest import NGP_AABB_SCALE, ngp_camera_rays  # noqa: E402


def _edge_positions(n, seed):
    """random positions in [0,1]^3 plus rows at exactly 0.0 and 1.0 in each coordinate (a corner index reaches `res`: the dense wrap)."""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3), dtype=np.float32)
    edge = np.array([[0, 0, 0], [1, 1, 1], [0, 0.3, 0.7], [1, 0.3, 0.7], [0.3, 0, 0.7], [0.3, 1, 0.7], [0.3, 0.7, 0], [0.3, 0.7, 1]], np.float32)
    return np.concatenate([p, edge])


@pytest.mark.parametrize("aabb_scale", [1, 4])
def test_hash_restatement_matches_the_oracle(aabb_scale):
    from oracle import ngp_oracle as N
    levels = N.grid_levels(aabb_scale)
    pos = _edge_positions(300, 3)
    grid = np.random.default_rng(4).uniform(-1, 1, levels["n_params"]).astype(np.float32)
    enc, cells = N.hash_encode_c(levels, grid, pos, want_cells=True)
    ent, frac, c = K.hash_geometry(levels, torch.as_tensor(pos))
    assert np.array_equal(c.numpy().astype(np.uint32), cells)                              # the oracle's own cells
    assert float(frac.min()) >= 0 and float(frac.max()) < 1
    assert int(ent.min()) >= 0 and int(ent.max()) < int(levels["offsets"][-1])
    mine = K.hash_encode_t(torch.as_tensor(grid).double(), ent, frac).numpy()
    assert np.abs(mine - enc).max() < 2e-6                                                  # composite_f64's bar for the encoding
    mine32 = K.hash_encode_t(torch.as_tensor(grid), ent, frac).numpy()
    assert np.abs(mine32 - enc).max() < 2e-6


def test_network_and_compositor_restatement_match_the_oracle(ngp_scene):
    from oracle import ngp_oracle as N
    levels, arrs = ngp_scene
    o, d = ngp_camera_rays(12, 12)
    coords, _, ns, _, _ = N.sample(o, d, arrs["density_grid_bitfield"], NGP_AABB_SCALE, N.Pcg32(1337).state)
    n_rows = coords.shape[0]
    ref_out, _ = F.network_f64(levels, arrs, coords)
    c = torch.as_tensor(coords)
    ent, frac, _ = K.hash_geometry(levels, c[:, :3])
    p = K.params_t(arrs, torch.float64, requires_grad=False)
    out = K.network_t(p, ent, frac, K.sh_t(c[:, 4:7].double()))
    assert np.abs(out.numpy() - ref_out).max() < 2e-4 * max(1.0, np.abs(ref_out).max())     # the network bar; fp64 both sides, the SH and blend orders differ
    assert np.abs(K.sh_t(c[:, 4:7]).numpy() - N.sh_encode_c(coords[:, 4:7])).max() < 2e-6
    # compositor: capacity does not bind, one background -> composite_f64, for the vectorised form and the loop
    bg = np.tile(np.asarray(F.BG, np.float32), (ns.shape[0], 1))                            # the kernels' background is fp32: the same values either side
    ref_out = ref_out.astype(np.float32)                                                    # network outputs are fp32 rows; composite_f64 reads them so
    rgb64, brk, margin, _ = F.composite_f64(ref_out, coords, ns, bg[0].astype(np.float64))
    rgb_t, stop = K.composite_t(torch.as_tensor(ref_out).double(), K.unwarp_dt_t(c[:, 3]), torch.as_tensor(ns), n_rows, torch.as_tensor(bg))
    loop = K.composite_loop(ref_out, coords, ns, n_rows, bg, np.float64)
    n = ns[:, 0].astype(np.int64)
    want_stop = np.where(brk >= 0, brk, n)
    assert np.array_equal(stop.numpy(), want_stop) and np.array_equal(loop["stop"], want_stop)
    assert np.abs(rgb_t.numpy() - rgb64).max() < 1e-10 and np.abs(loop["rgb"] - rgb64).max() < 1e-10
    assert (brk >= 0).any() and (n == 0).any()
    # a capacity that cuts: the loop and the vectorised form agree, rays behind the cut get 0, the ray it cuts gets no background
    cap = int(n_rows * 0.6)
    bgr = np.random.default_rng(1).random((ns.shape[0], 3), dtype=np.float32)
    rgb_c, stop_c = K.composite_t(torch.as_tensor(ref_out[:cap]).double(), K.unwarp_dt_t(c[:cap, 3]), torch.as_tensor(ns), cap, torch.as_tensor(bgr))
    loop_c = K.composite_loop(ref_out[:cap], coords[:cap], ns, cap, bgr, np.float64)
    assert np.array_equal(stop_c.numpy(), loop_c["stop"]) and np.abs(rgb_c.numpy() - loop_c["rgb"]).max() < 1e-10
    behind = (ns[:, 1] >= cap) & (n > 0)
    assert behind.any() and np.all(loop_c["rgb"][behind] == 0)
    empty = n == 0
    assert np.array_equal(loop_c["rgb"][empty], bgr[empty].astype(np.float64))


def _small_case(seed=0, R=6):
    """<= 8 rays with hand-made rows: step counts 0..7, one ray that breaks (large densities), random everything else."""
    rng = np.random.default_rng(seed)
    n = np.array([0, 1, 3, 7, 5, 4][:R])
    base = np.concatenate([[0], np.cumsum(n)[:-1]])
    ns = np.stack([n, base], 1).astype(np.int32)
    rows = int(n.sum())
    out = rng.normal(0, 1, (rows, 4))
    out[:, 3] += 5.0                                           # sigma ~ e^5, dt ~ 1e-3: optical depth ~0.15 per step
    out[base[3]:base[3] + 7, 3] = 9.5                          # ray 3: optical depth ~ 11 per step -> breaks at sample 1
    coords = np.zeros((rows, 7), np.float32)
    coords[:, 3] = rng.random(rows).astype(np.float32) * 0.05
    bg = rng.random((R, 3)).astype(np.float32)
    return out.astype(np.float32), coords, ns, bg


def test_compositor_gradient_against_autograd_and_finite_differences():
    out, coords, ns, bg = _small_case()
    rows = out.shape[0]
    g = np.random.default_rng(5).normal(0, 1, (ns.shape[0], 3)).astype(np.float32)
    for n_rows in (rows, rows - 2, int(ns[4, 1])):             # no cut, a cut inside the last ray, a cut exactly at a ray's end
        loop = K.composite_loop(out[:n_rows], coords[:n_rows], ns, n_rows, bg, np.float64, grad_rgb=g)
        assert loop["stop"][3] == 1 and loop["stop"][0] == 0
        x = torch.as_tensor(out[:n_rows]).double().requires_grad_(True)
        dt = K.unwarp_dt_t(torch.as_tensor(coords[:n_rows, 3]))
        stop = torch.as_tensor(loop["stop"])
        rgb, _ = K.composite_t(x, dt, torch.as_tensor(ns), n_rows, torch.as_tensor(bg), stop)
        assert np.abs(rgb.detach().numpy() - loop["rgb"]).max() < 1e-12
        rgb.backward(torch.as_tensor(g).double())
        assert np.abs(x.grad.numpy() - loop["grad"]).max() < 1e-10        # the analytic gradient of the header = autograd of the vectorised form
        dead = loop["ray"] < 0
        assert dead.any() and np.all(loop["grad"][dead] == 0)
        assert torch.autograd.gradcheck(lambda t: K.composite_t(t, dt, torch.as_tensor(ns), n_rows, torch.as_tensor(bg), stop)[0], (x.detach().requires_grad_(True),),
                                        eps=1e-6, atol=1e-7, rtol=1e-5)


def test_hash_encode_gradient_against_finite_differences():
    from oracle import ngp_oracle as N
    levels = N.grid_levels(1)
    pos = np.array([[0.1, 0.5, 0.9], [0.0, 1.0, 0.33], [0.77, 0.21, 0.5]], np.float32)
    ent, frac, _ = K.hash_geometry(levels, torch.as_tensor(pos))
    g = np.random.default_rng(2).normal(0, 1, (3, 32))
    ref, _, count = K.hash_backward_ref(levels, pos, g)
    grid = torch.zeros(levels["n_params"], dtype=torch.float64)
    touched = np.unique(ent.numpy())
    assert touched.size == int((count > 0).sum()) and int(count.sum()) == 3 * 16 * 8
    gt = torch.as_tensor(g)
    for e in touched[:: max(1, touched.size // 40)]:                      # the map is linear in the grid: one central difference per probed entry is exact
        for f in range(2):
            grid.zero_()
            grid[2 * e + f] = 1e-3
            up = float((K.hash_encode_t(grid, ent, frac) * gt).sum())
            grid[2 * e + f] = -1e-3
            dn = float((K.hash_encode_t(grid, ent, frac) * gt).sum())
            assert abs((up - dn) / 2e-3 - ref[e, f]) < 1e-9
    grid = torch.zeros(levels["n_params"], dtype=torch.float64, requires_grad=True)
    (K.hash_encode_t(grid, ent, frac) * gt).sum().backward()
    assert np.abs(grid.grad.view(-1, 2).numpy() - ref).max() < 1e-12


def test_designed_inputs_keep_break_decisions_off_the_threshold():
    from oracle import ngp_oracle as N
    _, _, coords, ns = F.designed_rows()
    total = int(ns[:, 0].sum())
    assert coords.shape[0] == total and ns.shape[0] == F.PERIOD
    for k in (1, 2, 33, 97, F.NO_BREAK):
        levels, arrs = F.designed_scene(k)
        sub = np.concatenate([np.arange(0, total, 997), [total - 1]])
        out = N.network_c(levels, arrs, coords[sub])
        assert np.ptp(out[:, 3]) < 1e-4                                   # one density everywhere: every row stands for all
        full = np.tile(out[:1], (total, 1))
        _, brk, margin, _ = F.composite_f64(full, coords, ns, F.BG)
        assert margin[np.isfinite(margin)].min() >= min(F.MARGIN, 0.495 * F.designed_tau(k))      # tau / 2 either side of the break by design
        loop = K.composite_loop(full, coords, ns, total, np.tile(np.float32(F.BG), (ns.shape[0], 1)), np.float64)
        assert np.array_equal(loop["stop"], np.where(brk >= 0, brk, ns[:, 0]))


# --------------------------------------------------------------------------------------------------------------- per-row step sizes
def _decisions(ref, r32, keep):
    """(T fp64, T fp32 as fp64) in front of every `T < 1e-4` test the loop makes on a compared ray: samples 0 .. stop (the breaking test included)."""
    j = np.arange(ref["T_seen"].shape[1])[None, :]
    dec = (j <= ref["stop"][:, None]) & (j < ref["nc"][:, None]) & keep[:, None]
    return ref["T_seen"][dec], r32["T_seen"][dec].astype(np.float64)


def _dt_spread(coords, ns, n_rows):
    """(distinct values of column 3, share of the rays with more than one step whose max dt / min dt exceeds 1.2) over the rows the capacity keeps."""
    idx, valid, _, nc = K.ray_rows(torch.as_tensor(np.asarray(ns, np.int64)), n_rows)
    idx, valid, nc = idx.numpy(), valid.numpy(), nc.numpy()
    dt = np.asarray(K.unwarp_dt_t(torch.as_tensor(np.ascontiguousarray(coords[:n_rows, 3]))).numpy(), np.float64)[idx]
    many = nc > 1
    ratio = np.where(valid, dt, -np.inf).max(1)[many] / np.where(valid, dt, np.inf).min(1)[many]
    return np.unique(coords[:n_rows, 3]).size, float((ratio > 1.2).mean())


def test_per_row_dt_inputs_meet_their_conditions():
    """The two inputs that give every row its own dt (ngp_train_common: "compositor cases") meet what the GPU tests lean on.  Measured (fp64 and fp32 loops on
    the CPU), random-dt ladder, seed 300: 29 508 distinct dt, every multi-step ray with max / min dt > 1.2; left out 0, 0, 0, 1, 0 of 421 rays for k = 1, 2, 33,
    97, 1000; breaks at 9 distinct samples (8..16) for k = 33 and at 12 (27..38) for k = 97; the fp32 loop's T differs from the fp64 loop's by 9.9e-7 / 1.4e-6 /
    1.5e-6 (k = 33 / 97 / 1000) at the decisions, 1/1000 of the margin 1e-3 or less.  For k = 1 and 2 ONE step takes T from 1 to about the threshold, so 1 - alpha
    cancels: its fp32 rounding (3e-8) is 3e-4 of the threshold (measured 7.3e-5 and 3.0e-4) and `1e-3 >= 20 x` cannot hold there at any seed; what holds, and what
    keeps a decision from flipping, is asserted for every scene: each decision lies at least 20 x farther from the threshold than the two loops lie apart at
    that decision (measured: 431 x at the least, k = 2).  Cone rows of the shared scene: 35 923 rows, 35 727 distinct dt (warped 0.069..0.205), 5 of 1024 rays
    left out, 302 rays break; the 40 x 40 CONE_POSE frame: 55 985 rows, 10 rays left out."""
    thr = K.THR
    for k in K.SCENES:
        for cap_kind in K.CAP_KINDS:
            out, coords, ns, bg, g, n_rows, ref, r32, keep = K.designed_case(k, cap_kind, "random")
            total = K.designed_inputs(k, "random")[5]["total"]
            distinct, spread = _dt_spread(coords, ns, min(n_rows, total))
            assert distinct > 100 and spread >= 0.5
            assert (~keep).mean() <= K.LEFT_OUT_SHARE
            assert np.array_equal(ref["stop"][keep], r32["stop"][keep])
            t64, t32 = _decisions(ref, r32, keep)
            # the two loops' distance at a decision: |d ln T| where T >= 1e-4, in units of the threshold below it (an fp32 T of exactly 0 has no logarithm)
            err = np.abs(t32 - t64) / np.maximum(t64, thr)
            margin = np.abs(np.log(np.maximum(t64, 1e-300) / thr))
            headroom = float((margin / np.maximum(err, 1e-300)).min())
            broke = ref["stop"] < ref["nc"]
            at = np.unique(ref["stop"][broke])
            print(f"random-dt ladder k={k} {cap_kind}: {distinct} distinct dt, spread share {spread:.2f}, {(~keep).sum()} of {keep.size} rays left out, breaks at "
                  f"{at.size} samples ({at.min(initial=1 << 30)}..{at.max(initial=-1)}), max |ln T_fp32 - ln T_fp64| at the decisions {err.max():.2e}, "
                  f"smallest margin / error {headroom:.0f}")
            assert margin.min() >= K.RANDOM_DT_MARGIN and headroom >= 20
            if k >= 33:                                              # no single step cancels 1 - alpha (docstring): the margin is 20 x the loops' distance outright
                assert K.RANDOM_DT_MARGIN >= 20 * err.max()
            if k in (33, 97):
                assert at.size >= 3
    for const_dt, what in ((False, "cone rows, shared scene"),):
        coords, ns, out, bg, g, keep = K.scene_inputs(const_dt)
        total = coords.shape[0]
        for n_rows in K.scene_capacities(total, const_dt).values():
            distinct, spread = _dt_spread(coords, ns, n_rows)
            ref = K.composite_loop(out[:n_rows], coords[:n_rows], ns, n_rows, bg, np.float64)
            r32 = K.composite_loop(out[:n_rows], coords[:n_rows], ns, n_rows, bg, np.float32)
            t64, t32 = _decisions(ref, r32, keep)
            err = np.abs(t32 - t64) / np.maximum(t64, thr)
            print(f"{what} n_rows={n_rows}: {distinct} distinct dt (warped {coords[:, 3].min():.3f}..{coords[:, 3].max():.3f}), spread share {spread:.2f}, "
                  f"{(~keep).sum()} of {keep.size} rays left out, {(ref['stop'] < ref['nc']).sum()} break, raw density max {out[:, 3].max():.1f}, "
                  f"max |ln T_fp32 - ln T_fp64| at the decisions {err.max():.2e} (network shift {F.network_shift(out):.2e})")
            assert distinct > 100 and spread >= 0.5
            assert (~keep).mean() <= K.LEFT_OUT_SHARE
            assert np.array_equal(ref["stop"][keep], r32["stop"][keep])
            assert F.network_shift(out) >= 20 * err.max()
        assert coords[:, 3].max() > 2 * coords[:, 3].min() > 0
    # the cone-stepping frame of test_gpu_ngp_frame.py, for the record: the same rule leaves out as few
    from oracle import ngp_oracle as N
    levels, arrs = K.scene_rows(False)[:2]
    o, d = ngp_camera_rays(F.CONE_WH, F.CONE_WH, pose_index=F.CONE_POSE)
    coords, ns = F.oracle_rows(o, d, arrs["density_grid_bitfield"], NGP_AABB_SCALE, const_dt=False)
    out = N.network_c(levels, arrs, coords)
    _, brk, margin, _ = F.composite_f64(out, coords, ns, F.BG)
    left = margin < F.network_shift(out)
    print(f"cone frame {F.CONE_WH} x {F.CONE_WH}: {coords.shape[0]} rows, {(brk >= 0).sum()} break, {left.sum()} of {left.size} rays left out")
    assert left.mean() <= K.LEFT_OUT_SHARE


def test_constant_dt_inputs_cannot_see_dt_defects():
    """Why the per-row-dt inputs exist: on the constant-dt ladder and the constant-dt shared scene every row holds one dt, so a loop that takes dt from the
    ray's first row, from the next row, or whose gradient uses a stale dt gives the unmutated loop's bytes.  The suite was blind to all three."""
    cases = [f"ladder-const-k{k}-total" for k in K.SCENES] + ["ladder-const-k33-inside", "ladder-const-k97-slack", "shared-total", "shared-cut"]
    for name in cases:
        out, coords, ns, bg, g, n_rows, _ = K.compositor_case(name)
        assert np.unique(coords[:min(n_rows, int(ns[:, 0].sum())), 3]).size == 1
        ref = K.composite_loop(out, coords, ns, n_rows, bg, np.float64, grad_rgb=g)
        for mutation in ("dt_first_row", "dt_next_row", "dt_backward_stale"):
            m = K.composite_loop(out, coords, ns, n_rows, bg, np.float64, grad_rgb=g, mutation=mutation)
            assert all(m[key].tobytes() == ref[key].tobytes() for key in ("rgb", "stop", "grad", "T_end")), (name, mutation)


@functools.lru_cache(maxsize=None)
def _power_reference(name):
    case = K.compositor_case(name)
    out, coords, ns, bg, g, n_rows, _ = case
    return case, K.composite_loop(out, coords, ns, n_rows, bg, np.float64, grad_rgb=g), K.composite_loop(out, coords, ns, n_rows, bg, np.float32, grad_rgb=g)


@pytest.mark.parametrize("name,mutation", K.COMPOSITOR_POWER)
def test_compositor_bars_have_power(name, mutation):
    """Each defect, restated in the fp64 loop, against the true fp64 loop by the GPU tests' own measures: the forward L-inf on the compared rays (bar 2e-5), the
    scaled backward error on their composited rows (bar max(4 e32, 1e-6), e32 from the unmutated fp32 loop on the same case) and the rows that must be exactly
    0 (bar: none; ten such rows count as 10 x).  One of them is exceeded at least tenfold.  Measured, error / bar:
      dt_first_row               cone-total forward 5.1e3, backward 1.9e4; ladder-random-k33-total 4.3e3, 7.0e4
      dt_next_row                cone-total forward 1.6e3, backward 1.3e4; ladder-random-k33-total 1.2e3, 1.2e5
      dt_backward_stale          forward 0 everywhere (the forward is untouched); backward 5.3e4 (cone-total), 1.8e5 (ladder-random-k33-total)
      suffix_without_background  backward 2.5e5 (cone-total), 6.2e4 (ladder-random-k1000-total)
      background_when_cut        forward 5.0e4 (cone-cut, ladder-random-k97-inside)
      stop_one_late              215 (cone-total) and 380 (ladder-random-k33-total) rows behind a break written; backward 14 and 67; forward 2.6 and 1.9 only."""
    case, ref, r32 = _power_reference(name)
    out, coords, ns, bg, g, n_rows, keep = case
    assert (~keep).mean() <= K.LEFT_OUT_SHARE
    m = K.composite_loop(out, coords, ns, n_rows, bg, np.float64, grad_rgb=g, mutation=mutation)
    clean = K.compositor_measures(case, ref["rgb"], ref["grad"], ref, r32)
    moved = K.compositor_measures(case, m["rgb"], m["grad"], ref, r32)
    assert clean["forward"] == 0 and clean["backward"] == 0 and clean["dead_nonzero"] == 0
    ratios = dict(forward=moved["forward"] / K.FORWARD_BAR, backward=moved["backward"] / K.backward_bar(moved["e32"]), dead_rows=float(moved["dead_nonzero"]))
    print(f"power {mutation} on {name}: error / bar forward {ratios['forward']:.3g}, backward {ratios['backward']:.3g} (e32 {moved['e32']:.2e}), "
          f"{moved['dead_nonzero']} of {moved['dead_rows']} dead rows written")
    assert max(ratios.values()) >= 10, (name, mutation, ratios)


def test_every_compositor_mutation_is_proven_on_some_case():
    assert {m for _, m in K.COMPOSITOR_POWER} == set(K.COMPOSITOR_MUTATIONS)
    for name, _ in K.COMPOSITOR_POWER:                                  # on the inputs with a dt per row, which the GPU tests run
        assert name.split("-")[0] == "cone" or name.startswith("ladder-random-")


def test_huber_expdecay_ema_and_batch_rays():
    from jittor_myc_nerfs_amd import ngp
    from jittor_myc_nerfs_amd.losses import huber_loss
    from jittor_myc_nerfs_amd.ngp_train import NGPEma, NGPExpDecay, ngp_adam
    d = 0.1
    x = torch.tensor([0.0, 0.04, 0.1, 0.1000001, 0.5, -0.3], dtype=torch.float64)
    want = torch.tensor([0.0, 0.5 / d * 0.04 ** 2, 0.5 / d * 0.1 ** 2, 0.1000001 - 0.05, 0.45, 0.25], dtype=torch.float64)
    assert torch.allclose(huber_loss(x, torch.zeros(6, dtype=torch.float64), d), want, rtol=0, atol=1e-15)
    assert float(huber_loss(torch.tensor(0.1), torch.tensor(0.0), d)) == pytest.approx(0.05)           # |x - t| == delta: the quadratic branch, both agree there
    assert huber_loss(torch.zeros(3, 2), torch.ones(3, 2)).shape == (3, 2)                               # elementwise
    # ExpDecay: the factor drops by decay_base at steps decay_start, decay_start + interval, ... (decided BEFORE the nested step)
    p = torch.nn.Parameter(torch.ones(4, dtype=torch.float64))
    adam = ngp_adam([p])
    assert adam.defaults["lr"] == 1e-1 and adam.defaults["eps"] == 1e-15 and adam.defaults["betas"] == (0.9, 0.99)
    opt = NGPExpDecay(adam, decay_start=2, decay_interval=2, decay_base=0.5)
    lrs = []
    for _ in range(5):
        p.grad = torch.ones_like(p)
        opt.step()
        lrs.append(adam.param_groups[0]["lr"])
    assert lrs == pytest.approx([0.1, 0.1, 0.05, 0.05, 0.025])
    # EMA: the parameters are rewritten with the debiased average; closed form over 5 steps of a known sequence
    q = torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))
    ema = NGPEma([q], decay=0.95)
    v, version = np.zeros(3), q._version
    for t in range(1, 6):
        with torch.no_grad():
            q += float(t)                                                # "the optimizer step"
        pv = q.detach().numpy().copy()
        ema.ema_step()
        v = ((1 - 0.95) * pv + 0.95 * v * (1 - 0.95 ** (t - 1))) / (1 - 0.95 ** t)
        assert np.allclose(q.detach().numpy(), v, rtol=0, atol=1e-12) and np.allclose(ema.values[0].numpy(), v, rtol=0, atol=1e-12)
    assert q._version > version                                           # an in-place write: NGPNetworks.packed() will repack
    # update_batch_rays: the reference's integers
    S = ngp.DensityGridSampler
    # hand-computed: 4096 * 2^18 / 150000 = 7158.3 -> 7158 -> 7168; nothing measured -> the capacity; 1024 * 2^16 / 700000 = 95.9 -> 95 -> 128;
    # 128 * 2^18 / 100 = 335544.3 -> above the capacity
    for n_rays, cap, measured, want_rays in ((4096, 1 << 18, 16 * 150000, 7168), (4096, 1 << 18, 0, 1 << 18), (1024, 1 << 16, 16 * 700000, 128),
                                             (128, 1 << 18, 16 * 100, 1 << 18)):
        assert S.batch_rays(n_rays, cap, measured) == want_rays
    assert S.batch_rays(4096, 1 << 18, 16 * (1 << 18)) == 4096


def test_train_data_rays_and_checkpoint_round_trip(tmp_path):
    from jittor_myc_nerfs_amd import ngp
    from jittor_myc_nerfs_amd.ngp_train import NGPTrainData, save_jnerf_checkpoint
    from jittor_myc_nerfs_amd import rays as R
    H = W = 8
    xforms = [ngp.matrix_nerf2ngp(np.asarray(p, np.float32)) for p in R.sphere_poses(3, 4.0)]
    imgs = np.random.default_rng(0).random((3, H, W, 4), dtype=np.float32)
    data = NGPTrainData(imgs, np.stack(xforms), [20.0, 20.0])
    gen = torch.Generator().manual_seed(3)
    ids, o, d, rgba = data.next_batch(257, gen)
    assert ids.shape == (257,) and o.shape == d.shape == (257, 3) and rgba.shape == (257, 4)
    assert int(ids.min()) >= 0 and int(ids.max()) < 3
    gen.manual_seed(3)
    ids2 = torch.randint(3, (257,), generator=gen)
    pix = torch.randint(H * W, (257,), generator=gen)
    assert torch.equal(ids, ids2)
    for i in range(3):
        fo, fd = ngp.generate_rays(xforms[i], W, H, (20.0, 20.0))
        m = ids == i
        assert torch.allclose(d[m], fd[pix[m]], rtol=0, atol=1e-6) and torch.equal(o[m], fo[pix[m]])
        assert torch.equal(rgba[m], torch.as_tensor(imgs[i]).reshape(-1, 4)[pix[m]])
    f, x, res = data.training_views()
    assert f.shape == (3, 2) and x.shape == (3, 3, 4) and res == (W, H)
    # checkpoint: what save writes, load reads back bit for bit (CPU tensors)
    model, model2 = ngp.NGPNetworks(1), ngp.NGPNetworks(1)
    sampler, sampler2 = ngp.DensityGridSampler(model, 1, rng=ngp.Pcg32(1)), ngp.DensityGridSampler(model2, 1, rng=ngp.Pcg32(1))
    with torch.no_grad():
        sampler.density_grid.uniform_(-1, 1)
        sampler.density_grid_bitfield.random_(0, 256)
        sampler.density_grid_mean.fill_(0.25)
    path = str(tmp_path / "params.pkl")
    save_jnerf_checkpoint(path, model, sampler, 123)
    assert ngp.load_jnerf_checkpoint(path, model2, sampler2) == 123
    for a, b in zip(model.parameters(), model2.parameters()):
        assert torch.equal(a, b)
    for k in ("density_grid", "density_grid_bitfield", "density_grid_mean"):
        assert torch.equal(getattr(sampler, k), getattr(sampler2, k))


def test_training_is_opt_in():
    from jittor_myc_nerfs_amd import ngp
    model = ngp.NGPNetworks(1)
    s = ngp.DensityGridSampler(model, 1, rng=ngp.Pcg32(1))
    assert model.hip_training is False and s.target_batch_size == 1 << 18 and s.update_den_freq == 16 and s.training_step == 0
    assert ngp.DensityGridSampler(model, 1, target_batch_size=1 << 16).target_batch_size == 1 << 16
    with pytest.raises(NotImplementedError):
        s.sample(None, torch.zeros(1, 3), torch.ones(1, 3), is_training=True)


def test_train_data_from_blender(tmp_path):
    import math
    from jittor_myc_nerfs_amd import ngp
    from jittor_myc_nerfs_amd.ngp_train import NGPTrainData
    root = str(tmp_path / "scene")
    imgs = K.tiny_blender_scene(root)
    data = NGPTrainData.from_blender(root)
    assert (data.n_images, data.H, data.W) == (3, 6, 6) and data.aabb_scale == 1
    assert np.array_equal(data.images.numpy(), imgs.astype(np.float32) / 255.0)
    focal = 0.5 * 6 / math.tan(0.5 * 0.6911)                                 # camera_angle_x at the images' own width, not the json's default 800
    assert np.allclose(data.focal_lengths.numpy(), focal, rtol=1e-6)
    views = ngp.NerfRays(root, mode="train")
    assert np.array_equal(data.transforms.numpy(), np.stack(views.transforms))
    ids, pix = torch.tensor([0, 2, 1]), torch.tensor([0, 35, 17])
    o, d = data.rays_of(ids, pix)
    for k in range(3):
        fo, fd = ngp.generate_rays(views.transforms[int(ids[k])], 6, 6, (focal, focal))
        assert torch.allclose(d[k], fd[int(pix[k])], rtol=0, atol=1e-6) and torch.equal(o[k], fo[int(pix[k])])
    with pytest.raises(ValueError, match="square"):
        NGPTrainData(np.zeros((1, 4, 6, 4), np.float32), np.zeros((1, 3, 4), np.float32), [10.0, 10.0])
