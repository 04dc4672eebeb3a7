"""CPU checks behind tests/test_gpu_ngp_frame.py, with the oracle alone: the fp64 compositing reference of ngp_frame_common agrees with
the oracle's two compositors, and the designed inputs really put the break, the step counts and the thresholds where the GPU tests
need them (a scene that misses its condition would let a wrong kernel pass, or fail a right one)."""
import numpy as np
import pytest

import ngp_frame_common as F
from conftest import NGP_AABB_SCALE, ngp_camera_rays


@pytest.fixture(scope="module")
def outs():
    """Oracle network outputs of the designed scenes on the 421-ray pattern, computed once per k."""
    from oracle import ngp_oracle as N
    cache = {}

    def get(k):
        if k not in cache:
            levels, arrs = F.designed_scene(k)
            cache[k] = N.network_c(levels, arrs, F.designed_rows(F.PERIOD, k != F.NO_BREAK)[2])
        return cache[k]
    return get


def test_ladder_has_every_step_count():
    _, _, coords, ns = F.designed_rows()
    have = set(ns[:, 0].tolist())
    assert set(F.STEP_COUNTS) <= have, sorted(set(F.STEP_COUNTS) - have)
    assert int(ns[:, 0].sum()) == coords.shape[0] and ns[0, 0] == 1024          # ray 0 is the cap ray; no ray was dropped
    assert sorted(have)[-2] > max(F.BREAKS) + 32                                 # ladder rays reach past the tile behind the last wanted break
    _, _, _, ns2 = F.designed_rows(F.PERIOD, False)
    assert ns2[0, 0] == 0 and np.array_equal(ns2[1:, 0], ns[1:, 0])              # without the cap ray nothing exceeds the ladder


@pytest.mark.parametrize("k", F.BREAKS + (F.NO_BREAK,))
def test_reference_matches_oracle_compositors(k, outs):
    """composite_f64 against the oracle's C compositor (fp32), the ray-by-ray fp64 loop and, on a subset, the oracle's numpy compositor.
    2e-6 is a tenth of the 2e-5 the GPU tests allow between a kernel and this reference."""
    from oracle import ngp_oracle as N
    _, _, coords, ns = F.designed_rows(F.PERIOD, k != F.NO_BREAK)
    out = outs(k)
    rgb, brk, margin, work = F.composite_f64(out, coords, ns, F.BG)
    loop_rgb, loop_brk = F.composite_loop_f64(out, coords, ns, F.BG)
    assert np.array_equal(brk, loop_brk) and np.abs(rgb - loop_rgb).max() < 1e-10      # two fp64 evaluation orders (a running sum over all rows / products per ray)
    c_rgb, T = N.composite_c(out, coords, ns, F.BG)
    err = np.abs(c_rgb - rgb).max()
    print(f"k={k}: fp32 C compositor vs fp64 reference {err:.2e}")
    assert err < 2e-6
    assert np.array_equal(T[brk >= 0] < 1e-4, np.ones((brk >= 0).sum(), bool))
    sub = slice(100, 164)
    assert np.abs(N.composite(out, coords, ns[sub], F.BG) - rgb[sub]).max() < 2e-6
    assert np.array_equal(rgb[ns[:, 0] == 0], np.tile(np.asarray(F.BG, np.float64), ((ns[:, 0] == 0).sum(), 1)))
    # other thresholds move the break the way the threshold moves
    _, b_lo, _, w_lo = F.composite_f64(out, coords, ns, F.BG, thr=1e-4 * np.exp(0.05))
    _, b_hi, _, w_hi = F.composite_f64(out, coords, ns, F.BG, thr=1e-4 * np.exp(-0.05))
    assert (w_lo <= work).all() and (work <= w_hi).all()


@pytest.mark.parametrize("k", F.BREAKS)
def test_designed_scene_breaks_at_k(k, outs):
    """Every ray longer than k breaks exactly at sample k, no other ray breaks, and no decision is close to the threshold.

    The wanted distance is |ln(T / 1e-4)| >= 0.05.  With one optical depth tau per step, T_j = exp(-j tau): the decisions at k - 1 and at k
    lie tau apart, so at best both are tau / 2 from the threshold — which tau = ln(1e4) / (k - 0.5) achieves.  tau / 2 is 0.0482 for k = 96
    and 0.0477 for k = 97 (0.05 is unreachable there for any constant tau); those two are held to 0.495 tau instead, all others to 0.05.
    What the distance has to cover is the network bar's effect on ln T (F.network_shift, ~0.009 here): it is checked to fit twice."""
    _, _, coords, ns = F.designed_rows()
    out = outs(k)
    rgb, brk, margin, work = F.composite_f64(out, coords, ns, F.BG)
    n = ns[:, 0]
    assert (n > k).sum() >= 40 and np.array_equal(brk[n > k], np.full((n > k).sum(), k)) and (brk[n <= k] == -1).all()
    tau = F.designed_tau(k)
    want = min(F.MARGIN, 0.495 * tau)
    print(f"k={k}: tau {tau:.4f}, smallest |ln(T/1e-4)| {margin.min():.4f} (wanted {want:.4f}), network bar moves ln T by <= {F.network_shift(out):.4f}, "
          f"work {int(work.sum())} of {int(n.sum())}, colours {rgb.min():.3f}..{rgb.max():.3f}")
    assert margin.min() >= want and margin.min() >= 2 * F.network_shift(out)
    assert rgb.min() >= 0.05 and rgb.max() <= 0.95
    assert np.array_equal(work, np.where(n > k, np.minimum(n, 32 * (k // 32 + 1)), n))
    sig = 1 / (1 + np.exp(-out[:, :3].astype(np.float64)))
    assert sig.min() > 0.05 and sig.max() < 0.95 and np.ptp(out[:, 3]) < 1e-4        # one density everywhere, colours off saturation


def test_work_jumps_at_the_tile_edges(outs):
    """The counter the GPU test pins moves only where the break crosses a tile: equal for k = 1, 2, 3, 31, then up at 32, 64 and 96."""
    _, _, coords, ns = F.designed_rows()
    w = {k: int(F.composite_f64(outs(k), coords, ns, F.BG)[3].sum()) for k in F.BREAKS}
    assert w[1] == w[2] == w[3] == w[31] < w[32] == w[33] < w[64] == w[65] < w[96] == w[97] < int(ns[:, 0].sum())


def test_no_break_scene(outs):
    _, _, coords, ns = F.designed_rows(F.PERIOD, False)
    rgb, brk, margin, work = F.composite_f64(outs(F.NO_BREAK), coords, ns, F.BG)
    assert (brk == -1).all() and margin.min() >= F.MARGIN and np.array_equal(work, ns[:, 0])
    assert rgb.min() >= 0.05 and rgb.max() <= 0.95
    assert np.abs(rgb - np.asarray(F.BG)).max() > 0.1                              # the long rays are visibly not the background


@pytest.mark.parametrize("R", F.RAY_COUNTS)
def test_ray_count_inputs(R):
    """Each ray count of the sweep holds the pattern it needs: rows for every ray, and (from 63 rays on) breaking rays."""
    o, d, coords, ns = F.designed_rows(R)
    assert o.shape == (R, 3) and ns.shape == (R, 2) and int(ns[:, 0].sum()) == coords.shape[0]
    if R == 0:
        return
    assert ns[0, 0] == 1024 and (ns[:, 0] > F.RAY_COUNT_K).sum() >= min(R, 60)
    if R > F.PERIOD:
        assert (ns[:, 0] == 0).sum() >= 2 * (R // F.PERIOD)
        assert not np.array_equal(ns[1:F.PERIOD, 0], ns[F.PERIOD + 1:2 * F.PERIOD, 0])   # another jitter in the next period


def test_cone_scene_band(ngp_scene):
    """Cone stepping on the shared scene: the break is not designed there, so the GPU test bounds the counter by the predictions for
    thresholds e^{+-0.05} away.  That band has to be narrow (<= 1 % of the samples) for the bound to pin anything."""
    from oracle import ngp_oracle as N
    levels, arrs = ngp_scene
    o, d = ngp_camera_rays(F.CONE_WH, F.CONE_WH, pose_index=F.CONE_POSE)
    coords, ns = F.oracle_rows(o, d, arrs["density_grid_bitfield"], NGP_AABB_SCALE, const_dt=False)
    out = N.network_c(levels, arrs, coords)
    total = int(ns[:, 0].sum())
    lo = int(F.composite_f64(out, coords, ns, F.BG, thr=1e-4 * np.exp(0.05))[3].sum())
    hi = int(F.composite_f64(out, coords, ns, F.BG, thr=1e-4 * np.exp(-0.05))[3].sum())
    rgb, brk, _, work = F.composite_f64(out, coords, ns, F.BG)
    dt = N.unwarp_dt(coords[:, 3])
    print(f"cone scene: {total} samples, band {lo}..{hi} ({100.0 * (hi - lo) / total:.2f} %), {(brk >= 0).sum()} breaking rays, dt {dt.min():.4f}..{dt.max():.4f} warped "
          f"{coords[:, 3].min():.3f}..{coords[:, 3].max():.3f}")
    assert lo <= int(work.sum()) <= hi and hi - lo <= 0.01 * total
    assert (brk >= 0).sum() > 100 and lo < 0.9 * total                              # many rays break, and breaking saves work
    assert coords[:, 3].max() > 2 * coords[:, 3].min() > 0                          # the warped dt really varies along the rays
    c_rgb, _ = N.composite_c(out, coords, ns, F.BG)
    assert np.abs(c_rgb - rgb).max() < 2e-6


def test_range_case():
    """The random-grid case sits at about half the fp16 range, and the oracle's fp32 network meets the network bar against fp64 there."""
    from oracle import ngp_oracle as N
    levels, arrs, coords, out, biggest = F.range_case()
    print(f"range case: largest value between layers {biggest:.0f}, largest output {np.abs(out).max():.0f}")
    assert 0.9 * F.HIDDEN_TARGET < biggest < 1.1 * F.HIDDEN_TARGET < 65504
    err = np.abs(N.network_c(levels, arrs, coords) - out).max()
    assert err < 2e-4 * max(1.0, np.abs(out).max())


@pytest.mark.parametrize("kind", ["sparse", "dense", "empty"])
def test_density_grids(kind):
    from oracle import ngp_oracle as N
    g = F.density_grid(kind)
    mean, thr, gap = F.grid_threshold_gap(g)
    bits, omean = N.update_bitfield(g)
    assert abs(omean - mean) < 1e-6
    cells = N.NERF_GRIDSIZE ** 3
    assert np.array_equal(bits[:cells // 8], np.packbits(g[:cells] > thr, bitorder="little"))
    if kind == "empty":
        assert mean == 0 and thr == 0 and not bits.any() and (g < 0).any()
        return
    assert gap > 0.2                                                               # no level near the threshold: the summation order of the mean cannot matter
    assert (mean < 0.01) == (kind == "sparse")
    between = g[:cells][(g[:cells] > min(mean, 0.01)) & (g[:cells] < max(mean, 0.01))]
    assert between.size > 1000                                                     # cells that tell the two candidate thresholds apart
    assert bits[cells // 8:].any() and bits[:cells // 8].any()
