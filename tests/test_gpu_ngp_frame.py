"""The fused frame kernel (ngp_render_kernel behind tvr_ngp_render / DensityGridSampler.render_frame) at its tile, ticket and break edges,
against the fp64 compositing reference of ngp_frame_common; with it the device-side row count of tvr_ngp_network, tvr_ngp_composite under
cone stepping, tvr_ngp_update_bitfield in both threshold regimes, and the fused network at half the fp16 range.  The inputs are the
designed scenes test_ngp_frame_host.py checks on the CPU.

Bars: pictures within 2e-5 of the fp64 reference fed with the device's own row-level network outputs (test_composite_matches_oracle's bar;
only compositing is under test); fused picture within 2e-6 of the row-level picture (test_render_img_and_render_frame's bar); network outputs
within 2e-4 * max(1, |out|) (test_fused_network_matches_oracle's bar); rows, counters, `evaluated`, backgrounds and bitfields exact.
What an MI355X gave is in each test's docstring."""
import numpy as np
import pytest
import torch

import ngp_frame_common as F
from conftest import NGP_AABB_SCALE, ngp_camera_rays

pytestmark = pytest.mark.gpu
SENTINEL = -12345.678


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def designed():
    """Model and sampler of the designed scenes (aabb_scale 1, full occupancy, background F.BG); a test sets the grid constant itself."""
    from jittor_myc_nerfs_amd import ngp
    levels, arrs = F.designed_scene(F.RAY_COUNT_K)
    dev = torch.device("cuda:0")
    model = ngp.NGPNetworks(F.AABB_SCALE).to(dev)
    sampler = ngp.DensityGridSampler(model, F.AABB_SCALE, background_color=F.BG, rng=ngp.Pcg32(1337)).to(dev)
    ngp.load_scene_arrays(model, sampler, arrs)
    assert np.array_equal(model.pos_encoder.offsets, levels["offsets"])
    return model, sampler, dev


def _set_grid(model, k):
    with torch.no_grad():
        model.pos_encoder.m_grid.fill_(F.designed_grid_value(k))


def _render_both(sampler, o, d):
    """(fused picture, its stats, row-level picture, its stats, device rows, device numsteps, device network outputs of the rows): three
    passes from the same generator state."""
    from jittor_myc_nerfs_amd import ngp
    dev = sampler.density_grid_bitfield.device
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    sampler.rng = ngp.Pcg32(1337)
    fs = {}
    fused = sampler.render_frame(to, td, stats=fs)
    after = (sampler.rng.state, sampler.rng.inc)
    sampler.rng = ngp.Pcg32(1337)
    rs = {}
    rows = sampler.render_frame_rows(to, td, stats=rs)
    assert (sampler.rng.state, sampler.rng.inc) == after
    sampler.rng = ngp.Pcg32(1337)
    coords, _, numsteps, counter = sampler._sample_raw(to, td, max(1, rs["samples"]), slab_rays=sampler.n_rays_per_batch)
    assert int(counter[1]) == rs["samples"]
    coords = coords[:rs["samples"]]
    out = sampler.model(coords[:, :3], coords[:, 4:])
    return fused.cpu().numpy(), fs, rows.cpu().numpy(), rs, coords.cpu().numpy(), numsteps.cpu().numpy(), out.cpu().numpy()


def _check_frame(sampler, o, d, want_coords, want_ns, bg, what):
    """The comparisons every frame case holds; returns the device's network outputs, rows and step counts, the fused call's stats and the
    reference's break indices, margins and predicted work for the caller's own checks."""
    R = o.shape[0]
    fused, fs, rows, rs, coords, ns, out = _render_both(sampler, o, d)
    assert fused.shape == (R, 3) and rows.shape == (R, 3)
    total = int(want_ns[:, 0].sum())
    assert np.array_equal(ns, want_ns) and np.array_equal(_bits(coords), _bits(want_coords)), f"{what}: device rows differ from the oracle's"
    assert fs["samples"] == total and rs["samples"] == total
    ref, brk, margin, work = F.composite_f64(out, coords, ns, bg)
    e_fused, e_rows = np.abs(fused - ref).max(initial=0), np.abs(rows - ref).max(initial=0)
    e_pair = np.abs(fused - rows).max(initial=0)
    print(f"{what}: R={R} samples={total} evaluated={fs['evaluated']} predicted={int(work.sum())} | fused-ref {e_fused:.2e} rows-ref {e_rows:.2e} "
          f"fused-rows {e_pair:.2e} | smallest |ln(T/1e-4)| {margin.min(initial=np.inf):.4f}")
    assert e_fused < 2e-5 and e_rows < 2e-5, f"{what}: picture vs fp64 reference: fused {e_fused:.3e}, rows {e_rows:.3e}"
    assert e_pair < 2e-6, f"{what}: fused vs row-level picture {e_pair:.3e}"
    zero = ns[:, 0] == 0
    bg32 = np.tile(np.asarray(bg, np.float32), (int(zero.sum()), 1))
    assert np.array_equal(_bits(fused[zero]), _bits(bg32)) and np.array_equal(_bits(rows[zero]), _bits(bg32)), f"{what}: a ray without steps is not the background"
    return out, coords, ns, fs, brk, margin, work


@pytest.mark.parametrize("k", F.BREAKS + (F.NO_BREAK,))
def test_break_ladder(designed, k):
    """Rays of 0 ... 137 and 1024 steps whose T falls below 1e-4 exactly at sample k: `evaluated` must be the samples up to the end of the
    tile that holds the break, no more and no fewer; broken rays get no background, unbroken ones T * bg, empty ones bg.
    MI355X, largest over the eleven k: fused-ref 4.4e-7, rows-ref 4.7e-7, fused-rows 3.0e-7, network 1.1e-5 (its bar here: 4.8e-4 ... 2.0e-3);
    `evaluated` equal to the prediction for every k (11731 of 29526 for k <= 31, 20385 for 32 / 33, 25974 for 64 / 65, 28488 for 96 / 97)."""
    from oracle import ngp_oracle as N
    model, sampler, _ = designed
    _set_grid(model, k)
    cap_ray = k != F.NO_BREAK
    o, d, want_coords, want_ns = F.designed_rows(F.PERIOD, cap_ray)
    out, coords, ns, fs, brk, margin, work = _check_frame(sampler, o, d, want_coords, want_ns, F.BG, f"k={k}")
    n = ns[:, 0]
    if cap_ray:
        assert np.array_equal(brk, np.where(n > k, k, -1)) and margin.min() >= min(F.MARGIN, 0.495 * F.designed_tau(k))
    else:
        assert (brk == -1).all() and margin.min() >= F.MARGIN
    assert fs["evaluated"] == int(work.sum()), f"k={k}: evaluated {fs['evaluated']} != predicted {int(work.sum())} (of {fs['samples']})"
    levels, arrs = F.designed_scene(k)
    want = N.network_c(levels, arrs, coords)
    err = np.abs(out - want).max()
    print(f"k={k}: network vs oracle {err:.2e} (bar {2e-4 * max(1.0, np.abs(want).max()):.2e})")
    assert err < 2e-4 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("R", F.RAY_COUNTS)
def test_ray_counts(designed, R):
    """The launch has (R+3)/4 blocks below 2048 rays and 512 from there on; a ticket of the ray queue covers 64 rays; the jitter restarts every
    4096 rays.  MI355X, largest over the nine R: fused-ref 1.2e-7, rows-ref 2.0e-7, fused-rows 1.8e-7; `evaluated` equal to the prediction at every R
    (201972 of 293392 samples at R = 4097)."""
    model, sampler, dev = designed
    k = F.RAY_COUNT_K
    _set_grid(model, k)
    o, d, want_coords, want_ns = F.designed_rows(R)
    out, coords, ns, fs, brk, margin, work = _check_frame(sampler, o, d, want_coords, want_ns, F.BG, f"R={R}")
    assert np.array_equal(brk, np.where(ns[:, 0] > k, k, -1))
    assert fs["evaluated"] == int(work.sum())
    if R == 0:
        assert fs == {"evaluated": 0, "samples": 0}


def test_cone_stepping(ngp_scene):
    """const_dt=False through the frame kernel (which recomputes every row's warped dt from t) and through tvr_ngp_composite (which reads it
    from the rows), on the shared aabb_scale-4 scene.  The break is not designed here, so `evaluated` is bounded by the predictions for
    thresholds e^{+-0.05} away, taken from the oracle's outputs (the band is 0.08 % of the samples wide: test_ngp_frame_host.py).
    MI355X: fused-ref 5.2e-7, rows-ref 5.1e-7, fused-rows 6.0e-7; evaluated 43892 in 43859..43906 of 55985 samples."""
    from jittor_myc_nerfs_amd import ngp
    from oracle import ngp_oracle as N
    levels, arrs = ngp_scene
    dev = torch.device("cuda:0")
    model = ngp.NGPNetworks(NGP_AABB_SCALE).to(dev)
    sampler = ngp.DensityGridSampler(model, NGP_AABB_SCALE, const_dt=False, background_color=F.BG, rng=ngp.Pcg32(1337)).to(dev)
    ngp.load_scene_arrays(model, sampler, arrs)                        # the oracle's bitfield
    o, d = ngp_camera_rays(F.CONE_WH, F.CONE_WH, pose_index=F.CONE_POSE)
    want_coords, _, want_ns, _, _ = N.sample(o, d, arrs["density_grid_bitfield"], NGP_AABB_SCALE, N.Pcg32(1337).state, const_dt=False, slab_rays=4096)
    out, coords, ns, fs, brk, margin, work = _check_frame(sampler, o, d, want_coords, want_ns, F.BG, "cone")
    assert coords[:, 3].max() > 2 * coords[:, 3].min() > 0 and (brk >= 0).sum() > 100
    # tvr_ngp_composite on these rows: the device's outputs against the fp64 reference, the oracle's outputs against the oracle's compositor
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = sampler._composite(t(out), t(coords), t(ns), F.BG).cpu().numpy()
    assert np.abs(got - F.composite_f64(out, coords, ns, F.BG)[0]).max() < 2e-5
    oout = N.network_c(levels, arrs, coords)
    got = sampler._composite(t(oout), t(coords), t(ns), F.BG).cpu().numpy()
    assert np.abs(got - N.composite_c(oout, coords, ns, F.BG)[0]).max() < 2e-5
    lo = int(F.composite_f64(oout, coords, ns, F.BG, thr=1e-4 * np.exp(0.05))[3].sum())
    hi = int(F.composite_f64(oout, coords, ns, F.BG, thr=1e-4 * np.exp(-0.05))[3].sum())
    print(f"cone: evaluated {fs['evaluated']} in {lo}..{hi} of {fs['samples']} ({100.0 * (hi - lo) / fs['samples']:.2f} %)")
    assert lo <= fs["evaluated"] <= hi, f"evaluated {fs['evaluated']} outside {lo}..{hi}"


@pytest.mark.parametrize("count", [0, 1, 31, 32, 33, 127, 128, 129, 1000])
def test_network_device_row_count(designed, count):
    """tvr_ngp_network with n_dev: rows below min(count, n_max) as without n_dev, bit for bit; every row behind keeps what it held."""
    model, _, dev = designed
    _set_grid(model, F.RAY_COUNT_K)
    with torch.no_grad():
        model.pos_encoder.m_grid[::3] *= 0.5                           # not one constant: rows differ from each other
    n_max = 160
    rng = np.random.default_rng(5)
    rows = torch.from_numpy(rng.random((n_max, 7), dtype=np.float32)).to(dev)
    plain = model(rows[:, :3], rows[:, 4:]).cpu().numpy()
    assert np.unique(plain[:, 3]).size > n_max // 2
    out = torch.full((n_max, 4), SENTINEL, device=dev)
    got = model._run(rows[:, :3], rows[:, 4:], n_dev=torch.tensor([count], dtype=torch.int32, device=dev), out=out)
    assert got.data_ptr() == out.data_ptr()
    got = got.cpu().numpy()
    n = min(count, n_max)
    assert np.array_equal(_bits(got[:n]), _bits(plain[:n])), f"count {count}: rows below the count differ from the plain call"
    assert np.array_equal(_bits(got[n:]), _bits(np.full((n_max - n, 4), SENTINEL, np.float32))), f"count {count}: a row behind the count was written"


@pytest.mark.parametrize("kind", ["sparse", "dense", "empty"])
def test_update_bitfield_regimes(designed, kind):
    """threshold = min(0.01, mean): a grid whose mean is below 0.01, one above it, and one without a positive cell (threshold 0, nothing set:
    a frame through it is the background and marches no sample)."""
    from jittor_myc_nerfs_amd import ngp
    from oracle import ngp_oracle as N
    model, _, dev = designed
    g = F.density_grid(kind)
    want_bits, want_mean = N.update_bitfield(g)
    sampler = ngp.DensityGridSampler(model, F.AABB_SCALE, background_color=F.BG, rng=ngp.Pcg32(1337)).to(dev)
    sampler.density_grid.copy_(torch.from_numpy(g))
    sampler.density_grid_bitfield.fill_(0x5A)                          # stale contents must not survive (the coarser cascades are OR-ed into)
    sampler.update_bitfield()
    got = sampler.density_grid_bitfield.cpu().numpy()
    print(f"{kind}: mean {float(sampler.density_grid_mean):.6f} vs {want_mean:.6f}, {int(np.unpackbits(want_bits).sum())} bits set")
    assert abs(float(sampler.density_grid_mean) - want_mean) < 1e-6
    assert np.array_equal(got, want_bits), f"{kind}: {np.count_nonzero(got != want_bits)} bitfield bytes differ"
    if kind != "empty":
        return
    assert not got.any()
    _set_grid(model, F.RAY_COUNT_K)
    o, d = F.designed_rays()
    st = {}
    img = sampler.render_frame(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), stats=st).cpu().numpy()
    assert st == {"evaluated": 0, "samples": 0}
    assert np.array_equal(_bits(img), _bits(np.tile(np.asarray(F.BG, np.float32), (o.shape[0], 1))))
    rs = {}
    img = sampler.render_frame_rows(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), stats=rs).cpu().numpy()
    assert rs["samples"] == 0 and np.array_equal(_bits(img), _bits(np.tile(np.asarray(F.BG, np.float32), (o.shape[0], 1))))


def test_network_at_half_the_fp16_range():
    """The fused network hands every activation to the next layer as two fp16 halves (include/tvr_ngp.h: valid while no such value exceeds
    65504).  A random grid scaled until the largest of them is 3e4: the network bar against fp64 still holds.
    MI355X: error 2.9e-2 against a bar of 3.4 (largest output 16821)."""
    from jittor_myc_nerfs_amd import ngp
    levels, arrs, coords, want, biggest = F.range_case()
    dev = torch.device("cuda:0")
    model = ngp.NGPNetworks(F.AABB_SCALE).to(dev)
    ngp.load_scene_arrays(model, None, arrs)
    c = torch.from_numpy(coords).to(dev)
    got = model(c[:, :3], c[:, 4:]).cpu().numpy()
    err = np.abs(got - want).max()
    print(f"range: largest value between layers {biggest:.0f}, largest output {np.abs(want).max():.0f}, error {err:.3e} (bar {2e-4 * max(1.0, np.abs(want).max()):.3e})")
    assert np.isfinite(got).all() and err < 2e-4 * max(1.0, np.abs(want).max())
