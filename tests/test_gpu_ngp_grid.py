"""GPU: the occupancy grid built and refreshed from the network (csrc/tvr_ngp_grid.hip, include/tvr_ngp.h) against the float32 numpy restatement of
tests/ngp_grid_common.py.  Bars: generator, mark-untrained and ema bit for bit; the density head bit-equal to column 3 of the fused network; the splat
within the derived bound of the hardware exponential; the fused update bit-equal to the stand-alone calls."""
import numpy as np
import pytest
import torch

import ngp_grid_common as K
from conftest import NGP_AABB_SCALE, ngp_camera_rays

pytestmark = pytest.mark.gpu
F, U32 = np.float32, np.uint32
assert NGP_AABB_SCALE == K.AABB_SCALE


@pytest.fixture(scope="module")
def setup(ngp_scene):
    from jittor_myc_nerfs_amd import ngp
    _, arrs = ngp_scene
    dev = torch.device("cuda:0")
    model = ngp.NGPNetworks(NGP_AABB_SCALE).to(dev)
    ngp.load_scene_arrays(model, None, arrs)
    grid = torch.from_numpy(arrs["density_grid"]).to(dev)
    return model, grid, arrs, dev


def _sampler(model, dev, grid=None):
    from jittor_myc_nerfs_amd import ngp
    s = ngp.DensityGridSampler(model, NGP_AABB_SCALE, rng=ngp.Pcg32(1337)).to(dev)
    if grid is not None:
        s.density_grid.copy_(torch.as_tensor(grid))
    return s


_marked = {}


def _marked_mixed_grid():
    """The restatement's mark-untrained of the mixed grid under the three cameras: -1, 0 and positive cells (reference of test 2, start of test 5)."""
    if "g" not in _marked:
        _marked["g"] = K.mark_untrained(K.mixed_grid(), *K.mark_cameras(3), K.MARK_RES)
    return _marked["g"]


def _bits(t):
    return t.cpu().numpy().view(U32)


# ------------------------------------------------------------------------------------------------------------------ 1. generator
@pytest.mark.parametrize("n", [1, 31, 4099])
def test_generator_bit_exact(setup, n):
    from jittor_myc_nerfs_amd import ngp
    _, grid, arrs, _ = setup
    lo, hi = K.AABB
    for advances in (0, 1):
        rng = ngp.Pcg32(1337)
        for _ in range(advances):
            rng.advance()
        before = (rng.state, rng.inc)
        for ema_step in (0, 3):
            for n_cascades in (1, 3):
                for thresh in (-0.01, 0.01):
                    pos, idx = ngp.grid_samples(grid, n, ema_step, n_cascades, thresh, rng, (lo[0], hi[0]))
                    want_pos, want_idx = K.grid_samples(n, ema_step, n_cascades, thresh, rng.state, rng.inc, lo, hi, arrs["density_grid"])
                    what = f"n {n} advances {advances} ema_step {ema_step} n_cascades {n_cascades} thresh {thresh}"
                    assert np.array_equal(_bits(idx), want_idx), what
                    assert np.array_equal(_bits(pos), want_pos.view(U32)), what
        assert (rng.state, rng.inc) == before                        # the caller's generator is read, not advanced


# ------------------------------------------------------------------------------------------------------------------ 2. mark-untrained
@pytest.mark.parametrize("case", ["three_cameras", "one_camera", "mixed_grid"])
def test_mark_untrained_bit_exact(setup, case):
    from jittor_myc_nerfs_amd import ngp
    model, _, _, dev = setup
    focal, xforms = K.mark_cameras(1 if case == "one_camera" else 3)
    s = _sampler(model, dev)
    if case == "mixed_grid":
        start = K.mixed_grid()
        s.density_grid.copy_(torch.from_numpy(start))
        ngp.grid_mark_untrained(s.density_grid, focal, xforms, K.MARK_RES)
        want = _marked_mixed_grid()
        seen = K.cells_seen(focal, xforms, K.MARK_RES)
        got = s.density_grid.cpu().numpy()
        assert np.array_equal(got[(start > 0) & seen], start[(start > 0) & seen]) and (got[(start < 0) & seen] == 0).all()
    else:
        s.density_grid.fill_(3.0)                                    # the wrapper starts from zeros whatever the grid held
        s.mark_untrained_density_grid(focal, xforms, K.MARK_RES)
        want = K.mark_untrained(np.zeros(K.N_CELLS_ALL, F), focal, xforms, K.MARK_RES)
        got = s.density_grid.cpu().numpy()
        assert set(np.unique(got).tolist()) == {-1.0, 0.0}
    assert np.array_equal(got.view(U32), want.view(U32)), f"{(got != want).sum()} of {got.size} cells differ"


# ------------------------------------------------------------------------------------------------------------------ 3. density head
@pytest.mark.parametrize("n", [1, 33, 4099])
def test_density_raw_bit_equal_to_the_fused_network(setup, n):
    """In the arithmetic the library is built with: TVR_NGP_MLP_F32 is a build switch of tvr_ngp_network itself, with no selection at run time.  The other
    arithmetic is this same file run on a variant build (`scripts/build_variant.sh ngp_f32 -DTVR_NGP_MLP_F32=1`, `TVR_LIB_PATH=.../libtvr_ngp_f32.so`)."""
    model, _, _, dev = setup
    g = torch.Generator().manual_seed(11 + n)
    if n == 4099:
        rows = torch.rand(n, 7, generator=g).to(dev)                 # the sampler's row layout: a row-strided view
        pos = rows[:, :3]
        assert pos.stride(0) == 7
    else:
        pos = torch.rand(n, 3, generator=g).to(dev)
    raw = model.density_raw(pos)
    full = model(pos, pos)
    assert raw.shape == (n,) and torch.isfinite(raw).all()
    assert np.array_equal(_bits(raw), _bits(full[:, 3].contiguous()))
    assert np.array_equal(_bits(model.density(pos)[:, 0].contiguous()), _bits(raw))
    if n > 1:
        assert float(raw.max() - raw.min()) > 1.0                    # not a constant


# ------------------------------------------------------------------------------------------------------------------ 4. splat and ema
def test_splat_within_the_exponentials_bound_and_ema_bit_exact(setup):
    """tmp against the fp64 restatement within relative (|raw| + 3) * 2^-23: one ulp (2^-23) of the hardware exp2, |raw| * 2^-24 from the rounding of
    raw * log2(e) (and a little from the constant's own), 2^-24 from the product with MIN_CONE_STEPSIZE."""
    from jittor_myc_nerfs_amd import ngp
    model, grid, _, dev = setup
    lo, hi = K.AABB
    pos, idx = ngp.grid_samples(grid, 4099, 0, 3, 0.01, ngp.Pcg32(1337), (lo[0], hi[0]))
    raw = model.density_raw(pos)
    idx2, raw2 = torch.cat([idx, idx]), torch.cat([raw, raw.roll(1)])   # every cell receives two samples
    tmp = torch.zeros(K.N_CELLS_ALL, device=dev)
    ngp.grid_splat(idx2, raw2, tmp)
    got = tmp.cpu().numpy()
    i_np, r_np = _bits(idx2), raw2.cpu().numpy()
    want = K.splat64(i_np, r_np)
    hit = np.zeros(K.N_CELLS_ALL, bool)
    hit[i_np] = True
    assert 4000 < hit.sum() <= 4099 and (got[~hit].view(U32) == 0).all()
    rabs = np.zeros(K.N_CELLS_ALL)
    np.maximum.at(rabs, i_np.astype(np.int64), np.abs(r_np.astype(np.float64)))
    err = np.abs(got[hit].astype(np.float64) - want[hit]) / want[hit]
    bound = (rabs[hit] + 3) * 2.0 ** -23
    print(f"splat: max relative error {err.max():.3e}, smallest bound {bound.min():.3e}, worst error / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    # max over duplicates: the larger of a cell's two samples, not the last one written
    first, second = np.exp(r_np[:4099].astype(np.float64)), np.exp(r_np[4099:].astype(np.float64))
    assert (first > second * 1.01).sum() > 500 and (second > first * 1.01).sum() > 500
    # the ema given that tmp, on a grid with negative, zero and positive cells
    start = _marked_mixed_grid()
    g = torch.from_numpy(start).to(dev)
    big = torch.from_numpy(np.where(hit, F(7.0), got).astype(F)).to(dev)   # and a tmp that beats the decayed positives where it hit
    for t in (tmp, big):
        gg = g.clone()
        ngp.grid_ema(t, gg, 0.95)
        assert np.array_equal(_bits(gg), K.ema(t.cpu().numpy(), start, 0.95).view(U32))
    assert (start[hit] < 0).sum() > 100 and (start[hit] > 0).sum() > 100


# ------------------------------------------------------------------------------------------------------------------ 5. fused update
def _pooled(prev_bytes):
    """update_bitfield's max-pool: bit j of byte morton(xyz(i) + 16) of the next cascade is set iff byte 8 i + j of this one is not 0."""
    i = np.arange(K.CELLS // 64, dtype=U32)
    b = np.zeros(K.CELLS // 64, np.uint8)
    for j in range(8):
        b |= ((prev_bytes[i * 8 + j] > 0).astype(np.uint8) << j).astype(np.uint8)
    x, y, z = [c + U32(K.G // 8) for c in K.cell_xyz(i)]
    out = np.zeros(K.CELLS // 8, np.uint8)
    out[K.morton3d(x, y, z)] = b
    return out


def _check_fused_equals_pieces(setup, counts, ema_step):
    model, _, _, dev = setup
    start = _marked_mixed_grid()
    sf, sp = _sampler(model, dev, start), _sampler(model, dev, start)
    sf.density_grid_ema_step = sp.density_grid_ema_step = ema_step
    sf.update_density_grid_nerf(0.5, *counts, fused=True)
    sp.update_density_grid_nerf(0.5, *counts, fused=False)
    what = f"counts {counts} ema_step {ema_step}"
    assert np.array_equal(_bits(sf.density_grid_tmp), _bits(sp.density_grid_tmp)), what
    assert np.array_equal(_bits(sf.density_grid), _bits(sp.density_grid)), what
    assert np.array_equal(sf.density_grid_bitfield.cpu().numpy(), sp.density_grid_bitfield.cpu().numpy()), what
    assert np.array_equal(_bits(sf.density_grid_mean), _bits(sp.density_grid_mean)), what
    assert (sf.rng.state, sf.density_grid_ema_step) == (sp.rng.state, ema_step + 1)
    tmp, grid = sf.density_grid_tmp.cpu().numpy(), sf.density_grid.cpu().numpy()
    n_hit = int((tmp > 0).sum())
    assert 0.5 * min(sum(counts), K.CELLS) < n_hit <= sum(counts), what                 # the samples landed
    assert np.array_equal(grid.view(U32), K.ema(tmp, start, 0.95).view(U32)) and np.array_equal((grid < 0), (start < 0))
    assert (tmp[3 * K.CELLS:] == 0).all()                             # aabb_scale 4: three cascades are sampled
    # an untrained cell is never occupied on its own account: its bit is 0 in cascade 0, and in a coarser cascade it is exactly what update_bitfield's
    # max-pool carries up from the eight finer cells under it (the pool does not look at the coarse cell's own value)
    bits = sf.density_grid_bitfield.cpu().numpy().reshape(5, K.CELLS // 8)
    cells = np.unpackbits(bits, axis=1, bitorder="little").astype(bool)
    neg = (grid < 0).reshape(5, K.CELLS)
    assert neg[0].sum() > 1000 and not cells[0][neg[0]].any()
    for c in range(1, 5):
        pooled = np.unpackbits(_pooled(bits[c - 1]), bitorder="little").astype(bool)
        assert neg[c].sum() > 1000 and np.array_equal(cells[c][neg[c]], pooled[neg[c]]), f"{what}: cascade {c}"
    assert cells[0].sum() > 1000
    return sf


@pytest.mark.parametrize("ema_step", [0, 3])
@pytest.mark.parametrize("counts", [(4099, 0), (1000, 1031)])
def test_fused_update_bit_equal_to_the_pieces(setup, counts, ema_step):
    _check_fused_equals_pieces(setup, counts, ema_step)


def test_fused_update_bit_equal_to_the_pieces_at_the_early_policy_size(setup):
    _check_fused_equals_pieces(setup, (K.CELLS * 3, 0), 0)


@pytest.mark.parametrize("counts", [(K.CELLS - 1, 0), (K.CELLS, K.CELLS), (K.CELLS + 33, 1000), (1000, 2 * K.CELLS + 31)])
def test_fused_update_bit_equal_to_the_pieces_around_a_whole_block(setup, counts):
    """The fused kernel reorders the samples of every whole block of 128^3 (by the Morton cell of their first candidate) and leaves the rest in order: just
    below one block, exactly one in either population, a block plus a ragged tail, two blocks plus a tail in the second population; at an ema_step whose
    product with n enters the index hash."""
    _check_fused_equals_pieces(setup, counts, 3)


def test_fused_update_at_a_count_whose_advance_reaches_bit_31(setup):
    """n = 2^29 + 2 is the first count at which 4 (n - 1), the lanes' largest generator advance, has bit 31 set; the samples live in registers, so the call
    needs no memory beyond the grids.  At ema_step 0 sample i does not depend on n, so tmp holds at least what the stand-alone calls give for any subset:
    the first 4099 samples, and the last 70 (i up to n - 1: the ragged tail behind 256 whole blocks, advances with bit 31 set) from the restatement."""
    from jittor_myc_nerfs_amd import ngp
    model, _, _, dev = setup
    n = (1 << 29) + 2
    start = _marked_mixed_grid()
    s = _sampler(model, dev, start)
    s.update_density_grid_nerf(0.5, n, 0, fused=True)
    tmp = s.density_grid_tmp.cpu().numpy()
    # 256 samples have a given cell as their first candidate, a third of them at its cascade, and a cell that is not untrained keeps them: (2/3)^256 to miss one
    assert (tmp[:3 * K.CELLS][start[:3 * K.CELLS] >= 0] > 0).all() and (tmp[3 * K.CELLS:] == 0).all()
    rng, box = ngp.Pcg32(1337), (K.AABB[0][0], K.AABB[1][0])
    g = torch.from_numpy(start).to(dev)
    pos, idx = ngp.grid_samples(g, 4099, 0, 3, -0.01, rng, box)
    last = np.arange(n - 70, n, dtype=U32)
    want_pos, want_idx = K.grid_samples(n, 0, 3, -0.01, rng.state, rng.inc, *K.AABB, start, only=last)
    pos = torch.cat([pos, torch.from_numpy(want_pos).to(dev)])
    idx = torch.cat([idx, torch.from_numpy(want_idx.view(np.int32)).to(dev)])
    few = torch.zeros(K.N_CELLS_ALL, device=dev)
    ngp.grid_splat(idx, model.density_raw(pos), few)
    few = few.cpu().numpy()
    assert (few > 0).sum() > 4100 and (tmp >= few).all()
    assert np.array_equal(s.density_grid.cpu().numpy().view(U32), K.ema(tmp, start, 0.95).view(U32))


# ------------------------------------------------------------------------------------------------------------------ 6. driver
def test_driver_updates_builds_and_renders(setup):
    from jittor_myc_nerfs_amd import ngp
    model, _, _, dev = setup
    s = _sampler(model, dev)
    old_state = {k: v.clone() for k, v in s.state_dict().items()}    # what a checkpoint written before the feature holds
    assert sorted(old_state) == ["density_grid", "density_grid_bitfield", "density_grid_mean"]
    s.update_density_grid(0)
    first = s.density_grid.clone()
    assert s.density_grid_ema_step == 1 and float(first.max()) > 0
    s.update_density_grid(1)
    assert s.density_grid_ema_step == 2
    from oracle import ngp_oracle as N
    want = N.Pcg32(1337)
    for _ in range(4):
        want.advance()
    assert (s.rng.state, s.rng.inc) == want.state
    assert not torch.equal(first, s.density_grid)
    frac = s.build_density_grid(4)
    assert s.density_grid_ema_step == 4 and 0.0 < frac < 1.0
    bits0 = np.unpackbits(s.density_grid_bitfield[:K.CELLS // 8].cpu().numpy())
    assert frac == bits0.sum() / K.CELLS
    o, d = ngp_camera_rays(48, 48)
    rgb = s.render_frame(torch.from_numpy(o), torch.from_numpy(d))
    assert rgb.shape == (48 * 48, 3) and torch.isfinite(rgb).all()
    assert float((rgb - 1.0).abs().max()) > 0.05                      # not the bare background: the built grid lets the march find the scene
    assert list(s.state_dict().keys()) == ["density_grid", "density_grid_bitfield", "density_grid_mean"]
    s.load_state_dict(old_state)
    assert float(s.density_grid.abs().max()) == 0.0
    # the later policy: a quarter uniform, a quarter among the occupied cells, through both paths
    s.build_density_grid(1, *K.mark_cameras(3), K.MARK_RES)
    assert float(s.density_grid.min()) == -1.0
    s2 = _sampler(model, dev, s.density_grid)
    s2.rng.state, s2.density_grid_ema_step = s.rng.state, s.density_grid_ema_step
    s.update_density_grid(256)
    s2.update_density_grid(256, fused=False)
    assert np.array_equal(_bits(s.density_grid), _bits(s2.density_grid)) and torch.equal(s.density_grid_bitfield, s2.density_grid_bitfield)


# ------------------------------------------------------------------------------------------------------------------ 7. loud errors
def test_loud_errors(setup):
    from jittor_myc_nerfs_amd import _lib as L, ngp
    model, grid, _, dev = setup
    rng, box = ngp.Pcg32(1337), (K.AABB[0][0], K.AABB[1][0])
    cpu_grid = torch.zeros(K.N_CELLS_ALL)
    with pytest.raises(L.TvrError, match="GPU"):
        ngp.grid_samples(cpu_grid, 16, 0, 3, 0.01, rng, box)
    with pytest.raises(L.TvrError, match="GPU"):
        ngp.grid_mark_untrained(cpu_grid, *K.mark_cameras(1), K.MARK_RES)
    with pytest.raises(L.TvrError, match="GPU"):
        ngp.grid_splat(torch.zeros(4, dtype=torch.int32), torch.zeros(4), grid.clone())
    with pytest.raises(L.TvrError, match="GPU"):
        ngp.grid_ema(cpu_grid, grid.clone(), 0.95)
    with pytest.raises(L.TvrError, match="GPU"):
        ngp.DensityGridSampler(ngp.NGPNetworks(1), 1, rng=ngp.Pcg32(1337)).update_density_grid(0)
    for nc in (0, 6):
        with pytest.raises(L.TvrError, match="n_cascades"):
            ngp.grid_samples(grid, 16, 0, nc, 0.01, rng, box)
    s = _sampler(model, dev)
    for nc in (0, 6):
        with pytest.raises(L.TvrError, match="n_cascades"):
            ngp.grid_update(model, s.density_grid, s._tmp(), s.density_grid_bitfield, s.density_grid_mean, box, 64, 0, 0, nc, 0.95, rng)
    with pytest.raises(L.TvrError, match="density_grid_tmp too small"):
        ngp.grid_update(model, s.density_grid, torch.zeros(K.N_CELLS_ALL - 1, device=dev), s.density_grid_bitfield, s.density_grid_mean, box, 64, 0, 0, 3, 0.95, rng)
    with pytest.raises(L.TvrError):
        ngp.grid_update(model, s.density_grid, s._tmp(), s.density_grid_bitfield, s.density_grid_mean, box, -1, 0, 0, 3, 0.95, rng)
    assert float(s.density_grid.abs().max()) == 0.0 and s.density_grid_ema_step == 0      # refused before anything ran
    with pytest.raises(NotImplementedError):
        s.sample(None, torch.zeros(1, 3), torch.ones(1, 3), is_training=True)
