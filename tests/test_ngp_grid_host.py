"""CPU: the numpy restatement of the occupancy-grid update (tests/ngp_grid_common.py) against the scalar pcg32 and hand-made grids, the power of the
inputs tests/test_gpu_ngp_grid.py uses, the argument checks of the new C calls (no GPU is touched), and the unchanged state dict."""
import ctypes as C

import numpy as np
import torch

import ngp_grid_common as K
from conftest import NGP_AABB_SCALE

F, U32 = np.float32, np.uint32


def _scalar_draws(state, inc, delta, n):
    from jittor_myc_nerfs_amd import ngp
    r = ngp.Pcg32(1337)
    r.state, r.inc = int(state), int(inc)
    r.advance(int(delta))
    return [r.next_uint() for _ in range(n)], r.state


def test_vectorised_pcg32_equals_the_scalar_generators():
    from jittor_myc_nerfs_amd import ngp
    from oracle import ngp_oracle as N
    a, b = ngp.Pcg32(1337), ngp.Pcg32(1337)
    assert N.Pcg32(1337).state == (a.state, a.inc)
    b.advance()
    rng = np.random.default_rng(3)
    for state, inc in ((a.state, a.inc), (b.state, b.inc)):
        delta = np.concatenate([np.arange(0, 260, dtype=np.uint64) * np.uint64(4), rng.integers(0, 1 << 34, 140).astype(np.uint64),
                                np.array([1 << 32, (1 << 32) + 4, (1 << 63) + 5], np.uint64)])
        st = K.pcg_advance(state, inc, delta)
        draws = []
        for _ in range(4):
            st, u = K.pcg_next_uint(st, inc)
            draws.append(u)
        st2, f = K.pcg_next_float(st, inc)
        for k, d in enumerate(delta):
            want, _ = _scalar_draws(state, inc, d, 5)
            assert [int(x[k]) for x in draws] == want[:4], f"delta {d}"
            assert f[k] == F(np.array([(want[4] >> 9) | 0x3F800000], U32).view(F)[0] - F(1))
            if state == a.state and k % 16 == 0:                     # the C oracle's generator, stepped one by one
                o = N.Pcg32(1337)
                o.advance(int(d))
                assert [o.next_uint() for _ in range(4)] == want[:4]
        assert 0 <= f.min() and f.max() < 1
    # ngp.Pcg32.advance is the same jump
    c = ngp.Pcg32(1337)
    c.advance(12345)
    assert c.state == int(K.pcg_advance(a.state, a.inc, [12345])[0])


def _hand_grid(occupied=()):
    g = np.zeros(K.N_CELLS_ALL, F)
    for c in occupied:
        g[c] = 1.0
    return g


def _candidates(i, n, ema_step, level):
    return [((((i + ema_step * n) * 56924617 + j * 19349663 + 96925573) & K.M32) % K.CELLS) + level * K.CELLS for j in range(10)]


def test_generator_on_hand_made_grids():
    from jittor_myc_nerfs_amd import ngp
    r = ngp.Pcg32(1337)
    lo, hi = K.AABB
    n = 257
    # an empty grid with thresh 0.01: nothing breaks, the TENTH index is kept; with thresh -0.01 every first probe breaks
    pos, idx, broke = K.grid_samples(n, 0, 3, 0.01, r.state, r.inc, lo, hi, _hand_grid(), want_break=True)
    assert (broke == 10).all()
    levels = idx // K.CELLS
    assert set(levels.tolist()) == {0, 1, 2}
    for i in (0, 1, 100, 256):
        assert int(idx[i]) == _candidates(i, n, 0, int(levels[i]))[9]
    pos0, idx0, broke0 = K.grid_samples(n, 0, 3, -0.01, r.state, r.inc, lo, hi, _hand_grid(), want_break=True)
    assert (broke0 == 0).all() and all(int(idx0[i]) == _candidates(i, n, 0, int(idx0[i]) // K.CELLS)[0] for i in (0, 7, 256))
    assert np.array_equal(idx0 // K.CELLS, levels)                   # the level does not depend on the grid
    # the position lies in the chosen cell of the chosen cascade, warped to the aabb
    for p, ix in ((pos, idx), (pos0, idx0)):
        lv = (ix // K.CELLS).astype(np.int32)
        unit = (p.astype(np.float64) * K.AABB_SCALE + lo[0] - 0.5) / np.ldexp(1.0, lv)[:, None] + 0.5
        cell = np.stack(K.cell_xyz(ix % U32(K.CELLS)), 1)
        assert (np.floor(unit * K.G + 1e-4) >= cell).all() and (np.floor(unit * K.G - 1e-4) <= cell).all()
    # one occupied cell: exactly the samples that have it among their candidates (at their level) break there, at its first occurrence
    i_pick, j_pick = 100, 6
    cell = _candidates(i_pick, n, 0, int(levels[i_pick]))[j_pick]
    _, idx1, broke1 = K.grid_samples(n, 0, 3, 0.01, r.state, r.inc, lo, hi, _hand_grid([cell]), want_break=True)
    assert broke1[i_pick] == j_pick and idx1[i_pick] == cell
    for i in range(n):
        cand = _candidates(i, n, 0, int(levels[i]))
        if cell in cand:
            assert broke1[i] == cand.index(cell) and idx1[i] == cell
        else:
            assert broke1[i] == 10 and idx1[i] == cand[9]
    # ema_step values at which (i + ema_step * n) and its product wrap uint32
    big_n = 4099
    for step in (0, 3, (1 << 32) // big_n + 1, 0xFFFFFFFF):
        _, ix, _ = K.grid_samples(big_n, step, 1, -0.01, r.state, r.inc, lo, hi, _hand_grid(), want_break=True)
        assert ((step * big_n) >> 32 > 0) == (step >= (1 << 32) // big_n + 1)
        for i in (0, 1, 4098):
            assert int(ix[i]) == _candidates(i, big_n, step, 0)[0]
    # the second call sees the generator one host advance later: other levels and positions, same index hash
    r2 = ngp.Pcg32(1337)
    r2.advance()
    pos2, idx2 = K.grid_samples(n, 0, 3, -0.01, r2.state, r2.inc, lo, hi, _hand_grid())
    assert not np.array_equal(idx2 // K.CELLS, levels) and np.array_equal(idx2 % K.CELLS, idx0 % K.CELLS)


def test_inputs_of_the_gpu_tests_have_power(ngp_scene):
    """The fixture's grid makes the generator take both exits of the probe loop often, and the cameras split every cascade."""
    from jittor_myc_nerfs_amd import ngp
    _, arrs = ngp_scene
    r = ngp.Pcg32(1337)
    lo, hi = K.AABB
    _, idx, broke = K.grid_samples(4099, 0, 3, 0.01, r.state, r.inc, lo, hi, arrs["density_grid"], want_break=True)
    assert (broke < 10).sum() >= 100 and (broke == 10).sum() >= 100
    assert ((broke > 0) & (broke < 10)).sum() >= 100                 # and breaks behind the first probe
    for n_cam in (3, 1):
        seen = K.cells_seen(*K.mark_cameras(n_cam), K.MARK_RES).reshape(5, K.CELLS)
        for c in range(5):
            assert 0 < seen[c].sum() < K.CELLS, f"{n_cam} cameras, cascade {c}: {seen[c].sum()} cells seen"
    g = K.mixed_grid()
    out = K.mark_untrained(g, *K.mark_cameras(3), K.MARK_RES)
    seen = K.cells_seen(*K.mark_cameras(3), K.MARK_RES)
    assert ((g > 0) & seen).sum() > 1000 and ((g < 0) & seen).sum() > 1000 and ((g >= 0) & ~seen).sum() > 1000
    assert np.array_equal(out[(g > 0) & seen], g[(g > 0) & seen]) and (out[(g < 0) & seen] == 0).all() and (out[~seen] == -1).all()


def test_max_pool_can_set_the_bit_of_an_untrained_coarse_cell():
    """Why tests/test_gpu_ngp_grid.py asserts 'the bit of a -1 cell is 0' for cascade 0 only and compares coarser cascades with the pool: with every seen
    cell occupied, update_bitfield's max-pool (the C oracle's, which the HIP call matches bit for bit) sets bits of cells that no camera sees."""
    from oracle import ngp_oracle as N
    seen = K.cells_seen(*K.mark_cameras(3), K.MARK_RES)
    bits, _ = N.update_bitfield(np.where(seen, F(1), F(-1)))
    stray = (np.unpackbits(bits, bitorder="little").astype(bool) & ~seen).reshape(5, K.CELLS).sum(1)
    assert stray[0] == 0 and stray[1:].sum() > 0, stray


def test_splat_and_ema_restatement():
    idx = np.array([5, 5, 9, K.N_CELLS_ALL - 1], U32)
    raw = np.array([0.0, 1.0, -2.0, 3.0], F)
    tmp = K.splat64(idx, raw)
    assert tmp[5] == np.exp(1.0) * float(K.MIN_CONE_STEPSIZE) and tmp[9] == np.exp(-2.0) * float(K.MIN_CONE_STEPSIZE) and tmp[0] == 0
    assert np.count_nonzero(tmp) == 3
    g = np.array([-1.0, 0.0, 2.0, 0.5], F)
    t = np.array([9.0, 0.25, 1.0, 0.5], F)
    assert K.ema(t, g, 0.95).tolist() == [-1.0, 0.25, float(F(2.0) * F(0.95)), 0.5]


def test_new_calls_refuse_bad_arguments_without_gpu():
    from jittor_myc_nerfs_amd import _lib as L, ngp
    lib = L.lib()
    P = 0x1000                                                        # never dereferenced: every case below is refused on the host
    lo, hi = (C.c_float * 3)(-1.5, -1.5, -1.5), (C.c_float * 3)(2.5, 2.5, 2.5)
    offsets, scale, _ = ngp.grid_levels(NGP_AABB_SCALE)
    cfg = ngp._grid_cfg(offsets, scale)
    inc = ngp.Pcg32(1337).inc
    INVALID, SCRATCH = -1, -3
    # mark-untrained
    assert lib.tvr_ngp_grid_mark_untrained(None, 1, P, P, 800, 800, None) == INVALID and b"NULL" in lib.tvr_last_error()
    assert lib.tvr_ngp_grid_mark_untrained(P, 1, None, P, 800, 800, None) == INVALID
    assert lib.tvr_ngp_grid_mark_untrained(P, 1, P, None, 800, 800, None) == INVALID
    assert lib.tvr_ngp_grid_mark_untrained(P, -1, P, P, 800, 800, None) == INVALID
    assert lib.tvr_ngp_grid_mark_untrained(P, 1, P, P, 0, 800, None) == INVALID
    # the generator
    args = lambda n=16, nc=3, i=inc, a=C.byref(lo), b=C.byref(hi), g=P, p=P, x=P: (n, 0, nc, 0.01, 1, i, a, b, g, p, x, None)
    for nc in (0, 6, -1):
        assert lib.tvr_ngp_grid_samples(*args(nc=nc)) == INVALID and b"n_cascades" in lib.tvr_last_error()
    assert lib.tvr_ngp_grid_samples(*args(n=-1)) == INVALID and lib.tvr_ngp_grid_samples(*args(n=1 << 30)) == INVALID
    assert b"sample count" in lib.tvr_last_error()
    assert lib.tvr_ngp_grid_samples(*args(n=(1 << 30) - 1, g=None)) == INVALID and b"NULL" in lib.tvr_last_error()    # the largest count passes the count check
    assert lib.tvr_ngp_grid_samples(*args(i=2)) == INVALID and b"odd" in lib.tvr_last_error()
    assert lib.tvr_ngp_grid_samples(*args(a=None)) == INVALID and lib.tvr_ngp_grid_samples(*args(a=C.byref(hi))) == INVALID
    assert lib.tvr_ngp_grid_samples(*args(g=None)) == INVALID and lib.tvr_ngp_grid_samples(*args(p=None)) == INVALID
    assert lib.tvr_ngp_grid_samples(*args(x=None)) == INVALID
    assert lib.tvr_ngp_grid_samples(*args(n=0, g=None)) == 0          # nothing to do
    # the density head
    assert lib.tvr_ngp_density(None, P, P, P, 3, 4, None, P, None) == INVALID
    assert lib.tvr_ngp_density(C.byref(cfg), None, P, P, 3, 4, None, P, None) == INVALID
    assert lib.tvr_ngp_density(C.byref(cfg), P, None, P, 3, 4, None, P, None) == INVALID
    assert lib.tvr_ngp_density(C.byref(cfg), P, P, None, 3, 4, None, P, None) == INVALID
    assert lib.tvr_ngp_density(C.byref(cfg), P, P, P, 3, 4, None, None, None) == INVALID
    assert lib.tvr_ngp_density(C.byref(cfg), P, P, P, 2, 4, None, P, None) == INVALID and b"pos_stride" in lib.tvr_last_error()
    assert lib.tvr_ngp_density(C.byref(cfg), P, P, P, 3, -4, None, P, None) == INVALID
    assert lib.tvr_ngp_density(C.byref(cfg), P, P + 4, P, 3, 4, None, P, None) == INVALID      # misaligned weight image
    # splat and ema
    assert lib.tvr_ngp_grid_splat(None, P, 4, P, None) == INVALID and lib.tvr_ngp_grid_splat(P, None, 4, P, None) == INVALID
    assert lib.tvr_ngp_grid_splat(P, P, 4, None, None) == INVALID and lib.tvr_ngp_grid_splat(P, P, -4, P, None) == INVALID
    assert lib.tvr_ngp_grid_ema(None, P, 0.95, None) == INVALID and lib.tvr_ngp_grid_ema(P, None, 0.95, None) == INVALID
    # the fused update
    full = K.N_CELLS_ALL * 4

    def upd(a=C.byref(lo), b=C.byref(hi), c=C.byref(cfg), hashgrid=P, net=P, grid=P, tmp=P, nbytes=full, bits=P, mean=P, nu=64, nn=64, nc=3, i=inc):
        return lib.tvr_ngp_grid_update(a, b, c, hashgrid, net, grid, tmp, nbytes, bits, mean, nu, nn, 0, nc, 0.95, 1, i, None)
    assert upd(nbytes=full - 4) == SCRATCH and b"density_grid_tmp" in lib.tvr_last_error()
    assert upd(tmp=None) == SCRATCH
    for kw in (dict(nu=1 << 30), dict(nn=1 << 30)):
        assert upd(**kw) == INVALID and b"sample count" in lib.tvr_last_error(), kw
    for kw in (dict(nu=(1 << 30) - 1, grid=None), dict(nn=(1 << 30) - 1, grid=None), dict(nu=(1 << 29) + 2, grid=None)):      # accepted counts: refused for the NULL only
        assert upd(**kw) == INVALID and b"NULL" in lib.tvr_last_error(), kw
    for kw in (dict(a=None), dict(b=None), dict(c=None), dict(hashgrid=None), dict(net=None), dict(grid=None), dict(bits=None), dict(mean=None),
               dict(nu=-1), dict(nn=-1), dict(nn=1 << 30), dict(nc=0), dict(nc=6), dict(i=4), dict(net=P + 8), dict(a=C.byref(hi))):
        assert upd(**kw) == INVALID, kw


def test_state_dict_keys_are_unchanged():
    from jittor_myc_nerfs_amd import ngp
    model = ngp.NGPNetworks(1)
    s = ngp.DensityGridSampler(model, 1, rng=ngp.Pcg32(1337))
    assert list(s.state_dict().keys()) == ["density_grid", "density_grid_bitfield", "density_grid_mean"]
    assert s.density_grid_ema_step == 0 and isinstance(s.density_grid_ema_step, int) and s.density_grid_tmp is None
    assert [ngp.DensityGridSampler(model, a).max_cascade for a in (1, 2, 4, 8, 16)] == [0, 1, 2, 3, 4]
    old = {"density_grid": torch.ones(K.N_CELLS_ALL), "density_grid_bitfield": torch.zeros(K.N_CELLS_ALL // 8, dtype=torch.uint8),
           "density_grid_mean": torch.zeros(1)}
    s.load_state_dict(old)                                           # strict: a state dict saved before the feature
    assert float(s.density_grid[5]) == 1.0


def test_nerf_rays_hands_out_the_training_views(tmp_path):
    import json
    from jittor_myc_nerfs_amd import ngp, rays as R
    poses = R.sphere_poses(4, 4.0)
    meta = {"camera_angle_x": 0.6911, "frames": [{"transform_matrix": np.asarray(p).tolist()} for p in poses]}
    (tmp_path / "transforms_test.json").write_text(json.dumps(meta))
    nr = ngp.NerfRays(str(tmp_path), H=40, W=60)
    focal, xforms, res = nr.training_views()
    assert focal.shape == (4, 2) and focal.dtype == np.float32 and xforms.shape == (4, 3, 4) and xforms.dtype == np.float32 and res == (60, 40)
    assert np.array_equal(xforms[2], nr.transforms[2]) and focal[1].tolist() == [F(nr.focal[0]), F(nr.focal[1])]
