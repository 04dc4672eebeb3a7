"""GPU (-m gpu): the trimmed volume march (csrc/tvr_march.hip march_vol_kernel<DENSE, PLAIN>, csrc/tvr_march_body.h).

A plain scene's frames run the PLAIN instantiation (no alpha volume, no explicit depths, no lam6, 32-bit volume offsets); `dense=True`, explicit depths and lam6 run the
general ones.  A1 / A3 hold the forms against each other bit for bit, A2 pins the order of the transmittance scan's products against a host restatement (so no parent
build is needed), B1 measures the volume marches' own exp / softplus against fp64 with OCML-class fp32 functions (numpy's) as the yardstick."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import TINY, make_model
from test_gpu_density_volume import ODD, _face_rays, scene_b  # noqa: F401  (scene_b: the 2013-ray, 126-tile case of test_invariances_bit_for_bit)
from test_gpu_parity import _np

pytestmark = pytest.mark.gpu


FINE = 0.15                                                 # step_ratio of the *_fine models: a ray crosses the box in up to ~160 samples instead of 48,
                                                            # so that 65 and 130 samples carry a transmittance below 1 across one and two chunk boundaries


@pytest.fixture(scope="module")
def models(tiny_arrays, hyper_tiny):
    from jittor_myc_nerfs_amd import synthetic
    odd = synthetic.make_scene_arrays(ODD["gridSize"], ODD["aabb"], seed=3)
    fine = dict(hyper_tiny, step_ratio=FINE)
    return dict(tiny=make_model(tiny_arrays, hyper_tiny), odd=make_model(odd, hyper_tiny), tiny_fine=make_model(tiny_arrays, fine), odd_fine=make_model(odd, fine))


@pytest.fixture(scope="module")
def rays64(tiny_dump, tiny_edge):
    """64 rays (four tiles): the five face / edge / corner rays, one that misses the box, 58 of the tiny dump's."""
    r = np.concatenate([_face_rays(TINY["aabb"]), tiny_edge["rays"][3:4], tiny_dump["rays"][:58]]).astype(np.float32)
    assert r.shape == (64, 6)
    return torch.tensor(r, device="cuda")


def _jitter(n, seed):
    return torch.rand(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def _render_z(m, rays, z, S, eps_T, white_bg=True):
    """tvr_render_z on the model's scene: explicit depths AND lam6, i.e. march_vol_kernel<false, false>."""
    from jittor_myc_nerfs_amd import _lib as L
    sc, lib = m._ensure_scene(), L.lib()
    n = rays.shape[0]
    rgb, depth, lam = torch.empty((n, 3), device="cuda"), torch.empty((n,), device="cuda"), torch.empty((n,), device="cuda")
    scratch = m._get_scratch(lib.tvr_render_scratch_bytes(sc, n, S))
    L.check(lib.tvr_render_z(sc, rays.data_ptr(), n, S, int(white_bg), z.data_ptr(), float(eps_T), rgb.data_ptr(), depth.data_ptr(), lam.data_ptr(), scratch.data_ptr(),
                             scratch.numel(), None, None, torch.cuda.current_stream().cuda_stream), "tvr_render_z")
    return rgb, depth


@pytest.mark.parametrize("which", ["tiny", "odd", "tiny_fine", "odd_fine"])
@pytest.mark.parametrize("S", [48, 65, 130])               # a partial chunk, one chunk carry, two
def test_a1_plain_equals_general_bit_for_bit(models, rays64, hyper_tiny, which, S):
    m = models[which]
    for jit in (None, _jitter(64, S)):
        for eps in (0.0, None):
            rgb, depth = (t.clone() for t in m.render_rays(rays64, white_bg=True, N_samples=S, jitter=jit, eps_T=eps))               # plain
            rgb_d, depth_d, d = m.render_rays(rays64, white_bg=True, N_samples=S, jitter=jit, eps_T=eps, dense=True)               # general, DENSE
            assert m._dvol is not None
            assert torch.equal(rgb, rgb_d) and torch.equal(depth, depth_d), (which, S, jit is not None, eps)
            # general, not DENSE: the same depths handed in explicitly.  Bit-equal by construction: sample j's far end z1 = tmin + step (float(j + 1) + u) is
            # sample j + 1's z, so z[j + 1] - z[j] is the distance the uniform form computes, and positions, masks and cells come from the same z
            e = eps if eps is not None else (m.eps_T if m.eps_T is not None else float(m.rayMarch_weight_thres))
            rgb_z, depth_z = _render_z(m, rays64, d["z"].contiguous(), S, e)
            assert torch.equal(rgb, rgb_z) and torch.equal(depth, depth_z), (which, S, jit is not None, eps, "explicit depths")
    assert bool((rgb < 0.99).any()) and bool((rgb[5] == 1.0).all())                                      # the scene is seen; ray 5 misses the box


def _host_weights(alpha):
    """weight[n, S] from alpha[n, S] in fp32 as the kernel forms it: fT = (1 - alpha) + 1e-10 per sample (1 in the lanes behind S), per 64-sample chunk the
    Hillis-Steele products x[l] <- x[l] * x[l - off] for off = 1, 2, 4, 8, 16, 32, T carried across the chunks, weight = alpha * (T * exclusive product)."""
    n, S = alpha.shape
    chunks = (S + 63) // 64
    a = np.zeros((n, chunks * 64), np.float32)
    a[:, :S] = alpha
    fT = ((np.float32(1.0) - a) + np.float32(1e-10)).astype(np.float32).reshape(n, chunks, 64)
    T = np.ones((n,), np.float32)
    w = np.empty((n, chunks, 64), np.float32)
    for c in range(chunks):
        x = fT[:, c].copy()
        for off in (1, 2, 4, 8, 16, 32):
            nx = x.copy()
            nx[:, off:] = x[:, off:] * x[:, :-off]
            x = nx
        excl = np.concatenate([np.ones((n, 1), np.float32), x[:, :-1]], axis=1)
        w[:, c] = a.reshape(n, chunks, 64)[:, c] * (T[:, None] * excl)
        T = T * x[:, 63]
    return w.reshape(n, chunks * 64)[:, :S], T


@pytest.mark.parametrize("which", ["tiny", "odd", "tiny_fine", "odd_fine"])
def test_a2_scan_order_is_pinned(models, rays64, which):
    m, S = models[which], 130
    for jit in (None, _jitter(64, 7)):
        _, _, d = m.render_rays(rays64, white_bg=True, N_samples=S, jitter=jit, eps_T=0.0, dense=True)
        alpha, weight = _np(d["alpha"]), _np(d["weight"])
        want, T = _host_weights(alpha)
        assert (weight > 0).sum() > 100                                                                        # the scene is seen
        if which == "tiny_fine":                                                                               # ... and behind both chunk carries, with T < 1 carried
            assert ((weight[:, :64] > 0).any(1) & (weight[:, 64:128] > 0).any(1) & (weight[:, 128:] > 0).any(1)).any()
        for j in (0, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80, 127, 128, 129):                                   # row, half and chunk boundaries
            assert np.array_equal(weight[:, j], want[:, j]), (which, j)
        assert np.array_equal(weight, want)
        assert np.array_equal(_np(d["bg_weight"]), T)


def _queue(m, n, S):
    """The march's per-ray counts and queue of the model's last single-launch-set call, read from its scratch."""
    from jittor_myc_nerfs_amd import _lib as L
    lay = L.ScratchLayout()
    L.check(L.lib().tvr_scratch_describe(n, S, C.byref(lay)), "tvr_scratch_describe")
    torch.cuda.synchronize()
    b = m._scratch
    u32 = lambda off, cnt: b[off:off + 4 * cnt].view(torch.int32).clone()
    total = int(u32(lay.counter, 1)[0])
    return dict(total=total, ray_off=u32(lay.ray_off, n), ray_cnt=u32(lay.ray_cnt, n), q_ray=u32(lay.q_ray, total), q_j=u32(lay.q_j, total),
                q_pos=b[lay.q_pos:lay.q_pos + 16 * total].view(torch.int32).view(total, 4).clone())


def _by_ray(q, n):
    """The queue in ray order (the order of the segments depends on which wave finished first; inside a segment the entries are in sample order)."""
    idx = torch.cat([torch.arange(int(o), int(o) + int(c), device="cuda") for o, c in zip(q["ray_off"].tolist(), q["ray_cnt"].tolist())]) if q["total"] else torch.zeros(0, dtype=torch.long, device="cuda")
    return idx


@pytest.mark.parametrize("which,S", [("tiny", 48), ("tiny_fine", 130), ("odd", 65), ("odd_fine", 130)])
def test_a3_counters_and_queue(models, rays64, hyper_tiny, which, S):
    m, n = models[which], 64
    for jit in (None, _jitter(64, 3)):
        m.render_rays(rays64, white_bg=True, N_samples=S, jitter=jit)
        p = _queue(m, n, S)                                                               # plain (no q_j: only `dense` calls with an rgb output write it)
        _, _, d = m.render_rays(rays64, white_bg=True, N_samples=S, jitter=jit, dense=True)
        g = _queue(m, n, S)
        assert p["total"] == g["total"] > 100 and int(p["ray_cnt"].sum()) == p["total"]
        assert torch.equal(p["ray_cnt"], g["ray_cnt"])
        ip, ig = _by_ray(p, n), _by_ray(g, n)
        assert torch.equal(p["q_ray"][ip], g["q_ray"][ig]) and torch.equal(p["q_pos"][ip], g["q_pos"][ig])        # the same entries: ray, position and weight bits
        # ... and the dense call's (ray, j) pairs are exactly the samples above the threshold, in sample order
        app = d["weight"] > float(hyper_tiny["rayMarch_weight_thres"])
        rj = torch.nonzero(app)
        assert torch.equal(g["q_ray"][ig].long(), rj[:, 0]) and torch.equal(g["q_j"][ig].long(), rj[:, 1])
        assert torch.equal(g["ray_cnt"].long(), app.sum(1))


def test_a3_invariances_of_the_plain_form(scene_b):
    m, rays, S, rgb, depth = (scene_b[k] for k in ("m", "rays", "S", "rgb", "depth"))
    again = m.render_rays(rays, white_bg=True, N_samples=S)
    assert torch.equal(again[0], rgb) and torch.equal(again[1], depth)
    parts = [m.render_rays(rays[a:a + 500], white_bg=True, N_samples=S) for a in range(0, rays.shape[0], 500)]
    assert torch.equal(torch.cat([p[0] for p in parts]), rgb) and torch.equal(torch.cat([p[1] for p in parts]), depth)
    perm = torch.randperm(rays.shape[0], device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    rp, dp = m.render_rays(rays[perm].contiguous(), white_bg=True, N_samples=S)
    assert torch.equal(rp, rgb[perm]) and torch.equal(dp, depth[perm])
    m.render_piece_rays = 256
    try:
        pieces = m.render_rays(rays, white_bg=True, N_samples=S)
        assert torch.equal(pieces[0], rgb) and torch.equal(pieces[1], depth)
    finally:
        m.render_piece_rays = 0
    rd, dd, _ = m.render_rays(rays, white_bg=True, N_samples=S, dense=True)
    assert torch.equal(rd, rgb) and torch.equal(dd, depth)
    jit = _jitter(rays.shape[0], 5)
    rj, dj = m.render_rays(rays, white_bg=True, N_samples=S, jitter=jit)
    rjd, djd, _ = m.render_rays(rays, white_bg=True, N_samples=S, jitter=jit, dense=True)
    assert torch.equal(rj, rjd) and torch.equal(dj, djd) and not torch.equal(rj, rgb)


def test_b1_lean_exp_and_softplus_against_fp64(tiny_arrays, hyper_tiny, rays64):
    """The tiny scene with its density planes scaled by (8, -6, -2), at the fine step: sigma_feature + density_shift spans about -32 .. +25 — across the x > 20 branch,
    and below -16.6, where 1 + e^x rounds to 1.  sigma and alpha of a dense render against softplus and 1 - exp(-sigma dist scale) in fp64 from the call's own sigma_feature and z; the
    yardstick is the error of numpy's fp32 log1p(exp(.)) and exp on the same inputs (a stand-in for OCML's, which the other kernels call): the kernel's worst relative
    error in sigma and worst absolute error in alpha may be 4 times the stand-in's (two 1-ulp hardware functions and a reciprocal compound), and in any case stay inside
    the bounds test_gpu_parity._check_dense holds sigma and alpha to."""
    arrs = dict(tiny_arrays)
    for i, k in enumerate((8.0, -6.0, -2.0)):
        arrs[f"density_plane.{i}"] = (tiny_arrays[f"density_plane.{i}"] * np.float32(k)).astype(np.float32)
    m = make_model(arrs, dict(hyper_tiny, step_ratio=FINE))
    shift, scale = float(hyper_tiny["density_shift"]), float(hyper_tiny["distance_scale"])
    S = 130
    _, _, d = m.render_rays(rays64, white_bg=True, N_samples=S, jitter=_jitter(64, 11), eps_T=0.0, dense=True)
    assert m._dvol is not None
    sf, z, sigma, alpha, valid = _np(d["sigma_feature"]), _np(d["z"]), _np(d["sigma"]), _np(d["alpha"]), _np(d["valid"]).astype(bool)
    x32 = (sf + np.float32(shift)).astype(np.float32)
    assert x32[valid].min() < -17.0 and x32[valid].max() > 20.0 and ((x32[valid] > -16.0) & (x32[valid] < 20.0)).sum() > 500
    dist32 = np.zeros_like(z)
    dist32[:, :-1] = z[:, 1:] - z[:, :-1]
    # fp64, from sigma_feature and z
    x64 = sf.astype(np.float64) + shift
    s64 = np.where(valid, np.where(x64 > 20.0, x64, np.log1p(np.exp(np.minimum(x64, 20.0)))), 0.0)
    a64 = -np.expm1(-s64 * dist32.astype(np.float64) * scale)
    # the stand-in: the same two quantities as the parent's kernel forms them, in numpy fp32
    with np.errstate(over="ignore"):
        s32 = np.where(valid, np.where(x32 > 20.0, x32, np.log1p(np.exp(np.minimum(x32, np.float32(20.0))))), np.float32(0.0)).astype(np.float32)
    a32 = (np.float32(1.0) - np.exp(-s32 * (dist32 * np.float32(scale)).astype(np.float32))).astype(np.float32)
    assert s32.dtype == np.float32 and a32.dtype == np.float32
    rel = lambda s: float((np.abs(s.astype(np.float64) - s64)[valid] / s64[valid]).max())
    err_s, ref_s = rel(sigma), rel(s32)
    err_a, ref_a = float(np.abs(alpha.astype(np.float64) - a64).max()), float(np.abs(a32.astype(np.float64) - a64).max())
    # (for information: the functions alone, i.e. against fp64 of the rounded fp32 argument the kernel and the stand-in both start from)
    sx = np.where(valid, np.where(x32 > 20.0, x32.astype(np.float64), np.log1p(np.exp(np.minimum(x32.astype(np.float64), 20.0)))), 0.0)
    fn = lambda s: float((np.abs(s.astype(np.float64) - sx)[valid] / sx[valid]).max() / 2.0 ** -24)
    print(f"    sigma: worst relative error {err_s:.3g} (numpy fp32 {ref_s:.3g}); alpha: worst absolute error {err_a:.3g} (numpy fp32 {ref_a:.3g}); "
          f"softplus alone, in units of 2^-24: kernel {fn(sigma):.2f}, numpy fp32 {fn(s32):.2f}; x in [{x32[valid].min():.1f}, {x32[valid].max():.1f}], {int(valid.sum())} samples")
    assert not sigma[~valid].any() and np.isfinite(sigma).all() and np.isfinite(alpha).all()
    assert err_s <= 4.0 * ref_s
    assert err_a <= 4.0 * ref_a
    assert np.abs(sigma.astype(np.float64) - s64).max() <= 1e-4 * max(1.0, s64.max()) and err_a < 2e-6
