"""GPU (-m gpu): the volume marches reserve queue space once per batch of rays (csrc/tvr_march_body.h MARCH_BATCH, march_flush).

A wave keeps the appearance lists of up to MARCH_PEND finished rays in its LDS list — a ring of S entries — and reserves once for all of them; the waiting rays leave
before a chunk of the ray in progress that may need their room.  What must hold: every ray's pixels, count and queue segment are those of the same ray rendered in a call
of its own (a call of one ray can never batch), the queue is contiguous and exact, and the invariances of the plain form stay bit for bit.  A wave marches several rays
only in a launch of more rays than the card has waves for (16 per compute unit), so the cases repeat their 128 or 79 rays until there are four per wave.  Every case first shows from
a `dense=True` render of the same call that it is not vacuous."""
import numpy as np
import pytest
import torch

from conftest import TINY, make_model
from test_gpu_density_volume import _face_rays, scene_b  # noqa: F401
from test_gpu_march_trim import FINE, _jitter, _queue, rays64  # noqa: F401

pytestmark = pytest.mark.gpu

MARCH_PEND = 8                                             # csrc/tvr_march_body.h
FOG_SCALE, FOG_SHIFT = 0.02, -3.94                         # chosen with the CPU oracle (oracle/c_oracle.py): the density planes times 0.02 leave sigma_feature within +-0.3,
                                                           # and softplus(-3.94) x step 0.0207 x distance_scale 25 = alpha 0.010 per sample (median 0.0100, max 0.018); behind
                                                           # 130 samples T = 0.27, so every in-box weight stays above the threshold 1e-4 by a factor of 25 or more


@pytest.fixture(scope="module")
def fog(tiny_arrays, hyper_tiny):
    """The tiny scene as fog, at the fine step (a ray along x crosses the box in 145 samples)."""
    arrs = dict(tiny_arrays)
    for i in range(3):
        arrs[f"density_plane.{i}"] = (tiny_arrays[f"density_plane.{i}"] * np.float32(FOG_SCALE)).astype(np.float32)
    m = make_model(arrs, dict(hyper_tiny, step_ratio=FINE, density_shift=FOG_SHIFT))
    m.render_piece_rays = 0
    return m


@pytest.fixture(scope="module")
def blob(tiny_arrays, hyper_tiny):
    """One grid node (8, 10, 12) of density feature 2 in an otherwise empty box: softplus(2 - 10) x step x 25 = alpha 5.8e-4 at the node, above the threshold within about
    0.9 cell of it — a ray along z (cells of 0.087, steps of 0.069) through the node's cell meets it in 1 - 3 samples (CPU oracle: 1 - 3 for all 49 rays below, with and
    without jitter, S = 48, 65, 130 and 192: the ray leaves the box after 29 samples)."""
    arrs = dict(tiny_arrays)
    for i in range(3):
        arrs[f"density_plane.{i}"] = np.zeros_like(tiny_arrays[f"density_plane.{i}"])
        arrs[f"density_line.{i}"] = np.zeros_like(tiny_arrays[f"density_line.{i}"])
    arrs["density_plane.0"][0, 0, 10, 8] = 2.0             # plane 0 is [1, C, gy, gx]
    arrs["density_line.0"][0, 0, 12, 0] = 1.0
    m = make_model(arrs, hyper_tiny)
    m.render_piece_rays = 0
    return m


MISS = np.asarray([-4.0, 3.0, 0.0, 1.0, 0.0, 0.0], np.float32)            # passes the box at y = 3


@pytest.fixture(scope="module")
def fog_rays(rays64):
    """128 rays: rays64 (face, edge and corner rays, one miss, 58 of the tiny dump's: chords of every length) interleaved with 64 rays along x, whose first 145 samples
    are all inside the box."""
    n = 64
    lr = [[-4.0, -1.0 + 2.0 * ((i * 7) % n) / (n - 1), -0.8 + 1.6 * ((i * 13) % n) / (n - 1), 1.0, 0.0, 0.0] for i in range(n)]
    r = torch.empty((128, 6), device="cuda")
    r[0::2] = rays64
    r[1::2] = torch.tensor(lr, device="cuda")
    return r.contiguous()


@pytest.fixture(scope="module")
def blob_rays():
    """49 grazing rays in a row (6 x MARCH_PEND), then 30 more places where a grazing ray alternates with a miss or one of the five face / edge / corner rays."""
    lo, hi = np.asarray(TINY["aabb"], np.float32)
    g = TINY["gridSize"]
    x8, y10 = np.linspace(lo[0], hi[0], g[0])[8], np.linspace(lo[1], hi[1], g[1])[10]
    graze = np.asarray([[x8 + 0.1 * u, y10 + 0.06 * v, -3.5, 0, 0, 1] for u in np.linspace(-0.9, 0.9, 7) for v in np.linspace(-0.9, 0.9, 7)], np.float32)
    face = _face_rays(TINY["aabb"])
    mixed = []
    for i in range(15):
        mixed += [graze[(i * 3) % 49], MISS if i % 3 else face[(i // 3) % 5]]
    return torch.tensor(np.concatenate([graze, np.stack(mixed)]).astype(np.float32), device="cuda")


def _call(m, rays, S, jit, eps, dense=False):
    """One call and what it left: pixels, the queue (read from the scratch), the call's TVR_STAT_APP; with dense, the per-sample arrays."""
    from jittor_myc_nerfs_amd import _lib as L
    stats = torch.zeros(L.STAT_COUNT, dtype=torch.int64, device="cuda")
    out = m.render_rays(rays, white_bg=True, N_samples=S, jitter=jit, eps_T=eps, dense=dense, stats=stats)
    q = _queue(m, rays.shape[0], S)
    return dict(rgb=out[0].clone(), depth=out[1].clone(), q=q, app=int(stats[L.STAT_APP]), dense=out[2] if dense else None)


def _copies(n, per_wave=4):
    """How often a set of n rays is repeated so that a launch has at least `per_wave` rays per wave of the march (16 waves per compute unit): only then does a wave hold
    finished rays while it marches the next, and the launcher picks the batched kernel at all (more rays than waves: csrc/tvr_march.hip launch_march_vol)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return -(-per_wave * 16 * cus // n)


def _rep(t, k):
    return None if t is None else t.repeat(k, *([1] * (t.dim() - 1))).contiguous()


def _by_ray_fast(q):
    cnt, off = q["ray_cnt"].long(), q["ray_off"].long()
    first = torch.cumsum(cnt, 0) - cnt
    return torch.repeat_interleave(off - first, cnt) + torch.arange(int(cnt.sum()), device="cuda")


def _check_queue(c, n, thres=None):
    """Issue, test 3: the counter is exact, the segments of the rays with entries tile [0, counter) without hole or overlap, q_ray is the ray on its segment; with the
    dense arrays, q_j is strictly increasing on a segment and names exactly the samples above the threshold."""
    q = c["q"]
    cnt, off = q["ray_cnt"].long(), q["ray_off"].long()
    assert int(cnt.sum()) == q["total"] == c["app"], (int(cnt.sum()), q["total"], c["app"])
    has = torch.nonzero(cnt > 0)[:, 0]
    order = has[torch.argsort(off[has])]
    ends = off[order] + cnt[order]
    if q["total"]:
        assert int(off[order][0]) == 0 and int(ends[-1]) == q["total"] and torch.equal(off[order][1:], ends[:-1])
    else:
        assert has.numel() == 0
    assert bool((off[cnt == 0] == 0).all())
    idx = _by_ray_fast(q)
    assert torch.equal(q["q_ray"][idx].long(), torch.repeat_interleave(torch.arange(n, device="cuda"), cnt))
    if c["dense"] is not None:
        rj = torch.nonzero(c["dense"]["weight"] > thres)                                     # (ray, j) in ray order, j increasing: strictly increasing q_j on a segment
        assert torch.equal(q["q_ray"][idx].long(), rj[:, 0]) and torch.equal(q["q_j"][idx].long(), rj[:, 1])
        assert torch.equal(cnt, (c["dense"]["weight"] > thres).sum(1))


def _check_against_single_ray_calls(c, k, singles):
    """Issue, tests 1 / 2 / 6: the call c renders k copies of a set of rays; `singles` are the same rays in calls of ONE ray each — a call of one ray can never batch
    (it runs the unbatched kernel).  rgb, depth, ray_cnt and every ray's q_pos segment, bit for bit."""
    q = c["q"]
    for i, one in enumerate(singles):
        assert int(one["q"]["ray_cnt"][0]) == one["q"]["total"] and bool((one["q"]["q_ray"] == 0).all()), i
    assert torch.equal(c["rgb"], torch.cat([o["rgb"] for o in singles]).repeat(k, 1)) and torch.equal(c["depth"], torch.cat([o["depth"] for o in singles]).repeat(k))
    assert torch.equal(q["ray_cnt"], torch.cat([o["q"]["ray_cnt"] for o in singles]).repeat(k))
    assert torch.equal(q["q_pos"][_by_ray_fast(q)], torch.cat([o["q"]["q_pos"] for o in singles]).repeat(k, 1))


def _case(m, rays, S, jit, eps, thres, k=None, extra=0):
    """k copies of `rays` (default: enough for 4 rays per wave) plus the first `extra` rays once more in ONE call: the call, its dense twin (of 4 rays per wave, where k
    asks for more: the dense arrays of a long call are large), the queue invariants of both, and the comparison with calls of one ray; returns the call, the dense
    twin's counts (the reference; its first rays are the set's), and k."""
    k4 = _copies(rays.shape[0])
    k = k4 if k is None else k
    big = torch.cat([_rep(rays, k), rays[:extra]]).contiguous()
    bjit = None if jit is None else torch.cat([_rep(jit, k), jit[:extra]]).contiguous()
    n = big.shape[0]
    assert n > 16 * torch.cuda.get_device_properties(0).multi_processor_count                # more rays than waves: the batched kernel
    if k == k4:
        d = _call(m, big, S, bjit, eps, dense=True)
        _check_queue(d, n, thres)
        ref_cnt = (d["dense"]["weight"] > thres).sum(1)
        want = ref_cnt
    else:
        d = _call(m, _rep(rays, k4), S, _rep(jit, k4), eps, dense=True)
        _check_queue(d, k4 * rays.shape[0], thres)
        ref_cnt = (d["dense"]["weight"] > thres).sum(1)
        assert extra == 0 and torch.equal(ref_cnt, ref_cnt[:rays.shape[0]].repeat(k4))
        want = ref_cnt[:rays.shape[0]].repeat(k)
        d = dict(rgb=d["rgb"][:rays.shape[0]].repeat(k, 1), depth=d["depth"][:rays.shape[0]].repeat(k))
    c = _call(m, big, S, bjit, eps)
    assert torch.equal(c["rgb"], d["rgb"]) and torch.equal(c["depth"], d["depth"])
    _check_queue(c, n)
    assert torch.equal(c["q"]["ray_cnt"].long(), want)
    singles = [_call(m, rays[i:i + 1].contiguous(), S, None if jit is None else jit[i:i + 1].contiguous(), eps) for i in range(rays.shape[0])]
    if extra:
        m0 = k * rays.shape[0]
        head = dict(rgb=c["rgb"][:m0], depth=c["depth"][:m0], q=dict(c["q"], ray_cnt=c["q"]["ray_cnt"][:m0], ray_off=c["q"]["ray_off"][:m0]))
        _check_against_single_ray_calls(head, k, singles)
        tail = dict(rgb=c["rgb"][m0:], depth=c["depth"][m0:], q=dict(c["q"], ray_cnt=c["q"]["ray_cnt"][m0:], ray_off=c["q"]["ray_off"][m0:]))
        _check_against_single_ray_calls(tail, 1, singles[:extra])
    else:
        _check_against_single_ray_calls(c, k, singles)
    return c, ref_cnt, k


@pytest.mark.parametrize("S", [48, 65, 130])
def test_1_ring_wrap_and_flush_with_a_ray_in_progress(fog, fog_rays, hyper_tiny, S):
    thres = float(hyper_tiny["rayMarch_weight_thres"])
    for jit in (None, _jitter(128, S)):
        c, ref_cnt, k = _case(fog, fog_rays, S, jit, None, thres)
        one = ref_cnt[:128]
        assert int((one >= S - 8).sum()) >= 16                                  # not vacuous: a wave's next ray finds the ring (almost) full ...
        assert int(((one > 0) & (one < S // 2)).sum()) >= 4                     # ... and short lists stand between the full ones (CPU oracle: 6 / 7 / 14 such rays)
        assert k * 128 >= 4 * 16 * torch.cuda.get_device_properties(0).multi_processor_count          # ... and a wave takes several rays


@pytest.mark.parametrize("S", [48, 65, 130, 192])
def test_2_pending_cap(blob, blob_rays, hyper_tiny, S):
    """At S = 48 and 65 the waiting rays leave for room (a chunk asks for 64 free entries of S) long before MARCH_PEND of them wait; at S = 130 and 192 eight rays of at
    most 3 entries and a chunk's 64 fit, so ONLY the cap (and the end of the ray loop) flushes: there the call has 24 rays per wave, four out of five with entries, and a
    wave fills all MARCH_PEND records several times over.  The samples behind the box (the ray leaves it after 29) are outside: the counts do not depend on S."""
    thres = float(hyper_tiny["rayMarch_weight_thres"])
    n = blob_rays.shape[0]
    per_wave = 24 if S >= 130 else 4
    for jit in (None, _jitter(n, 40 + S)):
        c, ref_cnt, k = _case(blob, blob_rays, S, jit, None, thres, k=_copies(n, per_wave))
        one = ref_cnt[:n]
        assert bool(((one[:49] >= 1) & (one[:49] <= 3)).all()) and 49 >= 4 * MARCH_PEND                   # not vacuous: 49 rays of 1 - 3 entries in a row
        assert bool(((one[49::2] >= 1) & (one[49::2] <= 3)).all()) and bool((one[50::2] == 0).all())      # ... then alternating with rays without entries
        if S >= 130:
            # not vacuous for the CAP: whatever MARCH_PEND rays a wave holds, their entries and a chunk's 64 fit (the room rule cannot fire before the cap does),
            # and a wave marches on average 24 rays of which 64 in 79 have entries: far more than MARCH_PEND
            assert MARCH_PEND * int(one.max()) + 64 <= S
            waves = 16 * torch.cuda.get_device_properties(0).multi_processor_count
            assert k * int((one > 0).sum()) >= 2 * MARCH_PEND * waves


@pytest.mark.parametrize("extra", [1, 15, 16, 17])
def test_4_exits_final_flush_and_partial_tile(fog, fog_rays, hyper_tiny, extra):
    """Whole tiles of fog rays for 4 rays per wave, and 1 / 15 / 16 / 17 rays behind them: the launch ends in a partial tile, and waves leave the ray loop with one or a
    few rays waiting.  (Calls of 1 .. 17 rays alone run the unbatched kernel: they are the references of every case here.)"""
    thres, S = float(hyper_tiny["rayMarch_weight_thres"]), 65
    c, ref_cnt, k = _case(fog, fog_rays, S, None, None, thres, extra=extra)
    assert c["rgb"].shape[0] % 16 == extra % 16 and int((ref_cnt[-extra:] > 0).sum()) >= extra // 2 and int((ref_cnt[:128] >= S - 8).sum()) >= 16


@pytest.mark.parametrize("n", [1, 15, 16, 17])
def test_4_exits_calls_of_few_rays(fog, fog_rays, hyper_tiny, n):
    """Calls of 1, 15, 16 and 17 rays alone (one ray per wave: the unbatched kernel; a partial tile at 15 and 17): the queue invariants, plain and dense."""
    thres, S = float(hyper_tiny["rayMarch_weight_thres"]), 65
    rays = fog_rays[1:1 + n].contiguous()                                        # ray 1 runs along x: S - 1 entries
    d = _call(fog, rays, S, None, None, dense=True)
    assert int((d["dense"]["weight"][0] > thres).sum()) >= S - 8
    c = _call(fog, rays, S, None, None)
    _check_queue(d, n, thres)
    _check_queue(c, n)
    assert torch.equal(c["rgb"], d["rgb"]) and torch.equal(c["depth"], d["depth"]) and torch.equal(c["q"]["ray_cnt"], d["q"]["ray_cnt"])


def test_4_exits_every_ray_misses(fog):
    n = 4 * 16 * torch.cuda.get_device_properties(0).multi_processor_count + 40
    rays = torch.tensor(MISS, device="cuda").repeat(n, 1)
    rays[:, 1] += 0.001 * torch.arange(n, device="cuda")
    d = _call(fog, rays.contiguous(), 65, None, None, dense=True)
    assert not bool(d["dense"]["bbox_valid"].any())                              # not vacuous: no sample of the call is inside the box
    c = _call(fog, rays.contiguous(), 65, None, None)
    assert c["q"]["total"] == 0 and c["app"] == 0 and not bool(c["q"]["ray_cnt"].any()) and not bool(c["q"]["ray_off"].any())
    assert bool((c["rgb"] == 1.0).all())


@pytest.mark.parametrize("jit_on", [False, True])
@pytest.mark.parametrize("eps", [0.0, None])
def test_4_exits_jitter_and_eps_T(fog, fog_rays, hyper_tiny, jit_on, eps):
    thres, S = float(hyper_tiny["rayMarch_weight_thres"]), 130
    c, ref_cnt, k = _case(fog, fog_rays, S, _jitter(128, 9) if jit_on else None, eps, thres)
    assert int((ref_cnt[:128] >= S - 8).sum()) >= 16


def test_4_exits_tail_zone_launch(scene_b, hyper_tiny):
    """scene_b's 2013 rays, 126 tiles (on a card of 126 compute units or more: one tile per group, the unbatched kernel): the queue invariants of the call and of its
    dense twin; and the same rays as often over in one call as gives every group 8 tiles or more (17 times with 256 compute units): the batched kernel,
    and the short hand-outs of the launch's end (MARCH_TAIL: launches of 8 tiles per group or more)."""
    m, rays, S = (scene_b[k] for k in ("m", "rays", "S"))
    thres = float(hyper_tiny["rayMarch_weight_thres"])
    n = rays.shape[0]
    d = _call(m, rays, S, None, None, dense=True)
    ref_cnt = (d["dense"]["weight"] > thres).sum(1)
    assert int((ref_cnt > 0).sum()) > 500 and int(ref_cnt.max()) > 16
    c = _call(m, rays, S, None, None)
    _check_queue(d, n, thres)
    _check_queue(c, n)
    assert torch.equal(c["rgb"], scene_b["rgb"]) and torch.equal(c["depth"], scene_b["depth"]) and torch.equal(c["q"]["ray_cnt"].long(), ref_cnt)
    k = -(-8 * 16 * torch.cuda.get_device_properties(0).multi_processor_count // n)
    big = _call(m, _rep(rays, k), S, None, None)
    _check_queue(big, k * n)
    assert torch.equal(big["rgb"], scene_b["rgb"].repeat(k, 1)) and torch.equal(big["depth"], scene_b["depth"].repeat(k))
    assert torch.equal(big["q"]["ray_cnt"], c["q"]["ray_cnt"].repeat(k))
    assert torch.equal(big["q"]["q_pos"][_by_ray_fast(big["q"])], c["q"]["q_pos"][_by_ray_fast(c["q"])].repeat(k, 1))


def _graph_replayed_twice(m, rays, S, rgb, depth):
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.render_rays(rays, white_bg=True, N_samples=S)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap_rgb, cap_depth = m.render_rays(rays, white_bg=True, N_samples=S)
    for _ in range(2):
        cap_rgb.zero_(); cap_depth.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap_rgb, rgb) and torch.equal(cap_depth, depth)


def test_5_invariances_bit_for_bit(scene_b):
    """test_a3_invariances_of_the_plain_form's list on scene_b, whose 2013 rays are one ray per wave, and on the same rays ten times over in one call (several rays per
    wave: the batched kernel), whose reference is the picture of the 2013."""
    m, rays1, S, rgb1, depth1 = (scene_b[k] for k in ("m", "rays", "S", "rgb", "depth"))
    _, _, d = m.render_rays(rays1, white_bg=True, N_samples=S, dense=True)
    cnt = (d["weight"] > float(m.rayMarch_weight_thres)).sum(1)
    assert int((cnt > 0).sum()) > 500 and int(cnt.sum()) > 8 * int((cnt > 0).sum())             # not vacuous: many rays with entries, lists worth batching
    k10 = max(10, _copies(rays1.shape[0]))
    for k in (1, k10):
        rays, rgb, depth = _rep(rays1, k), _rep(rgb1, k), _rep(depth1, k)
        again = m.render_rays(rays, white_bg=True, N_samples=S)
        assert torch.equal(again[0], rgb) and torch.equal(again[1], depth)
        parts = [m.render_rays(rays[a:a + 500 * k], white_bg=True, N_samples=S) for a in range(0, rays.shape[0], 500 * k)]
        assert torch.equal(torch.cat([p[0] for p in parts]), rgb) and torch.equal(torch.cat([p[1] for p in parts]), depth)
        perm = torch.randperm(rays.shape[0], device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
        rp, dp = m.render_rays(rays[perm].contiguous(), white_bg=True, N_samples=S)
        assert torch.equal(rp, rgb[perm]) and torch.equal(dp, depth[perm])
        m.render_piece_rays = 256 * k
        try:
            pieces = m.render_rays(rays, white_bg=True, N_samples=S)
            assert torch.equal(pieces[0], rgb) and torch.equal(pieces[1], depth)
        finally:
            m.render_piece_rays = 0
        rd, dd, _ = m.render_rays(rays, white_bg=True, N_samples=S, dense=True)
        assert torch.equal(rd, rgb) and torch.equal(dd, depth)
        _graph_replayed_twice(m, rays, S, rgb, depth)


def test_6_explicit_depths_and_lam6(fog, fog_rays, hyper_tiny):
    """tvr_render_z (the general instantiation: explicit depths and lam6) at S = 65: the same comparison with calls of one ray, the depths taken from a dense render."""
    thres, S = float(hyper_tiny["rayMarch_weight_thres"]), 65
    k = _copies(128)
    _, _, d = fog.render_rays(fog_rays, white_bg=True, N_samples=S, dense=True)
    ref_cnt = (d["weight"] > thres).sum(1)
    assert int((ref_cnt >= S - 8).sum()) >= 16
    z = d["z"].contiguous()

    def zcall(rays, zz):
        from jittor_myc_nerfs_amd import _lib as L
        sc, lib, n = fog._ensure_scene(), L.lib(), rays.shape[0]
        rgb, depth, lam = torch.empty((n, 3), device="cuda"), torch.empty((n,), device="cuda"), torch.empty((n,), device="cuda")
        stats = torch.zeros(L.STAT_COUNT, dtype=torch.int64, device="cuda")
        scratch = fog._get_scratch(lib.tvr_render_scratch_bytes(sc, n, S))
        L.check(lib.tvr_render_z(sc, rays.data_ptr(), n, S, 1, zz.data_ptr(), thres, rgb.data_ptr(), depth.data_ptr(), lam.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                 None, stats.data_ptr(), torch.cuda.current_stream().cuda_stream), "tvr_render_z")
        q = _queue(fog, n, S)
        return dict(rgb=rgb.clone(), depth=depth.clone(), q=q, app=int(stats[L.STAT_APP]), dense=None)
    c = zcall(_rep(fog_rays, k), _rep(z, k))
    assert torch.equal(c["q"]["ray_cnt"].long(), ref_cnt.repeat(k))
    _check_queue(c, k * 128)
    _check_against_single_ray_calls(c, k, [zcall(fog_rays[i:i + 1].contiguous(), z[i:i + 1].contiguous()) for i in range(128)])
