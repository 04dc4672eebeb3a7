"""GPU checks of Instant-NGP training: csrc/tvr_ngp_train.hip through the C-ABI (include/tvr_ngp.h, "training") and the host surface of
jittor_myc_nerfs_amd.ngp / ngp_train, against the fp64 references of tests/ngp_train_common.py.  Bars that are not fixed numbers are derived from the same
reference run in fp32 on the CPU (printed before they are asserted)."""
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

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCENES = (1, 2, 33, 97, F.NO_BREAK)
SLACK = 37                                                    # rows behind the total in the "slack" capacity: owned by no ray


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


# --------------------------------------------------------------------------------------------------------------- designed inputs
@functools.lru_cache(maxsize=None)
def _designed_inputs(k):
    """The 421-ray ladder in designed_scene(k): rows, network outputs (the C oracle's), a random background and gradient per ray, and the capacities."""
    from oracle import ngp_oracle as N
    _, _, coords, ns = F.designed_rows()
    levels, arrs = F.designed_scene(k)
    out = N.network_c(levels, arrs, coords)
    rng = np.random.default_rng(100 + k)
    R, total = ns.shape[0], coords.shape[0]
    bg = rng.random((R, 3), dtype=np.float32)
    g = rng.normal(0, 1, (R, 3)).astype(np.float32)
    n, base = ns[:, 0].astype(np.int64), ns[:, 1].astype(np.int64)
    inside = next(r for r in range(R // 2, R) if n[r] >= 3 and base[r] + n[r] < total)
    at_end = next(r for r in range(R // 3, R) if n[r] >= 1 and base[r] + n[r] < total)
    caps = {"total": total, "inside": int(base[inside] + n[inside] // 2), "ray_end": int(base[at_end] + n[at_end]), "slack": total + SLACK}
    return coords, ns, out, bg, g, caps


@functools.lru_cache(maxsize=None)
def _designed_case(k, cap_kind):
    """Inputs cut / padded to the capacity, and the loop reference in fp64 and fp32 (computed once, shared by the forward and the backward test)."""
    coords, ns, out, bg, g, caps = _designed_inputs(k)
    n_rows, total = caps[cap_kind], coords.shape[0]
    if n_rows > total:                                          # rows no ray owns hold NaN: nothing may read them, their gradient is exactly 0
        out_c = np.concatenate([out, np.full((n_rows - total, 4), np.nan, np.float32)])
        coords_c = np.concatenate([coords, np.full((n_rows - total, 7), np.nan, np.float32)])
    else:
        out_c, coords_c = out[:n_rows], coords[:n_rows]
    ref = K.composite_loop(out_c, coords_c, ns, n_rows, bg, np.float64, grad_rgb=g)
    r32 = K.composite_loop(out_c, coords_c, ns, n_rows, bg, np.float32, grad_rgb=g)
    return out_c, coords_c, ns, bg, g, n_rows, ref, r32


def _run_compositor(out, coords, ns, bg, g, n_rows):
    from jittor_myc_nerfs_amd import ngp_train
    x = _t(out).requires_grad_(True)
    rgb = ngp_train.composite_train(x, _t(coords), _t(ns), _t(bg))
    rgb.backward(_t(g))
    return rgb.detach().cpu().numpy(), x.grad.cpu().numpy()


def test_compositor_forward_designed():
    from jittor_myc_nerfs_amd import ngp
    seen = dict(cut_to_zero=False, no_steps=False, breaks=False, ends_dark=False)
    sampler = ngp.DensityGridSampler(ngp.NGPNetworks(1), 1, rng=ngp.Pcg32(1))
    for k in SCENES:
        for cap_kind in ("total", "inside", "ray_end", "slack"):
            out, coords, ns, bg, g, n_rows, ref, _ = _designed_case(k, cap_kind)
            rgb, _ = _run_compositor(out, coords, ns, bg, g, n_rows)
            err = float(np.abs(rgb - ref["rgb"]).max())
            print(f"forward k={k} {cap_kind}: n_rows {n_rows} L-inf {err:.3e}")
            assert err < 2e-5                                    # tvr_ngp_composite's bar
            n, nc, stop = ref["n"], ref["nc"], ref["stop"]
            zero = (nc == 0) & (n > 0)
            assert np.all(rgb[zero] == 0) and np.array_equal(rgb[n == 0], bg[n == 0])
            dark = (stop == n) & (n > 0) & (ref["T_end"] < 1e-4)   # T falls below the threshold only behind the last sample: background times that T
            seen["cut_to_zero"] |= bool(zero.any())
            seen["no_steps"] |= bool((n == 0).any())
            seen["breaks"] |= bool((stop < nc).any())
            seen["ends_dark"] |= bool(dark.any())
        # one background, no cut: the inference compositor's bits
        out, coords, ns, _, _, n_rows, _, _ = _designed_case(k, "total")
        from jittor_myc_nerfs_amd import ngp_train
        const = np.tile(np.asarray(F.BG, np.float32), (ns.shape[0], 1))
        a = ngp_train.composite_train(_t(out), _t(coords), _t(ns), _t(const))
        b = sampler._composite(_t(out), _t(coords), _t(ns), F.BG)
        assert torch.equal(a, b)
    assert all(seen.values()), seen


def test_compositor_backward_designed():
    worst = 0.0
    for k in SCENES:
        for cap_kind in ("total", "inside", "ray_end", "slack"):
            out, coords, ns, bg, g, n_rows, ref, r32 = _designed_case(k, cap_kind)
            _, grad = _run_compositor(out, coords, ns, bg, g, n_rows)
            _, grad2 = _run_compositor(out, coords, ns, bg, g, n_rows)
            assert grad.shape == (n_rows, 4) and grad.tobytes() == grad2.tobytes()          # one owner per row: the same bytes on every run
            e32 = K.backward_row_error(r32["grad"], ref, g)
            bar = max(4 * e32, 1e-6)
            err = K.backward_row_error(grad, ref, g)
            worst = max(worst, err / bar)
            print(f"backward k={k} {cap_kind}: scaled error {err:.3e}, fp32 loop {e32:.3e}, bar {bar:.3e}")
            assert np.array_equal(r32["stop"], ref["stop"])
            assert err <= bar
            dead = ref["ray"] < 0                                # behind a break, behind the cut, in [total, n_rows)
            assert dead.any() and not grad[dead].any() and np.isfinite(grad).all()
    print(f"backward designed: worst error / bar = {worst:.3f}")


# --------------------------------------------------------------------------------------------------------------- the shared scene
@functools.lru_cache(maxsize=None)
def _scene_rows():
    from jittor_myc_nerfs_amd import synthetic
    from oracle import ngp_oracle as N
    levels = N.grid_levels(NGP_AABB_SCALE)
    arrs = synthetic.make_ngp_scene_arrays(levels["offsets"])
    arrs["density_grid_bitfield"], _ = N.update_bitfield(arrs["density_grid"])
    o, d = ngp_camera_rays(32, 32)
    coords, _, ns, _, _ = N.sample(o, d, arrs["density_grid_bitfield"], NGP_AABB_SCALE, N.Pcg32(1337).state)
    out = N.network_c(levels, arrs, coords)
    return levels, arrs, o, d, coords, ns, out


def test_compositor_shared_scene():
    levels, arrs, _, _, coords, ns, out = _scene_rows()
    total, R = coords.shape[0], ns.shape[0]
    assert R == 1024 and total > 100000
    rng = np.random.default_rng(7)
    bg, g = rng.random((R, 3), dtype=np.float32), rng.normal(0, 1, (R, 3)).astype(np.float32)
    _, brk, margin, _ = F.composite_f64(out, coords, ns, F.BG)
    keep = margin >= F.network_shift(out)
    print(f"shared scene: {total} rows, {(ns[:, 0] > 0).sum()} live rays, {(brk >= 0).sum()} break, {(~keep).sum()} left out, raw density max {out[:, 3].max():.1f}")
    assert (~keep).mean() <= 0.02
    assert (brk >= 0).sum() > 100
    for n_rows in (total, 100000):
        ref = K.composite_loop(out[:n_rows], coords[:n_rows], ns, n_rows, bg, np.float64, grad_rgb=g)
        r32 = K.composite_loop(out[:n_rows], coords[:n_rows], ns, n_rows, bg, np.float32, grad_rgb=g)
        rgb, grad = _run_compositor(out[:n_rows], coords[:n_rows], ns, bg, g, n_rows)
        err = float(np.abs(rgb - ref["rgb"])[keep].max())
        rows_kept = (ref["ray"] >= 0) & keep[np.maximum(ref["ray"], 0)]
        sub = dict(ref, ray=np.where(rows_kept, ref["ray"], -1))
        e32, eg = K.backward_row_error(r32["grad"], sub, g), K.backward_row_error(grad, sub, g)
        bar = max(4 * e32, 1e-6)
        print(f"shared scene n_rows={n_rows}: rgb L-inf {err:.3e}; backward scaled error {eg:.3e}, fp32 loop {e32:.3e}, bar {bar:.3e}")
        assert err < 2e-5 and eg <= bar
        owner = np.repeat(np.arange(R), ref["nc"])                         # bases are the prefix sum: the rows lie in ray order
        assert owner.shape[0] == n_rows
        dead = (ref["ray"] < 0) & keep[owner]                             # behind a compared ray's break: exactly 0
        assert dead.any() and not grad[dead].any()


# --------------------------------------------------------------------------------------------------------------- hash grid backward
def _hash_positions(case, seed):
    rng = np.random.default_rng(seed)
    if case == "contention":
        n = 4099
        pos = np.tile(rng.random((1, 3), dtype=np.float32), (n, 1))
        pos[:3] = [[0, 0, 0], [1, 1, 1], [0, 1, 0.5]]
        return pos
    pos = rng.random((case, 3), dtype=np.float32)
    edge = np.array([[0, 0, 0], [1, 1, 1], [0, 0.3, 0.7], [1, 0.3, 0.7], [0.3, 0, 0.7], [0.3, 1, 0.7], [0.3, 0.7, 0], [0.3, 0.7, 1]], np.float32)
    if case >= 63:
        pos[:8] = edge
    return pos


@pytest.mark.parametrize("aabb_scale", [1, 4])
@pytest.mark.parametrize("case", [1, 63, 64, 65, 4099, "contention"])
def test_hash_grid_backward(case, aabb_scale):
    from jittor_myc_nerfs_amd import ngp, ngp_train
    from oracle import ngp_oracle as N
    levels = N.grid_levels(aabb_scale)
    pos = _hash_positions(case, 11 + aabb_scale)
    n = pos.shape[0]
    rng = np.random.default_rng(5)
    rows = rng.normal(0, 1, (n, 7)).astype(np.float32)            # stride-7 rows, read in place
    rows[:, :3] = pos
    g = rng.normal(0, 1, (n, 32)).astype(np.float32)
    ref, ab, count = K.hash_backward_ref(levels, pos, g)
    enc = ngp.HashEncoder(aabb_scale).to(DEV)
    assert enc.m_n_params == 2 * ref.shape[0]
    rows_t, g_t = _t(rows), _t(g)
    variants = (None, 0, 1) if case in (4099, "contention") else (None,)
    for variant in variants:
        got = ngp_train.hash_encode_backward(enc, rows_t[:, :3], g_t, variant=variant)
        first = got.cpu().numpy().reshape(-1, 2).astype(np.float64)
        bound = (count[:, None] + 8) * 2.0 ** -23 * ab
        ratio = float((np.abs(first - ref) / np.maximum(bound, 1e-300)).max()) if (count > 0).any() else 0.0
        print(f"hash backward case={case} aabb={aabb_scale} variant={variant}: max |err| / bound = {ratio:.3f}, busiest entry {int(count.max())} adds")
        assert np.all(np.abs(first - ref) <= bound)
        assert not first[count == 0].any()                        # entries without a contribution are exactly 0
        ngp_train.hash_encode_backward(enc, rows_t[:, :3], g_t, grad_grid=got, variant=variant)       # accumulates
        second = got.cpu().numpy().reshape(-1, 2).astype(np.float64)
        assert np.all(np.abs(second - 2 * ref) <= (2 * count[:, None] + 8) * 2.0 ** -23 * 2 * ab)
    if case == "contention":
        assert count.max() >= 4096


# --------------------------------------------------------------------------------------------------------------- networks and the whole step
@pytest.fixture(scope="module")
def setup():
    from jittor_myc_nerfs_amd import ngp
    levels, arrs, o, d, coords, ns, out = _scene_rows()
    model = ngp.NGPNetworks(NGP_AABB_SCALE).to(DEV)
    sampler = ngp.DensityGridSampler(model, NGP_AABB_SCALE, rng=ngp.Pcg32(1337), target_batch_size=1 << 16).to(DEV)
    ngp.load_scene_arrays(model, sampler, {k: v for k, v in arrs.items() if k != "density_grid_bitfield"})
    return model, sampler


def test_forward_train_matches_fp64_and_leaves_forward_alone(setup):
    model, _ = setup
    levels, arrs, _, _, coords, _, _ = _scene_rows()
    sub = coords[:8192]
    ref, _ = F.network_f64(levels, arrs, sub)
    c = _t(sub)
    before = model(c[:, :3], c[:, 4:])
    assert not before.requires_grad
    got = model.forward_train(c[:, :3], c[:, 4:])
    assert got.requires_grad and got.shape == (8192, 4)
    err = np.abs(got.detach().cpu().numpy() - ref)
    print(f"forward_train: max err {err.max():.3e}, |out| max {np.abs(ref).max():.2f}")
    assert np.all(err <= 2e-4 * np.maximum(1.0, np.abs(ref)))
    model.hip_training = True
    try:
        assert model(c[:, :3], c[:, 4:]).requires_grad                      # grad mode on: the training graph
        with torch.no_grad():
            assert torch.equal(model(c[:, :3], c[:, 4:]), before)           # grad mode off: the fused kernel
    finally:
        model.hip_training = False
    after = model(c[:, :3], c[:, 4:])
    assert not after.requires_grad and torch.equal(after, before)


def test_one_step_gradients(setup):
    from jittor_myc_nerfs_amd.losses import huber_loss
    model, sampler = setup
    levels, arrs, o, d, _, _, _ = _scene_rows()
    cap = sampler.target_batch_size
    rng = np.random.default_rng(21)
    R = o.shape[0]
    bg, target = rng.random((R, 3), dtype=np.float32), rng.random((R, 3), dtype=np.float32)
    from jittor_myc_nerfs_amd import ngp
    sampler.rng = ngp.Pcg32(1337)
    sampler.training_step = 5                                               # no grid update, no ray-count update on this step
    model.hip_training = True
    try:
        pos, dirs = sampler.sample(None, _t(o), _t(d), is_training=True)
        coords, ns = sampler._coords.cpu().numpy(), sampler._rays_numsteps.cpu().numpy()
        n_rows = coords.shape[0]
        assert n_rows == cap                                                # the capacity cuts this batch
        # reference first: it decides which rays are compared
        c = torch.as_tensor(coords)
        ent, frac, _ = K.hash_geometry(levels, c[:, :3])
        with torch.no_grad():
            out64 = K.network_t(K.params_t(arrs, torch.float64, requires_grad=False), ent, frac, K.sh_t(c[:, 4:7].double())).numpy()
        margin = F.composite_f64(out64.astype(np.float32), coords, sampler._rays_numsteps_compacted.cpu().numpy(), F.BG)[2]     # the decisions on the kept rows
        keep = margin >= F.network_shift(out64)
        print(f"one step: {n_rows} rows, {(~keep).sum()} of {R} rays left out")
        assert (~keep).mean() <= 0.02
        ref, stop = K.grads_of_step(arrs, levels, coords, ns, n_rows, bg, target, torch.float64, keep_rays=keep)
        g32, _ = K.grads_of_step(arrs, levels, coords, ns, n_rows, bg, target, torch.float32, keep_rays=keep)
        model.zero_grad(set_to_none=True)
        rgb = sampler.rays2rgb(model(pos, dirs), _t(bg))
        (huber_loss(rgb, _t(target)) * _t(keep.astype(np.float32))[:, None]).sum().backward()
    finally:
        model.hip_training = False
    got = {"grid": model.pos_encoder.m_grid.grad}
    got.update(zip(K.WEIGHT_KEYS, [w.grad for w in model._weights()]))
    bad = []
    for name, r in ref.items():
        scale = np.abs(r).max()
        e = float(np.abs(got[name].double().cpu().numpy().reshape(r.shape) - r).max() / scale)
        e32 = float(np.abs(g32[name] - r).max() / scale)
        print(f"one step {name}: max|grad| {scale:.3e}, HIP error {e:.3e}, fp32 restatement {e32:.3e}, bar {4 * e32:.3e}")
        if not e <= 4 * e32:
            bad.append(name)
    assert not bad, bad


def test_sampler_training_bookkeeping(setup):
    from jittor_myc_nerfs_amd import ngp
    model, _ = setup
    levels, arrs, o, d, _, _, _ = _scene_rows()
    cap = 50000
    s = ngp.DensityGridSampler(model, NGP_AABB_SCALE, rng=ngp.Pcg32(1337), target_batch_size=cap).to(DEV)
    s2 = ngp.DensityGridSampler(model, NGP_AABB_SCALE, rng=ngp.Pcg32(1337)).to(DEV)
    for x in (s, s2):
        ngp.load_scene_arrays(model, x, {k: v for k, v in arrs.items() if k != "density_grid_bitfield"})
    ot, dt = _t(o), _t(d)
    with pytest.raises(NotImplementedError):
        s.sample(None, ot, dt, is_training=True)                            # opt-in
    model.hip_training = True
    try:
        s.training_step = 5
        pos, dirs = s.sample(None, ot, dt, is_training=True)
        s2.sample(None, ot, dt)
        total = int(s._counter[1])
        assert total > cap and s._coords.shape[0] == cap and pos.shape == (cap, 3) and dirs.shape == (cap, 3)
        assert torch.equal(s._coords, s2._coords[:cap]) and torch.equal(s._rays_numsteps, s2._rays_numsteps)
        ns = s._rays_numsteps.cpu().numpy().astype(np.int64)
        want = np.minimum(cap - np.minimum(cap, ns[:, 1]), ns[:, 0])
        assert np.array_equal(s._rays_numsteps_compacted.cpu().numpy(), np.stack([want, ns[:, 1]], 1))
        assert (want < ns[:, 0]).any() and int(want.sum()) == cap
        once = ngp.Pcg32(1337)
        once.advance()
        assert (s.rng.state, s.rng.inc) == (once.state, once.inc) and s.measured_batch_size == total
        # the schedule over steps 0..17
        calls, totals = [], 0
        real = s.update_density_grid
        s.update_density_grid = lambda step, *a, **k: (calls.append(step), real(step, *a, **k))[1]
        s.measured_batch_size, rays0 = 0, s.n_rays_per_batch
        for step in range(18):
            s.training_step = step
            s.sample(None, ot, dt, is_training=True)
            if step <= 15:
                totals += int(s._counter[1])
            if step == 15:
                assert s.n_rays_per_batch == ngp.DensityGridSampler.batch_rays(rays0, cap, totals) and s.measured_batch_size == 0
                m = max(totals / 16, 1)
                assert s.n_rays_per_batch == int(min((int(rays0 * cap / m) + 127) // 128 * 128, cap))
        assert calls == [0, 16]
    finally:
        model.hip_training = False


# --------------------------------------------------------------------------------------------------------------- it learns
def test_it_learns(setup):
    from jittor_myc_nerfs_amd import ngp, ngp_train, rays as RY
    import math
    teacher, tsampler = setup
    levels, arrs, _, _, _, _, _ = _scene_rows()
    W = H = 64
    focal = 0.5 * W / math.tan(0.5 * 0.6911)
    xforms = [ngp.matrix_nerf2ngp(np.asarray(p, np.float32)) for p in RY.sphere_poses(8, 4.0)]
    ts = ngp.DensityGridSampler(teacher, NGP_AABB_SCALE, rng=ngp.Pcg32(7)).to(DEV)
    ts.density_grid_bitfield.copy_(tsampler.density_grid_bitfield)
    imgs = []
    for x in xforms:
        o, d = ngp.generate_rays(x, W, H, (focal, focal), device=DEV)
        rgb = ts.render_frame(o, d)
        imgs.append(torch.cat([rgb, torch.ones(H * W, 1, device=DEV)], 1).reshape(H, W, 4))
    held = 3
    train_ids = [i for i in range(8) if i != held]
    data = ngp_train.NGPTrainData(torch.stack([imgs[i] for i in train_ids]).cpu().numpy(), np.stack([xforms[i] for i in train_ids]), [focal, focal], device=DEV)

    class Yardstick(ngp_train.NGPTrainer):
        """The same trainer with the network and the compositor replaced by the fp32 torch restatement on the GPU."""

        def network(self, pos, dirs):
            m = self.model
            p = dict(zip(K.WEIGHT_KEYS, m._weights()), grid=m.pos_encoder.m_grid)
            ent, frac, _ = K.hash_geometry(levels, pos)
            return K.network_t(p, ent, frac, K.sh_t(dirs.to(torch.float32)))

        def composite(self, net_out, bg):
            s = self.sampler
            return K.composite_t(net_out, K.unwarp_dt_t(s._coords[:, 3]), s._rays_numsteps, s._coords.shape[0], bg)[0]

    def run(cls, batch_seed):
        torch.manual_seed(1234)                                             # the same fresh student every time
        model = ngp.NGPNetworks(NGP_AABB_SCALE).to(DEV)
        sampler = ngp.DensityGridSampler(model, NGP_AABB_SCALE, rng=ngp.Pcg32(1337), target_batch_size=1 << 16).to(DEV)
        gen = torch.Generator(device="cpu").manual_seed(batch_seed)
        tr = cls(model, sampler, data, n_rays_per_batch=1024, generator=gen)
        return tr.train(64), model, sampler

    hip, model, sampler = run(ngp_train.NGPTrainer, 0)
    yard = [run(Yardstick, s)[0] for s in (0, 1, 2)]
    tail = [float(np.mean(c[-16:])) for c in yard]
    spread = (max(tail) - min(tail)) / float(np.mean(tail))
    m = max(0.25, 2 * spread)
    hip_tail = float(np.mean(hip[-16:]))
    print(f"it learns: HIP first/last16 {hip[0]:.5f} / {hip_tail:.5f}; yardstick last16 {tail}; spread {spread:.3f}, m {m:.3f}")
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ngp_train_curves.txt")
    if os.access(os.path.dirname(path), os.W_OK):                           # the recorded curves: rewritten by every run that can write there
        with open(path, "w") as f:
            f.write("Instant-NGP training, 64 steps, 1024 rays per batch, row capacity 2^16, student NGPNetworks(4) on the shared scene's 7 views at 64x64.\n")
            f.write("mean Huber loss per step: the HIP path (batch seed 0) and the fp32 torch restatement on the GPU (batch seeds 0, 1, 2)\n")
            f.write(f"m = max(0.25, 2 * relative spread of the yardstick's last-16 means) = {m:.4f} (spread {spread:.4f})\n")
            f.write(f"last-16 mean: HIP {hip_tail:.6f}; yardstick {' '.join(f'{t:.6f}' for t in tail)}\n")
            f.write("step  hip        yard0      yard1      yard2\n")
            for i in range(64):
                f.write(f"{i:4d}  {hip[i]:.6f}  {yard[0][i]:.6f}  {yard[1][i]:.6f}  {yard[2][i]:.6f}\n")
    assert np.isfinite(hip).all() and hip_tail < hip[0]
    assert hip_tail <= (1 + m) * tail[0]
    # the held-out pose renders from the trained weights without a manual repack, through the grid the trainer refreshed
    o, d = ngp.generate_rays(xforms[held], W, H, (focal, focal), device=DEV)
    state = (sampler.rng.state, sampler.rng.inc)
    img = sampler.render_frame(o, d)
    sampler.rng.state, sampler.rng.inc = state
    model.packed(force=True)
    assert torch.isfinite(img).all() and torch.equal(img, sampler.render_frame(o, d))
    assert sampler.density_grid_ema_step == 4 and int(sampler.density_grid_bitfield.count_nonzero()) > 0
    mse = float(((img - imgs[held][..., :3].reshape(-1, 3)) ** 2).mean())
    print(f"it learns: held-out pose MSE {mse:.5f}")


def test_command_line_trains_and_writes_a_checkpoint(tmp_path):
    """`python -m jittor_myc_nerfs_amd.ngp_train`, in process: two steps on a generated 6x6 scene, then the checkpoint loads."""
    from jittor_myc_nerfs_amd import ngp, ngp_train
    root, out = str(tmp_path / "scene"), str(tmp_path / "params.pkl")
    K.tiny_blender_scene(root)
    assert ngp_train.main(["--data", root, "--steps", "2", "--out", out, "--device", DEV]) == 0
    model = ngp.NGPNetworks(1)
    sampler = ngp.DensityGridSampler(model, 1, rng=ngp.Pcg32(1))
    assert ngp.load_jnerf_checkpoint(out, model, sampler) == 2
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters()) and int(sampler.density_grid_bitfield.count_nonzero()) > 0
