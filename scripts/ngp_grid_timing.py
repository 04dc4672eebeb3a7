"""Alt path: time one occupancy-grid update (DensityGridSampler.update_density_grid_nerf) at the early-policy size on cuda:0 — the fused call, the
stand-alone pieces, and `NGPNetworks.density` on the same number of positions (all the library could do toward an update before it had one) — alternating
them in one process; then what a grid built from the network costs in picture against an all-occupied bitfield on an 800x800 frame.
Seeded synthetic scene (synthetic.make_ngp_scene_arrays).  Usage: python scripts/ngp_grid_timing.py [--aabb-scale 4] [--rounds 30] [--size 800] [--out FILE]"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jittor_myc_nerfs_amd import ngp, rays as R, synthetic  # noqa: E402


def timed(fn, rounds_ms):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    rounds_ms.append(a.elapsed_time(b))


def summary(ms):
    s = sorted(ms)
    return f"median {s[len(s) // 2]:7.3f} ms  min {s[0]:7.3f}  max {s[-1]:7.3f}  (n = {len(s)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aabb-scale", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ngp_grid_timing: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    model = ngp.NGPNetworks(a.aabb_scale).to(dev)
    arrs = synthetic.make_ngp_scene_arrays(model.pos_encoder.offsets)
    ngp.load_scene_arrays(model, None, arrs)

    def sampler():
        return ngp.DensityGridSampler(model, a.aabb_scale, rng=ngp.Pcg32(1337)).to(dev)
    W = H = a.size
    focal = 0.5 * W / math.tan(0.5 * 0.6911)
    poses = R.sphere_poses(8, 4.0)
    xforms = [ngp.matrix_nerf2ngp(p) for p in poses]
    cams = ([[focal, focal]] * len(xforms), xforms, (W, H))

    s_f, s_p, s_m = sampler(), sampler(), sampler()
    s_m.mark_untrained_density_grid(*cams)
    n = ngp.NERF_GRIDSIZE ** 3 * (s_f.max_cascade + 1)
    pos, _ = ngp.grid_samples(s_f.density_grid, n, 0, s_f.max_cascade + 1, -0.01, ngp.Pcg32(1337), s_f.aabb_range)
    say(f"{torch.cuda.get_device_name(0)}; aabb_scale {a.aabb_scale}: {n} samples per early-policy update ({s_f.max_cascade + 1} cascades); "
        f"{int((s_m.density_grid < 0).sum())} of {s_m.density_grid.numel()} cells untrained under {len(xforms)} cameras")
    runs = {
        "NGPNetworks.density on n positions (the parent's call)": lambda: model.density(pos),
        "NGPNetworks.density_raw on n positions": lambda: model.density_raw(pos),
        "update, fused (tvr_ngp_grid_update)": lambda: s_f.update_density_grid_nerf(0.0, n, 0, fused=True),
        "update, fused, grid marked by the cameras": lambda: s_m.update_density_grid_nerf(0.0, n, 0, fused=True),
        "update, pieces (fused=False)": lambda: s_p.update_density_grid_nerf(0.0, n, 0, fused=False),
    }
    ms = {k: [] for k in runs}
    for _ in range(3):                                                 # warm-up of every shape
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    for _ in range(a.rounds):                                          # alternating: one of each per round
        for k, f in runs.items():
            timed(f, ms[k])
    for k in runs:
        say(f"{k:58s} {summary(ms[k])}")
    assert torch.equal(s_f.density_grid, s_p.density_grid) and torch.equal(s_f.density_grid_bitfield, s_p.density_grid_bitfield), "fused and pieces disagree"
    say("fused and pieces: density_grid and bitfield bit-equal after the timed updates")
    # the later policy: a quarter uniform + a quarter among the occupied cells
    ms2 = {"update, fused, later policy (n/4 + n/4)": [], "update, pieces, later policy (n/4 + n/4)": []}
    for _ in range(a.rounds):
        timed(lambda: s_f.update_density_grid_nerf(0.0, n // 4, n // 4, fused=True), ms2["update, fused, later policy (n/4 + n/4)"])
        timed(lambda: s_p.update_density_grid_nerf(0.0, n // 4, n // 4, fused=False), ms2["update, pieces, later policy (n/4 + n/4)"])
    for k in ms2:
        say(f"{k:58s} {summary(ms2[k])}")

    # ---- what a built grid costs in picture
    o, d = ngp.generate_rays(xforms[0], W, H, (focal, focal), device=dev)
    s_b, s_a = sampler(), sampler()
    frac = s_b.build_density_grid(16)
    s_a.density_grid_bitfield.fill_(0xFF)
    imgs, times, stats = {}, {"built": [], "all": []}, {"built": {}, "all": {}}
    for name, s in (("built", s_b), ("all", s_a)):
        s.render_frame(o, d)
    torch.cuda.synchronize()
    for _ in range(5):
        for name, s in (("built", s_b), ("all", s_a)):
            s.rng = ngp.Pcg32(1337)                                    # the same jitter in both pictures
            timed(lambda: imgs.__setitem__(name, s.render_frame(o, d)), times[name])
    for name, s in (("built", s_b), ("all", s_a)):
        s.rng = ngp.Pcg32(1337)
        s.render_frame(o, d, stats=stats[name])
    linf = float((imgs["built"] - imgs["all"]).abs().max())
    mean = float((imgs["built"] - imgs["all"]).abs().mean())
    say(f"{W}x{H} frame, grid from build_density_grid(16) ({frac * 100:.1f} % of cascade 0 set): {summary(times['built'])}; "
        f"{stats['built']['samples'] / 1e6:.1f} M samples marched, {stats['built']['evaluated'] / 1e6:.1f} M evaluated")
    say(f"{W}x{H} frame, all-occupied bitfield:                                    {summary(times['all'])}; "
        f"{stats['all']['samples'] / 1e6:.1f} M samples marched, {stats['all']['evaluated'] / 1e6:.1f} M evaluated")
    say(f"RGB L-inf between the two pictures {linf:.4f}, mean absolute difference {mean:.6f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
