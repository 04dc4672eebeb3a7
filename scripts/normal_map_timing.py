#!/usr/bin/env python3
"""What a normal map of a frame costs: TensorBase.render_normals (tvr_render_normals: march + one fused normal kernel) against the composition
the calls without it offer — render_rays(dense=True) in 4096-ray chunks, positions from z on the host side of the API (o + d z, normalize_coord), the appearance
mask, compute_density_gradient on the masked points, surface_normals' arithmetic and a torch index_add per chunk — and render_rays of the same frame for scale.
Two scenes: the benchmark's 300^3 TensorVMSplit and a 96 / 288-component TensorCP on the same grid; one 800 x 800 frame at 512 samples per ray.

Timed by events on the stream after two seconds of load and 2 warm-up rounds; the three forms alternate within every round and the median of --runs rounds is
reported, with min and max.  The two normal maps are compared on the way (same entries, another summation order: rounding-level differences).  A record for the
next reader, not a gate.

    python scripts/normal_map_timing.py [--runs 7] [--samples 512] [--txt profiles/normal_map_timing.txt]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402

import bench  # noqa: E402
from gradient_timing import build_cp  # noqa: E402

CHUNK = 4096


def composed(model, rays, S):
    """(normal [n,3], acc [n], entries) from calls that exist without tvr_render_normals"""
    n = rays.shape[0]
    normal = torch.zeros((n, 3), device=rays.device)
    acc = torch.empty((n,), device=rays.device)
    thres = float(model.rayMarch_weight_thres)
    inv = model.invaabbSize.to(device=rays.device, dtype=torch.float32)
    entries = 0
    for a in range(0, n, CHUNK):
        r = rays[a:a + CHUNK]
        _, _, d = model.render_rays(r, white_bg=True, N_samples=S, dense=True)
        app = d["weight"] > thres
        ray_idx, _ = app.nonzero(as_tuple=True)
        xyz = r[:, None, :3] + r[:, None, 3:6] * d["z"][..., None]
        _, g = model.compute_density_gradient(model.normalize_coord(xyz[app]))
        v = -(g * inv)
        ne = v / torch.sqrt(torch.clamp((v * v).sum(-1, keepdim=True), min=1e-30))
        normal[a:a + CHUNK].index_add_(0, ray_idx, d["weight"][app][:, None] * ne)
        acc[a:a + CHUNK] = d["acc"]
        entries += int(ray_idx.shape[0])
    return normal, acc, entries


def time_forms(model, rays, S, runs):
    forms = {"render_normals": lambda: model.render_normals(rays, N_samples=S),
             "composed": lambda: composed(model, rays, S),
             "render_rays": lambda: model.render_rays(rays, white_bg=True, N_samples=S)}
    N, acc, _ = forms["render_normals"]()
    Nc, accc, entries = forms["composed"]()
    torch.cuda.synchronize()
    diff = float((N - Nc).abs().max())
    same_acc = bool(torch.equal(acc, accc))
    t_end = time.perf_counter() + 2.0
    while time.perf_counter() < t_end:
        forms["render_normals"]()
        forms["render_rays"]()
        torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    names = list(forms)
    for r in range(-2, runs):
        order = names[r % 3:] + names[:r % 3]
        for name in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            forms[name]()
            e1.record()
            e1.synchronize()
            if r >= 0:
                ms[name].append(e0.elapsed_time(e1))
    return ms, entries, diff, same_acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--txt", default="profiles/normal_map_timing.txt")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    vm, _, A = bench.build_model(dev, "TensorVMSplit")
    cp = build_cp(dev, A)
    rays = bench.frames(A)[2].to(dev).contiguous()
    med = lambda v: sorted(v)[len(v) // 2]
    rows = {}
    for label, model in (("TensorVMSplit 300^3", vm), ("TensorCP 96 / 288 components 300^3", cp)):
        ms, entries, diff, same_acc = time_forms(model, rays, args.samples, args.runs)
        S = args.samples
        chunk_rays = max(256, int(model.NORMALS_SCRATCH_BOUND / (model_scratch(model, S) / 4096.0)) // 256 * 256)
        rows[label] = {"rays": int(rays.shape[0]), "samples_per_ray": S, "entries_per_frame": entries, "max_abs_difference_of_the_two_normal_maps": diff,
                       "acc_bit_equal": same_acc, "render_normals_rays_per_call": min(chunk_rays, int(rays.shape[0])),
                       "ms_median": {k: med(v) for k, v in ms.items()}, "ms_min": {k: min(v) for k, v in ms.items()}, "ms_max": {k: max(v) for k, v in ms.items()},
                       "composed_over_fused": med(ms["composed"]) / med(ms["render_normals"])}
    out = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "half_width": "one cell per axis", "composition_chunk_rays": CHUNK, "cases": rows,
           "note": "render_normals = tvr_render_normals calls sized to a 1 GiB scratch; composed = render_rays(dense=True) per 4096 rays + positions from z + "
                   "compute_density_gradient + torch index_add (host reads of the entry count included: the composition cannot avoid them); render_rays = the "
                   "colour frame, for scale; events around the calls, the three forms rotating"}
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.txt:
        path = args.txt if os.path.isabs(args.txt) else os.path.join(ROOT, args.txt)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")
    return 0


def model_scratch(model, S):
    from jittor_myc_nerfs_amd import _lib as L
    return L.lib().tvr_render_normals_scratch_bytes(model._ensure_scene(), 4096, S)


if __name__ == "__main__":
    sys.exit(main())
