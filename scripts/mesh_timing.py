#!/usr/bin/env python3
"""What the HIP marching cubes (csrc/tvr_mesh.hip) costs on the benchmark's scene: the dense alpha volume of synthetic.SCENE_A at 300^3,
extracted at level 0.0005 (the reference's value, train.py:59).

Timed by events on the stream after the card has been under load for two seconds and 3 warm-up rounds; the median of --runs rounds is reported.  The two
library calls are timed separately: `count` = tvr_mesh_count (the count kernel, the tile scan and the per-tile scan: three launches) and `emit` =
tvr_mesh_emit; the host read of the two totals between them is part of an export but not of either figure.  Bytes per second are the COMPULSORY traffic
(volume 4 B + count byte written 1 B + read 1 B + two bases written 8 B per point for `count`; count byte 1 B per point plus the output for
`emit`) over the measured time, i.e. a lower bound of what the memory system moved.

There is no reference implementation to time against on any machine (the reference calls skimage on the CPU, which is not installed): this is a record for
the next reader, not a gate.

    python scripts/mesh_timing.py [--runs 20] [--grid 300] [--level 0.0005] [--json profiles/mesh_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--level", type=float, default=0.0005)
    ap.add_argument("--json", default="profiles/mesh_timing.json")
    args = ap.parse_args()
    from jittor_myc_nerfs_amd import mesh
    dev = torch.device("cuda:0")
    model = bench.build_model(dev, "TensorVMSplit")[0]
    t0 = time.perf_counter()
    alpha = model.getDenseAlpha([args.grid] * 3)[0].contiguous()
    torch.cuda.synchronize()
    dense_alpha_s = time.perf_counter() - t0
    points = alpha.numel()
    t_end = time.perf_counter() + 2.0                                                # two seconds of load before anything is timed
    while time.perf_counter() < t_end:
        mesh.marching_cubes(alpha, args.level)
    ms = {"count": [], "emit": [], "whole_call_host_clock": []}
    for r in range(-3, args.runs):
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        vol, scratch, nv, nt = mesh.mesh_count(alpha, args.level)
        e[1].record()                                                                # (behind the host read of the totals: the kernels have finished)
        e[2].record()
        verts, faces, flag = mesh.mesh_emit(vol, args.level, scratch, nv, nt)
        e[3].record()
        e[3].synchronize()
        h1 = time.perf_counter()
        assert int(flag.item()) == 0
        if r >= 0:
            ms["count"].append(e[0].elapsed_time(e[1]))
            ms["emit"].append(e[2].elapsed_time(e[3]))
            ms["whole_call_host_clock"].append(1e3 * (h1 - h0))
    med = lambda v: sorted(v)[len(v) // 2]
    count_bytes = points * (4 + 1 + 1 + 8)
    emit_bytes = points * 1 + nv * 12 + nt * 12
    out = {"workload": f"dense alpha of synthetic.SCENE_A sampled at {args.grid}^3, level {args.level}", "device": torch.cuda.get_device_name(0), "runs": args.runs,
           "points": points, "vertices": nv, "triangles": nt, "scratch_bytes": int(scratch.numel()), "dense_alpha_seconds_first_call": dense_alpha_s,
           "ms_median": {k: med(v) for k, v in ms.items()}, "ms_min": {k: min(v) for k, v in ms.items()}, "ms_max": {k: max(v) for k, v in ms.items()},
           "compulsory_bytes": {"count": count_bytes, "emit": emit_bytes},
           "compulsory_GB_per_s": {"count": count_bytes / med(ms["count"]) / 1e6, "emit": emit_bytes / med(ms["emit"]) / 1e6},
           "note": "count includes the host's wait for the two totals (events are recorded behind the read); emit is the one launch"}
    print(json.dumps(out), flush=True)
    if args.json:
        path = args.json if os.path.isabs(args.json) else os.path.join(ROOT, args.json)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
