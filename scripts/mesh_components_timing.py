#!/usr/bin/env python3
"""What dropping floaters costs next to the extraction itself (csrc/tvr_mesh_cc.hip): connected components plus the component filter
(keep_largest = 1) beside the HIP marching cubes, on the same volume, box and build.  Two volumes at --grid^3:

  scene   the dense alpha volume of synthetic.SCENE_A at level 0.0005 (the benchmark's scene; what an export meets)
  noise   uniform noise inside a zero boundary layer at level 0.5: ONE huge component plus a very large number of tiny ones — the adversarial case for the
          labelling (every union of the big component meets the same few roots) and for the size policy (many tied roots)

Timed by events on the stream after two seconds of load and 3 warm-up rounds; median of --runs rounds with min and max.  Every figure is a whole Python-level call,
so it includes the host reads that call makes (the totals, the fault flag): `marching_cubes` = count + read + emit + flag; `mesh_components` = the five launches + flag
and count reads; `keep_mask` = the torch plumbing of the size policy; `filter_count` / `filter_emit` = the two library calls.  Bytes per face are the COMPULSORY traffic
of the labelling and the filter over the measured time: a lower bound of what the memory system moved, not a counter reading.

There is no comparator on the parent commit (the feature did not exist) and none in the reference: a record for the next reader, not a gate.

    python scripts/mesh_components_timing.py [--runs 30] [--grid 300] [--json profiles/mesh_components_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402


def noise_volume(n, seed=0):
    vol = np.zeros((n, n, n), np.float32)
    vol[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed).random((n - 2,) * 3, dtype=np.float32)
    return vol


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def measure(volume, level, runs):
    from jittor_myc_nerfs_amd import mesh
    t_end = time.perf_counter() + 2.0                                                # two seconds of load before anything is timed
    while time.perf_counter() < t_end:
        mesh.marching_cubes(volume, level)
    names = ("marching_cubes", "mesh_components", "keep_mask", "filter_count", "filter_emit")
    ms = {k: [] for k in names}
    stats = {}
    for r in range(-3, runs):
        t = {}
        (verts, faces), t["marching_cubes"] = timed(lambda: mesh.marching_cubes(volume, level))
        V = verts.shape[0]
        (label, sizes, n_comp), t["mesh_components"] = timed(lambda: mesh.mesh_components(faces, V, stats=stats))
        keep, t["keep_mask"] = timed(lambda: mesh.component_keep_mask(label, sizes, keep_largest=1))
        (scratch, n_v, n_f, flag), t["filter_count"] = timed(lambda: mesh.filter_count(faces, V, label, keep))
        out, t["filter_emit"] = timed(lambda: mesh.filter_emit(verts, faces, V, scratch, n_v, n_f, flag))
        assert int(flag.item()) == 0
        if r >= 0:
            for k in names:
                ms[k].append(t[k])
        del out, scratch
    med = lambda v: sorted(v)[len(v) // 2]
    F = int(faces.shape[0])
    # labelling: check 12 B + hook 12 B + sizes 4 B of every face (the first index), init 8 B + flatten 8 B per vertex; the gathers of parent[] come on top
    label_bytes = F * (12 + 12 + 4) + V * (8 + 8)
    # filter: count reads 12 B per face and 4 B per vertex and writes 1 B per element, the scan reads 1 B and writes 8 B per element; emit reads 1 B + 4 B per element,
    # 12 B per face and per vertex kept, and writes 12 B per face kept, 16 B per vertex kept
    n_el = max(V, F)
    filter_bytes = F * 12 + V * 4 + n_el * (1 + 1 + 8) + n_el * 5 + n_f * 24 + n_v * 28
    both = med(ms["mesh_components"]) + med(ms["keep_mask"]) + med(ms["filter_count"]) + med(ms["filter_emit"])
    return {"points": int(volume.numel()), "level": level, "vertices": V, "triangles": F, "components": n_comp, "kept_vertices": n_v, "kept_triangles": n_f,
            "longest_walk_steps": stats["max_walk_steps"], "walk_step_bound": stats["walk_step_bound"],
            "ms_median": {k: med(v) for k, v in ms.items()}, "ms_min": {k: min(v) for k, v in ms.items()}, "ms_max": {k: max(v) for k, v in ms.items()},
            "components_plus_filter_ms_median_sum": both, "ratio_to_marching_cubes": both / med(ms["marching_cubes"]),
            "compulsory_bytes_per_face": {"labelling": label_bytes / F, "filter": filter_bytes / F},
            "compulsory_GB_per_s": {"labelling": label_bytes / med(ms["mesh_components"]) / 1e6,
                                    "filter": filter_bytes / (med(ms["filter_count"]) + med(ms["filter_emit"])) / 1e6}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--json", default="profiles/mesh_components_timing.json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = bench.build_model(dev, "TensorVMSplit")[0]
    alpha = model.getDenseAlpha([args.grid] * 3)[0].contiguous()
    out = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "grid": args.grid,
           "note": "every figure is a whole Python-level call including its host reads; see the script's docstring",
           "scene": measure(alpha, 0.0005, args.runs)}
    del alpha, model
    out["noise"] = measure(torch.as_tensor(noise_volume(args.grid)).to(dev), 0.5, args.runs)
    print(json.dumps(out), flush=True)
    if args.json:
        path = args.json if os.path.isabs(args.json) else os.path.join(ROOT, args.json)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
