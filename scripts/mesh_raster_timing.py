#!/usr/bin/env python3
"""What tvr_mesh_raster costs on the meshes export_mesh makes, at 800 x 800 from the benchmark's poses:

  * scene A's 300^3 export (keep_largest=1): millions of mostly sub-pixel triangles,
  * the same after simplify=4: larger triangles, a mix of the two paths,
  * one screen-filling quad (two triangles): the large path alone,

each at the default large_bbox and at the two extremes (large_bbox = H * W: every triangle walked by its own lane; large_bbox = 1: every triangle through the queue and
a workgroup).  The pictures of the three settings are compared bit for bit on the way.  Timed by events on the stream after two seconds of load and 3 warm-up rounds;
the settings alternate within every round and the median of --runs rounds is reported, with min and max, per pose 0 and as the mean over the eight poses.
The parent commit has no rasteriser and neither has the reference: a record for the next reader, not a gate.

    python scripts/mesh_raster_timing.py [--runs 10] [--json profiles/mesh_raster_timing.json]
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


def time_settings(verts, faces, poses, H, W, focal, settings, runs):
    from jittor_myc_nerfs_amd import mesh

    def draw(pose, lb, stats=None):
        return mesh.render_mesh(verts, faces, pose, H, W, focal, large_bbox=lb, stats=stats)

    stats = {name: {} for name, _ in settings}
    base = None
    same = True
    for name, lb in settings:
        out = draw(poses[0], lb, stats[name])
        if base is None:
            base = out
        else:
            same = same and all(torch.equal(a, b) for a, b in zip(out[:3], base[:3]))
    t_end = time.perf_counter() + 2.0
    while time.perf_counter() < t_end:
        for _, lb in settings:
            draw(poses[0], lb)
    ms = {name: [] for name, _ in settings}
    allposes = {name: [] for name, _ in settings}
    for r in range(-3, runs):
        order = settings if r % 2 == 0 else settings[::-1]
        for name, lb in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            draw(poses[0], lb)
            e1.record()
            e1.synchronize()
            if r >= 0:
                ms[name].append(e0.elapsed_time(e1))
    for name, lb in settings:
        for pose in poses:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            draw(pose, lb)
            e1.record()
            e1.synchronize()
            allposes[name].append(e0.elapsed_time(e1))
    med = lambda v: sorted(v)[len(v) // 2]
    return {name: {"large_bbox": lb, "ms_median_pose0": med(ms[name]), "ms_min_pose0": min(ms[name]), "ms_max_pose0": max(ms[name]),
                   "ms_mean_over_poses_single_runs": float(np.mean(allposes[name])), **stats[name]} for name, lb in settings}, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--json", default="profiles/mesh_raster_timing.json")
    args = ap.parse_args()
    from jittor_myc_nerfs_amd import rays as R
    dev = torch.device("cuda:0")
    vm, _, A = bench.build_model(dev, "TensorVMSplit")
    W, H = A["img_wh"]
    focal = R.focal_from_angle(A["camera_angle_x"], W)
    poses = [(M @ R.BLENDER2OPENCV).astype(np.float32) for M in R.sphere_poses(bench.N_POSES, A["cam_radius"])]
    settings = [("default", 0), ("everything small", H * W), ("everything large", 1)]
    meshes = {}
    v, f = vm.export_mesh(os.devnull, level=0.0005, spacing="samples", keep_largest=1)
    meshes["scene A 300^3 export"] = (v, f)
    v, f = vm.export_mesh(os.devnull, level=0.0005, spacing="samples", keep_largest=1, simplify=4.0)
    meshes["scene A 300^3 export, simplify=4"] = (v, f)
    c2w = poses[0].astype(np.float64)
    o, right, up, back = c2w[:3, 3], c2w[:3, 0], c2w[:3, 1], c2w[:3, 2]
    centre = o - 4.0 * back
    quad = np.stack([centre - 9 * right - 9 * up, centre + 9 * right - 9 * up, centre + 9 * right + 9 * up, centre - 9 * right + 9 * up]).astype(np.float32)
    meshes["one screen-filling quad"] = (torch.from_numpy(quad).to(dev), torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=dev))
    rows = {}
    for label, (v, f) in meshes.items():
        use = poses if "quad" not in label else poses[:1]
        res, same = time_settings(v, f, use, H, W, focal, settings, args.runs)
        rows[label] = {"vertices": int(v.shape[0]), "triangles": int(f.shape[0]), "pictures_bit_equal_across_settings": same, "settings": res}
    out = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "image": [H, W], "meshes": rows,
           "note": "events around mesh.render_mesh (scratch and output allocation, five kernels, one host read of the fault flag); settings alternate within a round; "
                   "not measured: the kernels one by one, the rate of 64-bit integer minimum atomics, images above 800 x 800"}
    print(json.dumps(out), flush=True)
    if args.json:
        path = args.json if os.path.isabs(args.json) else os.path.join(ROOT, args.json)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as fjson:
            json.dump(out, fjson, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
