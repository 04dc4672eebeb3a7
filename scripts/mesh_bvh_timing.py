#!/usr/bin/env python3
"""What the BVH and its ray queries cost on a marching-cubes mesh of a few hundred thousand triangles (a bumpy sphere from a 256^3 volume):

  build      key generation + torch.sort + tvr_mesh_bvh_build (mesh.build_bvh), and the three parts one by one
  cast       closest hits of an 800 x 800 camera frame (mesh.cast_rays) against mesh.render_mesh of the same frame on the same device, compared on the way
  occlusion  one K = 64 ambient-occlusion pass over every vertex (mesh.ambient_occlusion): any-hit rays per second

Every step runs in a child process of its own under its own time limit, one after the other; a step that fails or runs out of time ends the run.  Timed by events on the
stream after warm-up rounds; the median of --runs rounds is reported with min and max.  The parent commit has no ray query and neither has the reference: a record
for the next reader, not a gate.

    python scripts/mesh_bvh_timing.py [--runs 7] [--grid 256] [--json profiles/mesh_bvh_timing.json]
"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("build", 240), ("cast", 240), ("occlusion", 300))         # (step, its time limit in seconds)


def make_mesh(n, dev):
    import torch
    from jittor_myc_nerfs_amd import mesh
    g = torch.linspace(-0.5, 0.5, n, dtype=torch.float32, device=dev)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    r = torch.sqrt(x * x + y * y + z * z)
    vol = 0.36 + 0.03 * torch.sin(18 * x) * torch.sin(18 * y) * torch.sin(18 * z) - r
    sp = 1.0 / (n - 1)
    verts, faces = mesh.marching_cubes(vol, 0.0, spacing=(sp, sp, sp), origin=(-0.5, -0.5, -0.5))
    return verts * (1.0 / 0.36), faces


def timed(fn, runs, warm=3):
    import torch
    ms = []
    for r in range(-warm, runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r >= 0:
            ms.append(e0.elapsed_time(e1))
    ms.sort()
    return {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}


def step(name, args):
    import numpy as np
    import torch
    from jittor_myc_nerfs_amd import _lib as L, mesh, rays as R
    from jittor_myc_nerfs_amd.autograd_ops import _stream_ptr
    dev = torch.device("cuda:0")
    v, f = make_mesh(args.grid, dev)
    V, F = int(v.shape[0]), int(f.shape[0])
    out = {"device": torch.cuda.get_device_name(0), "vertices": V, "triangles": F}
    if name == "build":
        st = {}
        mesh.build_bvh(v, f, stats=st)
        out.update(st, build_bvh=timed(lambda: mesh.build_bvh(v, f), args.runs))
        lib = L.lib()
        scratch = torch.empty(lib.tvr_mesh_bvh_scratch_bytes(F), dtype=torch.uint8, device=dev)
        blob = torch.empty(lib.tvr_mesh_bvh_bytes(F), dtype=torch.uint8, device=dev)
        keys = torch.empty(F, dtype=torch.int64, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        s = _stream_ptr(dev)
        out["keys"] = timed(lambda: L.check(lib.tvr_mesh_bvh_keys(v.data_ptr(), V, f.data_ptr(), F, keys.data_ptr(), 8 * F, scratch.data_ptr(), scratch.numel(),
                                                                  flag.data_ptr(), s)), args.runs)
        ordered = torch.sort(keys)[0]
        out["sort"] = timed(lambda: torch.sort(keys), args.runs)
        out["build"] = timed(lambda: L.check(lib.tvr_mesh_bvh_build(v.data_ptr(), V, f.data_ptr(), F, ordered.data_ptr(), blob.data_ptr(), blob.numel(), scratch.data_ptr(),
                                                                    scratch.numel(), None, flag.data_ptr(), s)), args.runs)
        assert int(flag.item()) == 0
    elif name == "cast":
        H = W = 800
        pose = (R.sphere_poses(8, 4.0)[1] @ R.BLENDER2OPENCV).astype(np.float32)
        focal = 0.42 * W / math.tan(math.asin(1.0 / 4.0))
        o, d = R.get_rays(R.get_ray_directions(H, W, [focal, focal]), pose)
        rays = torch.from_numpy(np.ascontiguousarray(np.concatenate([o, d], 1), dtype=np.float32)).to(dev)
        bvh = mesh.build_bvh(v, f)
        st = {}
        t, tri, _ = mesh.cast_rays(bvh, rays, stats=st)
        depth, rtri, _, _ = mesh.render_mesh(v, f, pose, H, W, focal)
        out.update(image=[H, W], pixels_hit=st["rays_hit"], node_tests_per_ray=st["node_tests"] / (H * W), triangle_tests_per_ray=st["triangle_tests"] / (H * W),
                   pixels_with_another_triangle_than_the_rasteriser=int((tri.view(H, W) != rtri).sum()),
                   cast_rays=timed(lambda: mesh.cast_rays(bvh, rays), args.runs), render_mesh=timed(lambda: mesh.render_mesh(v, f, pose, H, W, focal), args.runs))
        out["mrays_per_s"] = H * W / out["cast_rays"]["ms_median"] / 1e3
        out["cast_over_render_mesh"] = out["cast_rays"]["ms_median"] / out["render_mesh"]["ms_median"]
    else:
        bvh = mesh.build_bvh(v, f)
        n = v / v.norm(dim=1, keepdim=True)                          # the bumps are shallow: the radial direction stands in for the normal
        st = {}
        ao = mesh.ambient_occlusion(bvh, n, n_dirs=64, bias=0.5 / (args.grid - 1) / 0.36, stats=st)
        out.update(directions=64, rays=V * 64, rays_hit=st["rays_hit"], ao_mean=float(ao.mean()), ao_min=float(ao.min()), node_tests_per_ray=st["node_tests"] / (V * 64),
                   triangle_tests_per_ray=st["triangle_tests"] / (V * 64),
                   ambient_occlusion=timed(lambda: mesh.ambient_occlusion(bvh, n, n_dirs=64, bias=0.5 / (args.grid - 1) / 0.36), args.runs, warm=1))
        out["mrays_per_s"] = V * 64 / out["ambient_occlusion"]["ms_median"] / 1e3
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--json", default="profiles/mesh_bvh_timing.json")
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None, help="run one step in this process (what the parent starts for each step)")
    args = ap.parse_args()
    if args.step:
        return step(args.step, args)
    out = {"runs": args.runs, "grid": args.grid,
           "note": "events around the Python calls (allocation of outputs and scratch, the kernels, one host read of the fault flag and the counters); not measured: the "
                   "kernels one by one, incoherent rays, meshes with long thin triangles"}
    for name, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--runs", str(args.runs), "--grid", str(args.grid)], capture_output=True,
                               text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"step {name} ran past its {limit} s: nothing more is started", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"step {name} ended with status {r.returncode}: nothing more is started\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out), flush=True)
    if args.json:
        path = args.json if os.path.isabs(args.json) else os.path.join(ROOT, args.json)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as fjson:
            json.dump(out, fjson, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
