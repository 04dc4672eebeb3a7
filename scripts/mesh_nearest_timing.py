#!/usr/bin/env python3
"""What the closest-point query and the mesh-to-mesh distance cost on scripts/mesh_bvh_timing.py's marching-cubes mesh (a bumpy sphere from a 256^3
volume, a few hundred thousand triangles):

  near       mesh.closest_points for the mesh's own surface_samples(subdiv=2) moved by up to +- 2 voxels along their face normal: points per second, node and triangle
             tests per point
  scaled     the same points at 0.5 x and 3 x their radius (deep inside, far outside)
  distance   mesh.mesh_distance of the simplify_clustering(cell = 2 voxels) mesh against the original, both directions, hierarchies built outside the timing
  brute      the yardstick: a brute-force torch composition on the device over ALL triangles, for a 4 096-point subset of `near` — nothing else in the project answers
             the query, the parent commit has no comparator; its distances are compared with the kernel's on the way

Every step runs in a child process of its own under its own time limit, one after the other; a step that fails or runs out of time ends the run.  Timed by events on the
stream after warm-up rounds; the median of --runs rounds is reported with min and max.  No bar is set: a record for the next reader, not a gate.

    python scripts/mesh_nearest_timing.py [--runs 7] [--grid 256] [--json profiles/mesh_nearest_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mesh_bvh_timing import make_mesh, timed  # noqa: E402

STEPS = (("near", 240), ("scaled", 240), ("distance", 300), ("brute", 300))         # (step, its time limit in seconds)
BRUTE_POINTS = 4096


def near_points(v, f, voxel):
    """surface_samples(subdiv=2) without the vertex rows, each moved by a seeded offset in +- 2 voxels along its face's normal"""
    import torch
    from jittor_myc_nerfs_amd import mesh
    pts = mesh.surface_samples(v, f, 2)[0][:4 * f.shape[0]]
    n = mesh.face_normals(v, f).repeat_interleave(4, 0)
    g = torch.Generator(device="cpu").manual_seed(18)
    step = ((torch.rand(pts.shape[0], 1, generator=g) * 4.0 - 2.0) * voxel).to(pts.device)
    return (pts + step * n).contiguous()


def brute_force(v, f, p, chunk=128):
    """fp32 torch on the device, every (point, triangle) pair: the plane projection if it lies inside, else the nearest of the three edges -> dist [N]"""
    import torch
    c0, c1, c2 = (v[f[:, k].long()][None] for k in range(3))
    e0, e1, e2 = c1 - c0, c2 - c1, c0 - c2
    n = torch.linalg.cross(e0, -e2, dim=-1)
    nn = (n * n).sum(-1).clamp_min(1e-30)
    out = torch.empty(p.shape[0], dtype=torch.float32, device=p.device)

    def seg(q, a, e):
        s = (((q - a) * e).sum(-1) / (e * e).sum(-1).clamp_min(1e-30)).clamp(0.0, 1.0)
        r = q - (a + s[..., None] * e)
        return (r * r).sum(-1)

    for i0 in range(0, p.shape[0], chunk):
        q = p[i0:i0 + chunk, None, :]
        h = ((q - c0) * n).sum(-1)
        foot = q - (h / nn)[..., None] * n
        inside = torch.ones_like(h, dtype=torch.bool)
        for c, e in ((c0, e0), (c1, e1), (c2, e2)):
            inside &= (torch.linalg.cross(e.expand_as(foot), foot - c, dim=-1) * n).sum(-1) >= 0
        d2 = torch.where(inside, h * h / nn, torch.minimum(torch.minimum(seg(q, c0, e0), seg(q, c1, e1)), seg(q, c2, e2)))
        out[i0:i0 + chunk] = d2.min(1)[0].sqrt()
    return out


def query(bvh, p, runs):
    from jittor_myc_nerfs_amd import mesh
    st = {}
    d = mesh.closest_points(bvh, p, stats=st)[0]
    r = {"points": int(p.shape[0]), "answered": st["points_answered"], "node_tests_per_point": st["node_tests"] / p.shape[0],
         "triangle_tests_per_point": st["triangle_tests"] / p.shape[0], "dist_mean": float(d.mean()), "dist_max": float(d.max()),
         "closest_points": timed(lambda: mesh.closest_points(bvh, p), runs)}
    r["mpoints_per_s"] = p.shape[0] / r["closest_points"]["ms_median"] / 1e3
    return r


def step(name, args):
    import torch
    from jittor_myc_nerfs_amd import mesh
    dev = torch.device("cuda:0")
    v, f = make_mesh(args.grid, dev)
    voxel = 1.0 / (args.grid - 1) / 0.36
    out = {"device": torch.cuda.get_device_name(0), "vertices": int(v.shape[0]), "triangles": int(f.shape[0]), "voxel": voxel}
    if name == "near":
        out.update(query(mesh.build_bvh(v, f), near_points(v, f, voxel), args.runs))
    elif name == "scaled":
        bvh, p = mesh.build_bvh(v, f), near_points(v, f, voxel)
        out.update(half_radius=query(bvh, (p * 0.5).contiguous(), args.runs), triple_radius=query(bvh, (p * 3.0).contiguous(), args.runs))
    elif name == "distance":
        cell = 2.0 * voxel
        vs, fs, _ = mesh.simplify_clustering(v, f, cell, origin=(-0.5 / 0.36,) * 3)
        bvh, bvh_s = mesh.build_bvh(v, f), mesh.build_bvh(vs, fs)
        st = {}
        d = mesh.mesh_distance(vs, fs, v, f, unit=voxel, bvh_a=bvh_s, bvh_b=bvh, stats=st)
        out.update(simplified_vertices=int(vs.shape[0]), simplified_triangles=int(fs.shape[0]), unit="voxels", a_is="simplified", b_is="original", distance=d,
                   cell_diagonal_voxels=2.0 * 3.0 ** 0.5, queries=d["a_to_b"]["samples"] + d["b_to_a"]["samples"], node_tests=st["node_tests"],
                   triangle_tests=st["triangle_tests"], mesh_distance=timed(lambda: mesh.mesh_distance(vs, fs, v, f, unit=voxel, bvh_a=bvh_s, bvh_b=bvh), args.runs),
                   mesh_distance_with_builds=timed(lambda: mesh.mesh_distance(vs, fs, v, f, unit=voxel), args.runs))
    else:
        p = near_points(v, f, voxel)
        p = p[torch.randperm(p.shape[0], generator=torch.Generator().manual_seed(19))[:BRUTE_POINTS].to(dev)].contiguous()
        bvh = mesh.build_bvh(v, f)
        want, got = brute_force(v, f, p), mesh.closest_points(bvh, p)[0]
        out.update(points=BRUTE_POINTS, largest_difference_in_voxels=float((want - got).abs().max()) / voxel, brute_force=timed(lambda: brute_force(v, f, p), args.runs, warm=1),
                   closest_points=timed(lambda: mesh.closest_points(bvh, p), args.runs))
        out["brute_over_closest_points"] = out["brute_force"]["ms_median"] / out["closest_points"]["ms_median"]
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--json", default="profiles/mesh_nearest_timing.json")
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None, help="run one step in this process (what the parent starts for each step)")
    args = ap.parse_args()
    if args.step:
        return step(args.step, args)
    out = {"runs": args.runs, "grid": args.grid,
           "note": "events around the Python calls (allocation of the outputs, the kernel, one host read of the fault flag and the counters; mesh_distance also the "
                   "sampling, two sorts and the statistics); not measured: the kernel alone, points in random order (these follow the faces, i.e. the marching order "
                   "of the volume), meshes with long thin triangles, more than one stream"}
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
