#!/usr/bin/env python3
"""What the signed distance costs on scripts/mesh_bvh_timing.py's marching-cubes mesh (a bumpy sphere from a 256^3 volume, a few hundred thousand
triangles), beside what it is built on:

  query      mesh.signed_distance against mesh.closest_points on scripts/mesh_nearest_timing.py's `near` points (the mesh's own surface_samples(subdiv=2) moved by up to
             +- 2 voxels along their face normal), the two timed alternately; the table's counters, the points inside, the points undecided
  build      mesh.build_pseudonormals (keys, two sorts, the build; the kept table dropped before every round) against mesh.build_bvh
  lattice    mesh.signed_distance_grid on a 256^3 lattice over the mesh's bounding box + 5 %: points per second, the share of grid points inside

Every step runs in a child process of its own under its own time limit, one after the other; a step that fails or runs out of time ends the run.  Timed by events on the
stream after warm-up rounds; the median of --runs rounds is reported with min and max.  No bar is set: a record for the next reader, not a gate.

    python scripts/mesh_signed_timing.py [--runs 7] [--grid 256] [--lattice 256] [--json profiles/mesh_signed_timing.json]
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
from mesh_nearest_timing import near_points  # noqa: E402

STEPS = (("query", 240), ("build", 240), ("lattice", 300))         # (step, its time limit in seconds)


def step(name, args):
    import torch
    from jittor_myc_nerfs_amd import mesh
    dev = torch.device("cuda:0")
    v, f = make_mesh(args.grid, dev)
    voxel = 1.0 / (args.grid - 1) / 0.36
    out = {"device": torch.cuda.get_device_name(0), "vertices": int(v.shape[0]), "triangles": int(f.shape[0]), "voxel": voxel}
    bvh = mesh.build_bvh(v, f)
    if name == "query":
        p = near_points(v, f, voxel)
        cs, st = {}, {}
        mesh.build_pseudonormals(bvh, stats=cs)
        sd = mesh.signed_distance(bvh, p, stats=st)[0]
        d = mesh.closest_points(bvh, p)[0]
        rounds = [(timed(lambda: mesh.closest_points(bvh, p), args.runs), timed(lambda: mesh.signed_distance(bvh, p), args.runs)) for _ in range(3)]
        out.update(points=int(p.shape[0]), closedness=cs, counters=st, inside=int((sd < 0).sum()), same_bits_as_closest_points=bool(torch.equal(sd.abs(), d)),
                   closest_points=[a for a, _ in rounds], signed_distance=[b for _, b in rounds])
        out["signed_over_closest_points"] = sorted(b["ms_median"] / a["ms_median"] for a, b in rounds)[1]
    elif name == "build":
        def table():
            bvh.pseudonormals = None
            mesh.build_pseudonormals(bvh)
        cs = {}
        mesh.build_pseudonormals(bvh, stats=cs)
        out.update(closedness=cs, build_bvh=timed(lambda: mesh.build_bvh(v, f), args.runs), build_pseudonormals=timed(table, args.runs))
    else:
        n = args.lattice
        lo, hi = v.min(0)[0], v.max(0)[0]
        pad = 0.05 * (hi - lo)
        origin = (lo - pad).tolist()
        spacing = ((hi - lo + 2 * pad) / (n - 1)).tolist()
        st = {}
        vol = mesh.signed_distance_grid(bvh, (n, n, n), origin, spacing, stats=st)
        out.update(dims=[n, n, n], origin=origin, spacing=spacing, counters=st, inside_share=float((vol < 0).double().mean()), largest=float(vol.abs().max()),
                   node_tests_per_point=st["node_tests"] / n ** 3, triangle_tests_per_point=st["triangle_tests"] / n ** 3,
                   signed_distance_grid=timed(lambda: mesh.signed_distance_grid(bvh, (n, n, n), origin, spacing), args.runs, warm=1))
        out["mpoints_per_s"] = n ** 3 / out["signed_distance_grid"]["ms_median"] / 1e3
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--lattice", type=int, default=256)
    ap.add_argument("--json", default="profiles/mesh_signed_timing.json")
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None, help="run one step in this process (what the parent starts for each step)")
    args = ap.parse_args()
    if args.step:
        return step(args.step, args)
    out = {"runs": args.runs, "grid": args.grid,
           "note": "events around the Python calls (allocation of the outputs, the kernel, one host read of the fault flag and the counters; build_pseudonormals also "
                   "the two sorts and the read of the counters); closest_points and signed_distance are timed alternately, three rounds of --runs each; not measured: the "
                   "kernels alone, points in random order, several streams"}
    for name, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--runs", str(args.runs), "--grid", str(args.grid), "--lattice",
                                str(args.lattice)], capture_output=True, text=True, timeout=limit)
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
