#!/usr/bin/env python3
"""What the winding numbers cost on scripts/mesh_bvh_timing.py's marching-cubes mesh (a bumpy sphere from a 256^3 volume, a few hundred thousand
triangles):

  build      mesh.build_winding (62 passes and the finish; the kept table dropped before every round) against mesh.build_bvh
  grid2      mesh.winding_number_grid at beta = 2 on a --lattice^3 lattice over the mesh's bounding box + 5 %: points per second, node visits, dipoles and
  grid3      triangles per point, the share of grid points inside, the largest |w - exact| on the --exact^3 sub-lattice below; the same at beta = 3
  exact      beta = inf, the sum over every triangle, on an --exact^3 lattice over the same box (every point costs F solid angles: a small lattice)
  remesh     mesh.remesh_watertight of the mesh at --resolution: the whole step (hierarchy, table, field, marching cubes), the result's counters

Every step runs in a child process of its own under its own time limit, one after the other; a step that fails or runs out of time ends the run.  Timed by events on the
stream after warm-up rounds; the median of --runs rounds is reported with min and max.  No bar is set: a record for the next reader, not a gate.

    python scripts/mesh_winding_timing.py [--runs 5] [--grid 256] [--lattice 256] [--exact 32] [--resolution 256] [--json profiles/mesh_winding_timing.json]
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

STEPS = (("build", 120), ("grid2", 240), ("grid3", 240), ("exact", 240), ("remesh", 240))         # (step, its time limit in seconds)


def lattice(v, n):
    lo, hi = v.min(0)[0], v.max(0)[0]
    pad = 0.05 * (hi - lo)
    return (n, n, n), (lo - pad).tolist(), ((hi - lo + 2 * pad) / (n - 1)).tolist()


def step(name, args):
    import torch
    from jittor_myc_nerfs_amd import mesh
    dev = torch.device("cuda:0")
    v, f = make_mesh(args.grid, dev)
    out = {"device": torch.cuda.get_device_name(0), "vertices": int(v.shape[0]), "triangles": int(f.shape[0])}
    bvh = mesh.build_bvh(v, f)
    if name == "build":
        def table():
            bvh.winding = None
            mesh.build_winding(bvh)
        st = {}
        mesh.build_winding(bvh, stats=st)
        out.update(table=st, height=bvh.height, build_bvh=timed(lambda: mesh.build_bvh(v, f), args.runs), build_winding=timed(table, args.runs))
    elif name in ("grid2", "grid3"):
        beta = 2.0 if name == "grid2" else 3.0
        dims, origin, spacing = lattice(v, args.lattice)
        st = {}
        vol = mesh.winding_number_grid(bvh, dims, origin, spacing, beta, stats=st)
        n = args.lattice ** 3
        out.update(beta=beta, dims=list(dims), counters=st, inside_share=float((vol > 0.5).double().mean()), node_visits_per_point=st["node_visits"] / n,
                   dipoles_per_point=st["dipole_terms"] / n, triangles_per_point=st["triangle_terms"] / n,
                   winding_number_grid=timed(lambda: mesh.winding_number_grid(bvh, dims, origin, spacing, beta), args.runs, warm=1))
        out["mpoints_per_s"] = n / out["winding_number_grid"]["ms_median"] / 1e3
        small = lattice(v, args.exact)
        err = (mesh.winding_number_grid(bvh, *small, beta) - mesh.winding_number_grid(bvh, *small, float("inf"))).abs()
        out.update(exact_dims=list(small[0]), max_error_against_exact=float(err.max()), mean_error_against_exact=float(err.double().mean()))
    elif name == "exact":
        dims, origin, spacing = lattice(v, args.exact)
        st = {}
        vol = mesh.winding_number_grid(bvh, dims, origin, spacing, float("inf"), stats=st)
        n = args.exact ** 3
        out.update(beta="inf", dims=list(dims), counters=st, inside_share=float((vol > 0.5).double().mean()), smallest_margin=float((vol - 0.5).abs().min()),
                   winding_number_grid=timed(lambda: mesh.winding_number_grid(bvh, dims, origin, spacing, float("inf")), args.runs, warm=1))
        out["mpoints_per_s"] = n / out["winding_number_grid"]["ms_median"] / 1e3
        out["gtriangles_per_s"] = st["triangle_terms"] / out["winding_number_grid"]["ms_median"] / 1e6
    else:
        st = {}
        ov, of = mesh.remesh_watertight(v, f, resolution=args.resolution, stats=st)
        out.update(resolution=args.resolution, stats=st, result_vertices=int(ov.shape[0]), result_triangles=int(of.shape[0]),
                   remesh_watertight=timed(lambda: mesh.remesh_watertight(v, f, resolution=args.resolution), args.runs, warm=1))
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--lattice", type=int, default=256)
    ap.add_argument("--exact", type=int, default=32)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--json", default="profiles/mesh_winding_timing.json")
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None, help="run one step in this process (what the parent starts for each step)")
    args = ap.parse_args()
    if args.step:
        return step(args.step, args)
    out = {"runs": args.runs, "grid": args.grid,
           "note": "events around the Python calls (allocation of the output, the kernel, one host read of the fault flag and, where asked for, the counters; "
                   "build_winding: 62 pass launches and the finish; remesh_watertight: everything from the hierarchy to marching cubes, without the stats); not "
                   "measured: the kernels alone, points in random order, several streams"}
    for name, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--runs", str(args.runs), "--grid", str(args.grid), "--lattice",
                                str(args.lattice), "--exact", str(args.exact), "--resolution", str(args.resolution)], capture_output=True, text=True, timeout=limit)
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
