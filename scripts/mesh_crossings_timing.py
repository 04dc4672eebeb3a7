#!/usr/bin/env python3
"""What the triangle-pair query costs on scripts/mesh_bvh_timing.py's marching-cubes mesh (a bumpy sphere from a 256^3 volume, a few hundred thousand
triangles), and what it finds on one export:

  query      mesh.crossings_count and mesh.crossings_emit (the two passes of mesh.self_intersections, each with its host read), the whole of self_intersections with the
             sort, node tests and triangle-pair tests per triangle; for orientation mesh.cast_rays(any_hit=True) over the same 3 F edge segments — the existing kernel
             on the same tree, which answers less (one bit per segment, no pairs, no sharing rule: every segment hits its own neighbours at once)
  exports    mesh.mesh_check of one export of bench.py's synthetic scene: plain, with simplify = 2, with smooth = 10, with refine = 4 (each on its own, after
             keep_largest = 1) — the crossings behind the README's "does not remove self-intersections" / "nothing protects against fold-over" / "not promised"

Every step runs in a child process of its own under its own time limit, one after the other; a step that fails or runs out of time ends the run.  Timed by events on the
stream after warm-up rounds; the median of --runs rounds is reported with min and max.  No bar is set: a record for the next reader, not a gate.

    python scripts/mesh_crossings_timing.py [--runs 5] [--grid 256] [--export_grid 200] [--json profiles/mesh_crossings_timing.json]
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

STEPS = (("query", 240), ("exports", 300))           # (step, its time limit in seconds)
EXPORTS = (("plain", {}), ("simplify=2", {"simplify": 2.0}), ("smooth=10", {"smooth": 10}), ("refine=4", {"refine": 4}))


def edge_segments(v, f):
    """(origins, dirs) [3F, 3] of every triangle side, from the smaller vertex index to the larger: the segments the pair query tests"""
    import torch
    a, b = f[:, [1, 2, 0]].reshape(-1).long(), f[:, [2, 0, 1]].reshape(-1).long()
    u, w = torch.minimum(a, b), torch.maximum(a, b)
    return v[u].contiguous(), (v[w] - v[u]).contiguous()


def step(name, args):
    import torch
    from jittor_myc_nerfs_amd import mesh
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0)}
    if name == "query":
        v, f = make_mesh(args.grid, dev)
        F = int(f.shape[0])
        bvh = mesh.build_bvh(v, f)
        st = {}
        per, P = mesh.crossings_count(bvh, stats=st)
        o, d = edge_segments(v, f)
        cast = {}
        hit = mesh.cast_rays(bvh, o, d, t_min=0.0, t_max=1.0, any_hit=True, stats=cast)
        out.update(vertices=int(v.shape[0]), triangles=F, height=bvh.height, counters=st, pairs=P, node_tests_per_triangle=st["node_tests"] / F,
                   pair_tests_per_triangle=st["pair_tests"] / F, most_pairs_of_one_triangle=int(per.max()) if F else 0,
                   crossings_count=timed(lambda: mesh.crossings_count(bvh), args.runs), crossings_emit=timed(lambda: mesh.crossings_emit(bvh, per, P, points=True), args.runs),
                   self_intersections=timed(lambda: mesh.self_intersections(bvh, points=True), args.runs),
                   cast_any_hit_3F_segments=dict(timed(lambda: mesh.cast_rays(bvh, o, d, t_min=0.0, t_max=1.0, any_hit=True), args.runs), segments=3 * F,
                                                 segments_hit=int(hit.sum()), node_tests_per_segment=cast["node_tests"] / (3 * F),
                                                 triangle_tests_per_segment=cast["triangle_tests"] / (3 * F)))
    else:
        import bench
        model = bench.build_model(dev, "TensorVMSplit")[0]
        grid = [args.export_grid] * 3
        out.update(scene="bench.py's synthetic scene, TensorVMSplit", export_grid=grid, level=0.0005, keep_largest=1, meshes={})
        for label, kw in EXPORTS:
            v, f = model.export_mesh(os.devnull, level=0.0005, gridSize=grid, keep_largest=1, **kw)
            bvh = mesh.build_bvh(v, f)
            rep = mesh.mesh_check(v, f, bvh=bvh)
            rep["self_intersections"] = timed(lambda: mesh.self_intersections(bvh, points=True), args.runs, warm=1)
            out["meshes"][label] = rep
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--export_grid", type=int, default=200)
    ap.add_argument("--json", default="profiles/mesh_crossings_timing.json")
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None, help="run one step in this process (what the parent starts for each step)")
    args = ap.parse_args()
    if args.step:
        return step(args.step, args)
    out = {"runs": args.runs, "grid": args.grid,
           "note": "events around the Python calls (allocation of the outputs, the kernel, the host reads of the fault flag and of the total; crossings_emit includes the "
                   "scan of the counts, self_intersections both passes and the sort); crossing_length is in the mesh's units; not measured: the kernels alone, a mesh "
                   "with one triangle that spans it (DESIGN.md §4.21: one lane then walks the whole tree), two-mesh queries"}
    for name, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--runs", str(args.runs), "--grid", str(args.grid), "--export_grid",
                                str(args.export_grid)], capture_output=True, text=True, timeout=limit)
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
