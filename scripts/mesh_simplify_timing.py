#!/usr/bin/env python3
"""What shrinking an exported mesh costs, stage by stage (csrc/tvr_mesh_simplify.hip): the export pipeline of synthetic.SCENE_A (the benchmark's
TensorVMSplit scene) at --grid^3 with keep_largest = 1 and simplify = --simplify, taken apart into its stages

  marching_cubes -> components + filter -> simplify_count -> simplify_emit -> attributes (normals + colours) -> write_ply

and, beside the two simplify calls, the same simplification COMPOSED FROM EXISTING TORCH CALLS on the same filtered mesh, interleaved round by round:
torch.unique(return_inverse) on the packed keys, index_add_ for the sums, torch.unique(dim=0) on the rotated triples.  The composition sums floats, so it is compared
with the kernels by its COUNTS only (vertices and triangles out), which must agree; the ratio of the two times is printed as measured.

Timed by events on the stream after a warm-up export and 2 warm-up rounds; median of --runs rounds with min and max.  Every figure is a whole Python-level call, so it
includes the host reads that call makes (totals, fault flags); write_ply is host work (device -> host copy, numpy, file write) bracketed by the same events.  The two
whole exports at the end (simplify = 0 and simplify = --simplify, through TensorBase.export_mesh) are SINGLE runs and give the file sizes.

Not measured: the kernels' clocks, grids above --grid, hash-table occupancy on other meshes than this one.  A record for the next reader, not a gate.

    python scripts/mesh_simplify_timing.py [--runs 10] [--grid 300] [--simplify 2.0] [--out profiles/mesh_simplify.txt]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def torch_simplify(verts, faces, lat):
    """The yardstick: vertex clustering from torch.unique / index_add_ -> (positions [V',3], triangles [F',3] rotated smallest-first and SORTED by torch.unique).
    lat = (origin, cell, inv_cell) as fp32 triples: the very numbers the kernels get, so that both sort every vertex into the same cell."""
    dev = verts.device
    o = torch.as_tensor(lat[0], dtype=torch.float32, device=dev)
    inv = torch.as_tensor(lat[2], dtype=torch.float32, device=dev)
    ci = torch.floor((verts - o) * inv).to(torch.int64)
    key = ci[:, 0] | (ci[:, 1] << 21) | (ci[:, 2] << 42)
    uniq, inverse = torch.unique(key, return_inverse=True)
    n = uniq.shape[0]
    sums = torch.zeros((n, 3), dtype=torch.float32, device=dev).index_add_(0, inverse, verts)
    cnt = torch.zeros(n, dtype=torch.float32, device=dev).index_add_(0, inverse, torch.ones_like(verts[:, 0]))
    pos = sums / cnt[:, None]
    m = inverse[faces.long()]
    m = m[(m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])]
    k = torch.argmin(m, dim=1, keepdim=True)
    rot = torch.gather(m, 1, (k + torch.arange(3, device=dev)[None]) % 3)
    tri = torch.unique(rot, dim=0)
    return pos, tri


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--simplify", type=float, default=2.0)
    ap.add_argument("--level", type=float, default=0.0005)
    ap.add_argument("--out", default="profiles/mesh_simplify.txt")
    args = ap.parse_args()
    from jittor_myc_nerfs_amd import mesh
    dev = torch.device("cuda:0")
    model = bench.build_model(dev, "TensorVMSplit")[0]
    grid = [args.grid] * 3
    tmp = tempfile.mkdtemp(prefix="mesh_simplify_")
    p_plain, p_small, p_stage = (os.path.join(tmp, n) for n in ("plain.ply", "small.ply", "stage.ply"))
    model.export_mesh(p_small, level=args.level, gridSize=grid, normals=True, colors=True, keep_largest=1, simplify=args.simplify)      # the warm-up export
    alpha = model.getDenseAlpha(grid)[0].contiguous()
    aabb = model.aabb.to(device=dev, dtype=torch.float32)
    voxel = ((aabb[1] - aabb[0]) / torch.tensor([float(s) for s in alpha.shape], device=dev)).tolist()
    cell, origin = model.mesh_simplify_lattice(alpha.shape, "reference", args.simplify)
    lat = mesh._lattice(cell, origin)
    names = ("marching_cubes", "components_filter", "simplify_count", "simplify_emit", "attributes", "write_ply", "torch_composition")
    ms = {k: [] for k in names}
    counts = {}
    for r in range(-2, args.runs):
        t = {}
        (v0, f0), t["marching_cubes"] = timed(lambda: mesh.marching_cubes(alpha, args.level, spacing=voxel, origin=origin))
        (v1, f1, _), t["components_filter"] = timed(lambda: mesh.filter_components(v0, f0, keep_largest=1))
        (scratch, n_v, n_f, flag), t["simplify_count"] = timed(lambda: mesh.simplify_count(v1, f1, *lat))
        assert int(flag.item()) == 0
        (v2, f2, vmap), t["simplify_emit"] = timed(lambda: mesh.simplify_emit(v1, f1, *lat, scratch, n_v, n_f, flag))
        assert int(flag.item()) == 0
        max_probe = int(scratch[4:8].view(torch.int32).item())
        (pos, tri), t["torch_composition"] = timed(lambda: torch_simplify(v1, f1, lat))
        assert (pos.shape[0], tri.shape[0]) == (n_v, n_f), ("the torch composition counts differently", pos.shape[0], tri.shape[0], n_v, n_f)
        attrs, t["attributes"] = timed(lambda: model.mesh_vertex_attributes(model.mesh_sample_positions(v2, alpha.shape, "reference")))
        _, t["write_ply"] = timed(lambda: mesh.write_ply(p_stage, v2, f2, normals=attrs["normals"], colors=attrs["colors"]))
        counts = {"marching_cubes": (v0.shape[0], f0.shape[0]), "components_filter": (v1.shape[0], f1.shape[0]), "simplify": (n_v, n_f)}
        if r >= 0:
            for k in names:
                ms[k].append(t[k])
        del scratch, pos, tri, attrs
    med = lambda v: sorted(v)[len(v) // 2]
    stage_bytes = os.path.getsize(p_stage)
    # two whole exports, single runs, for the file sizes
    t0 = time.perf_counter()
    model.export_mesh(p_plain, level=args.level, gridSize=grid, normals=True, colors=True, keep_largest=1)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    model.export_mesh(p_small, level=args.level, gridSize=grid, normals=True, colors=True, keep_largest=1, simplify=args.simplify)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    st = dict(model.mesh_export_stats)
    kernels = med(ms["simplify_count"]) + med(ms["simplify_emit"])
    cap_v, cap_t = mesh.simplify_table_capacities(*counts["components_filter"])
    lines = [f"mesh_simplify_timing: {torch.cuda.get_device_name(0)}, synthetic.SCENE_A at {args.grid}^3, level {args.level}, keep_largest 1, simplify {args.simplify}",
             f"median of {args.runs} rounds [min .. max] in ms after a warm-up export and 2 warm-up rounds; whole Python-level calls, host reads included",
             "", f"{'stage':<20}{'median':>10}{'min':>10}{'max':>10}   vertices / triangles out"]
    out_counts = {"marching_cubes": counts["marching_cubes"], "components_filter": counts["components_filter"], "simplify_count": counts["simplify"],
                  "simplify_emit": counts["simplify"], "attributes": counts["simplify"], "write_ply": counts["simplify"], "torch_composition": counts["simplify"]}
    for k in names:
        lines.append(f"{k:<20}{med(ms[k]):>10.3f}{min(ms[k]):>10.3f}{max(ms[k]):>10.3f}   {out_counts[k][0]} / {out_counts[k][1]}")
    lines += ["", f"simplify count + emit (sum of medians): {kernels:.3f} ms; torch composition: {med(ms['torch_composition']):.3f} ms; "
                  f"torch / kernels = {med(ms['torch_composition']) / kernels:.2f}",
              f"counts agree between the kernels and the composition in every round: {counts['simplify'][0]} vertices, {counts['simplify'][1]} triangles",
              f"triangles kept by the simplifier: {counts['simplify'][1] / max(counts['components_filter'][1], 1):.3f} of the filtered mesh",
              f"hash tables: {cap_v} cell slots for {counts['components_filter'][0]} vertices, {cap_t} triangle slots for {counts['components_filter'][1]} triangles; "
              f"longest probe sequence {max_probe} slots",
              f"scratch: {mesh.L.lib().tvr_mesh_simplify_scratch_bytes(*counts['components_filter'])} B",
              "", "whole exports through export_mesh (normals + colours, keep_largest 1), SINGLE runs, wall clock, getDenseAlpha included:",
              f"  simplify 0:  {(t1 - t0) * 1e3:.0f} ms, {os.path.getsize(p_plain)} B",
              f"  simplify {args.simplify}: {(t2 - t1) * 1e3:.0f} ms, {os.path.getsize(p_small)} B ({os.path.getsize(p_small) / os.path.getsize(p_plain):.3f} of the plain file; "
              f"the staged file above: {stage_bytes} B)",
              f"  mesh_export_stats: {json.dumps(st)}",
              "", "not measured: the kernels' clocks, grids above this one, hash-table occupancy on other meshes"]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        path = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    for p in (p_plain, p_small, p_stage):
        os.remove(p)
    os.rmdir(tmp)
    return 0


if __name__ == "__main__":
    sys.exit(main())
