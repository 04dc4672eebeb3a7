#!/usr/bin/env python3
"""What smoothing an exported mesh costs, stage by stage (csrc/tvr_mesh_smooth.hip): the mesh is the export of synthetic.SCENE_A (the benchmark's
TensorVMSplit scene) at --grid^3 with keep_largest = 1, once as it is and once after simplify = --simplify, and the stages are

  adjacency_count -> adjacency_emit -> smooth (--iterations Taubin iterations over the emitted adjacency)

Beside them, interleaved round by round, the same operation COMPOSED FROM EXISTING TORCH CALLS on the same mesh: the adjacency is torch.unique(return_counts) on the
packed directed pairs, a half step is index_add_ over them.  The composition adds floats in an unspecified order, so it is compared with the kernels by its COUNTS
(half-edges, boundary and non-manifold edges), which must agree, and by a loose closeness of the positions (largest difference against the mesh's extent, printed).

Timed by events on the stream after 2 warm-up rounds; median of --runs rounds with min and max.  Every figure is a whole Python-level call, so it includes the host
reads that call makes (counts, fault flags) and its allocations.

Not measured: the kernels' clocks, grids above --grid, meshes with long rows (the fan of the tests), 12-byte against 16-byte position rows.  A record for the next
reader, not a gate.

    python scripts/mesh_smooth_timing.py [--runs 10] [--grid 300] [--simplify 2.0] [--iterations 10] [--out profiles/mesh_smooth.txt]
"""
import argparse
import os
import sys

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


def torch_adjacency(faces, V):
    """The yardstick's adjacency: (row [H], neighbour [H], edge_faces [H], degree [V]) from torch.unique on the packed directed pairs."""
    f = faces.long()
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    proper = a != b
    a, b = a[proper], b[proper]
    uniq, count = torch.unique(torch.cat((a, b)) * V + torch.cat((b, a)), return_counts=True)
    row, nbr = uniq // V, uniq % V
    return row, nbr, count, torch.bincount(row, minlength=V)


def torch_smooth(verts, row, nbr, count, deg, iterations, lam, mu):
    """The yardstick's smoothing: per half step one index_add_ over the half-edges; boundary vertices pinned."""
    V = verts.shape[0]
    pinned = torch.zeros(V, dtype=torch.bool, device=verts.device)
    pinned[row[count == 1]] = True
    moves = ((deg > 0) & ~pinned)[:, None]
    n = deg.clamp(min=1).to(torch.float32)[:, None]
    p = verts
    for _ in range(iterations):
        for w in (lam, mu):
            s = torch.zeros_like(p).index_add_(0, row, p[nbr])
            p = torch.where(moves, p + w * (s / n - p), p)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--simplify", type=float, default=2.0)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--level", type=float, default=0.0005)
    ap.add_argument("--out", default="profiles/mesh_smooth.txt")
    args = ap.parse_args()
    from jittor_myc_nerfs_amd import mesh
    lib = mesh.L.lib()
    dev = torch.device("cuda:0")
    model = bench.build_model(dev, "TensorVMSplit")[0]
    grid = [args.grid] * 3
    alpha = model.getDenseAlpha(grid)[0].contiguous()
    aabb = model.aabb.to(device=dev, dtype=torch.float32)
    voxel = ((aabb[1] - aabb[0]) / torch.tensor([float(s) for s in alpha.shape], device=dev)).tolist()
    v0, f0 = mesh.marching_cubes(alpha, args.level, spacing=voxel, origin=aabb[0].tolist())
    v1, f1, _ = mesh.filter_components(v0, f0, keep_largest=1)
    cell, origin = model.mesh_simplify_lattice(alpha.shape, "reference", args.simplify)
    v2, f2, _ = mesh.simplify_clustering(v1, f1, cell, origin=origin)
    lam, mu = mesh.SMOOTH_LAMBDA, mesh.SMOOTH_MU
    names = ("adjacency_count", "adjacency_emit", "smooth", "torch_adjacency", "torch_smooth")
    lines = [f"mesh_smooth_timing: {torch.cuda.get_device_name(0)}, synthetic.SCENE_A at {args.grid}^3, level {args.level}, keep_largest 1; Taubin x {args.iterations} "
             f"(lam {lam}, mu {mu}, boundaries pinned)",
             f"median of {args.runs} rounds [min .. max] in ms after 2 warm-up rounds; whole Python-level calls, host reads and allocations included"]
    for label, verts, faces in (("unsimplified", v1, f1), (f"simplify {args.simplify}", v2, f2)):
        V, F = verts.shape[0], faces.shape[0]
        ms = {k: [] for k in names}
        for r in range(-2, args.runs):
            t = {}
            (scratch, counts, flag), t["adjacency_count"] = timed(lambda: mesh.adjacency_count(faces, V))
            assert int(flag.item()) == 0
            adj, t["adjacency_emit"] = timed(lambda: mesh.adjacency_emit(faces, V, scratch, counts[0], flag))
            assert int(flag.item()) == 0
            out, t["smooth"] = timed(lambda: mesh.smooth_taubin(verts, faces, args.iterations, adjacency=adj))
            (row, nbr, count, deg), t["torch_adjacency"] = timed(lambda: torch_adjacency(faces, V))
            ref, t["torch_smooth"] = timed(lambda: torch_smooth(verts, row, nbr, count, deg, args.iterations, lam, mu))
            once = row < nbr
            theirs = (int(row.shape[0]), int((once & (count == 1)).sum()), int((once & (count > 2)).sum()), int(deg.max()))
            assert theirs == counts, ("the torch composition counts differently", theirs, counts)
            extent = float((verts.amax(0) - verts.amin(0)).max())
            gap = float((out - ref).abs().max())
            assert gap <= 1e-4 * extent, ("the torch composition lands elsewhere", gap, extent)
            if r >= 0:
                for k in names:
                    ms[k].append(t[k])
            del scratch, adj, row, nbr, count, deg, ref
        med = lambda v: sorted(v)[len(v) // 2]
        ours = med(ms["adjacency_count"]) + med(ms["adjacency_emit"])
        lines += ["", f"{label}: {V} vertices, {F} triangles; half-edges {counts[0]}, boundary edges {counts[1]}, non-manifold edges {counts[2]}, largest degree {counts[3]}",
                  f"{'stage':<20}{'median':>10}{'min':>10}{'max':>10}"]
        for k in names:
            lines.append(f"{k:<20}{med(ms[k]):>10.3f}{min(ms[k]):>10.3f}{max(ms[k]):>10.3f}")
        lines += [f"adjacency count + emit (sum of medians): {ours:.3f} ms; torch.unique composition: {med(ms['torch_adjacency']):.3f} ms; "
                  f"torch / kernels = {med(ms['torch_adjacency']) / ours:.2f}",
                  f"smoothing x {args.iterations}: {med(ms['smooth']):.3f} ms ({med(ms['smooth']) / (2 * args.iterations) * 1e3:.1f} us a half step, the call's fixed cost spread over them); "
                  f"index_add_ composition: {med(ms['torch_smooth']):.3f} ms; torch / kernels = {med(ms['torch_smooth']) / med(ms['smooth']):.2f}",
                  f"counts agree between the kernels and the composition in every round; largest position difference {gap:.3g} on an extent of {extent:.3g}",
                  f"scratch: adjacency {lib.tvr_mesh_adjacency_scratch_bytes(V, F)} B, smoothing {lib.tvr_mesh_smooth_scratch_bytes(V, counts[0])} B"]
    lines += ["", "not measured: the kernels' clocks, grids above this one, meshes with long rows, 12-byte against 16-byte position rows"]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        path = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
