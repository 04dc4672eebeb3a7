#!/usr/bin/env python3
"""What tvr_density_gradient costs against the composition existing code would need: seven tvr_density_feature calls on the centre and the six
shifted point sets (the shifted sets are prepared before the clock starts, so the composition is charged for its seven launches only, not for forming its inputs
nor for the difference quotient).  Two scenes: the benchmark's 300^3 TensorVMSplit and a 96-component TensorCP on the same grid; --points points (default 2^20),
uniform in the box plus a 5 % margin, and — third row — the vertices of a real export of the VM scene (clustered on the surface, as export_mesh queries them).

Timed by events on the stream after two seconds of load and 3 warm-up rounds; the two forms alternate within every round and the median of --runs rounds is
reported, with min and max.  The outputs of the two forms are compared bit for bit on the way.  A record for the next reader, not a gate.

    python scripts/gradient_timing.py [--runs 30] [--points 1048576] [--json profiles/gradient_timing.json]
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


def build_cp(device, A, rank=96):
    from jittor_myc_nerfs_amd import TensorCP, synthetic
    arrs = synthetic.make_cp_scene_arrays(A["gridSize"], A["aabb"], rank, 288)
    H = synthetic.HYPER
    m = TensorCP(arrs["aabb"], A["gridSize"], device, density_n_comp=[rank], appearance_n_comp=[288], app_dim=27, near_far=A["near_far"], shadingMode="MLP_Fea",
                 alphaMask_thres=1e-4, density_shift=H["density_shift"], distance_scale=H["distance_scale"], rayMarch_weight_thres=H["rayMarch_weight_thres"], pos_pe=6,
                 view_pe=2, fea_pe=2, featureC=128, step_ratio=A["step_ratio"], fea2denseAct=H["fea2denseAct"])
    return m.load_arrays(arrs)


def time_pair(model, x, runs):
    """(ms of one tvr_density_gradient call, ms of seven tvr_density_feature calls) per round, and whether the results agree bit for bit"""
    h = torch.tensor([2.0 / (int(g) - 1) for g in model.gridSize], dtype=torch.float32, device=x.device)
    sets = [x]
    for k in range(3):
        for sign in (1.0, -1.0):
            s = x.clone()
            s[:, k] = x[:, k] + sign * h[k]
            sets.append(s)
    inv2h = (torch.tensor(0.5) / h.cpu()).to(x.device)

    def fused():
        return model.compute_density_gradient(x)

    def composed():
        return [model.compute_densityfeature(s) for s in sets]

    sf, g = fused()
    f = composed()
    comp = torch.stack([(f[1 + 2 * k] - f[2 + 2 * k]) * inv2h[k] for k in range(3)], -1)
    same = bool(torch.equal(g, comp)) and bool(torch.equal(sf, f[0]))
    t_end = time.perf_counter() + 2.0
    while time.perf_counter() < t_end:
        fused()
        composed()
    ms = {"fused": [], "composed": []}
    for r in range(-3, runs):
        for name, fn in (("fused", fused), ("composed", composed)) if r % 2 == 0 else (("composed", composed), ("fused", fused)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= 0:
                ms[name].append(e0.elapsed_time(e1))
    return ms, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--json", default="profiles/gradient_timing.json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    vm, _, A = bench.build_model(dev, "TensorVMSplit")
    cp = build_cp(dev, A)
    g = torch.Generator(device="cpu").manual_seed(0)
    x = ((torch.rand((args.points, 3), generator=g) * 2 - 1) * 1.05).to(dev).contiguous()
    med = lambda v: sorted(v)[len(v) // 2]
    rows = {}
    t0 = time.perf_counter()
    verts, faces = vm.export_mesh(os.devnull, level=0.0005, spacing="samples", normals=True, colors=True)
    torch.cuda.synchronize()
    export_s = time.perf_counter() - t0
    cases = [("TensorVMSplit 300^3, uniform points", vm, x), ("TensorCP 96 components 300^3, uniform points", cp, x),
             ("TensorVMSplit 300^3, the vertices of its own export", vm, vm.normalize_coord(verts).contiguous())]
    for label, model, pts in cases:
        ms, same = time_pair(model, pts, args.runs)
        rows[label] = {"points": int(pts.shape[0]), "bit_equal_to_the_composition": same,
                       "ms_median": {k: med(v) for k, v in ms.items()}, "ms_min": {k: min(v) for k, v in ms.items()}, "ms_max": {k: max(v) for k, v in ms.items()},
                       "composed_over_fused": med(ms["composed"]) / med(ms["fused"])}
    out = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "half_width": "one cell per axis",
           "export": {"what": "TensorVMSplit 300^3 (synthetic.SCENE_A), level 0.0005, spacing samples, normals and colours, written to the null device",
                      "vertices": int(verts.shape[0]), "triangles": int(faces.shape[0]), "seconds_first_call_host_clock": export_s},
           "cases": rows,
           "note": "fused = one tvr_density_gradient call (sigma_feature and grad); composed = seven tvr_density_feature calls on prepared point sets, "
                   "without the difference quotient; events around the calls, the two forms alternating"}
    print(json.dumps(out), flush=True)
    if args.json:
        path = args.json if os.path.isabs(args.json) else os.path.join(ROOT, args.json)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
