#!/usr/bin/env python3
"""What a TensorCP frame costs on the HIP path, and whether tvr_render's fused launch sequence beats the same work composed from the public staged calls.

Workload: a synthetic CP scene (synthetic.make_cp_scene_arrays) at 96 / 288 components, the bench's 8 poses of 800 x 800 rays x 512 samples, at 300^3 and 500^3.
Interleaved in one process, timed by events on the stream after the card has been under load for two seconds, 3 warm-up frames:
  (A) the frame through tvr_render (default pieces);
  (B) the same frame from the staged calls with ONE HOST READ of the queue length per call: per chunk of --chunk rays a render leaves the march queue in its scratch
      (a CP handle has no tvr_march_forward); then tvr_app_feature on the queue's positions, tvr_mlp_render, a torch index_add and the background.  Only the staged
      part behind the queue is timed per chunk (events around it); the march's own time comes from the tvr_profile of the very renders that filled the queues, so
      (B) = march + staged part and shares no kernel time with anything else;
  (C) the TensorVMSplit frame of the benchmark (synthetic.SCENE_A, 16 / 48 components per plane) on the same card, for orientation only.
Condition: (A) <= (B) — (A) does the same work without the host reads and the extra tensors.  There is no bar against (C).

    python scripts/cp_frame_timing.py [--frames 20] [--grids 300,500] [--json profiles/cp_frame_timing.json] [--only-a]
(--only-a --frames 2: the run to put under `rocprofv3 --kernel-trace --stats` for the per-kernel split.)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402


def build_cp(dev, grid, A, H):
    from jittor_myc_nerfs_amd import TensorCP, synthetic
    arrs = synthetic.make_cp_scene_arrays([grid] * 3, A["aabb"], 96, 288, 0)
    m = TensorCP(arrs["aabb"], [grid] * 3, dev, density_n_comp=[96], appearance_n_comp=[288], app_dim=27, near_far=A["near_far"], shadingMode="MLP_Fea",
                 alphaMask_thres=1e-4, density_shift=H["density_shift"], distance_scale=H["distance_scale"], rayMarch_weight_thres=H["rayMarch_weight_thres"], pos_pe=6,
                 view_pe=2, fea_pe=2, featureC=128, step_ratio=A["step_ratio"], fea2denseAct=H["fea2denseAct"])
    return m.load_arrays(arrs)


def staged_frame(m, rays, S, chunk, prof, L):
    """(B): returns (rgb_map, ms of the staged part); the march's ms are in `prof`."""
    lib, dev = L.lib(), rays.device
    n = rays.shape[0]
    rgb_map = torch.empty((n, 3), device=dev)
    lay = L.ScratchLayout()
    marks = []
    m.render_piece_rays = 0
    for a in range(0, n, chunk):
        r = rays[a:a + chunk]
        k = r.shape[0]
        m.render_rays(r, white_bg=True, N_samples=S, profile=prof)                     # fills the queue in the model's scratch (its picture is discarded)
        L.check(lib.tvr_scratch_describe(k, S, C.byref(lay)), "tvr_scratch_describe")
        sb = m._scratch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cnt = int(sb[lay.counter:lay.counter + 4].view(torch.int32).item())             # THE host read
        q_pos = sb[lay.q_pos:lay.q_pos + 16 * cnt].view(torch.float32).view(cnt, 4)
        q_ray = sb[lay.q_ray:lay.q_ray + 4 * cnt].view(torch.int32).long()
        acc = sb[lay.acc:lay.acc + 4 * k].view(torch.float32)
        feats = m.compute_appfeature(q_pos[:, :3].contiguous())
        rgb = m._mlp_render(r[q_ray, 3:6].contiguous(), feats)
        out = torch.zeros((k, 3), device=dev).index_add_(0, q_ray, q_pos[:, 3:4] * rgb)
        rgb_map[a:a + k] = (out + (1.0 - acc[:, None])).clamp(0, 1)
        e1.record()
        marks.append((e0, e1))
    m.render_piece_rays = None
    return rgb_map, marks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--grids", default="300,500")
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--json", default="")
    ap.add_argument("--only-a", action="store_true")
    args = ap.parse_args()
    from jittor_myc_nerfs_amd import _lib as L, synthetic
    dev = torch.device("cuda:0")
    A, H = synthetic.SCENE_A, synthetic.HYPER
    S = A["N_samples"]
    fr = [f.to(dev) for f in bench.frames(A)]
    vm = None if args.only_a else bench.build_model(dev, "TensorVMSplit")[0]
    result = {"workload": "8 poses, 800x800 rays x 512 samples, 96 / 288 CP components", "frames_timed": args.frames, "grids": {}}
    for grid in [int(g) for g in args.grids.split(",")]:
        m = build_cp(dev, grid, A, H)
        lib = L.lib()
        prof = C.c_void_p()
        L.check(lib.tvr_profile_create(4096, C.byref(prof)), "tvr_profile_create")
        stats = torch.zeros(8, dtype=torch.int64, device=dev)
        ref = m.render_rays(fr[3], white_bg=True, N_samples=S, stats=stats)
        torch.cuda.synchronize()
        if not args.only_a:                                                          # (B) computes the picture (A) computes
            got, _ = staged_frame(m, fr[3], S, args.chunk, prof, L)
            torch.cuda.synchronize()
            diff = float((got - ref[0]).abs().max())
            assert diff < 2e-5, diff                                                 # (index_add's summation order is not the composite kernel's: rounding only)
        t_end = time.perf_counter() + 2.0                                            # two seconds of load before anything is timed
        while time.perf_counter() < t_end:
            m.render_rays(fr[0], white_bg=True, N_samples=S)
            torch.cuda.synchronize()
        ms = {"A": [], "B": [], "B_march": [], "B_staged": [], "C": []}
        for f in range(-3, args.frames):                                             # 3 warm-up rounds, then interleaved A, B, C per frame
            rays = fr[f % len(fr)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            m.render_rays(rays, white_bg=True, N_samples=S)
            e1.record()
            e1.synchronize()
            if f >= 0:
                ms["A"].append(e0.elapsed_time(e1))
            if args.only_a:
                continue
            L.check(lib.tvr_profile_reset(prof), "tvr_profile_reset")
            _, marks = staged_frame(m, rays, S, args.chunk, prof, L)
            torch.cuda.synchronize()
            pm = (C.c_float * 3)()
            lib.tvr_profile_read(prof, C.byref(pm))
            staged = sum(a.elapsed_time(b) for a, b in marks)
            if f >= 0:
                ms["B_march"].append(float(pm[0]))
                ms["B_staged"].append(staged)
                ms["B"].append(float(pm[0]) + staged)
            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0.record()
            vm.render_rays(rays, white_bg=True, N_samples=S)
            c1.record()
            c1.synchronize()
            if f >= 0:
                ms["C"].append(c0.elapsed_time(c1))
        lib.tvr_profile_destroy(prof)
        med = lambda v: sorted(v)[len(v) // 2] if v else None
        st = stats.cpu().tolist()
        g = {"packed_bytes": int(m._packed.numel()), "samples_evaluated": st[0], "appearance_samples": st[2],
             "ms_per_frame_median": {k: med(v) for k, v in ms.items()}, "ms_per_frame_min": {k: (min(v) if v else None) for k, v in ms.items()}}
        if not args.only_a:
            g["A_le_B"] = bool(med(ms["A"]) <= med(ms["B"]))
        result["grids"][str(grid)] = g
        print(json.dumps({str(grid): g}), flush=True)
        del m
    if args.json:
        with open(os.path.join(ROOT, args.json) if not os.path.isabs(args.json) else args.json, "w") as f:
            json.dump(result, f, indent=1)
    if not args.only_a and not all(g["A_le_B"] for g in result["grids"].values()):
        print("CONDITION MISSED: the fused frame (A) is slower than the staged composition (B)")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
