#!/usr/bin/env python3
"""GPU box (round 5): a STREAM of frames on one card with the march of one frame beside the shade kernel of another.

The frame is energy-limited as a whole: the shade kernel runs against the chip's power limit (on half the CUs it clocks 2.34 GHz instead of 1.67 and
takes 1.42 x, not 2 x, as long), the march is bound by the L1 path per CU.  Two streams, two models (own scratch), frames alternating between them, full grids: the kernels
queue for the CUs.  Prints ms per frame over 24 frames against the plain serial loop.  (The same with the grids limited to disjoint CU sets, through a build hook that no
longer exists, was worse at every split: DESIGN.md 5, profiles/r05_overlap_stream.txt.  Round 2 measured -2.4 % for batches of ONE frame, profiles/r02_overlap_experiment.txt.)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench


def run(overlap, n_frames=24):
    dev = torch.device("cuda")
    models = [bench.build_model(dev)[0] for _ in range(2 if overlap else 1)]
    A = bench.build_model(dev)[2]
    fr = [f.to(dev) for f in bench.frames(A)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = [[torch.empty((fr[0].shape[0], 3), device=dev), torch.empty((fr[0].shape[0],), device=dev)] for _ in range(2)]

    def go(n):
        for k in range(n):
            if overlap:
                with torch.cuda.stream(streams[k % 2]):
                    models[k % 2].render_rays(fr[k % len(fr)], white_bg=True, N_samples=512, out=tuple(outs[k % 2]))
            else:
                models[0].render_rays(fr[k % len(fr)], white_bg=True, N_samples=512, out=tuple(outs[0]))
    go(4); torch.cuda.synchronize()
    t0 = time.perf_counter(); go(n_frames); torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n_frames * 1e3


if __name__ == "__main__":
    print(f"serial, one stream, full grids                       : {run(False):6.2f} ms per frame")
    print(f"two streams, full grids (kernels queue for the CUs)  : {run(True):6.2f}")
    print(f"serial, one stream, full grids (again)               : {run(False):6.2f}")
