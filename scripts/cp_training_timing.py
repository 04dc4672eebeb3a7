#!/usr/bin/env python3
"""GPU box: what a TensorCP training step costs (cp.TensorCP with cp_training on; csrc/tvr_cp_train.hip) — 4096 rays, 96 / 288 components on scene A's 300^3 box, the
eager chain split by device events into march forward, feature forward, network (forward + backward), feature backward and march backward — with TensorVMSplit's eager
chain (static_training = False) on the same box as context, and the float-atomic bytes a step adds against the chip-wide rate of 1.3 TB/s.

    python3 scripts/cp_training_timing.py [--steps 40] [--warmup 10] [--rays 4096]
The atomic bytes are COUNTED on the host from the step's own samples (a retired line tap is one 4-B add per component of the packed texel, cp.rd = 96 / cp.ra = 288 floats):
per ray one flush per line and cell crossed plus the two taps left at its end; per workgroup of 256 entries the same for the appearance lines plus its basis columns."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from jittor_myc_nerfs_amd import TensorCP, rays as R, synthetic
from jittor_myc_nerfs_amd.autograd_ops import _CpAppFn, _CpMarchFn

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rays", type=int, default=4096)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("cp_training_timing.py measures on the GPU; there is none here")
dev = torch.device("cuda")
A, H = synthetic.SCENE_A, synthetic.HYPER
ATOMIC_RATE = 1.3e12                                         # bytes of float atomic adds per second, chip-wide

arrs = synthetic.make_cp_scene_arrays(A["gridSize"], A["aabb"], 96, 288)
m = TensorCP(arrs["aabb"], A["gridSize"], dev, density_n_comp=[96], appearance_n_comp=[288], app_dim=27, near_far=A["near_far"], shadingMode="MLP_Fea",
             alphaMask_thres=1e-4, density_shift=H["density_shift"], distance_scale=H["distance_scale"], rayMarch_weight_thres=H["rayMarch_weight_thres"], pos_pe=6,
             view_pe=2, fea_pe=2, featureC=128, step_ratio=A["step_ratio"], fea2denseAct=H["fea2denseAct"]).load_arrays(arrs)
m.cp_training = True
S = m.nSamples
frame = R.frame_rays(R.sphere_poses(8, A["cam_radius"])[2], 800, 800, A["camera_angle_x"]).to(dev)
gen = torch.Generator(device=dev).manual_seed(0)
batches = [frame[torch.randint(0, frame.shape[0], (a.rays,), device=dev, generator=gen)] for _ in range(4)]
target = torch.rand((a.rays, 3), device=dev, generator=gen)
net = list(m.renderModule.parameters())
STAGES = ("march forward", "feature forward", "network", "feature backward", "march backward")


def cp_step(rays, ev=None):
    """one eager step, the chain of TensorCP.render_rays_autograd cut at the Functions' seams so that events can stand between them"""
    mark = (lambda i: ev[i].record()) if ev else (lambda i: None)
    eps_T = float(m.rayMarch_weight_thres)
    for p in m.parameters():
        p.grad = None
    mark(0)
    w, acc, xyz, ray_id, _ = _CpMarchFn.apply(m, rays, None, S, eps_T, *m.density_line)
    mark(1)
    feats = _CpAppFn.apply(m, xyz, *m.app_line, m.basis_mat.weight)
    mark(2)
    wd, ad, fd = w.detach().requires_grad_(), acc.detach().requires_grad_(), feats.detach().requires_grad_()
    rgb = m.renderModule.forward_autograd(rays[ray_id, 3:6], fd)
    rgb_map = torch.zeros((rays.shape[0], 3), device=dev).index_add_(0, ray_id, wd[:, None] * rgb) + (1.0 - ad[:, None])
    loss = ((rgb_map.clamp(0, 1) - target) ** 2).mean()
    g = torch.autograd.grad(loss, [wd, ad, fd] + net)
    mark(3)
    torch.autograd.backward([feats], [g[2]])
    mark(4)
    torch.autograd.backward([w, acc], [g[0], g[1]])
    mark(5)


def timed(fn, steps, warmup, n_ev):
    for i in range(warmup):
        fn(batches[i % len(batches)])
    torch.cuda.synchronize()
    sums = np.zeros(n_ev - 1)
    for i in range(steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n_ev)]
        fn(batches[i % len(batches)], ev)
        torch.cuda.synchronize()
        sums += [ev[k].elapsed_time(ev[k + 1]) for k in range(n_ev - 1)]
    return sums / steps


t = timed(cp_step, a.steps, a.warmup, 6)
t = [t[0], t[1], t[2], t[3], t[4]]
print("TensorCP 96 / 288 on %s, %d rays x %d samples, eager step: %.3f ms" % (list(m.gridSize.tolist()), a.rays, S, sum(t)))
for name, v in zip(STAGES, t):
    print("  %-17s %.3f ms" % (name, v))

# ---- the atomic bytes of one step, counted from its own samples -------------------------------------------------------------------------------------
with torch.no_grad():
    rays = batches[0]
    _, _, d = m.render_rays(rays, white_bg=True, N_samples=S, dense=True)
    xyz = _CpMarchFn.apply(m, rays, None, S, float(m.rayMarch_weight_thres), *m.density_line)[2]
valid, cell = d["valid"].bool(), d["cell"].long()                        # [n,S], [n,S,3]: the march's own cells; only samples whose gradient is not zero count
rd, ra = 96, 288
dens = 0
for k in range(3):
    c = torch.where(valid, cell[..., k], torch.full_like(cell[..., k], -1))
    for row, ok in zip(c.cpu().numpy(), valid.cpu().numpy()):
        v = row[ok]
        if v.size:
            dens += int((np.diff(v) != 0).sum()) + 2
dens_bytes = dens * rd * 4
g = torch.tensor([float(x - 1) for x in m.gridSize.tolist()], device=dev)
ci = torch.floor((xyz + 1.0) / 2.0 * g).long().cpu().numpy()
M = ci.shape[0]
app = 0
for k in range(3):
    for e0 in range(0, M, 256):
        v = ci[e0:e0 + 256, k]
        app += int((np.diff(v) != 0).sum()) + 2
n_wg = (M + 255) // 256
app_bytes = app * ra * 4 + n_wg * 27 * ra * 4
print("atomic adds of one step (%d appearance samples): density lines %.1f MB, appearance lines + basis %.1f MB; at %.1f TB/s chip-wide that is %.3f + %.3f ms"
      % (M, dens_bytes / 1e6, app_bytes / 1e6, ATOMIC_RATE / 1e12, dens_bytes / ATOMIC_RATE * 1e3, app_bytes / ATOMIC_RATE * 1e3))

# ---- context: TensorVMSplit's eager chain on the same box ---------------------------------------------------------------------------------------------
vm, _, _ = bench.build_model(dev, "TensorVMSplit")
vm.static_training = False


def vm_step(rays, ev=None):
    if ev:
        ev[0].record()
    for p in vm.parameters():
        p.grad = None
    rgb, _ = vm.render_rays_autograd(rays, white_bg=True, N_samples=S)
    ((rgb - target) ** 2).mean().backward()
    if ev:
        ev[1].record()


tv = timed(vm_step, a.steps, a.warmup, 2)
print("context: TensorVMSplit 16 / 48, eager chain (static_training = False), same rays and samples: %.3f ms per step" % tv[0])
