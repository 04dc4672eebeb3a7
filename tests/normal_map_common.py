"""Shared by tests/test_gpu_normal_map.py: the tests' own restatement of tvr_render_normals (include/tvr.h) on the CPU, in fp64 (the oracle) and in fp32 (what
measures the error fp32 arithmetic makes on the same inputs).

    N_i = sum_e w_e n_e over the ray's appearance samples e (weight > rayMarch_weight_thres),  n_e = surface_normals' value at the sample

The march is TensorBase.execute's from oracle.tensorf_oracle's public functions — cp_common.cp_execute for CP, the same composition with TO.compute_densityfeature on
gradient_common.vm_oracle for VM — and the normals are gradient_common.gradient_restatement / normals_restatement at xyz_n[app].  Positions, depths and the fp32 masks
are inputs of both restatements, as they are in cp_execute; everything behind the normalised coordinate runs in `dtype`."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import cp_common as CC
import gradient_common as GC
from conftest import GOLDEN, TINY

S = TINY["N_samples"]
THRES = 1e-4                        # synthetic.HYPER's rayMarch_weight_thres: what one sample whose app mask flips can carry
FLOOR = 1e-5                        # the project's bar on acc for the same march (tests/test_gpu_cp.py): |n_e| <= 1, so a weight error enters N no larger than it enters acc
MAX_FLIPS = 2                       # cap on app-mask differences in a whole batch (tests/test_gpu_cp.py)


def hyper():
    from jittor_myc_nerfs_amd import synthetic
    return dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=TINY["step_ratio"])


def vm_execute(arrs, hyp, rays, N_samples, jitter=None, dtype=torch.float32):
    """cp_common.cp_execute's march with the VM density field (no colours: the normal pass shades nothing).  The same keys as cp_execute where they exist."""
    from oracle import tensorf_oracle as TO
    sc = GC.vm_oracle(arrs, hyp, dtype)
    rays = torch.as_tensor(rays, dtype=torch.float32)
    o, d = rays[:, :3], rays[:, 3:6]
    xyz, z, valid, t_min = TO.sample_ray(sc, o, d, N_samples, jitter)
    dists = torch.cat((z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])), dim=-1)
    if sc.alpha_volume is not None:
        alphas = TO.alpha_sample(sc, xyz[valid])
        invalid = ~valid
        invalid[valid] |= ~(alphas > 0)
        valid = ~invalid
    xyz_n = TO.normalize_coord(sc, xyz)
    n, S_ = z.shape
    sf = torch.zeros((n, S_), dtype=dtype)
    sigma = torch.zeros((n, S_), dtype=dtype)
    if valid.any():
        sf[valid] = TO.compute_densityfeature(sc, xyz_n[valid].to(dtype))
        sigma[valid] = F.softplus(sf[valid] + sc.density_shift) if sc.fea2denseAct == "softplus" else F.relu(sf[valid])
    alpha, weight, _ = TO.raw2alpha(sigma, dists.to(dtype) * sc.distance_scale)
    acc = torch.sum(weight, -1)
    depth = torch.sum(weight * z.to(dtype), -1) + (1.0 - acc) * rays[:, 5].to(dtype)
    return dict(z=z, valid=valid, xyz_n=xyz_n, sigma_feature=sf, sigma=sigma, alpha=alpha, weight=weight, app=weight > sc.thres, acc=acc, depth=depth)


def normal_map_restatement(arrs, hyp, rays, N_samples, kind, jitter=None, half_width=None, dtype=torch.float32):
    """dict(N [n,3], acc [n], depth [n], app [n,S], weight [n,S], gmin): the definition in `dtype`.  kind: "vm" or "cp".  gmin: the smallest |g| (normalised units)
    over the contributing samples — how well conditioned the normalisation is."""
    if kind == "cp":
        e = CC.cp_execute(arrs, hyp, rays, N_samples, jitter=jitter, dtype=dtype)
        f = GC.cp_density_fn(arrs, dtype)
    else:
        e = vm_execute(arrs, hyp, rays, N_samples, jitter=jitter, dtype=dtype)
        f = GC.vm_density(arrs, hyp, dtype)
    h32 = GC.cell(arrs["gridSize"]) if half_width is None else torch.as_tensor(half_width, dtype=torch.float32)
    app = e["app"]
    n = app.shape[0]
    N = torch.zeros((n, 3), dtype=dtype)
    gmin = float("inf")
    if app.any():
        x32 = e["xyz_n"][app].to(torch.float32).contiguous()
        g = GC.gradient_restatement(f, x32, h32, dtype)
        gmin = float(g.double().norm(dim=-1).min())
        ne = GC.normals_restatement(g, arrs["aabb"], dtype)
        contrib = torch.zeros(app.shape + (3,), dtype=dtype)
        contrib[app] = e["weight"][app][:, None] * ne
        N = contrib.sum(1)
    return dict(N=N, acc=e["acc"], depth=e["depth"], app=app, weight=e["weight"], gmin=gmin)


def bar(N32, N64, flips_per_ray, eps_T=0.0):
    """Per-ray allowance [n] on |N - N64|_inf: max(4 max|N32 - N64|, FLOOR) + THRES f_i (+ eps_T: the transmittance left when a ray stops bounds the summed weight of
    everything behind).  From the two restatements and the mask difference alone, never from the kernel's normals."""
    base = max(4.0 * float((N32.double() - N64).abs().max()), FLOOR)
    return base + THRES * torch.as_tensor(flips_per_ray, dtype=torch.float64) + float(eps_T)


# ---- the scenes of test 1 ---------------------------------------------------------------------------------------------------------------------------------------
SCENES = ["vm", "vm583", "ref", "cp96", "cp5", "cp1"]


@functools.lru_cache(maxsize=None)
def scene_arrays(name):
    """(arrays, kind) — built once, shared, never written to"""
    from jittor_myc_nerfs_amd import synthetic
    dump = dict(np.load(f"{GOLDEN}/tiny_dump.npz"))
    tiny = {k[len("scene."):]: v for k, v in dump.items() if k.startswith("scene.")}
    if name == "vm":
        return tiny, "vm"
    if name == "vm583":
        return synthetic.make_scene_arrays(TINY["gridSize"], TINY["aabb"], seed=5, density_n_comp=[5, 8, 3], appearance_n_comp=[7, 12, 5]), "vm"
    if name == "ref":
        ref = dict(np.load(f"{GOLDEN}/tiny_ref.npz"))
        a = dict(tiny)
        a.update({k[len("scene."):]: v for k, v in ref.items() if k.startswith("scene.")})
        return a, "vm"
    if name == "blob":
        return GC.gaussian_cp_arrays(), "cp"
    return CC.cp_arrays(*{"cp96": (96, 288), "cp5": (5, 50), "cp1": (1, 1)}[name]), "cp"


def golden_rays():
    return np.load(f"{GOLDEN}/tiny_dump.npz")["rays"]


@functools.lru_cache(maxsize=None)
def tiny_case(name):
    """(fp64 restatement, fp32 restatement) of the 64 golden rays on a scene — computed once, shared, never written to"""
    arrs, kind = scene_arrays(name)
    rays = golden_rays()
    return tuple(normal_map_restatement(arrs, hyper(), rays, S, kind, dtype=dt) for dt in (torch.float64, torch.float32))


def make_model(name):
    from conftest import make_model as vm_model
    arrs, kind = scene_arrays(name)
    if kind == "cp":
        return CC.make_cp_model(arrs, hyper())
    if name == "vm583":
        return GC.make_vm_model(arrs, hyper(), [5, 8, 3], [7, 12, 5])
    return vm_model(arrs, hyper())
