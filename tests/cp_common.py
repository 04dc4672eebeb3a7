"""Shared by tests/test_cp_host.py and tests/test_gpu_cp.py: the tests' own restatement of TensorCP (reference tensorf-myc/models/tensoRF.py:345-376) in torch on the
CPU, and TensorBase.execute (tensorBase.py:476-536) around it from oracle.tensorf_oracle's public functions.  The oracle has no CP functions; test_cp_host.py checks this
restatement against a dense trilinear lookup before any GPU test leans on it."""
import numpy as np
import torch
import torch.nn.functional as F

from conftest import TINY

RANKS = [(96, 288), (16, 48), (5, 50), (1, 1)]
VEC_MODE = (2, 1, 0)


def cp_arrays(r_sigma, r_app, gridSize=None, aabb=None, seed=0):
    from jittor_myc_nerfs_amd import synthetic
    return synthetic.make_cp_scene_arrays(TINY["gridSize"] if gridSize is None else gridSize, TINY["aabb"] if aabb is None else aabb, r_sigma, r_app, seed)


def make_cp_model(arrs, hyper, device="cuda", view_pe=2, fea_pe=2):
    from jittor_myc_nerfs_amd import TensorCP
    m = TensorCP(arrs["aabb"], [int(x) for x in arrs["gridSize"]], device, density_n_comp=[arrs["density_line.0"].shape[1]],
                 appearance_n_comp=[arrs["app_line.0"].shape[1]], app_dim=27, near_far=hyper["near_far"], shadingMode="MLP_Fea", alphaMask_thres=1e-4,
                 density_shift=hyper["density_shift"], distance_scale=hyper["distance_scale"], rayMarch_weight_thres=hyper["rayMarch_weight_thres"], pos_pe=6,
                 view_pe=view_pe, fea_pe=fea_pe, featureC=128, step_ratio=hyper["step_ratio"], fea2denseAct=hyper["fea2denseAct"])
    return m.load_arrays(arrs)


def _line_points(lines, xyz, dtype):
    """tensoRF.py:347-356 / :364-374: prod_i grid_sample(line[i], (0, xyz[vecMode[i]])) -> [R, n]"""
    xyz = xyz.to(dtype)
    coord = torch.stack((xyz[..., VEC_MODE[0]], xyz[..., VEC_MODE[1]], xyz[..., VEC_MODE[2]]))
    coord = torch.stack((torch.zeros_like(coord), coord), dim=-1).view(3, -1, 1, 2)
    out = None
    for i in range(3):
        v = F.grid_sample(torch.as_tensor(lines[i]).to(dtype), coord[[i]], align_corners=True).view(-1, xyz.shape[0])
        out = v if out is None else out * v
    return out


def cp_density(arrs, xyz, dtype=torch.float32):                 # tensoRF.py:345-360
    return torch.sum(_line_points([arrs[f"density_line.{i}"] for i in range(3)], xyz, dtype), dim=0)


def cp_app(arrs, xyz, dtype=torch.float32):                     # tensoRF.py:362-376
    h = _line_points([arrs[f"app_line.{i}"] for i in range(3)], xyz, dtype)
    return h.T @ torch.as_tensor(arrs["basis_mat"]).to(dtype).T


def oracle_scene(arrs, hyper, dtype=torch.float32):
    """An OracleScene without planes; with dtype = float64 the network's arrays are doubles (sample positions stay the fp32 ones: they are inputs here)."""
    from oracle import tensorf_oracle as TO
    kw = {k: v for k, v in hyper.items()}
    sc = TO.OracleScene(arrs["aabb"], arrs["gridSize"], [], [arrs[f"density_line.{i}"] for i in range(3)], [], [arrs[f"app_line.{i}"] for i in range(3)],
                        arrs["basis_mat"], {k: arrs[k] for k in ("W1", "b1", "W2", "b2", "W3", "b3")}, alpha_volume=arrs.get("alpha_volume"),
                        alpha_aabb=arrs.get("alpha_aabb"), **kw)
    sc.mlp = {k: v.to(dtype) for k, v in sc.mlp.items()}
    return sc


def cp_execute(arrs, hyper, rays, N_samples, white_bg=True, jitter=None, dtype=torch.float32):
    """TensorBase.execute (tensorBase.py:476-536, ndc_ray=False) with the CP field.  Positions, depths and masks are computed in fp32 as the reference does (they are what
    the kernels reproduce bit for bit); everything behind the normalised coordinate — the field, the density, the compositing, the network — runs in `dtype`."""
    from oracle import tensorf_oracle as TO
    sc = oracle_scene(arrs, hyper, dtype)
    rays = torch.as_tensor(rays, dtype=torch.float32)
    o, d = rays[:, :3], rays[:, 3:6]
    xyz, z, valid, t_min = TO.sample_ray(sc, o, d, N_samples, jitter)
    dists = torch.cat((z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])), dim=-1)
    view = d.view(-1, 1, 3).expand(xyz.shape)
    bbox_valid = valid.clone()
    if sc.alpha_volume is not None:
        alphas = TO.alpha_sample(sc, xyz[valid])
        invalid = ~valid
        invalid[valid] |= ~(alphas > 0)
        valid = ~invalid
    xyz_n = TO.normalize_coord(sc, xyz)
    n, S = z.shape
    sf = torch.zeros((n, S), dtype=dtype)
    sigma = torch.zeros((n, S), dtype=dtype)
    rgb = torch.zeros((n, S, 3), dtype=dtype)
    if valid.any():
        sf[valid] = cp_density(arrs, xyz_n[valid], dtype)
        x = sf[valid] + sc.density_shift
        sigma[valid] = F.softplus(x) if sc.fea2denseAct == "softplus" else F.relu(sf[valid])
    alpha, weight, bg = TO.raw2alpha(sigma, dists.to(dtype) * sc.distance_scale)
    app = weight > sc.thres
    if app.any():
        rgb[app] = TO.mlp_render_fea(sc, view[app].to(dtype), cp_app(arrs, xyz_n[app], dtype))
    acc = torch.sum(weight, -1)
    rgb_map = torch.sum(weight[..., None] * rgb, -2)
    if white_bg:
        rgb_map = rgb_map + (1.0 - acc[..., None])
    rgb_map = rgb_map.clamp(0, 1)
    depth = torch.sum(weight * z.to(dtype), -1) + (1.0 - acc) * rays[:, 5].to(dtype)
    return dict(z=z, valid=valid, bbox_valid=bbox_valid, t_min=t_min, xyz_n=xyz_n, sigma_feature=sf, sigma=sigma, alpha=alpha, weight=weight, app=app, rgb=rgb,
                acc=acc, rgb_map=rgb_map, depth=depth)


def allowance(ref32, ref64, floor=1e-6, relative=False):
    """The tests' error allowance for a quantity the kernels compute in fp32: 4 x the error the fp32 restatement (torch on the CPU) makes against the fp64 one on the same
    inputs — the kernel sums up to 96 terms in another order and uses other exp / log1p implementations — and never below `floor`.  relative: in units of max |ref64|."""
    scale = max(1.0, float(ref64.abs().max())) if relative else 1.0
    err = float((ref32.double() - ref64).abs().max()) / scale
    return max(4.0 * err, floor) * scale
