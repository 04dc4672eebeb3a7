"""Shared by tests/test_gpu_gradient.py: the tests' own restatement of tvr_density_gradient (include/tvr.h) and of TensorBase.surface_normals on the CPU, in fp64
(the oracle) and in fp32 (what measures the error fp32 arithmetic makes on the same inputs: cp_common.allowance), the point sets, and the scenes.

    grad[k] = (f(p + h_k e_k) - f(p - h_k e_k)) * (0.5 / h_k)

f is oracle.tensorf_oracle.compute_densityfeature (VM) or cp_common.cp_density (CP).  The shifted coordinate is part of the definition and is formed in fp32 — it is
an INPUT of both restatements, as sample positions are in cp_common.cp_execute; everything behind it (the field, the difference, the quotient) runs in `dtype`."""
import numpy as np
import torch

import cp_common as CC
from conftest import TINY


def cell(gridSize):
    """one cell of the grid per axis in normalised units, as fp32 (the default half width)"""
    return torch.tensor([2.0 / (int(g) - 1) for g in gridSize], dtype=torch.float32)


def half_widths(gridSize):
    """{name: fp32 [3]}: the default, half a cell, and 0.37 of a cell (no tap of p +- h coincides with one of p).  The axes differ because the TINY grid's do."""
    c = cell(gridSize)
    return {"cell": c, "half": c * 0.5, "0.37": c * 0.37}


def point_set(gridSize, seed=0):
    """fp32 [m,3] normalised coordinates, shuffled: uniform in the box, exactly on grid nodes (corners included), on the faces +-1, uniform out to +-1.3, and
    points at 1 + s cells beyond / before each face for s such that, for half widths of 1, 0.5 and 0.37 cells, p, p + h and p - h each fall outside in turn."""
    g = torch.Generator().manual_seed(seed)
    gs = [int(x) for x in gridSize]
    parts = [torch.rand((1000, 3), generator=g) * 2 - 1]
    idx = torch.stack([torch.randint(0, n, (61,), generator=g) for n in gs], -1)
    corners = torch.tensor([[(c >> k) & 1 for k in range(3)] for c in range(8)]) * (torch.tensor(gs) - 1)
    idx = torch.cat((idx, corners))
    parts.append(-1.0 + 2.0 * idx.float() / (torch.tensor(gs).float() - 1))
    face = torch.rand((60, 3), generator=g) * 2 - 1
    for i in range(60):
        face[i, i % 3] = 1.0 if (i // 3) % 2 else -1.0
    parts.append(face)
    parts.append((torch.rand((300, 3), generator=g) * 2 - 1) * 1.3)
    c = cell(gs)
    edge = []
    for k in range(3):
        for sign in (-1.0, 1.0):
            for s in (-1.5, -0.9, -0.45, -0.3, -0.1, 0.0, 0.1, 0.3, 0.45, 0.9, 1.5, 2.5):
                p = torch.rand(3, generator=g) * 2 - 1
                p[k] = sign * (1.0 + s * float(c[k]))
                edge.append(p)
    parts.append(torch.stack(edge))
    pts = torch.cat(parts).to(torch.float32)
    return pts[torch.randperm(pts.shape[0], generator=g)].contiguous()


def shifted(xyz32, h32, k, sign):
    """p + sign * h_k e_k with the sum rounded to fp32"""
    out = xyz32.clone()
    out[:, k] = xyz32[:, k] + h32[k] if sign > 0 else xyz32[:, k] - h32[k]
    return out


def gradient_restatement(f, xyz32, h32, dtype):
    """[m,3] in `dtype`: f takes [m,3] coordinates in `dtype`"""
    cols = []
    for k in range(3):
        fp, fm = f(shifted(xyz32, h32, k, +1).to(dtype)), f(shifted(xyz32, h32, k, -1).to(dtype))
        cols.append((fp - fm) * (torch.tensor(0.5, dtype=dtype) / h32[k].to(dtype)))
    return torch.stack(cols, -1)


def normals_restatement(grad, aabb, dtype):
    """TensorBase.surface_normals from a normalised-unit gradient: -(g * 2 / extent) / sqrt(max(|.|^2, 1e-30))"""
    aabb = torch.as_tensor(aabb, dtype=torch.float32).reshape(2, 3)
    g = -(grad.to(dtype) * (2.0 / (aabb[1] - aabb[0])).to(dtype))
    return g / torch.sqrt(torch.clamp((g * g).sum(-1, keepdim=True), min=1e-30))


def angles(a, b):
    """angle between rows (radians, fp64), accurate near zero: atan2(|a x b|, a . b)"""
    a, b = a.double(), b.double()
    return torch.atan2(torch.linalg.cross(a, b).norm(dim=-1), (a * b).sum(-1))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------------------------
def vm_oracle(arrs, hyper, dtype):
    """OracleScene of a VM scene with every array in `dtype`"""
    from oracle import tensorf_oracle as TO
    sc = TO.scene_from_arrays(arrs, **hyper)
    for name in ("density_plane", "density_line", "app_plane", "app_line"):
        setattr(sc, name, [p.to(dtype) for p in getattr(sc, name)])
    sc.basis_mat = sc.basis_mat.to(dtype)
    sc.mlp = {k: v.to(dtype) for k, v in sc.mlp.items()}
    return sc


def vm_density(arrs, hyper, dtype):
    from oracle import tensorf_oracle as TO
    sc = vm_oracle(arrs, hyper, dtype)
    return lambda x: TO.compute_densityfeature(sc, x)


def cp_density_fn(arrs, dtype):
    return lambda x: CC.cp_density(arrs, x, dtype)


def make_vm_model(arrs, hyper, dc, ac):
    from jittor_myc_nerfs_amd import TensorVMSplit
    m = TensorVMSplit(arrs["aabb"], [int(x) for x in arrs["gridSize"]], "cuda", density_n_comp=list(dc), appearance_n_comp=list(ac), app_dim=27,
                      near_far=hyper["near_far"], shadingMode="MLP_Fea", alphaMask_thres=1e-4, density_shift=hyper["density_shift"],
                      distance_scale=hyper["distance_scale"], rayMarch_weight_thres=hyper["rayMarch_weight_thres"], pos_pe=6, view_pe=2, fea_pe=2,
                      featureC=128, step_ratio=hyper["step_ratio"], fea2denseAct=hyper["fea2denseAct"])
    return m.load_arrays(arrs)


GAUSS_NODE = (7, 10, 12)             # the node of the TINY grid (16 x 20 x 24) the Gaussian blob sits on, per axis x, y, z
GAUSS_WIDTH = (0.50, 0.45, 0.55)     # normalised units


def gaussian_cp_arrays(peak=32.0):
    """A rank-1 CP scene whose three density lines are positive Gaussians sampled on the grid, each centred ON a grid node: the field is unimodal and symmetric
    about that node along every axis (within the 7 nodes either side that every line has).  Appearance and network: cp_common.cp_arrays(1, 1)."""
    arrs = dict(CC.cp_arrays(1, 1))
    gs = [int(x) for x in TINY["gridSize"]]
    for i in range(3):
        axis = CC.VEC_MODE[i]
        t = np.linspace(-1.0, 1.0, gs[axis])
        ln = np.exp(-((t - t[GAUSS_NODE[axis]]) / GAUSS_WIDTH[axis]) ** 2) * (peak if i == 0 else 1.0)
        arrs[f"density_line.{i}"] = ln[None, None, :, None].astype(np.float32)
    return arrs


def gaussian_centre_world():
    aabb = np.asarray(TINY["aabb"], np.float64)
    gs = np.asarray(TINY["gridSize"], np.float64)
    return aabb[0] + np.asarray(GAUSS_NODE, np.float64) / (gs - 1) * (aabb[1] - aabb[0])
