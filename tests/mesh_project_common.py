"""Shared by tests/test_mesh_project_host.py and tests/test_gpu_mesh_project.py: the tests' own restatement of tvr_mesh_project (include/tvr.h) in torch on the CPU,
in any dtype, written from the header's definition and NOT from the kernel — it is vectorised over the vertices with masks where the kernel iterates lanes — and a
numpy extractor of iso-surface edge crossings, so that the host test has marching-cubes-like vertices without a GPU.

The field is oracle.tensorf_oracle.compute_densityfeature (VM) or cp_common.cp_density (CP).  In fp64 every quantity behind the fp32 input vertices (normalised
coordinate, shifted coordinate, field, step, clamps) is fp64: it is the mathematics the kernel's fp32 approximates, not a bit model of it."""
import math

import numpy as np
import torch

import cp_common as CC
import gradient_common as GC
from conftest import TINY

LEVELS = (0.0005, 0.05)
ITERATIONS = 8


def field(kind, arrs, hyper, dtype):
    """x [m,3] normalised coordinates in `dtype` -> density feature [m] in `dtype`"""
    return GC.vm_density(arrs, hyper, dtype) if kind == "vm" else GC.cp_density_fn(arrs, dtype)


def step_size(aabb, gridSize, step_ratio):
    """TensorBase.update_stepSize in fp32: mean(extent / (gridSize - 1)) * step_ratio"""
    aabb = torch.as_tensor(np.asarray(aabb), dtype=torch.float32).reshape(2, 3)
    g = torch.tensor([int(x) for x in gridSize], dtype=torch.int32)
    return float(torch.mean((aabb[1] - aabb[0]) / (g - 1)) * step_ratio)


def units(aabb, gridSize):
    aabb = torch.as_tensor(np.asarray(aabb), dtype=torch.float32).reshape(2, 3)
    g = torch.tensor([int(x) for x in gridSize], dtype=torch.int32)
    return (aabb[1] - aabb[0]) / (g - 1)


def target_feature(level, length, hyper):
    """f* in fp64, restated: the feature at which 1 - exp(-feature2density(f) * length) == level"""
    sigma = -math.log1p(-level) / length
    if hyper["fea2denseAct"] == "softplus":
        return math.log(math.expm1(sigma)) - float(hyper["density_shift"])
    return sigma


def alpha_of_feature(f, length, hyper):
    """compute_alpha's formula (tensorBase.py:451-473, no mask) on a feature tensor"""
    sigma = torch.nn.functional.softplus(f + hyper["density_shift"]) if hyper["fea2denseAct"] == "softplus" else torch.relu(f)
    return 1.0 - torch.exp(-sigma * length)


def quarter_cell(gridSize):
    return GC.cell(gridSize) * 0.25


def default_tol(target):
    return 1e-3 * max(1.0, abs(target))


def normalize(p, aabb, dtype):
    aabb = torch.as_tensor(np.asarray(aabb), dtype=torch.float32).reshape(2, 3)
    return (p.to(dtype) - aabb[0].to(dtype)) * (2.0 / (aabb[1] - aabb[0])).to(dtype) - 1.0


def feature_and_gradient(f, n, h):
    """(f(n), symmetric-difference gradient) with n and h in the same dtype"""
    cols = []
    for k in range(3):
        e = torch.zeros(3, dtype=n.dtype)
        e[k] = h[k]
        cols.append((f(n + e) - f(n - e)) * (0.5 / h[k]))
    return f(n), torch.stack(cols, -1)


def project_restatement(f, verts32, aabb, target, iterations, h32, max_move32, tol, dtype, pinned=None):
    """include/tvr.h tvr_mesh_project, PER VERTEX, in `dtype`.  f: field(...) of that dtype.  Returns a dict of out [V,3], residual_in, residual_out and the bool
    masks converged / moved / clamped / nonfinite."""
    aabb = torch.as_tensor(np.asarray(aabb), dtype=torch.float32).reshape(2, 3)
    lo, hi, inv = aabb[0].to(dtype), aabb[1].to(dtype), (2.0 / (aabb[1] - aabb[0])).to(dtype)
    h, mm = h32.to(dtype), torch.as_tensor(max_move32, dtype=torch.float32).to(dtype)
    target = torch.tensor(float(np.float32(target)), dtype=dtype)          # the one float the library is handed
    p0 = verts32.to(dtype)
    V = p0.shape[0]
    p, best = p0.clone(), p0.clone()
    best_a = torch.full((V,), float("inf"), dtype=dtype)
    have_best = torch.zeros(V, dtype=torch.bool)
    nonfinite = ~torch.isfinite(p0).all(-1)
    held = nonfinite.clone()
    converged, clamped = torch.zeros(V, dtype=torch.bool), torch.zeros(V, dtype=torch.bool)
    pin = torch.zeros(V, dtype=torch.bool) if pinned is None else pinned.bool()
    r0 = best_r = None
    for k in range(iterations + 1):
        fk, g = feature_and_gradient(f, (p - lo) * inv - 1.0, h)
        r = fk - target
        if k == 0:
            r0, best_r = r.clone(), r.clone()
        bad = ~held & ~torch.isfinite(r)
        nonfinite |= bad
        held |= bad
        a = r.abs()
        better = ~held & (~have_best | (a < best_a))
        best[better], best_r[better], best_a[better] = p[better], r[better], a[better]
        have_best |= better
        conv = ~held & (a <= tol)
        converged |= conv
        held |= conv | pin
        if k == iterations:
            break
        gw = g * inv
        s = r / torch.clamp((gw[:, 0] * gw[:, 0] + gw[:, 1] * gw[:, 1]) + gw[:, 2] * gw[:, 2], min=1e-30)
        q = p - s[:, None] * gw
        badq = ~held & ~torch.isfinite(q).all(-1)
        nonfinite |= badq
        held |= badq
        c = torch.minimum(torch.maximum(q, p0 - mm), p0 + mm)
        c = torch.minimum(torch.maximum(c, lo), hi)
        step = ~held
        clamped |= step & (c != q).any(-1)
        p = torch.where(step[:, None], c, p)
    moved = (best != p0).any(-1) & torch.isfinite(p0).all(-1)
    return dict(out=best, residual_in=r0, residual_out=best_r, converged=converged, moved=moved, clamped=clamped, nonfinite=nonfinite)


def edge_crossings(alpha, level, origin, voxel):
    """float32 [V,3]: where the iso-surface alpha == level crosses the edges of the sample grid alpha [nx,ny,nz] (numpy), by linear interpolation along the edge —
    the positions a marching-cubes extractor places its vertices at, without the triangles.  Sample (i, j, k) sits at origin + (i, j, k) * voxel."""
    alpha = np.asarray(alpha, np.float64)
    origin, voxel = np.asarray(origin, np.float64), np.asarray(voxel, np.float64)
    out = []
    for axis in range(3):
        a0 = np.take(alpha, np.arange(alpha.shape[axis] - 1), axis)
        a1 = np.take(alpha, np.arange(1, alpha.shape[axis]), axis)
        idx = np.argwhere((a0 < level) != (a1 < level))
        if not len(idx):
            continue
        v0, v1 = a0[tuple(idx.T)], a1[tuple(idx.T)]
        pos = idx.astype(np.float64)
        pos[:, axis] += (level - v0) / (v1 - v0)
        out.append(origin + pos * voxel)
    return np.concatenate(out).astype(np.float32) if out else np.zeros((0, 3), np.float32)


def dense_alpha(f64, aabb, gridSize, length, hyper):
    """getDenseAlpha without a mask, in fp64 on the CPU: alpha [nx,ny,nz] at aabb[0] * (1 - s) + aabb[1] * s, s = linspace(0, 1, n) (fp32 positions, as the model's)"""
    aabb = torch.as_tensor(np.asarray(aabb), dtype=torch.float32).reshape(2, 3)
    gs = [int(g) for g in gridSize]
    s = torch.stack(torch.meshgrid(*[torch.linspace(0, 1, g) for g in gs], indexing="ij"), -1)
    xyz = (aabb[0] * (1 - s) + aabb[1] * s).view(-1, 3)
    return alpha_of_feature(f64(normalize(xyz, aabb, torch.float64)), length, hyper).view(gs).numpy()


def surface_vertices(f64, aabb, gridSize, level, length, hyper):
    """edge crossings of the level set on a grid of gridSize samples spanning the aabb (spacing "samples": vertices lie where the field was sampled)"""
    a = np.asarray(aabb, np.float64).reshape(2, 3)
    voxel = (a[1] - a[0]) / (np.asarray([int(g) for g in gridSize], np.float64) - 1)
    return torch.from_numpy(edge_crossings(dense_alpha(f64, aabb, gridSize, length, hyper), level, a[0], voxel))


def scene(name, tiny_arrays):
    """(kind, arrays) of the scenes both test files use: "vm" = the tiny golden scene, "cp-R" = the synthetic CP scene of density rank R"""
    if name == "vm":
        return "vm", tiny_arrays
    r = int(name.split("-")[1])
    return "cp", CC.cp_arrays(r, dict(CC.RANKS)[r])


GRID = [int(g) for g in TINY["gridSize"]]
