"""Shared by tests/test_cp_train_host.py and tests/test_gpu_cp_train.py: a float64 reference of TensorCP's TRAINING march and features, written from the formulas
(tensorBase.py:17-24 raw2alpha, :444-448 feature2density, :487-527 the march and compositing of execute; tensoRF.py:345-376 the CP field), the inputs both files run it on,
and the conditions that keep those inputs from being vacuous.

It follows tests/march_backward_common.py, whose pieces it reuses: the fp32 oracle's sample positions, in-box and alpha-mask tests are INPUTS (march_backward_common.sample),
the early exit is restated in chunks of 64 (march_backward_common.walk), the march's scalar loss is
    L = sum_rj [w_rj > thres] g(x_rj) w_rj + sum_r a_r acc_r
with march_backward_common.g_of, and rays on which an fp32 / fp64 flip of a threshold is not the kernel's error are dropped by that file's border rule, at most MAX_DROPPED
of them.  The CP field itself is cp_common._line_points on float64 leaves.

MUTATIONS are deliberate defects of the REFERENCE; tests/test_cp_train_host.py asserts that the 5e-4 bar sees each of them on these inputs."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import cp_common as CC
import march_backward_common as MB
from conftest import TINY

BAR_GRAD, BAR_FWD, MAX_DROPPED, CHUNK = MB.BAR_GRAD, MB.BAR_FWD, MB.MAX_DROPPED, MB.CHUNK
POSES = (2, 5, 7)          # frames of rays.sphere_poses(8, 4.0): 18 / 16 / 7 / 5 of the 768 rays fall to the border rule at ranks (96,288) / (16,48) / (5,50) / (1,1)
RANKS = CC.RANKS
MUTATIONS = ("lines_0_2_swapped", "uw_swapped", "T_not_carried", "basis_transposed")
DENSITY_NAMES = [f"density_line.{i}" for i in range(3)]
APP_NAMES = [f"app_line.{i}" for i in range(3)] + ["basis_mat"]
NET_NAMES = ["W1", "b1", "W2", "b2", "W3", "b3"]


def hyper(act="softplus"):
    return MB.hyper(act=act)                                # step ratio 0.15: S = 210 on the tiny grid, three full chunks and one of 18


def n_samples(hyp):
    return int(CC.oracle_scene(CC.cp_arrays(1, 1), hyp).nSamples)


def mirror_in_cell(x, L):
    """the coordinate at which the two taps' weights are exchanged: f -> 2 floor(f) + 1 - f on an axis of L points (mutation uw_swapped)"""
    f = (x + 1.0) / 2.0 * (L - 1)
    fl = torch.floor(f)
    return (2.0 * fl + 1.0 - f) / (L - 1) * 2.0 - 1.0


def field_lines(lines, xyz, mutation=None):
    """[R, m] float64: prod_i line_i(xyz[vecMode[i]]) through cp_common._line_points; the two field mutations change the coordinates it is given"""
    if mutation == "lines_0_2_swapped":                     # line 0 read at x and line 2 at z: vecMode [0, 1, 2]
        xyz = torch.stack((xyz[:, 2], xyz[:, 1], xyz[:, 0]), -1)
    elif mutation == "uw_swapped":
        gx, gy, gz = (int(lines[2].shape[2]), int(lines[1].shape[2]), int(lines[0].shape[2]))
        xyz = torch.stack((mirror_in_cell(xyz[:, 0], gx), mirror_in_cell(xyz[:, 1], gy), mirror_in_cell(xyz[:, 2], gz)), -1)
    return CC._line_points(lines, xyz, torch.float64)


class _BasisProduct(torch.autograd.Function):
    """features = h^T B^T with, under the mutation, B read transposed (as [R, 27] memory taken for [27, R]) where the backward forms dh"""

    @staticmethod
    def forward(ctx, h, B, transposed):
        ctx.save_for_backward(h, B)
        ctx.transposed = transposed
        return h.T @ B.T

    @staticmethod
    def backward(ctx, dF):
        h, B = ctx.saved_tensors
        Bd = B.T.contiguous().view(B.shape) if ctx.transposed else B
        return (dF @ Bd).T, dF.T @ h.T, None


def features64(app_lines, basis, xyz, mutation=None):
    """tensoRF.py:362-376 in float64: [m,27]"""
    h = field_lines(app_lines, xyz, None)
    return _BasisProduct.apply(h, basis, mutation == "basis_transposed")


def leaves_of(arrs, names, grad=True):
    return [torch.tensor(np.asarray(arrs[k]), dtype=torch.float64).requires_grad_(grad) for k in names]


def march64(case, dlines, mutation=None):
    """The differentiable part of the training march in float64 on a case's samples.  -> dict(w [n,S], acc [n], app [n,S] bool, keep, end, T_end, xyz [n,S,3])"""
    sc, smp, S = case.sc, case.smp, case.S
    valid = smp["valid"]
    n = valid.shape[0]
    xyz = smp["xyz_n"].double()
    sigma = torch.zeros((n, S), dtype=torch.float64)
    if valid.any():
        sf = field_lines(dlines, xyz[valid], mutation if mutation in ("lines_0_2_swapped", "uw_swapped") else None).sum(0)
        sigma = sigma.masked_scatter(valid, F.softplus(sf + sc.density_shift) if sc.fea2denseAct == "softplus" else F.relu(sf))      # :444-448
    z = smp["z"].double()
    dist = torch.cat((z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])), -1) * sc.distance_scale   # :488, :511
    alpha_all = 1.0 - torch.exp(-sigma * dist)                                                   # :19
    keep, end, T_end = MB.walk(alpha_all.detach(), valid, case.eps_T)
    alpha = alpha_all * keep
    T = torch.ones(n, dtype=torch.float64)
    ws = []
    for c in range(MB.n_chunks(S)):
        sl = slice(c * CHUNK, min((c + 1) * CHUNK, S))
        f = 1.0 - alpha[:, sl] + 1e-10                                                           # :21
        incl = torch.cumprod(f, 1)
        excl = torch.cat((torch.ones((n, 1), dtype=torch.float64), incl[:, :-1]), 1)
        T_in = torch.ones_like(T) if mutation == "T_not_carried" else T
        ws.append(alpha[:, sl] * (T_in[:, None] * excl))                                         # :23
        walked = (valid[:, sl] & keep[:, sl]).any(1)
        T = torch.where(walked, T * incl[:, -1], T)
    w = torch.cat(ws, 1)
    return dict(w=w, acc=w.sum(1), app=w.detach() > sc.thres, keep=keep, end=end, T_end=T_end, xyz=xyz)


def march_reference(case, leaves=None, mutation=None, grad=True):
    """the march's loss and its gradients w.r.t. the three density lines"""
    assert mutation is None or mutation in MUTATIONS
    if leaves is None:
        leaves = leaves_of(case.arrs, DENSITY_NAMES, grad)
    r = march64(case, leaves, mutation)
    g = MB.g_of(r["xyz"])
    loss = (r["app"] * g * r["w"]).sum() + (case.a * r["acc"]).sum()
    out = dict(w=r["w"].detach(), acc=r["acc"].detach(), app=r["app"], keep=r["keep"], end=r["end"], T_end=r["T_end"], xyz=r["xyz"], loss=float(loss.detach()))
    if grad:
        out["grads"] = [t.detach() for t in torch.autograd.grad(loss, leaves, allow_unused=True)]
    return out


def app_reference(arrs, xyz, G, mutation=None):
    """L = sum G * features at points xyz [m,3] (normalised): features [m,27] and the gradients of the three appearance lines and of basis_mat, float64"""
    leaves = leaves_of(arrs, APP_NAMES)
    xyz = torch.as_tensor(xyz).double()
    Fe = features64(leaves[:3], leaves[3], xyz, mutation)
    loss = (torch.as_tensor(G).double() * Fe).sum()
    return dict(features=Fe.detach(), grads=[t.detach() for t in torch.autograd.grad(loss, leaves, allow_unused=True)])


def step_reference(case, target, white_bg=True, dtype=torch.float64):
    """The whole training step (tensorBase.py:487-527 with the CP field, MSE against `target` [n,3]) under autograd in `dtype`; sample positions, masks, the appearance mask
    and the early exit are the float64 march's (detached), so the fp32 pass differs from the fp64 one by rounding alone.
    -> dict(rgb_map, loss, grads {name: tensor} for the seven parameter groups and the network)"""
    names = DENSITY_NAMES + APP_NAMES + NET_NAMES
    lv64 = leaves_of(case.arrs, DENSITY_NAMES, grad=False)
    ref = march64(case, lv64)
    leaves = [torch.tensor(np.asarray(case.arrs[k]), dtype=dtype).requires_grad_(True) for k in names]
    P = dict(zip(names, leaves))
    if dtype == torch.float64:
        m = march64(case, leaves[:3])
        w = m["w"]
    else:
        w = _march32(case, leaves[:3], ref["keep"])
    app = ref["app"]
    xyz_app = ref["xyz"][app].to(dtype)
    h = CC._line_points(leaves[3:6], xyz_app, dtype)
    feats = h.T @ P["basis_mat"].T
    sc = CC.oracle_scene(case.arrs, case.hyper, dtype)
    sc.mlp = {k: P[k] for k in NET_NAMES}
    rays = torch.as_tensor(case.rays)
    view = rays[:, None, 3:6].expand(-1, case.S, -1)[app].to(dtype)
    from oracle import tensorf_oracle as TO
    rgb = TO.mlp_render_fea(sc, view, feats)
    n = case.n
    ray_id = torch.nonzero(app)[:, 0]
    rgb_map = torch.zeros((n, 3), dtype=dtype).index_add(0, ray_id, w[app][:, None] * rgb)
    if white_bg:
        rgb_map = rgb_map + (1.0 - w.sum(1)[:, None])
    rgb_map = rgb_map.clamp(0, 1)
    loss = ((rgb_map - torch.as_tensor(target).to(dtype)) ** 2).mean()
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    return dict(rgb_map=rgb_map.detach(), loss=float(loss.detach()), grads={k: g.detach() for k, g in zip(names, grads)}, n_app=int(app.sum()))


def _march32(case, dlines, keep):
    """march64's arithmetic in float32 (the error a torch fp32 restatement makes: cp_common.allowance's yardstick); the early exit is the float64 walk's"""
    sc, smp, S = case.sc, case.smp, case.S
    valid = smp["valid"]
    n = valid.shape[0]
    sigma = torch.zeros((n, S), dtype=torch.float32)
    if valid.any():
        sf = CC._line_points(dlines, smp["xyz_n"][valid], torch.float32).sum(0)
        sigma = sigma.masked_scatter(valid, F.softplus(sf + sc.density_shift) if sc.fea2denseAct == "softplus" else F.relu(sf))
    z = smp["z"]
    dist = torch.cat((z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])), -1) * sc.distance_scale
    alpha = (1.0 - torch.exp(-sigma * dist)) * keep
    T = torch.cumprod(torch.cat((torch.ones((n, 1)), 1.0 - alpha + 1e-10), 1), 1)[:, :-1]
    return alpha * T


def march_reference32(case):
    """{w, acc, grads} of the march's loss through the fp32 restatement, for cp_common.allowance"""
    leaves = [torch.tensor(np.asarray(case.arrs[k]), dtype=torch.float32).requires_grad_(True) for k in DENSITY_NAMES]
    ref = case.ref()
    w = _march32(case, leaves, ref["keep"])
    g = MB.g_of(ref["xyz"]).float()
    loss = (ref["app"] * g * w).sum() + (case.a.float() * w.sum(1)).sum()
    return dict(w=w.detach(), acc=w.sum(1).detach(), grads=[t.detach() for t in torch.autograd.grad(loss, leaves)])


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------
class CpCase:
    """march_backward_common.Case for a CP scene: arrays (cp_common.cp_arrays, optionally with alpha_volume / alpha_aabb) + hyper-parameters, rays, S, eps_T, jitter, and
    the oracle's sampling of the rays the border rule keeps."""

    def __init__(self, arrs, hyp, rays, S, eps_T, jitter=False, seed=0):
        self.arrs, self.hyper, self.S, self.eps_T = arrs, hyp, int(S), float(eps_T)
        self.sc = CC.oracle_scene(arrs, hyp)
        rng = np.random.default_rng(1000 + seed)
        n0 = rays.shape[0]
        self.rays = np.ascontiguousarray(rays, np.float32)
        self.jitter = rng.random(n0).astype(np.float32) if jitter else None
        self.a = torch.tensor(rng.standard_normal(n0))
        self.smp = MB.sample(self.sc, self.rays, self.S, self.jitter)
        r = march_reference(self, grad=False)
        border = ((r["w"] / self.sc.thres - 1.0).abs() < 1e-3).any(1)
        if self.eps_T > 0:
            border |= ((r["T_end"] / self.eps_T - 1.0).abs() < 1e-2).any(1)                  # (nan behind a ray's end compares False)
        self.n_dropped, self.n_before = int(border.sum()), n0
        kept = ~border
        kn = kept.numpy()
        self.rays = np.ascontiguousarray(self.rays[kn])
        self.jitter = None if self.jitter is None else np.ascontiguousarray(self.jitter[kn])
        self.a = self.a[kept]
        self.smp = {k: v[kept] for k, v in self.smp.items()}
        self._ref = {}

    @property
    def n(self):
        return self.rays.shape[0]

    def ref(self, mutation=None):
        if mutation not in self._ref:
            self._ref[mutation] = march_reference(self, mutation=mutation)
        return self._ref[mutation]

    def stats(self):
        r = self.ref()
        nc = MB.n_chunks(self.S)
        return dict(n=self.n, dropped=self.n_dropped, before=self.n_before, miss=int((~self.smp["bbox"].any(1)).sum()), n_app=int(r["app"].sum()),
                    ends_in=[int((r["end"] == c).sum()) for c in range(nc)], never_ends=int((r["end"] < 0).sum()),
                    masked=int((self.smp["bbox"] & ~self.smp["valid"]).sum()))

    def assert_not_vacuous(self):
        """the conditions every test asserts: the border rule's cap, rays that end early, rays that never end, rays that miss the box, appearance samples"""
        s = self.stats()
        assert s["dropped"] <= MAX_DROPPED * s["before"], s
        assert s["n_app"] > 0 and s["never_ends"] > 0, s
        return s


@functools.lru_cache(maxsize=None)
def frames():
    return MB.frames(poses=POSES)


@functools.lru_cache(maxsize=None)
def cp_case(r, jitter=False, act="softplus", eps_T=1e-4):
    """the tiny 16x20x24 grid at ranks r, 768 rays of three 16x16 frames, S = 210"""
    hyp = hyper(act)
    return CpCase(CC.cp_arrays(*r), hyp, frames(), n_samples(hyp), eps_T, jitter=jitter, seed=r[0])


def masked_case(arrs, eps_T=1e-4):
    """the (16,48) case on arrays that carry an alpha mask (alpha_volume / alpha_aabb, as TensorBase.updateAlphaMask left them)"""
    hyp = hyper()
    return CpCase(arrs, hyp, frames(), n_samples(hyp), eps_T, seed=77)


def app_points(kind, m, seed=0):
    """[m,3] fp32 normalised points of tests/test_gpu_cp_train.py's tvr_cp_app_backward cases on the tiny grid (gx, gy, gz = 16, 20, 24)"""
    rng = np.random.default_rng(100 + seed)
    g = np.asarray(TINY["gridSize"], np.float64)
    if kind == "random":                                    # every entry jumps cells
        p = rng.uniform(-1.0, 1.0, (m, 3))
    elif kind == "one_cell":                                # a sorted run inside one cell: the windows never flush before the end
        lo = (np.array([5.0, 7.0, 11.0]) + 0.02) / (g - 1) * 2 - 1
        hi = (np.array([5.0, 7.0, 11.0]) + 0.98) / (g - 1) * 2 - 1
        p = lo + np.sort(rng.random((m, 1)), 0) * (hi - lo)
    elif kind == "upper_boundary":                          # coordinate +1 on one axis per point: the lower tap is L - 1 and the upper one is the pad, weight 0
        p = rng.uniform(-1.0, 1.0, (m, 3))
        p[np.arange(m), rng.integers(0, 3, m)] = 1.0
    elif kind == "outside":                                 # beyond one cell outside [-1, 1]^3 on at least one axis: every tap of that axis has weight 0
        p = rng.uniform(-1.0, 1.0, (m, 3))
        ax = rng.integers(0, 3, m)
        p[np.arange(m), ax] = rng.choice([-1.0, 1.0], m) * rng.uniform(1.3, 1.8, m)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p, np.float32)
