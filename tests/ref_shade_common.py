"""Shared by tests/test_ref_shade_host.py and tests/test_gpu_ref_kernels.py: a float64 reference of REFTensoRF's appearance branch (the four heads, the normalised
normal, the reflection, -dot, MLPRender_Fea_Ref and the colour mix), the inputs the two test files run it on, and the conditions that keep those inputs from being
vacuous.

The reference is written from the formulas (REFTensoRF.py:107-133 the heads, :217-239 normalisation, reflection, network, colour mix, penalty; jt.normalize as
oracle/tensorf_oracle.py:jt_normalize restates it), in torch on the CPU, float64 unless asked otherwise:

    f = h B^T                    n = h Wn^T + bn          tint_raw = h Ws^T + bs        rgb_d = h Wd^T + bd
    nh = n / sqrt(max(n.n, 1e-30))      d = -view      dot = d.nh      refl = 2 dot nh - d      in0 = -dot
    X = [in0, f, refl, PE2(f), PE2(refl)]   (151 columns)      rgb_s = sigmoid(MLP(X))      rgb = relu(tint_raw) * rgb_s + rgb_d

Scalar loss both sides differentiate:
    L = sum(rgb * cw) + sum(a * relu(in0)^2)
with cw ~ 3e-5 (the size of a real loss gradient: MSE mean over a 4096-ray batch) and a >= 0 seeded per sample; the form without the second term leaves the
autograd function's grad_in0 NULL.

MUTATIONS are deliberate defects of the REFERENCE's gradient (its forward values stay): each restates one way a backward kernel could be wrong, and
tests/test_ref_shade_host.py asserts that the 2e-4 bar would see it on these inputs.

The second half holds the whole-step case of tests/test_gpu_ref_kernels.py: the long-ray case of tests/march_backward_common.py (S = 192, early exit on) with the
REFTensoRF arrays and a diffuse bias shifted so that pixels leave [0, 1] on both sides."""
import functools
import os

import numpy as np
import torch

import march_backward_common as MB
from conftest import GOLDEN

BAR_FWD = 2e-5             # rgb, in0 (and the saved forward tensors), absolute: tests/test_gpu_training.py::test_fused_mlp_training_kernels_match_float64_autograd's bar
BAR_GRAD = 2e-4            # max |g - g_ref| / max |g_ref| per tensor: the same test's
MS = (37, 4099, 10007)     # one ragged 32-tile; just past the 4096 switch to tvr_gemm_tn; many groups, ragged for 32, 128 and 256
CW_SIZE = 3e-5
SPIKE = (4099, 1234)       # (M, row) of the batch with one colour gradient 1e3 times the others'
# |tint_raw| of every row is kept this far from the gate: relu'(tint_raw) is the one discontinuous factor outside the network, and a row whose fp32 tint lands on the
# other side of zero than its fp64 tint is a difference of the inputs' rounding, not of the kernels (the heads' fp32 products round at ~1e-6)
TINT_MARGIN = 1e-4
MUTATIONS = ("tint_gate_ignored", "projection_dropped", "inv_norm_dropped", "din0_wrong_sign", "grad_in0_not_added", "dot_row_omitted_from_dW1",
             "factor_2_dropped", "heads_dh_dropped", "heads_dh_doubled")
PARAM_NAMES = ("basis_mat", "normal_W", "normal_b", "diffuse_W", "diffuse_b", "specular_W", "specular_b", "rho_W", "rho_b", "W1", "b1", "W2", "b2", "W3", "b3")
GRAD_NAMES = ("dh",) + PARAM_NAMES


@functools.lru_cache(maxsize=None)
def ref_arrays():
    """the tiny scene's arrays with those tests/golden/tiny_ref.npz adds or replaces (what conftest.tiny_ref_arrays holds)"""
    a = dict(MB.tiny_arrays())
    d = np.load(os.path.join(GOLDEN, "tiny_ref.npz"))
    a.update({k[len("scene."):]: d[k] for k in d.files if k.startswith("scene.")})
    return a


def pe2(x):
    """tensorBase.py:9-15 with two frequencies, in x's dtype"""
    pts = (x[..., None] * torch.tensor([1.0, 2.0], dtype=x.dtype)).reshape(x.shape[0], -1)
    return torch.cat([torch.sin(pts), torch.cos(pts)], dim=-1)


class _ScaleGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return g * ctx.s, None


def _scale_grad(x, s):
    """x in the forward, s * (the incoming gradient) in the backward; s a number or a detached tensor"""
    return _ScaleGrad.apply(x, s)


def shade(h, view, P, mutation=None):
    """The appearance branch on h [M,144], view [M,3], P = {name: tensor} (PARAM_NAMES), all of one dtype.
    -> dict(f, n, tint_raw, rgb_d, nh, dot, refl, in0, X, rgb_s, rgb).  A mutation changes gradients only."""
    assert mutation is None or mutation in MUTATIONS
    hh = h                                                                                   # what the heads see
    if mutation == "heads_dh_dropped":
        hh = h.detach()
    elif mutation == "heads_dh_doubled":
        hh = _scale_grad(h, 2.0)
    f = h @ P["basis_mat"].T
    n = hh @ P["normal_W"].T + P["normal_b"]
    tint_raw = hh @ P["specular_W"].T + P["specular_b"]
    rgb_d = hh @ P["diffuse_W"].T + P["diffuse_b"]
    rho_raw = hh @ P["rho_W"].T + P["rho_b"]                                                 # k = 1 / relu(rho) is handed to MLPRender_Fea_Ref and unused there (:18)
    if mutation == "inv_norm_dropped":                                                       # d n = d nh - nh (nh . d nh)
        n = _scale_grad(n, n.detach().norm(dim=-1, keepdim=True))
    nrm = torch.sqrt(torch.clamp((n * n).sum(-1, keepdim=True), min=1e-30))
    nh = n / (nrm.detach() if mutation == "projection_dropped" else nrm)                     # mutated: d n = d nh / |n|
    d = -view
    dot = (d * nh).sum(-1, keepdim=True)
    nh_direct = _scale_grad(nh, 0.5) if mutation == "factor_2_dropped" else nh               # d refl / d nh at fixed dot = 2 dot I
    refl = 2.0 * dot * nh_direct - d
    in0 = -dot
    if mutation == "din0_wrong_sign":                                                        # d dot = 2 nh . d refl + d in0
        in0 = _scale_grad(in0, -1.0)
    W1 = P["W1"]
    if mutation == "dot_row_omitted_from_dW1":
        W1 = torch.cat([W1[:, :1].detach(), W1[:, 1:]], dim=1)
    X = torch.cat([in0, f, refl, pe2(f), pe2(refl)], dim=-1)
    rgb_s = torch.sigmoid(torch.relu(torch.relu(X @ W1.T + P["b1"]) @ P["W2"].T + P["b2"]) @ P["W3"].T + P["b3"])
    gate = torch.relu(tint_raw)
    if mutation == "tint_gate_ignored":                                                      # d tint_raw = sum_c grad_rgb_c rgb_s_c on every row
        gate = gate.detach() + (tint_raw - tint_raw.detach())
    rgb = gate * torch.clamp(rgb_s, min=0) + rgb_d                                           # :232
    return dict(f=f, n=n, tint_raw=tint_raw, rgb_d=rgb_d, rho_raw=rho_raw, nh=nh, dot=dot, refl=refl, in0=in0[:, 0], X=X, rgb_s=rgb_s, rgb=rgb)


def loss_of(out, cw, a, with_in0, mutation=None):
    loss = (out["rgb"] * cw).sum()
    if with_in0:
        in0 = out["in0"].detach() if mutation == "grad_in0_not_added" else out["in0"]
        loss = loss + (a * torch.relu(in0) ** 2).sum()
    return loss


class Inputs:
    """One vetted batch: h [M,144], unit view directions, cw, a (float64), the parameters (the golden REFTensoRF arrays with moved head biases) as numpy fp32 arrays
    (what conftest.make_model takes) and as float64 tensors."""

    def __init__(self, M, spike_row=None):
        self.M = int(M)
        arrs = dict(ref_arrays())
        g = torch.Generator().manual_seed(1000 + self.M)
        W = {k: torch.tensor(arrs[k], dtype=torch.float64) for k in PARAM_NAMES}
        # 1.25 x M candidate rows; the first M whose tint stays TINT_MARGIN off the gate are kept
        n_cand = self.M + self.M // 4 + 16
        h = (0.7 * torch.randn((n_cand, 144), generator=g, dtype=torch.float64)).float().double()      # fp32-representable: both sides start from the same numbers
        v = torch.randn((n_cand, 3), generator=g, dtype=torch.float64)
        v = (v / v.norm(dim=-1, keepdim=True)).float().double()
        # the head biases, moved: the golden scene's tint is positive on 98.7 % of its samples and its normal bias is small against h Wn^T
        #   specular: the median of h Ws^T to zero -> the gate is closed on half of the rows;
        #   normal  : a bias of the size of h Wn^T's spread along (1, -1, 1) / sqrt(3): |n| stays away from zero (the clamp branch n.n <= 1e-30 is out of scope: the
        #             reference's own gradient there is scaled by 1e15), the sign of -dot is decided by the seeded view directions
        #   specular weights: times 2^-6 (exact).  The golden weights are sized for h = plane * line products (|h| ~ 0.05); on h = 0.7 randn they give a tint of +-60,
        #             which multiplies the network's fp32 rounding (1e-6 on rgb_s) past the 2e-5 forward bar whatever computes it: the fp32 evaluation of this very
        #             reference then misses its float64 self by 1.4e-4.  With the scale the tint is of order one, as on a real scene
        #   diffuse weights: times 2^-5, for the same reason: |rgb_d| reaches 26 on these h, and the rounding of its own 144-term fp32 sum (1.8e-5) sits at the bar
        arrs["specular_W"] = (np.asarray(arrs["specular_W"], np.float32) * np.float32(2.0 ** -6)).astype(np.float32)
        arrs["diffuse_W"] = (np.asarray(arrs["diffuse_W"], np.float32) * np.float32(2.0 ** -5)).astype(np.float32)
        W["specular_W"] = torch.tensor(arrs["specular_W"], dtype=torch.float64)
        t0 = h @ W["specular_W"].T
        n0 = h @ W["normal_W"].T
        arrs["specular_b"] = np.asarray([-float(t0.median())], np.float32)
        arrs["normal_b"] = (2.0 * float(n0.std()) * np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)).astype(np.float32)
        self.arrs = arrs
        self.P64 = {k: torch.tensor(arrs[k], dtype=torch.float64) for k in PARAM_NAMES}
        tint = h @ self.P64["specular_W"].T + self.P64["specular_b"]
        ok = torch.nonzero(tint[:, 0].abs() > TINT_MARGIN)[:, 0][:self.M]
        assert ok.shape[0] == self.M
        self.n_skipped = int(ok[-1]) + 1 - self.M
        self.h, self.view = h[ok].contiguous(), v[ok].contiguous()
        self.cw = (CW_SIZE * torch.randn((self.M, 3), generator=g, dtype=torch.float64)).float().double()
        if spike_row is not None:                                                                       # one row's colour gradient 1e3 times the others'
            self.cw[spike_row] = self.cw[spike_row] * 1e3
        self.a = (CW_SIZE * torch.rand((self.M,), generator=g, dtype=torch.float64)).float().double()
        self._ref = {}

    def leaves(self, dtype=torch.float64):
        h = self.h.to(dtype).requires_grad_(True)
        P = {k: v.to(dtype).requires_grad_(True) for k, v in self.P64.items()}
        return h, P

    def run(self, with_in0=True, mutation=None, dtype=torch.float64):
        """-> dict(rgb, in0, the forward's intermediates, grads = {GRAD_NAMES: tensor}) of the reference in `dtype`"""
        key = (with_in0, mutation, dtype)
        if key not in self._ref:
            h, P = self.leaves(dtype)
            out = shade(h, self.view.to(dtype), P, mutation)
            loss = loss_of(out, self.cw.to(dtype), self.a.to(dtype), with_in0, mutation)
            gs = torch.autograd.grad(loss, [h] + [P[k] for k in PARAM_NAMES], allow_unused=True)
            res = {k: v.detach() for k, v in out.items()}
            res["grads"] = {k: (torch.zeros_like(x) if gx is None else gx.detach()) for k, x, gx in zip(GRAD_NAMES, [h] + [P[k] for k in PARAM_NAMES], gs)}
            self._ref[key] = res
        return self._ref[key]

    def stats(self):
        r = self.run()
        nn = r["n"].norm(dim=-1)
        return dict(M=self.M, skipped=self.n_skipped, tint_closed=float((r["tint_raw"] <= 0).double().mean()), in0_pos=float((r["in0"] > 0).double().mean()),
                    n_min=float(nn.min()), n_median=float(nn.median()), tint_margin=float(r["tint_raw"].abs().min()))


@functools.lru_cache(maxsize=None)
def inputs(M, spike_row=None):
    return Inputs(M, spike_row)


def rel_err(g, ref):
    return MB.rel_err(g, ref)


def worst_move(a, b):
    """the largest rel_err over the gradient tensors of two reference runs (b the reference): (name, value)"""
    moves = {k: rel_err(a["grads"][k], b["grads"][k]) for k in GRAD_NAMES if float(b["grads"][k].abs().max()) > 0}
    k = max(moves, key=moves.get)
    return k, moves[k]


# ---- the whole step past one chunk, with early exit and the clamp ---------------------------------------------------------------------------------
STEP_CASE = "S192-eps0.0001-nojitter"
# added to diffuse_b: the red channel is pushed below 0, the blue one above 1, green stays; found with the oracle (tests/test_ref_shade_host.py asserts what it gives)
DIFFUSE_SHIFT = (-1.5, 0.0, 1.5)
CLAMP_MARGIN = MB.BAR_FWD  # a pixel channel this close to 0 or 1 before the clamp may fall on either side in a forward that meets the whole step's bar: its cw is zero


def step_case():
    return MB.KERNEL_CASES[STEP_CASE]()


@functools.lru_cache(maxsize=None)
def step_arrays():
    c = step_case()
    a = dict(c.arrs)
    r = ref_arrays()
    for k in ("W1", "b1", "normal_W", "normal_b", "diffuse_W", "diffuse_b", "specular_W", "specular_b", "rho_W", "rho_b"):
        a[k] = r[k]
    a["diffuse_b"] = (np.asarray(r["diffuse_b"], np.float32) + np.asarray(DIFFUSE_SHIFT, np.float32)).astype(np.float32)
    return a


def step_leaves(sc):
    leaves = {f"{name}.{i}": t for name in ("density_plane", "density_line", "app_plane", "app_line") for i, t in enumerate(getattr(sc, name))}
    leaves["basis_mat"] = sc.basis_mat
    leaves.update(sc.mlp)
    leaves.update({k: t for k, t in sc.ref.items() if not k.startswith("rho")})              # rho feeds only the unused k argument of MLPRender_Fea_Ref: no gradient
    return leaves


@functools.lru_cache(maxsize=None)
def step_forward(white_bg):
    """the oracle's forward on the step case: the pixels before the clamp [n,3], the number of appearance samples, the penalty"""
    from oracle import tensorf_oracle as TO
    c = step_case()
    sc = TO.scene_from_arrays(step_arrays(), **c.hyper)
    keep = c.keep_mask()
    with torch.no_grad():
        d = TO.execute(sc, torch.tensor(c.rays), white_bg=white_bg, N_samples=c.S, sample_keep=keep, dump=True)
    pre = torch.sum(d["weight"][..., None] * d["rgb"], -2)                                    # tensorBase.py:524-527
    if white_bg:
        pre = pre + (1.0 - d["acc_map"][..., None])
    assert torch.equal(pre.clamp(0, 1), d["rgb_map"])
    return dict(pre=pre, M=int(d["app_mask"].sum()), penalty=float(sc.penalty), rgb_map=d["rgb_map"])


def step_cw(white_bg, which="free"):
    """cw [n,3] fp32, seeded.  "free": zero within CLAMP_MARGIN of a clamp edge, random elsewhere (clamped channels included: their gradient must vanish);
    "clamped": non-zero only on channels the oracle clamps by more than CLAMP_MARGIN."""
    pre = step_forward(white_bg)["pre"]
    cw = torch.tensor(np.random.default_rng(12).standard_normal(tuple(pre.shape)).astype(np.float32))
    near = ((pre - 0.0).abs() < CLAMP_MARGIN) | ((pre - 1.0).abs() < CLAMP_MARGIN)
    out = (pre < -CLAMP_MARGIN) | (pre > 1.0 + CLAMP_MARGIN)
    return cw * (~near).float() if which == "free" else cw * out.float()


def step_stats(white_bg):
    c = step_case()
    f = step_forward(white_bg)
    pre = f["pre"]
    ends = c.stats()["ends_in"]
    return dict(below=float((pre < 0).float().mean()), above=float((pre > 1).float().mean()), inside=float(((pre > 0) & (pre < 1)).float().mean()),
                near=float((((pre - 0.0).abs() < CLAMP_MARGIN) | ((pre - 1.0).abs() < CLAMP_MARGIN)).float().mean()),
                ends_early=(ends[0] + ends[1]) / c.n, M=f["M"], n=c.n)


@functools.lru_cache(maxsize=None)
def oracle_step(white_bg, which="free", penalty=True):
    """every leaf's gradient of sum(rgb_map * cw) + 0.5 * penalty through oracle.tensorf_oracle.execute with the reference's keep mask standing for the early exit"""
    from oracle import tensorf_oracle as TO
    c = step_case()
    sc = TO.scene_from_arrays(step_arrays(), **c.hyper)
    leaves = step_leaves(sc)
    for t in leaves.values():
        t.requires_grad_(True)
    rgb, _ = TO.execute(sc, torch.tensor(c.rays), white_bg=white_bg, N_samples=c.S, sample_keep=c.keep_mask())
    loss = (rgb * step_cw(white_bg, which)).sum()
    if penalty:
        loss = loss + 0.5 * sc.penalty
    loss.backward()
    return rgb.detach(), float(sc.penalty.detach()), {k: (torch.zeros_like(t) if t.grad is None else t.grad.clone()) for k, t in leaves.items()}
