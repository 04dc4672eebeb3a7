"""Shared by tests/test_march_backward_host.py and tests/test_gpu_march_backward.py: a float64 reference of the training march's differentiable outputs
(the appearance weights, acc_map and, in the explicit-depth form, lam6 = prod_j (1 - alpha_j + 1e-6)) past one 64-sample chunk and with early exit on, the inputs
the two test files run it on, and the conditions that keep those inputs from being vacuous.

The reference is written from the formulas (tensorBase.py:17-24 raw2alpha, :340-360 sample_ray, :444-448 feature2density, :487-513 the march of execute;
tensoRF.py:209-225 the density feature), in torch float64 on the CPU.  Only the sample positions, z, the in-box test and the alpha-mask test come from the fp32
oracle (oracle.tensorf_oracle.sample_ray / alpha_sample): they are INPUTS here, their bit-exactness against the kernels has tests of its own.

Early exit, restated (the kernels walk a ray in chunks of 64 samples):
  * chunk c covers samples 64c .. min(64c + 63, S - 1);
  * a ray ends after the first chunk at whose end T < eps_T; later samples have weight 0 and do not enter acc (a detached keep-mask on alpha);
  * a chunk without a valid sample leaves T unchanged (and is never the chunk a ray ends after);
  * leaving the box changes no value.

Scalar loss both sides differentiate:
    L = sum_rj [w_rj > thres] g(x_rj) w_rj + sum_r a_r acc_r  (+ sum_r b_r lam6_r in the explicit-depth form)
with g a fixed smooth function of the normalised position and a, b seeded per-ray vectors.  The GPU side evaluates the same g at the queue's own positions and hands
it over as grad_w, so no queue-entry <-> sample-index mapping is needed.

MUTATIONS are deliberate defects of the REFERENCE (tests/test_march_backward_host.py): each restates one way the backward kernel's chunk loop could go wrong, and
the host test asserts that the 5e-4 bar would see it on these inputs."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLDEN, TINY

CHUNK = 64
BAR_GRAD = 5e-4            # max |g - g_ref| / max |g_ref| per tensor: tests/test_gpu_training.py::test_gradients_match_oracle_autograd's bar, unchanged
BAR_FWD = 2e-4             # forward outputs, absolute: the same test's
BASE_STEP_RATIO = 0.15     # the tiny scene at this ratio: 130-260 samples through the box
POSES = (1, 4, 6)          # frames of rays.sphere_poses(8, 4.0)
MAX_DROPPED = 0.03
MUTATIONS = ("T_not_carried", "prefix_reset", "cut_early", "cut_late", "skip_first_dropped")
DENSITY_NAMES = [f"density_plane.{i}" for i in range(3)] + [f"density_line.{i}" for i in range(3)]
APP_NAMES = [f"app_plane.{i}" for i in range(3)] + [f"app_line.{i}" for i in range(3)]
MAT_MODE = ((0, 1), (0, 2), (1, 2))   # tensorBase.py:168
VEC_MODE = (2, 1, 0)                  # tensorBase.py:169


def g_of(x):
    """the loss's per-sample factor: a fixed smooth function of the normalised position [..., 3]"""
    return torch.sin(3.0 * x[..., 0] + 2.0 * x[..., 1] - x[..., 2]) + 0.5


@functools.lru_cache(maxsize=None)
def tiny_arrays():
    d = np.load(os.path.join(GOLDEN, "tiny_dump.npz"))
    return {k[len("scene."):]: d[k] for k in d.files if k.startswith("scene.")}


def hyper(step_ratio=BASE_STEP_RATIO, act="softplus", thres=None):
    from jittor_myc_nerfs_amd import synthetic
    h = dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=float(step_ratio), fea2denseAct=act)
    return h if thres is None else dict(h, rayMarch_weight_thres=float(thres))


def step_ratio_for(gridSize, aabb=None):
    """the step_ratio at which a grid marches with the step the tiny 16x20x24 grid has at BASE_STEP_RATIO (stepSize = mean(units) * step_ratio, tensorBase.py:197-209)"""
    aabb = np.asarray(TINY["aabb"] if aabb is None else aabb, np.float64)
    size = aabb[1] - aabb[0]
    base = np.mean(size / (np.asarray(TINY["gridSize"]) - 1)) * BASE_STEP_RATIO
    return float(base / np.mean(size / (np.asarray(gridSize) - 1)))


def frames(poses=POSES, elevation_deg=30.0, wh=16):
    """rays [len(poses) * wh * wh, 6] fp32 of rays.frame_rays frames on rays.sphere_poses(8, 4.0)"""
    from jittor_myc_nerfs_amd import rays as R, synthetic
    ps = R.sphere_poses(8, 4.0, elevation_deg)
    return np.concatenate([R.frame_rays(ps[k], wh, wh, synthetic.SCENE_A["camera_angle_x"]).numpy() for k in poses]).astype(np.float32)


# ---- sampling: the fp32 oracle's, an input of the reference ------------------------------------------------------------------------------------------
def sample(sc, rays, S, jitter=None, z_vals=None):
    """{xyz_n [n,S,3] fp32, z [n,S] fp32, bbox, valid [n,S] bool} as oracle.tensorf_oracle.execute forms them (:476-503); z_vals: explicit depths [n,S] fp32"""
    from oracle import tensorf_oracle as TO
    rays = torch.as_tensor(rays, dtype=torch.float32)
    o, d = rays[:, :3], rays[:, 3:6]
    if z_vals is None:
        xyz, z, bbox, _ = TO.sample_ray(sc, o, d, S, jitter)
        z = z.expand(rays.shape[0], -1).contiguous()
    else:
        z = torch.as_tensor(z_vals, dtype=torch.float32)
        xyz = o[:, None, :] + d[:, None, :] * z[..., None]                                   # a sampler override's positions (nerfplusplus.py:263)
        bbox = ~((sc.aabb[0] > xyz) | (xyz > sc.aabb[1])).any(dim=-1)
    valid = bbox.clone()
    if sc.alpha_volume is not None:                                                          # :491-496
        ok = TO.alpha_sample(sc, xyz[bbox]) > 0
        valid[bbox] = ok
    return dict(xyz_n=TO.normalize_coord(sc, xyz), z=z, bbox=bbox, valid=valid)


def explicit_depths(sc, rays, S, seed):
    """[n,S] fp32 depths, increasing and unevenly spaced: t_min + step * (j + 0.8 u_rj)"""
    from oracle import tensorf_oracle as TO
    rays = torch.as_tensor(rays, dtype=torch.float32)
    _, _, _, t_min = TO.sample_ray(sc, rays[:, :3], rays[:, 3:6], S)
    u = torch.tensor(np.random.default_rng(seed).random((rays.shape[0], S)).astype(np.float32))
    return (t_min[:, None] + sc.stepSize * (torch.arange(S).float()[None] + 0.8 * u)).contiguous()


# ---- the float64 reference -----------------------------------------------------------------------------------------------------------------------
def grid_sample64(img, x, y):
    """bilinear, align_corners=True, zero padding: img [1,C,H,W] float64 at normalised (x -> W, y -> H), both [m] -> [C,m]"""
    pts = torch.stack((x, y), -1).view(1, -1, 1, 2)
    return F.grid_sample(img, pts, mode="bilinear", padding_mode="zeros", align_corners=True).view(img.shape[1], -1)


def density_feature64(planes, lines, xyz):
    """tensoRF.py:209-225 in float64: sum over the three (plane, line) pairs and their components of bilinear(plane) * linear(line)"""
    sf = torch.zeros(xyz.shape[0], dtype=torch.float64)
    zero = torch.zeros(xyz.shape[0], dtype=torch.float64)
    for i in range(3):
        p = grid_sample64(planes[i], xyz[:, MAT_MODE[i][0]], xyz[:, MAT_MODE[i][1]])
        l = grid_sample64(lines[i], zero, xyz[:, VEC_MODE[i]])
        sf = sf + (p * l).sum(0)
    return sf


def app_h64(planes, lines, xyz):
    """tensoRF.py:228-241 in float64: h [m, sum of components] = bilinear(app_plane) * linear(app_line), plane after plane"""
    zero = torch.zeros(xyz.shape[0], dtype=torch.float64)
    cols = [grid_sample64(planes[i], xyz[:, MAT_MODE[i][0]], xyz[:, MAT_MODE[i][1]]) * grid_sample64(lines[i], zero, xyz[:, VEC_MODE[i]]) for i in range(3)]
    return torch.cat(cols).T


def n_chunks(S):
    return (S + CHUNK - 1) // CHUNK


def walk(alpha, valid, eps_T, shift=0):
    """The chunk walk without gradients.  alpha [n,S] float64 (0 where not valid), valid [n,S] bool.
    -> keep [n,S] bool (samples of chunks the ray still walks), end [n] int64 (the chunk the ray ends after, -1: never), T_end [n, chunks] float64 (T at the end of
    each chunk the ray walks, nan behind its end).  shift = -1 / +1: the cut-off one chunk early / late (mutations)."""
    n, S = alpha.shape
    T = torch.ones(n, dtype=torch.float64)
    end = torch.full((n,), -1, dtype=torch.int64)
    T_end = torch.full((n, n_chunks(S)), float("nan"), dtype=torch.float64)
    for c in range(n_chunks(S)):
        sl = slice(c * CHUNK, min((c + 1) * CHUNK, S))
        alive = end < 0
        has_valid = valid[:, sl].any(1)
        T = torch.where(alive & has_valid, T * torch.prod(1.0 - alpha[:, sl] + 1e-10, 1), T)
        T_end[alive, c] = T[alive]
        end[alive & has_valid & (T < eps_T)] = c
    last = torch.where(end >= 0, end + shift, torch.full_like(end, n_chunks(S)))
    keep = (torch.arange(S)[None] // CHUNK) <= last[:, None]
    return keep, end, T_end


def reference(case, leaves=None, mutation=None, grad=True):
    """The float64 reference on a case.  leaves: six float64 density factors (planes, then lines) with requires_grad; made from the case's arrays when None.
    -> dict(w [n,S], app [n,S] bool, acc [n], lam6 [n], loss, keep, end, T_end, grads (six tensors, when grad))."""
    assert mutation is None or mutation in MUTATIONS
    if leaves is None:
        leaves = [torch.tensor(case.arrs[k], dtype=torch.float64).requires_grad_(grad) for k in DENSITY_NAMES]
    sc, smp, S = case.sc, case.smp, case.S
    valid = smp["valid"]
    n = valid.shape[0]
    xyz = smp["xyz_n"].double()
    sf = density_feature64(leaves[:3], leaves[3:], xyz[valid])
    if mutation == "skip_first_dropped":
        sf = torch.where(first_after_skip(valid)[valid], sf.detach(), sf)
    sig = F.softplus(sf + sc.density_shift) if sc.fea2denseAct == "softplus" else F.relu(sf)   # :444-448
    sigma = torch.zeros((n, S), dtype=torch.float64)
    sigma[valid] = sig
    z = smp["z"].double()
    dist = torch.cat((z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])), -1) * sc.distance_scale   # :488, :511
    alpha_all = 1.0 - torch.exp(-sigma * dist)                                                   # :19
    _, end, T_end = walk(alpha_all.detach(), valid, case.eps_T)
    keep = walk(alpha_all.detach(), valid, case.eps_T, {"cut_early": -1, "cut_late": 1}.get(mutation, 0))[0]
    alpha = alpha_all * keep
    T = torch.ones(n, dtype=torch.float64)
    ws, logs = [], []
    for c in range(n_chunks(S)):
        sl = slice(c * CHUNK, min((c + 1) * CHUNK, S))
        f = 1.0 - alpha[:, sl] + 1e-10                                                           # :21
        incl = torch.cumprod(f, 1)
        excl = torch.cat((torch.ones((n, 1), dtype=torch.float64), incl[:, :-1]), 1)
        T_in = torch.ones_like(T) if mutation == "T_not_carried" else T
        ws.append(alpha[:, sl] * (T_in[:, None] * excl))                                         # :23
        walked = (valid[:, sl] & keep[:, sl]).any(1)
        T = torch.where(walked, T * incl[:, -1], T)
        logs.append(torch.where(walked, torch.log(f).sum(1), torch.zeros_like(T)))
    w = torch.cat(ws, 1)
    acc = w.sum(1)
    lam6 = torch.prod(1.0 - alpha + 1e-6, 1)                                                     # nerfplusplus.py:277-278
    app = w.detach() > sc.thres                                                                  # :513
    dLdw = app * g_of(xyz) + case.a[:, None]
    loss = (app * g_of(xyz) * w).sum() + (case.a * acc).sum()
    if case.z_form:
        loss = loss + (case.b * lam6).sum()
    if mutation == "prefix_reset":
        # the backward's dL/dalpha_j holds -(sum_{k > j} dL/dw_k w_k) / (1 - alpha_j + 1e-10); a running prefix of dL/dw_k w_k that restarts at a chunk boundary adds
        # the sum over all earlier chunks, P_c, to that suffix: d/dalpha_j of P_c log(1 - alpha_j + 1e-10) is exactly that extra term
        contrib = (dLdw * w).detach()
        for c in range(1, n_chunks(S)):
            loss = loss + (contrib[:, :c * CHUNK].sum(1) * logs[c]).sum()
    out = dict(w=w.detach(), app=app, acc=acc.detach(), lam6=lam6.detach(), loss=float(loss.detach()), keep=keep, end=end, T_end=T_end, xyz=xyz)
    if grad:
        out["grads"] = [g.detach() for g in torch.autograd.grad(loss, leaves, allow_unused=True)]
    return out


def first_after_skip(valid):
    """[n,S] bool: the first valid sample of a chunk that follows one or more chunks without a valid sample, themselves behind a chunk with one"""
    n, S = valid.shape
    out = torch.zeros_like(valid)
    seen = torch.zeros(n, dtype=torch.bool)
    skipped = torch.zeros(n, dtype=torch.bool)
    for c in range(n_chunks(S)):
        sl = slice(c * CHUNK, min((c + 1) * CHUNK, S))
        has = valid[:, sl].any(1)
        hit = has & seen & skipped
        first = valid[:, sl].int().argmax(1) + c * CHUNK
        out[torch.nonzero(hit)[:, 0], first[hit]] = True
        skipped = torch.where(has, torch.zeros_like(skipped), skipped | seen)
        seen = seen | has
    return out


def rel_err(g, ref):
    """max |g - ref| / max |ref|: the bar's measure"""
    g, ref = torch.as_tensor(g).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((g - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """One vetted input: arrays + hyper-parameters (what conftest.make_model takes), rays, S, eps_T, jitter / z_vals, the oracle's sampling of the kept rays."""

    def __init__(self, arrs, hyp, rays, S, eps_T, jitter=None, z_form=False, seed=0):
        from oracle import tensorf_oracle as TO
        self.arrs, self.hyper, self.S, self.eps_T, self.z_form = arrs, hyp, int(S), float(eps_T), bool(z_form)
        self.sc = TO.scene_from_arrays(arrs, **hyp)
        rng = np.random.default_rng(1000 + seed)
        n0 = rays.shape[0]
        self.rays = np.ascontiguousarray(rays, np.float32)
        self.jitter = rng.random(n0).astype(np.float32) if jitter else None
        self.z_vals = explicit_depths(self.sc, self.rays, self.S, 2000 + seed).numpy() if z_form else None
        self.a = torch.tensor(rng.standard_normal(n0))
        self.b = torch.tensor(rng.standard_normal(n0))
        self.smp = sample(self.sc, self.rays, self.S, self.jitter, self.z_vals)
        # drop the rays on which an fp32 / fp64 flip of a threshold is not the kernel's error: a weight within 1e-3 of the appearance threshold, an end-of-chunk T
        # within 1e-2 of eps_T
        r = reference(self, grad=False)
        border = ((r["w"] / self.sc.thres - 1.0).abs() < 1e-3).any(1)
        if self.eps_T > 0:
            border |= ((r["T_end"] / self.eps_T - 1.0).abs() < 1e-2).any(1)                  # (nan behind a ray's end compares False)
        self.n_dropped, self.n_before = int(border.sum()), n0
        kept = ~border
        kn = kept.numpy()
        self.rays = np.ascontiguousarray(self.rays[kn])
        self.jitter = None if self.jitter is None else np.ascontiguousarray(self.jitter[kn])
        self.z_vals = None if self.z_vals is None else np.ascontiguousarray(self.z_vals[kn])
        self.a, self.b = self.a[kept], self.b[kept]
        self.smp = {k: v[kept] for k, v in self.smp.items()}
        self._ref = {}

    @property
    def n(self):
        return self.rays.shape[0]

    def ref(self, mutation=None):
        if mutation not in self._ref:
            self._ref[mutation] = reference(self, mutation=mutation)
        return self._ref[mutation]

    def keep_mask(self):
        """the detached [n,S] mask oracle.tensorf_oracle.execute takes as sample_keep"""
        return self.ref()["keep"].float()

    def stats(self):
        """what the conditions of tests/test_march_backward_host.py count, from the reference alone"""
        r, S = self.ref(), self.S
        nc = n_chunks(S)
        ch = torch.arange(S) // CHUNK
        valid, bbox, end = self.smp["valid"], self.smp["bbox"], r["end"]
        has_valid = torch.stack([valid[:, ch == c].any(1) for c in range(nc)], 1)
        has_bbox = torch.stack([bbox[:, ch == c].any(1) for c in range(nc)], 1)
        has_app = torch.stack([r["app"][:, ch == c].any(1) for c in range(nc)], 1)
        walked = torch.arange(nc)[None] <= torch.where(end >= 0, end, torch.full_like(end, nc))[:, None]
        before = torch.cumsum(has_valid.int(), 1) - has_valid.int() > 0                         # a chunk with a valid sample lies before
        after = torch.flip(torch.cumsum(torch.flip(has_valid.int(), [1]), 1), [1]) - has_valid.int() > 0
        skipped_between = (~has_valid & before & after & walked).any(1)
        # a chunk the backward kernel reaches (the ray has not ended before it) that holds no in-box sample, behind a chunk with a valid one: `seen && mb == 0`
        reached = torch.arange(nc)[None] <= torch.where(end >= 0, end, torch.full_like(end, nc))[:, None] + 1
        past_exit = (~has_bbox & before & reached).any(1)
        return dict(n=self.n, dropped=self.n_dropped, before=self.n_before, hit=int(valid.any(1).sum()), n_app=int(r["app"].sum()),
                    ends_in=[int((end == c).sum()) for c in range(nc)], never_ends=int((end < 0).sum()),
                    never_ends_app_in_two_chunks=int(((end < 0) & (has_app.sum(1) >= 2)).sum()),
                    skipped_between=int(skipped_between.sum()), past_exit=int(past_exit.sum()),
                    first_after_skip=int((first_after_skip(valid) & r["keep"]).sum()))


@functools.lru_cache(maxsize=None)
def long_case(S=192, eps_T=1e-4, jitter=False, act="softplus", z_form=False, step_ratio=BASE_STEP_RATIO, thres=None):
    """The tiny scene marched finely: three 16x16 frames, 768 rays, more than one chunk, rays that end after chunk 0, after a later chunk, and never."""
    return Case(tiny_arrays(), hyper(step_ratio, act, thres), frames(), S, eps_T, jitter=jitter, z_form=z_form, seed=S)


HOLLOW_STEP_RATIO = 0.05   # 64 samples = 0.44 of the box's 2.0 along z
HOLLOW_S = 384             # six chunks: the box is left in the fifth at the latest
HOLLOW_SLAB = (-0.45, 0.65)


@functools.lru_cache(maxsize=None)
def hollow_arrays(kind):
    """The tiny scene with its own alpha mask (updateAlphaMask, tensorBase.py:385-409, at the scene's resolution) and the planes of the mask with z inside
    HOLLOW_SLAB zeroed.  kind "bits": the 0 / 1 volume as updateAlphaMask leaves it; "float": the same cells scaled by seeded factors in [0.25, 1] — alpha > 0 holds
    at the same positions, but only a trilinear lookup of the values themselves can tell."""
    from oracle import tensorf_oracle as TO
    arrs = dict(tiny_arrays())
    sc = TO.scene_from_arrays(arrs, **hyper(HOLLOW_STEP_RATIO))
    vol, _ = TO.updateAlphaMask(sc, TINY["gridSize"], 1e-4)                                      # (gz, gy, gx)
    zs = torch.linspace(TINY["aabb"][0][2], TINY["aabb"][1][2], TINY["gridSize"][2])
    vol = vol.clone()
    vol[(zs >= HOLLOW_SLAB[0]) & (zs <= HOLLOW_SLAB[1])] = 0.0
    if kind == "float":
        vol = vol * torch.tensor(np.random.default_rng(7).uniform(0.25, 1.0, tuple(vol.shape)).astype(np.float32))
    arrs["alpha_volume"], arrs["alpha_aabb"] = vol.numpy(), arrs["aabb"]
    return arrs


@functools.lru_cache(maxsize=None)
def hollow_case(kind, eps_T=1e-4):
    """Rays from above, roughly along z (the slab's normal): a chunk without a valid sample between two chunks that have some (the tap windows are carried over a
    `continue`), and a whole chunk behind the box (the `seen && mb == 0` break)."""
    rays = frames(POSES, elevation_deg=78.0)
    return Case(hollow_arrays(kind), hyper(HOLLOW_STEP_RATIO), rays, HOLLOW_S, eps_T, seed=17)


def grid_case(arrs, gridSize, S=130, eps_T=1e-4):
    """The same field on another grid (the arrays a model hands back after upsample_volume_grid), marched with the base case's step."""
    arrs = dict(arrs, gridSize=np.asarray(gridSize, np.int32))
    return Case(arrs, hyper(step_ratio_for(gridSize)), frames(), S, eps_T, seed=int(sum(gridSize)))


CUT_LATE_EPS_T = 0.05      # see KERNEL_CASES


def _kernel_cases():
    cases = {}
    for S in (64, 65, 130, 192, 256):
        for eps_T in (0.0, 1e-4):
            for jit in (False, True):
                cases[f"S{S}-eps{eps_T:g}-{'jitter' if jit else 'nojitter'}"] = functools.partial(long_case, S=S, eps_T=eps_T, jitter=jit)
    # first endings in chunk 1 and 2 instead of 0 and 1
    cases["S192-eps0.0001-step0.1"] = functools.partial(long_case, S=192, eps_T=1e-4, step_ratio=0.1)
    # behind a cut-off at eps_T = 1e-4 a ray holds less than 1e-4 of its weight: walking one chunk too many moves no gradient by more than 1e-3 of its tensor's
    # largest entry, whatever the inputs.  A larger eps_T makes that defect visible to the bar (tests/test_march_backward_host.py measures it); the library takes
    # eps_T up to rayMarch_weight_thres, so the scene's threshold goes up with it
    cases[f"S192-eps{CUT_LATE_EPS_T:g}-cutlate"] = functools.partial(long_case, S=192, eps_T=CUT_LATE_EPS_T, thres=CUT_LATE_EPS_T)
    cases["S192-eps0.0001-relu"] = functools.partial(long_case, S=192, eps_T=1e-4, act="relu")
    cases["hollow-bits-continue-and-leftbox-break"] = functools.partial(hollow_case, "bits")
    cases["hollow-float-continue-and-leftbox-break"] = functools.partial(hollow_case, "float")
    cases["zform-S130-eps0"] = functools.partial(long_case, S=130, eps_T=0.0, z_form=True)
    cases["zform-S130-eps0.0001"] = functools.partial(long_case, S=130, eps_T=1e-4, z_form=True)
    return cases


KERNEL_CASES = _kernel_cases()

# (case, mutation) pairs the host test proves the bar's power on; every mutation appears, and every case with the defects it can show
POWER = ([("S192-eps0.0001-nojitter", m) for m in ("T_not_carried", "prefix_reset", "cut_early")]
         + [(f"S192-eps{CUT_LATE_EPS_T:g}-cutlate", m) for m in ("T_not_carried", "prefix_reset", "cut_early", "cut_late")]
         + [(f"hollow-{k}-continue-and-leftbox-break", m) for k in ("bits", "float") for m in ("T_not_carried", "prefix_reset", "cut_early", "skip_first_dropped")])
