"""Shared by tests/test_ngp_frame_host.py and tests/test_gpu_ngp_frame.py: designed Instant-NGP scenes that put the fused frame kernel's
`T < 1e-4` break, its 32-step tiles and its 64-ray tickets where the tests want them, and a vectorised fp64 restatement of
`compute_rgbs_inference` (oracle/ngp_oracle.c: ngp_oracle_composite) that also reports where each ray breaks, how close any break
decision came to the threshold, and how many samples a kernel that stops at the end of the breaking tile evaluates.  numpy and the
project's CPU oracle only; test_ngp_frame_host.py checks the reference against the oracle's two compositors and checks that the
designed scenes meet the conditions the GPU tests lean on.

The designed scene (aabb_scale 1, every occupancy bit set, const_dt):
  * the hash grid is ONE constant s, so every position has the same 32 features (the trilinear weights sum to 1); the five Linears
    are bias-free and ReLU is positively homogeneous, so density_raw = s * c1 with c1 = the density head's output for s = 1;
  * with sigma = exp(density_raw) every step has the optical depth tau = sigma * dt and T before sample j is exp(-j tau); choosing
    tau = ln(1e4) / (k - 0.5) makes `T < 1e-4` first true at sample k, with ln(T / 1e-4) = -+ tau / 2 on either side of it;
  * rays start inside the box (the sampler's near_distance 0.2 in front of their origin) and leave through the face z = 1; origins
    step by a third of dt, so the step counts form a ladder 0 ... ~137; one more ray crosses the whole box and stops at the 1024-step
    cap.  Ray i of any ray count R is rung i mod 421 of that pattern (rung 0 = the cap ray), so every R reuses the same geometry while
    the jitter (drawn per ray index) differs from period to period.
"""
import functools

import numpy as np

BG = (0.2, 0.5, 0.9)                                  # three different channels, none of them 0 or 1
THR = 1e-4
LN1E4 = float(np.log(1e4))                            # 9.2103...
BREAKS = (1, 2, 3, 31, 32, 33, 64, 65, 96, 97)        # wanted break samples: lane 0 / 1 / 31 of a tile, and both sides of three tile edges
NO_BREAK = 1000                                       # tau of k = 1000: no ladder ray (<= ~137 steps) breaks; used without the cap ray
STEP_COUNTS = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 1024)
RAY_COUNTS = (0, 1, 63, 64, 65, 2047, 2048, 2049, 4097)   # the launch switches at 2048 rays, a ticket covers 64, a slab 4096
RAY_COUNT_K = 33                                      # the ray-count sweep breaks in the second tile
MARGIN = 0.05                                         # wanted |ln(T / 1e-4)| at every break decision
N_RUNGS = 420
PERIOD = N_RUNGS + 1
AABB_SCALE = 1
CONE_POSE, CONE_WH = 1, 40                            # the cone-stepping frame: ngp_camera_rays(40, 40, pose_index=1) on the shared ngp_scene
HIDDEN_TARGET = 3.0e4                                 # range case: largest value any layer hands to the next, about half the fp16 range


def const_dt_seen():
    """The constant step as the compositor sees it: dt = MIN_CONE_STEPSIZE / 2, warped by the sampler, unwarped again (all fp32)."""
    from oracle import ngp_oracle as N
    f32 = np.float32
    mn = N.MIN_CONE_STEPSIZE
    dt = f32(np.float64(mn) * 0.5)
    mx = mn * f32(16)
    return float(N.unwarp_dt(f32(f32(dt - mn) / f32(mx - mn))))


def designed_rays(R=PERIOD, cap_ray=True):
    """rays_o, rays_d [R,3] fp32 of the ladder pattern.  cap_ray=False replaces the box-crossing ray by one more zero-step ray."""
    dt = np.sqrt(3.0) / 1024 * 0.5
    i = np.arange(R)
    p = i % PERIOD
    rung = (N_RUNGS - p).astype(np.float64)            # p = 1 is the longest ladder ray
    d = np.stack([0.02 * np.sin(0.7 * p), 0.03 * np.cos(1.7 * p), np.ones(R)], -1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # the march starts near_distance = 0.2 along the ray (plus up to one dt of jitter); it leaves the box at z = 1
    z_start = 1.0 - (rung - 6.0) * dt / 3.0
    o = np.stack([np.full(R, 0.5), np.full(R, 0.5), z_start], -1) - 0.2 * d
    cap = p == 0
    o[cap] = [0.47, 0.52, -0.3] if cap_ray else [0.5, 0.5, 0.9]      # enters through z = 0 and needs ~1180 steps to cross / starts outside
    d[cap] = [0.0, 0.0, 1.0]
    return o.astype(np.float32), d.astype(np.float32)


def full_bitfield():
    from oracle import ngp_oracle as N
    return np.full(N.NERF_GRIDSIZE ** 3 * N.NERF_CASCADES // 8, 255, np.uint8)


@functools.lru_cache(maxsize=None)
def _designed_base():
    """(levels, the five weights, c1): seeded U(+-0.3) weights with the colour head scaled by 0.02 (post-sigmoid colours stay near
    0.5, far from saturation); the density head's sign is chosen so that c1 > 0."""
    from oracle import ngp_oracle as N
    levels = N.grid_levels(AABB_SCALE)
    rng = np.random.default_rng(20)
    w = {}
    for name, shape in (("density_mlp.0", (64, 32)), ("density_mlp.2", (16, 64)), ("rgb_mlp.0", (64, 32)), ("rgb_mlp.2", (64, 64)), ("rgb_mlp.4", (3, 64))):
        w[name + ".weight"] = rng.uniform(-0.3, 0.3, shape).astype(np.float32)
    w["rgb_mlp.4.weight"] *= np.float32(0.02)
    enc = np.ones(32)
    c1 = float((w["density_mlp.2.weight"].astype(np.float64) @ np.maximum(w["density_mlp.0.weight"].astype(np.float64) @ enc, 0))[0])
    if c1 < 0:
        w["density_mlp.2.weight"] = -w["density_mlp.2.weight"]
        c1 = -c1
    return levels, w, c1


def designed_tau(k):
    return LN1E4 / (k - 0.5)


def designed_grid_value(k):
    """The constant s that gives every step the optical depth tau(k)."""
    _, _, c1 = _designed_base()
    return float(np.float32(np.log(designed_tau(k) / const_dt_seen()) / c1))


def designed_scene(k):
    """(levels, arrays) of the designed scene whose rays break at sample k; arrays are keyed like conftest's ngp_scene."""
    levels, w, _ = _designed_base()
    arrs = dict(w)
    arrs["grid"] = np.full(levels["n_params"], designed_grid_value(k), np.float32)
    arrs["density_grid_bitfield"] = full_bitfield()
    return levels, arrs


def oracle_rows(o, d, bitfield, aabb_scale=AABB_SCALE, const_dt=True):
    """The rows `render_frame` / `render_frame_rows` march for these rays from a fresh Pcg32(1337): (coords [n,7], numsteps [R,2])."""
    from oracle import ngp_oracle as N
    coords, _, numsteps, _, _ = N.sample(o, d, bitfield, aabb_scale, N.Pcg32(1337).state, const_dt=const_dt, slab_rays=4096)
    return coords, numsteps


@functools.lru_cache(maxsize=None)
def designed_rows(R=PERIOD, cap_ray=True):
    """(rays_o, rays_d, coords, numsteps) of the ladder pattern: the rows do not depend on k (the occupancy is full in every designed scene)."""
    o, d = designed_rays(R, cap_ray)
    coords, numsteps = oracle_rows(o, d, full_bitfield())
    return o, d, coords, numsteps


def network_shift(net_out):
    """How far the network bar (2e-4 * max(1, |out|)) on density_raw can move ln T in front of a break decision: d ln T = -(optical depth) *
    d density_raw, and the optical depth in front of a decision that matters is about ln(1e4)."""
    return (LN1E4 + 0.1) * 2e-4 * max(1.0, float(np.abs(net_out).max()))


# --------------------------------------------------------------------------------------------------------------- fp64 reference
def composite_f64(net_out, coords, numsteps, bg=(1.0, 1.0, 1.0), thr=THR):
    """`compute_rgbs_inference` in fp64, vectorised over all rays.  net_out [n,4], coords [n,7] (column 3: warped dt), numsteps [R,2].
    Returns per ray
      rgb    [R,3] fp64;
      brk    [R] the break index b = first j with T_j < thr (T_j = T before sample j), -1 where the ray never breaks;
      margin [R] the smallest |ln(T_j / thr)| over the decisions the loop makes (j = 0..b, or 0..n-1 without a break; inf for n = 0);
      work   [R] the samples a kernel evaluates that walks 32 steps at a time and stops behind the tile holding the break:
             n without a break, else min(n, 32 * (b // 32 + 1)).
    T_j is exp(-(optical depth in front of j)): the products of the loop's (1 - alpha) factors, without their rounding."""
    from oracle import ngp_oracle as N
    ns = np.asarray(numsteps, np.int64).reshape(-1, 2)
    n, base = ns[:, 0], ns[:, 1]
    R = n.shape[0]
    bgv = np.asarray(bg, np.float64)
    rgb = np.tile(bgv, (R, 1))                                         # a ray without steps: T = 1 times the background
    brk = np.full(R, -1, np.int64)
    margin = np.full(R, np.inf)
    work = n.copy()
    live = np.nonzero(n > 0)[0]
    if live.size == 0:
        return rgb, brk, margin, work
    nl = n[live]
    start = np.concatenate([[0], np.cumsum(nl)[:-1]])                  # each live ray's first entry in the packed arrays below
    j = np.arange(int(nl.sum())) - np.repeat(start, nl)                # sample index within its ray
    row = np.repeat(base[live], nl) + j
    out = np.asarray(net_out, np.float32)[row].astype(np.float64)
    dt = np.asarray(N.unwarp_dt(np.asarray(coords, np.float32)[row, 3]), np.float32).astype(np.float64)      # an input: fp32 as the rows hold it
    tau = np.exp(out[:, 3]) * dt
    incl = np.cumsum(tau)
    before = (incl - tau) - np.repeat((incl - tau)[start], nl)         # optical depth in front of sample j
    ln_ratio = -before - np.log(thr)                                   # ln(T_j / thr)
    big = np.iinfo(np.int64).max
    first = np.minimum.reduceat(np.where(ln_ratio < 0, j, big), start)
    has = first < big
    stop = np.repeat(np.where(has, first, nl), nl)                     # samples j < stop are composited
    margin[live] = np.minimum.reduceat(np.where(j <= stop, np.abs(ln_ratio), np.inf), start)
    w = np.where(j < stop, -np.expm1(-tau) * np.exp(-before), 0.0)
    col = 1.0 / (1.0 + np.exp(-out[:, :3]))
    c = np.add.reduceat(w[:, None] * col, start, axis=0)
    t_end = np.exp(-(before + tau)[start + nl - 1])
    c += np.where(has, 0.0, t_end)[:, None] * bgv                      # the background only behind a ray that never broke
    rgb[live] = c
    brk[live] = np.where(has, first, -1)
    work[live] = np.where(has, np.minimum(nl, 32 * (first // 32 + 1)), nl)
    return rgb, brk, margin, work


def composite_loop_f64(net_out, coords, numsteps, bg=(1.0, 1.0, 1.0), thr=THR):
    """The same loop written out ray by ray (T multiplied up as the reference does); checks composite_f64 in the host test."""
    from oracle import ngp_oracle as N
    R = numsteps.shape[0]
    rgb, brk = np.zeros((R, 3)), np.full(R, -1, np.int64)
    bgv = np.asarray(bg, np.float64)
    for i in range(R):
        n, base = int(numsteps[i, 0]), int(numsteps[i, 1])
        T, c, j = 1.0, np.zeros(3), 0
        while j < n:
            if T < thr:
                brk[i] = j
                break
            o = np.asarray(net_out[base + j], np.float64)
            alpha = 1.0 - np.exp(-np.exp(o[3]) * float(N.unwarp_dt(coords[base + j, 3])))
            c = c + alpha * T / (1.0 + np.exp(-o[:3]))
            T *= 1.0 - alpha
            j += 1
        if j == n:
            c = c + T * bgv
        rgb[i] = c
    return rgb, brk


# --------------------------------------------------------------------------------------------------------------- network in fp64
def network_f64(levels, arrs, coords):
    """NGPNetworks.execute_ in fp64 on the oracle's fp32 encodings (which the kernels reproduce: the hash features bit for bit, SH to
    2e-6).  Returns (out [n,4] fp64, the largest magnitude any layer hands to the next one — features, hidden activations, the 16
    density outputs and SH: everything the fused kernel splits into fp16 hi + lo halves)."""
    from oracle import ngp_oracle as N
    c = np.ascontiguousarray(coords, np.float32)
    W = {k: np.asarray(arrs[k + ".weight"], np.float64) for k in ("density_mlp.0", "density_mlp.2", "rgb_mlp.0", "rgb_mlp.2", "rgb_mlp.4")}
    enc = N.hash_encode_c(levels, arrs["grid"], c[:, :3]).astype(np.float64)
    h = np.maximum(enc @ W["density_mlp.0"].T, 0)
    den = h @ W["density_mlp.2"].T
    x = np.concatenate([den, N.sh_encode_c(c[:, 4:7]).astype(np.float64)], -1)
    h2 = np.maximum(x @ W["rgb_mlp.0"].T, 0)
    h3 = np.maximum(h2 @ W["rgb_mlp.2"].T, 0)
    rgb = h3 @ W["rgb_mlp.4"].T
    biggest = max(float(np.abs(a).max()) for a in (enc, h, x, h2, h3))
    return np.concatenate([rgb, den[:, :1]], -1), biggest


@functools.lru_cache(maxsize=None)
def range_case():
    """(levels, arrays, coords [4099,7], out fp64, biggest): a random hash grid scaled so that the largest value handed from one layer
    to the next is about HIDDEN_TARGET = 3e4.  The fused network splits every such value into two fp16 halves, rounding toward zero;
    above 65504 the high half saturates and the split no longer sums to the value, so the kernel's valid range ends there and this
    case stays at half of it."""
    from oracle import ngp_oracle as N
    levels = N.grid_levels(AABB_SCALE)
    rng = np.random.default_rng(11)
    arrs = {"grid": rng.uniform(-1, 1, levels["n_params"]).astype(np.float32)}
    for name, shape in (("density_mlp.0", (64, 32)), ("density_mlp.2", (16, 64)), ("rgb_mlp.0", (64, 32)), ("rgb_mlp.2", (64, 64)), ("rgb_mlp.4", (3, 64))):
        arrs[name + ".weight"] = rng.uniform(-0.3, 0.3, shape).astype(np.float32)
    n = 4099                                                           # several blocks and a ragged last tile
    coords = np.concatenate([rng.random((n, 3), dtype=np.float32), np.zeros((n, 1), np.float32), rng.random((n, 3), dtype=np.float32)], 1)
    for _ in range(3):                                                 # SH does not scale with the grid, so the map is only nearly linear
        _, biggest = network_f64(levels, arrs, coords)
        arrs["grid"] = (arrs["grid"] * np.float32(HIDDEN_TARGET / biggest)).astype(np.float32)
    out, biggest = network_f64(levels, arrs, coords)
    return levels, arrs, coords, out, biggest


# --------------------------------------------------------------------------------------------------------------- density grids
def density_grid(kind, seed=0):
    """Synthetic density grids [5*128^3] for update_bitfield (threshold = min(0.01, mean of cascade 0 clamped at 0)).  Cell values come
    from a few discrete levels, none near either candidate threshold, so the bitfield cannot depend on how the mean was summed:
      'sparse' mean ~0.0046 < 0.01: the threshold is the mean; the level 0.007 lies between the two candidates (set only if the mean is used);
      'dense'  mean ~0.05  > 0.01: the threshold is 0.01; the level 0.03 lies between the two candidates (set only if 0.01 is used);
      'empty'  no positive cell: mean 0, threshold 0, `> 0` never holds."""
    from oracle import ngp_oracle as N
    n = N.NERF_GRIDSIZE ** 3 * N.NERF_CASCADES
    rng = np.random.default_rng(100 + seed)
    if kind == "sparse":
        levels, p = [0.0, -0.5, 0.001, 0.007, 0.02, 1.0], [0.597, 0.1, 0.2, 0.05, 0.05, 0.003]
    elif kind == "dense":
        levels, p = [0.0, -0.5, 0.001, 0.03, 1.0], [0.46, 0.1, 0.2, 0.2, 0.04]
    elif kind == "empty":
        levels, p = [0.0, -1.0, -0.25], [0.5, 0.25, 0.25]
    else:
        raise ValueError(kind)
    return np.asarray(levels, np.float32)[rng.choice(len(levels), size=n, p=p)]


def grid_threshold_gap(grid):
    """(mean, threshold, the smallest relative distance of any positive cell level from the threshold) in fp64."""
    from oracle import ngp_oracle as N
    c0 = grid[:N.NERF_GRIDSIZE ** 3].astype(np.float64)
    mean = float(np.maximum(c0, 0).mean())
    thr = min(0.01, mean)
    vals = np.unique(grid)
    gap = float(np.min(np.abs(vals - thr)) / thr) if thr > 0 else float("inf")
    return mean, thr, gap
