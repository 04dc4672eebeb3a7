"""Shared by tests/test_ngp_train_host.py and tests/test_gpu_ngp_train.py: references for Instant-NGP training.

  * hash_geometry / hash_encode_t   the hash grid in torch: cells and fractions in fp32 exactly as the oracle forms them (fmaf(pos, scale, 0.5), floor,
                                    subtraction — at scale 8192 an fp64 fraction differs from the kernel's by 1e-3), entries by grid_index's arithmetic,
                                    the trilinear blend in the tensor's dtype.  Differentiable with respect to the grid.
  * network_t                       the five bias-free Linears around it (SH from the oracle, no gradient).
  * composite_t                     the training compositor vectorised over rays (a padded [rays, steps] layout, per-ray prefix sums), with the stop index
                                    held fixed: differentiable with respect to the network outputs.
  * composite_loop                  the compositor's loop as the kernel runs it — T multiplied up step by step, colour added in sample order — in a chosen
                                    numpy dtype, serial over the steps and vectorised over the rays (every ray sees exactly its own loop's operations in
                                    order), plus the analytic gradient of include/tvr_ngp.h; `mutation=` restates six defects a kernel could have.
  * designed_case / scene_inputs    the compositor tests' inputs: the designed ladder (constant dt, or a random dt per row) and the shared scene (constant dt, or
                                    cone-stepped), with the rays that are compared; COMPOSITOR_POWER lists the (case, mutation) pairs the host test proves.
  * step_t                          one whole step's loss sum from (parameters, rows, background, target).
fp64 on the CPU is the reference; the same code in fp32 is the yardstick the GPU tests derive their bars from.
"""
import functools
import os

import numpy as np
import torch

import ngp_frame_common as F

M32 = 0xFFFFFFFF
THR = 1e-4
WEIGHT_KEYS = ("density_mlp.0.weight", "density_mlp.2.weight", "rgb_mlp.0.weight", "rgb_mlp.2.weight", "rgb_mlp.4.weight")


# --------------------------------------------------------------------------------------------------------------- hash grid
def level_table(levels):
    """[(offset, size, scale fp32, res, hashed)] per level; `hashed` by grid_index's stride loop (HashEncode.h:75-93) in uint32 arithmetic."""
    out = []
    for l in range(len(levels["scale"])):
        off, size = int(levels["offsets"][l]), int(levels["offsets"][l + 1]) - int(levels["offsets"][l])
        scale = np.float32(levels["scale"][l])
        res = int(np.ceil(scale)) + 1
        stride, dims = 1, 0
        while dims < 3 and stride <= size:
            stride = (stride * res) & M32
            dims += 1
        out.append((off, size, scale, res, size < stride))
    return out


def hash_geometry(levels, pos):
    """pos [n,3] (torch, any device; read as fp32) -> (entries [n,L,8] int64 = global entry index of each corner, frac [n,L,3] fp32, cells [n,L,3] int64).
    p = fmaf(pos, scale, 0.5) is formed in fp64 (the product of two fp32 values is exact there) and rounded once to fp32."""
    pos = pos.to(torch.float32)
    ents, fracs, cells = [], [], []
    for off, size, scale, res, hashed in level_table(levels):
        p = (pos.double() * float(scale) + 0.5).float()
        c0 = torch.floor(p)
        f = p - c0
        c = c0.to(torch.int64)
        e8 = []
        for idx in range(8):
            x, y, z = c[:, 0] + (idx & 1), c[:, 1] + ((idx >> 1) & 1), c[:, 2] + ((idx >> 2) & 1)
            if hashed:
                index = x ^ ((y * 19349663) & M32) ^ ((z * 83492791) & M32)
            else:
                index = (x + y * res + z * res * res) & M32
            e8.append(index % size + off)
        ents.append(torch.stack(e8, -1))
        fracs.append(f)
        cells.append(c)
    return torch.stack(ents, 1), torch.stack(fracs, 1), torch.stack(cells, 1)


def corner_weights(frac, dtype):
    """[n,L,8] trilinear weights in the forward's factor order (x, then y, then z), formed in `dtype` from the fp32 fractions."""
    f = frac.to(dtype)
    ws = []
    for idx in range(8):
        w = torch.ones_like(f[..., 0])
        for k in range(3):
            w = w * (f[..., k] if idx & (1 << k) else 1 - f[..., k])
        ws.append(w)
    return torch.stack(ws, -1)


def hash_encode_t(grid, entries, frac):
    """grid [n_params] (any float dtype) -> [n,32]: sum over corners of weight * table entry, in corner order."""
    tab = grid.view(-1, 2)
    w = corner_weights(frac, grid.dtype)
    out = 0
    for idx in range(8):
        out = out + w[:, :, idx, None] * tab[entries[:, :, idx]]
    return out.reshape(entries.shape[0], -1)


def hash_backward_ref(levels, pos, grad_enc):
    """kernel_grid_backward in fp64 from the fp32 cells and fractions.  pos [n,3] fp32 numpy, grad_enc [n,32] numpy ->
    (grad [n_entries,2] fp64, abs [n_entries,2] fp64 = sum |w g|, count [n_entries] = contributions per entry)."""
    ent, frac, _ = hash_geometry(levels, torch.as_tensor(np.ascontiguousarray(pos, np.float32)))
    n, L = ent.shape[:2]
    w = corner_weights(frac, torch.float64)                                  # [n,L,8]
    g = torch.as_tensor(np.asarray(grad_enc, np.float64)).reshape(n, L, 1, 2)
    contrib = (w[..., None] * g).reshape(-1, 2)
    flat = ent.reshape(-1)
    n_entries = int(levels["offsets"][-1])
    grad = torch.zeros(n_entries, 2, dtype=torch.float64).index_add_(0, flat, contrib)
    ab = torch.zeros(n_entries, 2, dtype=torch.float64).index_add_(0, flat, contrib.abs())
    count = torch.zeros(n_entries, dtype=torch.float64).index_add_(0, flat, torch.ones(flat.shape[0], dtype=torch.float64))
    return grad.numpy(), ab.numpy(), count.numpy()


# --------------------------------------------------------------------------------------------------------------- networks
def params_t(arrs, dtype, device="cpu", requires_grad=True):
    """{'grid', the five weights} as torch leaves in `dtype` from a scene's arrays."""
    p = {"grid": torch.as_tensor(np.asarray(arrs["grid"], np.float32)).reshape(-1).to(device, dtype)}
    for k in WEIGHT_KEYS:
        p[k] = torch.as_tensor(np.asarray(arrs[k], np.float32)).to(device, dtype)
    for v in p.values():
        v.requires_grad_(requires_grad)
    return p


def sh_t(dirs):
    """SH-16 of directions warped to [0,1] (torch restatement of SphericalEncode.h:60-100, in the input's dtype)."""
    x, y, z = dirs[:, 0] * 2 - 1, dirs[:, 1] * 2 - 1, dirs[:, 2] * 2 - 1
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    return torch.stack([torch.full_like(x, 0.28209479177387814), -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
                        1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.94617469575755997 * z2 - 0.31539156525251999, -1.0925484305920792 * xz,
                        0.54627421529603959 * x2 - 0.54627421529603959 * y2, 0.59004358992664352 * y * (-3.0 * x2 + y2), 2.8906114426405538 * xy * z,
                        0.45704579946446572 * y * (1.0 - 5.0 * z2), 0.3731763325901154 * z * (5.0 * z2 - 3.0), 0.45704579946446572 * x * (1.0 - 5.0 * z2),
                        1.4453057213202769 * z * (x2 - y2), 0.59004358992664352 * x * (-x2 + 3.0 * y2)], -1)


def network_t(p, entries, frac, sh):
    """NGPNetworks.execute_ in the parameters' dtype -> [n,4] = (rgb raw, density raw)."""
    enc = hash_encode_t(p["grid"], entries, frac)
    h = torch.relu(enc @ p["density_mlp.0.weight"].t())
    den = h @ p["density_mlp.2.weight"].t()
    x = torch.cat([den, sh.to(den.dtype)], 1)
    h = torch.relu(x @ p["rgb_mlp.0.weight"].t())
    h = torch.relu(h @ p["rgb_mlp.2.weight"].t())
    return torch.cat([h @ p["rgb_mlp.4.weight"].t(), den[:, :1]], 1)


# --------------------------------------------------------------------------------------------------------------- compositor
def unwarp_dt_t(w):
    """Column 3 of the rows, unwarped in fp32 as the compositor does (an input like the rows themselves)."""
    mn = torch.tensor(1.73205080757, dtype=torch.float32) / 1024
    mx = mn * 16
    return w.to(torch.float32) * (mx - mn).to(w.device) + mn.to(w.device)


def ray_rows(numsteps, n_rows):
    """numsteps [R,2] (torch int) -> (idx [R,M] int64 rows (0 where invalid), valid [R,M] bool, n [R], nc [R]) with nc the capacity clamp."""
    ns = numsteps.to(torch.int64)
    n, base = ns[:, 0], ns[:, 1]
    nc = torch.minimum(n_rows - torch.clamp(base, max=n_rows), n)
    M = int(nc.max()) if nc.numel() else 0
    j = torch.arange(M, device=ns.device)[None, :]
    valid = j < nc[:, None]
    return torch.where(valid, base[:, None] + j, torch.zeros_like(j)), valid, n, nc


def composite_t(net_out, dt, numsteps, n_rows, bg, stop=None):
    """The training compositor, vectorised.  net_out [n_rows,4] (its dtype is the arithmetic's), dt [n_rows] (unwarped), numsteps [R,2], bg [R,3].
    `stop` [R] = samples composited per ray; None: decided here from the (detached) forward, T_j = exp(-optical depth in front of j) < 1e-4.
    Returns (rgb [R,3], stop).  Differentiable with respect to net_out with the stop index fixed."""
    idx, valid, n, nc = ray_rows(numsteps, n_rows)
    R, M = idx.shape
    dtype = net_out.dtype
    if M == 0:
        return torch.where((n == 0)[:, None], bg.to(dtype), torch.zeros_like(bg, dtype=dtype)), torch.zeros(R, dtype=torch.int64, device=idx.device)
    o = net_out[idx]                                                            # [R,M,4]
    tau = torch.where(valid, torch.exp(o[..., 3]) * dt.to(dtype)[idx], torch.zeros((), dtype=dtype, device=o.device))
    before = torch.cumsum(tau, 1) - tau
    T = torch.exp(-before)
    if stop is None:
        dead = valid & (T.detach() < THR)
        first = torch.where(dead, torch.arange(M, device=idx.device)[None, :].expand(R, M), torch.full((R, M), M, device=idx.device)).min(1).values
        stop = torch.minimum(first, nc)
    live = valid & (torch.arange(M, device=idx.device)[None, :] < stop[:, None])
    w = torch.where(live, -torch.expm1(-tau) * T, torch.zeros((), dtype=dtype, device=o.device))
    rgb = (w[..., None] * torch.sigmoid(o[..., :3])).sum(1)
    t_end = torch.exp(-(torch.where(live, tau, torch.zeros((), dtype=dtype, device=o.device))).sum(1))
    full = (stop == n)
    return rgb + torch.where(full, t_end, torch.zeros_like(t_end))[:, None] * bg.to(dtype), stop


COMPOSITOR_MUTATIONS = ("dt_first_row", "dt_next_row", "dt_backward_stale", "suffix_without_background", "background_when_cut", "stop_one_late")


def composite_loop(net_out, coords, numsteps, n_rows, bg, dtype=np.float64, grad_rgb=None, mutation=None):
    """The kernel's loop in numpy `dtype`: per ray T = 1; for j < nc: stop if T < 1e-4; rgb += alpha T c; T *= 1 - alpha; background if all n steps were
    walked.  Serial over j, vectorised over rays.  Returns dict(rgb [R,3], stop [R] samples composited, n, nc, T_end [R], T_seen [R,M] = T in front of sample j
    (frozen behind the stop), and with grad_rgb: grad [n_rows,4], sigma_dt [n_rows] (0 on rows not composited), ray [n_rows] = owning ray of each composited
    row, -1 elsewhere).
    `mutation` (one of COMPOSITOR_MUTATIONS) restates a defect a kernel could have; tests/test_ngp_train_host.py proves that the GPU tests' bars see each:
      dt_first_row               every row of a ray uses the dt of the ray's first row;
      dt_next_row                row j uses the dt of row j + 1, the ray's last row keeps its own;
      dt_backward_stale          T, w and rgb use the true dt; the sigma dt factor and the alpha of the gradient use the first row's (the backward's second walk
                                 disagreeing with its first);
      suffix_without_background  the gradient's suffix leaves out T_end * bg;
      background_when_cut        the background is added when stop == nc instead of stop == n;
      stop_one_late              the T < 1e-4 test comes after the sample is added: the sample in front of which T fell below the threshold is composited too."""
    from oracle import ngp_oracle as N
    assert mutation is None or mutation in COMPOSITOR_MUTATIONS
    ns = np.asarray(numsteps, np.int64).reshape(-1, 2)
    n, base = ns[:, 0], ns[:, 1]
    R = n.shape[0]
    nc = np.minimum(n_rows - np.minimum(n_rows, base), n)
    M = int(nc.max()) if R else 0
    j = np.arange(M)[None, :]
    valid = j < nc[:, None]
    idx = np.where(valid, base[:, None] + j, 0)
    one = dtype(1)
    o = np.asarray(net_out, np.float32)[idx].astype(dtype) if M else np.zeros((R, 0, 4), dtype)
    dt = np.asarray(N.unwarp_dt(np.asarray(coords, np.float32)[idx, 3]), np.float32).astype(dtype) if M else np.zeros((R, 0), dtype)
    dt_true = dt
    if M and mutation == "dt_first_row":
        dt = np.broadcast_to(dt[:, :1], dt.shape).copy()
    elif M and mutation == "dt_next_row":
        dt = np.where(j + 1 < nc[:, None], np.concatenate([dt[:, 1:], dt[:, -1:]], 1), dt)
    sigma_dt = np.exp(o[..., 3]) * dt
    alpha = one - np.exp(-sigma_dt)
    c = one / (one + np.exp(-o[..., :3]))
    T = np.ones(R, dtype)
    Tj = np.zeros((R, M), dtype)
    live = np.zeros((R, M), bool)
    alive = np.ones(R, bool)
    for k in range(M):
        late = alive & valid[:, k] & (T < dtype(THR)) if mutation == "stop_one_late" else None
        alive = alive & valid[:, k] & ~(T < dtype(THR))
        live[:, k] = alive
        Tj[:, k] = T
        T = np.where(alive, T * (one - alpha[:, k]), T)
        if late is not None:
            live[:, k] |= late                                                 # added, and only then tested: T stays what the test saw
    stop = live.sum(1)
    w = np.where(live, alpha * Tj, dtype(0))
    prefix = np.cumsum(w[..., None] * c, axis=1, dtype=dtype)                  # sequential: the loop's own order of additions
    bgv = np.asarray(bg, np.float32).astype(dtype).reshape(-1, 3)
    broke_late = (live & (Tj < dtype(THR))).any(1)                             # stop_one_late only: that loop left through its break, so no background
    walked = (stop == nc) if mutation == "background_when_cut" else (stop == n) & ~broke_late
    back = np.where(walked, T, dtype(0))[:, None] * bgv
    rgb = (prefix[:, -1] if M else np.zeros((R, 3), dtype)) + back
    res = dict(rgb=rgb, stop=stop, n=n, nc=nc, T_end=T, T_seen=Tj)
    if grad_rgb is not None:
        g = np.asarray(grad_rgb, np.float32).astype(dtype)[:, None, :]
        suffix = (rgb - back if mutation == "suffix_without_background" else rgb)[:, None, :] - prefix
        sigma_dt_g, alpha_g = sigma_dt, alpha
        if M and mutation == "dt_backward_stale":
            sigma_dt_g = np.exp(o[..., 3]) * dt_true[:, :1]
            alpha_g = one - np.exp(-sigma_dt_g)
        Tn = Tj * (one - alpha_g)
        d_c = g * w[..., None] * (c * (one - c))
        d_s = sigma_dt_g * (g * (Tn[..., None] * c - suffix)).sum(-1)
        grad = np.zeros((n_rows, 4), dtype)
        sd = np.zeros(n_rows, dtype)
        ray = np.full(n_rows, -1, np.int64)
        grad[idx[live]] = np.concatenate([d_c, d_s[..., None]], -1)[live]
        sd[idx[live]] = sigma_dt[live]
        ray[idx[live]] = np.broadcast_to(np.arange(R)[:, None], (R, M))[live]
        res.update(grad=grad, sigma_dt=sd, ray=ray)
    return res


def backward_row_error(got, ref, grad_rgb):
    """Test 2's measure: the error of row j scaled by max|g_ray| * max(1, sigma_j dt_j), maximised over the rows a ray composited (`ref` is composite_loop's
    fp64 result; rows outside are compared exactly by the caller)."""
    own = ref["ray"] >= 0
    if not own.any():
        return 0.0
    gmax = np.abs(np.asarray(grad_rgb, np.float64)).max(1)[ref["ray"][own]]
    scale = np.maximum(gmax, 1e-30) * np.maximum(1.0, ref["sigma_dt"][own])
    return float((np.abs(np.asarray(got, np.float64)[own] - ref["grad"][own]).max(1) / scale).max())


# --------------------------------------------------------------------------------------------------------------- compositor cases
# Inputs of the compositor tests, built from the CPU oracle only: the host test checks their conditions and the bars' power on them, the GPU test runs the
# kernels on them.  Two of them give every row its own step size, which no constant-dt input can (column 3 is one value there: a kernel that took dt from
# another row, or whose backward walks disagreed about it, would compute the same bits):
#   * the designed ladder with column 3 redrawn per row (`random_dt_rows`): the network's outputs are an input there, so only the compositor's own rounding
#     moves ln T and a ray is compared when its smallest break margin |ln(T / 1e-4)| is at least RANDOM_DT_MARGIN;
#   * the shared scene sampled with const_dt=False (cone stepping), rays kept by the network bar's shift of ln T as on the constant-dt scene.
SCENES = (1, 2, 33, 97, F.NO_BREAK)
CAP_KINDS = ("total", "inside", "ray_end", "slack")
SLACK = 37                                                    # rows behind the total in the "slack" capacity: owned by no ray
RANDOM_DT_SEED = 300                                          # chosen on the fp64 reference alone: at most 2 % of the ladder's rays fall below the margin
RANDOM_DT_MARGIN = 1e-3
RANDOM_DT_MAX = 0.1                                           # warped; unwarped dt then runs from 0.00085 (the constant step) to 0.0042
LEFT_OUT_SHARE = 0.02
FORWARD_BAR = 2e-5                                            # tvr_ngp_composite's bar


def const_warped_dt():
    """Column 3 of a const_dt row: dt = MIN_CONE_STEPSIZE / 2 warped as the sampler warps it (-1/30 in fp32)."""
    from oracle import ngp_oracle as N
    f32 = np.float32
    mn = N.MIN_CONE_STEPSIZE
    return f32(f32(f32(np.float64(mn) * 0.5) - mn) / f32(mn * f32(16) - mn))


def random_dt_rows(coords, seed):
    """A copy of `coords` with column 3 redrawn per row, uniform in [the constant warped dt, RANDOM_DT_MAX], as fp32."""
    c = np.array(coords, np.float32, copy=True)
    c[:, 3] = np.random.default_rng(seed).uniform(float(const_warped_dt()), RANDOM_DT_MAX, c.shape[0]).astype(np.float32)
    return c


def backward_bar(e32):
    """The compositor backward's bar from the fp32 loop's own scaled error."""
    return max(4 * e32, 1e-6)


def row_owner(numsteps, n_rows):
    """[n_rows] the ray whose capacity-clamped steps hold each row, -1 for rows no ray owns."""
    idx, valid, _, _ = ray_rows(torch.as_tensor(np.asarray(numsteps, np.int64)), n_rows)
    owner = np.full(n_rows, -1, np.int64)
    idx, valid = idx.numpy(), valid.numpy()
    owner[idx[valid]] = np.broadcast_to(np.arange(idx.shape[0])[:, None], idx.shape)[valid]
    return owner


@functools.lru_cache(maxsize=None)
def designed_inputs(k, dt_kind="const"):
    """The 421-ray ladder in designed_scene(k): rows (dt_kind "random": column 3 redrawn per row), network outputs (the C oracle's; the network does not read
    column 3), a random background and gradient per ray, the capacities, and the rays that are compared (all of them for "const")."""
    from oracle import ngp_oracle as N
    assert dt_kind in ("const", "random")
    _, _, coords, ns = F.designed_rows()
    levels, arrs = F.designed_scene(k)
    out = N.network_c(levels, arrs, coords)
    rng = np.random.default_rng(100 + k)
    R, total = ns.shape[0], coords.shape[0]
    bg = rng.random((R, 3), dtype=np.float32)
    g = rng.normal(0, 1, (R, 3)).astype(np.float32)
    n, base = ns[:, 0].astype(np.int64), ns[:, 1].astype(np.int64)
    inside = next(r for r in range(R // 2, R) if n[r] >= 3 and base[r] + n[r] < total)
    at_end = next(r for r in range(R // 3, R) if n[r] >= 1 and base[r] + n[r] < total)
    caps = {"total": total, "inside": int(base[inside] + n[inside] // 2), "ray_end": int(base[at_end] + n[at_end]), "slack": total + SLACK}
    keep = np.ones(R, bool)
    if dt_kind == "random":
        coords = random_dt_rows(coords, RANDOM_DT_SEED)
        keep = F.composite_f64(out, coords, ns, F.BG)[2] >= RANDOM_DT_MARGIN       # every decision of the uncut ray: a superset of any capacity's
    return coords, ns, out, bg, g, caps, keep


@functools.lru_cache(maxsize=None)
def designed_case(k, cap_kind, dt_kind="const"):
    """Inputs cut / padded to the capacity, and the loop reference in fp64 and fp32 (computed once, shared by the tests that need it)."""
    coords, ns, out, bg, g, caps, keep = designed_inputs(k, dt_kind)
    n_rows, total = caps[cap_kind], coords.shape[0]
    if n_rows > total:                                          # rows no ray owns hold NaN: nothing may read them, their gradient is exactly 0
        out_c = np.concatenate([out, np.full((n_rows - total, 4), np.nan, np.float32)])
        coords_c = np.concatenate([coords, np.full((n_rows - total, 7), np.nan, np.float32)])
    else:
        out_c, coords_c = out[:n_rows], coords[:n_rows]
    ref = composite_loop(out_c, coords_c, ns, n_rows, bg, np.float64, grad_rgb=g)
    r32 = composite_loop(out_c, coords_c, ns, n_rows, bg, np.float32, grad_rgb=g)
    return out_c, coords_c, ns, bg, g, n_rows, ref, r32, keep


@functools.lru_cache(maxsize=None)
def scene_rows(const_dt=True):
    """The shared aabb_scale-4 scene under ngp_camera_rays(32, 32), marched by the oracle from Pcg32(1337): (levels, arrays, rays_o, rays_d, coords, numsteps,
    the C oracle's network outputs).  const_dt=False: cone stepping, every row its own dt."""
    from conftest import NGP_AABB_SCALE, ngp_camera_rays
    from jittor_myc_nerfs_amd import synthetic
    from oracle import ngp_oracle as N
    levels = N.grid_levels(NGP_AABB_SCALE)
    arrs = synthetic.make_ngp_scene_arrays(levels["offsets"])
    arrs["density_grid_bitfield"], _ = N.update_bitfield(arrs["density_grid"])
    o, d = ngp_camera_rays(32, 32)
    coords, _, ns, _, _ = N.sample(o, d, arrs["density_grid_bitfield"], NGP_AABB_SCALE, N.Pcg32(1337).state, const_dt=const_dt)
    out = N.network_c(levels, arrs, coords)
    return levels, arrs, o, d, coords, ns, out


def scene_capacities(total, const_dt):
    """The row counts the shared-scene compositor tests run: all rows, and a cut (100 000 on the constant-dt rows, two thirds of the cone rows)."""
    return {"total": total, "cut": 100000 if const_dt else total * 2 // 3}


@functools.lru_cache(maxsize=None)
def scene_inputs(const_dt=True):
    """(coords, numsteps, out, bg, g, keep) of the shared scene: a random background and gradient per ray; rays are compared when the network bar cannot move
    ln T across any of their break decisions."""
    _, _, _, _, coords, ns, out = scene_rows(const_dt)
    rng = np.random.default_rng(7 if const_dt else 8)
    R = ns.shape[0]
    bg, g = rng.random((R, 3), dtype=np.float32), rng.normal(0, 1, (R, 3)).astype(np.float32)
    keep = F.composite_f64(out, coords, ns, F.BG)[2] >= F.network_shift(out)
    return coords, ns, out, bg, g, keep


def compositor_case(name):
    """(out, coords, numsteps, bg, g, n_rows, keep) of a named case: 'ladder-{const|random}-k{K}-{capacity}' or '{shared|cone}-{total|cut}'."""
    parts = name.split("-")
    if parts[0] == "ladder":
        out, coords, ns, bg, g, n_rows, _, _, keep = designed_case(int(parts[2][1:]), parts[3], parts[1])
        return out, coords, ns, bg, g, n_rows, keep
    const_dt = {"shared": True, "cone": False}[parts[0]]
    coords, ns, out, bg, g, keep = scene_inputs(const_dt)
    n_rows = scene_capacities(coords.shape[0], const_dt)[parts[1]]
    return out[:n_rows], coords[:n_rows], ns, bg, g, n_rows, keep


def compositor_measures(case, got_rgb, got_grad, ref, r32=None):
    """The GPU tests' own measures of a compositor result against the fp64 loop `ref` on `case` (compositor_case's tuple): rgb L-inf on the kept rays, the
    scaled backward error on the kept rays' composited rows, and the number of rows that must be exactly 0 (behind a kept ray's break, behind the cut, owned
    by no ray) but are not.  With `r32` (the fp32 loop) also its scaled backward error, from which the backward bar derives."""
    _, _, ns, _, g, n_rows, keep = case
    fwd = float(np.abs(np.asarray(got_rgb, np.float64) - ref["rgb"])[keep].max())
    rows_kept = (ref["ray"] >= 0) & keep[np.maximum(ref["ray"], 0)]
    sub = dict(ref, ray=np.where(rows_kept, ref["ray"], -1))
    owner = row_owner(ns, n_rows)
    dead = (ref["ray"] < 0) & ((owner < 0) | keep[np.maximum(owner, 0)])
    res = dict(forward=fwd, backward=backward_row_error(got_grad, sub, g), dead_rows=int(dead.sum()), dead_nonzero=int(np.asarray(got_grad)[dead].any(1).sum()))
    if r32 is not None:
        res["e32"] = backward_row_error(r32["grad"], sub, g)
    return res


# (case, mutation) pairs the host test proves the bars' power on; every mutation appears
COMPOSITOR_POWER = ([("cone-total", m) for m in ("dt_first_row", "dt_next_row", "dt_backward_stale", "suffix_without_background", "stop_one_late")]
                    + [("cone-cut", m) for m in ("dt_first_row", "dt_next_row", "dt_backward_stale", "background_when_cut")]
                    + [("ladder-random-k33-total", m) for m in ("dt_first_row", "dt_next_row", "dt_backward_stale", "stop_one_late")]
                    + [("ladder-random-k97-inside", m) for m in ("dt_first_row", "dt_next_row", "dt_backward_stale", "background_when_cut")]
                    + [(f"ladder-random-k{F.NO_BREAK}-total", m) for m in ("dt_first_row", "dt_next_row", "dt_backward_stale", "suffix_without_background")])


# --------------------------------------------------------------------------------------------------------------- one step
def huber_t(x, target, delta=0.1):
    rel = (x - target).abs()
    return torch.where(rel > delta, rel - 0.5 * delta, 0.5 / delta * rel * rel)


def step_t(p, entries, frac, sh, dt, numsteps, n_rows, bg, target, stop=None, delta=0.1):
    """(loss sum, rgb, net_out, stop) of one training step from its rows, in the parameters' dtype."""
    out = network_t(p, entries, frac, sh)
    rgb, stop = composite_t(out, dt, numsteps, n_rows, bg, stop)
    return huber_t(rgb, target.to(rgb.dtype), delta).sum(), rgb, out, stop


def grads_of_step(arrs, levels, coords, numsteps, n_rows, bg, target, dtype, stop=None, keep_rays=None, device="cpu"):
    """Every parameter's gradient of the Huber sum over `keep_rays` (bool [R], None: all) on these rows, in `dtype`.  Returns ({name: grad numpy fp64}, stop)."""
    c = torch.as_tensor(np.ascontiguousarray(coords[:n_rows], np.float32)).to(device)
    ent, frac, _ = hash_geometry(levels, c[:, :3])
    p = params_t(arrs, dtype, device)
    sh = sh_t(c[:, 4:7].to(dtype))
    ns = torch.as_tensor(np.asarray(numsteps, np.int32)).to(device)
    out = network_t(p, ent, frac, sh)
    rgb, stop = composite_t(out, unwarp_dt_t(c[:, 3]), ns, n_rows, torch.as_tensor(np.asarray(bg, np.float32)).to(device), None if stop is None else torch.as_tensor(stop).to(device))
    loss = huber_t(rgb, torch.as_tensor(np.asarray(target, np.float32)).to(device, dtype))
    if keep_rays is not None:
        loss = loss * torch.as_tensor(np.asarray(keep_rays)).to(device, dtype)[:, None]
    loss.sum().backward()
    return {k: v.grad.detach().double().cpu().numpy() for k, v in p.items()}, stop.cpu().numpy()


# --------------------------------------------------------------------------------------------------------------- data
def tiny_blender_scene(root, n=3, size=6):
    """A NeRF-synthetic style directory: transforms_train.json and n RGBA PNGs of size x size."""
    import json
    from PIL import Image
    from jittor_myc_nerfs_amd import rays as R
    rng = np.random.default_rng(9)
    os.makedirs(os.path.join(root, "train"))
    frames, imgs = [], []
    for i, pose in enumerate(R.sphere_poses(n, 4.0)):
        img = rng.integers(0, 256, (size, size, 4), dtype=np.uint8)
        Image.fromarray(img, "RGBA").save(os.path.join(root, "train", f"r_{i}.png"))
        imgs.append(img)
        m = np.asarray(pose, np.float64).copy()
        m[:, 0] *= -1                                                       # rays.sphere_poses looks down +z of its own frame; the json's cameras (read with
        m[:, 2] *= -1                                                       # NerfRays' correct_pose = (1, -1, -1)) look down -z: the same view either way
        frames.append({"file_path": f"./train/r_{i}", "transform_matrix": m.tolist()})
    with open(os.path.join(root, "transforms_train.json"), "w") as f:
        json.dump({"camera_angle_x": 0.6911, "frames": frames}, f)
    return np.stack(imgs)
