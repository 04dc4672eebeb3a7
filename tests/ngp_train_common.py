"""Shared by tests/test_ngp_train_host.py and tests/test_gpu_ngp_train.py: references for Instant-NGP training.

  * hash_geometry / hash_encode_t   the hash grid in torch: cells and fractions in fp32 exactly as the oracle forms them (fmaf(pos, scale, 0.5), floor,
                                    subtraction — at scale 8192 an fp64 fraction differs from the kernel's by 1e-3), entries by grid_index's arithmetic,
                                    the trilinear blend in the tensor's dtype.  Differentiable with respect to the grid.
  * network_t                       the five bias-free Linears around it (SH from the oracle, no gradient).
  * composite_t                     the training compositor vectorised over rays (a padded [rays, steps] layout, per-ray prefix sums), with the stop index
                                    held fixed: differentiable with respect to the network outputs.
  * composite_loop                  the compositor's loop as the kernel runs it — T multiplied up step by step, colour added in sample order — in a chosen
                                    numpy dtype, serial over the steps and vectorised over the rays (every ray sees exactly its own loop's operations in
                                    order), plus the analytic gradient of include/tvr_ngp.h.
  * step_t                          one whole step's loss sum from (parameters, rows, background, target).
fp64 on the CPU is the reference; the same code in fp32 is the yardstick the GPU tests derive their bars from.
"""
import os

import numpy as np
import torch

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


def composite_loop(net_out, coords, numsteps, n_rows, bg, dtype=np.float64, grad_rgb=None):
    """The kernel's loop in numpy `dtype`: per ray T = 1; for j < nc: stop if T < 1e-4; rgb += alpha T c; T *= 1 - alpha; background if all n steps were
    walked.  Serial over j, vectorised over rays.  Returns dict(rgb [R,3], stop [R] samples composited, n, nc, T_end [R], and with grad_rgb: grad [n_rows,4],
    sigma_dt [n_rows] (0 on rows not composited), ray [n_rows] = owning ray of each composited row, -1 elsewhere)."""
    from oracle import ngp_oracle as N
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
    sigma_dt = np.exp(o[..., 3]) * dt
    alpha = one - np.exp(-sigma_dt)
    c = one / (one + np.exp(-o[..., :3]))
    T = np.ones(R, dtype)
    Tj = np.zeros((R, M), dtype)
    live = np.zeros((R, M), bool)
    alive = np.ones(R, bool)
    for k in range(M):
        alive = alive & valid[:, k] & ~(T < dtype(THR))
        live[:, k] = alive
        Tj[:, k] = T
        T = np.where(alive, T * (one - alpha[:, k]), T)
    stop = live.sum(1)
    w = np.where(live, alpha * Tj, dtype(0))
    prefix = np.cumsum(w[..., None] * c, axis=1, dtype=dtype)                  # sequential: the loop's own order of additions
    bgv = np.asarray(bg, np.float32).astype(dtype).reshape(-1, 3)
    rgb = (prefix[:, -1] if M else np.zeros((R, 3), dtype)) + np.where(stop == n, T, dtype(0))[:, None] * bgv
    res = dict(rgb=rgb, stop=stop, n=n, nc=nc, T_end=T)
    if grad_rgb is not None:
        g = np.asarray(grad_rgb, np.float32).astype(dtype)[:, None, :]
        suffix = rgb[:, None, :] - prefix
        Tn = Tj * (one - alpha)
        d_c = g * w[..., None] * (c * (one - c))
        d_s = sigma_dt * (g * (Tn[..., None] * c - suffix)).sum(-1)
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
