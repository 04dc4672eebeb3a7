"""Training the Instant-NGP field on HIP kernels: `Runner.train` (jnerf-myc/python/jnerf/runner/runner.py:62-86) at row level, eager, one host read per
step (the sampler's count).  New kernels: csrc/tvr_ngp_train.hip (the hash grid's scatter-add backward, the training compositor forward and backward; C-ABI
in include/tvr_ngp.h); the five Linears train through autograd_ops._LinearFn.  No CPU fallback: a missing kernel or a CPU tensor raises.

Mirrors, under jnerf-myc/python/jnerf/:
  network_train          models/networks/ngp_network.py:78-85 under autograd (NGPNetworks.forward_train)
  composite_train        ops/code_ops/calc_rgb.py:35-116 (CalcRgb.execute / grad), DensityGridSampler.rays2rgb(inference=False)
  NGPExpDecay, NGPEma    optims/expdecay.py, optims/ema.py over torch.optim.Adam with ngp_comp.py's values
  NGPTrainData           dataset/dataset.py (train mode: images, NGP-convention cameras, uniformly drawn pixels)
  NGPTrainer             runner/runner.py:62-86
  save_jnerf_checkpoint  runner/runner.py:127-135 (what ngp.load_jnerf_checkpoint reads)

Command line:  python -m jittor_myc_nerfs_amd.ngp_train --data DIR --steps N --out params.pkl [--aabb_scale S]
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import ngp
from .autograd_ops import _LinearFn
from .losses import huber_loss


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


# ------------------------------------------------------------------------------------------------------------------ autograd over the kernels
class _HashEncodeFn(torch.autograd.Function):
    """`HashEncoder.execute` with the gradient of `m_grid`: forward `tvr_ngp_hash_encode`, backward `tvr_ngp_hash_encode_backward` into a zeroed buffer
    (float atomics: the last bits depend on arrival order).  Positions get no gradient (the reference detaches them)."""

    @staticmethod
    def forward(ctx, grid, cfg, pos):
        n = pos.shape[0]
        out = torch.empty(n, 32, device=grid.device)
        L.check(L.lib().tvr_ngp_hash_encode(C.byref(cfg), grid.data_ptr(), pos.data_ptr(), pos.stride(0) if n else 3, n, out.data_ptr(), _stream(grid.device)),
                "tvr_ngp_hash_encode")
        ctx.cfg, ctx.pos, ctx.n_params = cfg, pos, grid.numel()
        return out

    @staticmethod
    def backward(ctx, g_out):
        pos, n = ctx.pos, ctx.pos.shape[0]
        g = g_out.to(torch.float32).contiguous()
        grad = torch.zeros(ctx.n_params, device=g.device)
        L.check(L.lib().tvr_ngp_hash_encode_backward(C.byref(ctx.cfg), pos.data_ptr(), pos.stride(0) if n else 3, n, g.data_ptr(), grad.data_ptr(), _stream(g.device)),
                "tvr_ngp_hash_encode_backward")
        return grad, None, None


def hash_encode_backward(encoder: "ngp.HashEncoder", pos: torch.Tensor, grad_enc: torch.Tensor, grad_grid: Optional[torch.Tensor] = None,
                         variant: Optional[int] = None) -> torch.Tensor:
    """`tvr_ngp_hash_encode_backward` on its own: ACCUMULATES into `grad_grid` (a new zeroed buffer when None).  `pos` [n, >=3] may be row-strided (the
    sampler's rows).  `variant` (0, 1, 2) selects a kernel variant through the library's measurement hook; None is the shipped call."""
    ngp._need_gpu(grad_enc, "hash_encode_backward")
    ngp._need_gpu(pos, "hash_encode_backward")
    if pos.dim() != 2 or pos.shape[1] < 3 or pos.stride(1) != 1 or pos.dtype != torch.float32:
        raise L.TvrError("hash_encode_backward: positions must be fp32 rows [n, >=3] with unit column stride")
    n = pos.shape[0]
    g = grad_enc.to(torch.float32).contiguous()
    if tuple(g.shape) != (n, 32):
        raise L.TvrError(f"hash_encode_backward: grad_enc is {tuple(g.shape)}, expected ({n}, 32)")
    if grad_grid is None:
        grad_grid = torch.zeros(encoder.m_n_params, device=g.device)
    if grad_grid.numel() != encoder.m_n_params or grad_grid.dtype != torch.float32 or not grad_grid.is_contiguous() or not grad_grid.is_cuda:
        raise L.TvrError(f"hash_encode_backward: grad_grid must be a contiguous fp32 device tensor of {encoder.m_n_params} elements")
    args = (C.byref(encoder.cfg), pos.data_ptr(), pos.stride(0) if n else 3, n, g.data_ptr(), grad_grid.data_ptr())
    if variant is None:
        L.check(L.lib().tvr_ngp_hash_encode_backward(*args, _stream(g.device)), "tvr_ngp_hash_encode_backward")
    else:                                                               # the library's measurement hook: exported, but not part of the C-ABI
        fn = L.lib().tvr_ngp_hash_encode_backward_variant
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(L.NgpGridCfg), C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.check(fn(*args, int(variant), _stream(g.device)), "tvr_ngp_hash_encode_backward_variant")
    return grad_grid


def network_train(model: "ngp.NGPNetworks", pos: torch.Tensor, dirs: torch.Tensor) -> torch.Tensor:
    """The graph of `NGPNetworks.forward_train`: hash grid -> relu(Linear) -> Linear = the 16 density outputs; cat with SH (no gradient) -> the three colour
    Linears; output (rgb raw, density raw).  `pos` / `dirs` are detached fp32 rows on the device (row-strided views are read in place)."""
    grid = model.pos_encoder.m_grid
    ngp._need_gpu(grid, "NGPNetworks.forward_train")
    ngp._need_gpu(pos, "NGPNetworks.forward_train")
    ngp._need_gpu(dirs, "NGPNetworks.forward_train")
    w = model._weights()
    enc = _HashEncodeFn.apply(grid, model.pos_encoder.cfg, pos)
    h = torch.relu(_LinearFn.apply(enc, w[0], None))
    den = _LinearFn.apply(h, w[1], None)
    x = torch.cat([den, model.dir_encoder(dirs)], 1)
    h = torch.relu(_LinearFn.apply(x, w[2], None))
    h = torch.relu(_LinearFn.apply(h, w[3], None))
    rgb = _LinearFn.apply(h, w[4], None)
    return torch.cat([rgb, den[:, :1]], 1)


class _CompositeFn(torch.autograd.Function):
    """`CalcRgb` (calc_rgb.py:35-116): forward `tvr_ngp_composite_train`, backward `tvr_ngp_composite_backward`.  The rows past the capacity are cut by the
    kernels themselves from (numsteps, n_rows)."""

    @staticmethod
    def forward(ctx, net_out, coords, numsteps, bg):
        dev = numsteps.device
        o = net_out.detach().to(dev, torch.float32).contiguous()
        b = bg.detach().to(dev, torch.float32).contiguous()
        R, n_rows = numsteps.shape[0], o.shape[0]
        rgb = torch.empty(R, 3, device=dev)
        L.check(L.lib().tvr_ngp_composite_train(o.data_ptr(), coords.data_ptr(), numsteps.data_ptr(), R, n_rows, b.data_ptr(), rgb.data_ptr(), _stream(dev)),
                "tvr_ngp_composite_train")
        ctx.save_for_backward(o, coords, numsteps, b)
        return rgb

    @staticmethod
    def backward(ctx, g_rgb):
        o, coords, numsteps, b = ctx.saved_tensors
        dev = numsteps.device
        g = g_rgb.to(torch.float32).contiguous()
        R, n_rows = numsteps.shape[0], o.shape[0]
        grad = L.dev_empty((n_rows, 4), torch.float32, dev, "tvr_ngp_composite_backward grad_net_out")
        L.check(L.lib().tvr_ngp_composite_backward(o.data_ptr(), coords.data_ptr(), numsteps.data_ptr(), R, n_rows, b.data_ptr(), None, g.data_ptr(),
                                                   grad.data_ptr(), _stream(dev)), "tvr_ngp_composite_backward")      # rgb_out: in the signature only
        return grad, None, None, None


def composite_train(net_out: torch.Tensor, coords: torch.Tensor, numsteps: torch.Tensor, bg: torch.Tensor) -> torch.Tensor:
    """rgb [n_rays,3] of the training compositor under autograd.  net_out [n_rows,4], coords [n_rows,7] (contiguous), numsteps [n_rays,2] int32 = the
    sampler's UNCOMPACTED (steps, base), bg [n_rays,3].  n_rows is the row capacity actually used: a ray's steps past it are cut."""
    ngp._need_gpu(numsteps, "composite_train")
    ngp._need_gpu(coords, "composite_train")
    if coords.shape[0] != net_out.shape[0] or (coords.shape[0] and (tuple(coords.shape[1:]) != (7,) or not coords.is_contiguous())) or coords.dtype != torch.float32:
        raise L.TvrError("composite_train: coords must be contiguous fp32 [n_rows,7] with one row per network output")
    if numsteps.dtype != torch.int32 or not numsteps.is_contiguous() or numsteps.dim() != 2 or numsteps.shape[1] != 2:
        raise L.TvrError("composite_train: numsteps must be contiguous int32 [n_rays,2]")
    if tuple(bg.shape) != (numsteps.shape[0], 3):
        raise L.TvrError(f"composite_train: the background is {tuple(bg.shape)}, expected ({numsteps.shape[0]}, 3)")
    return _CompositeFn.apply(net_out, coords, numsteps, bg)


# ------------------------------------------------------------------------------------------------------------------ optimizers
def ngp_adam(params, lr: float = 1e-1, eps: float = 1e-15, betas: Tuple[float, float] = (0.9, 0.99)) -> torch.optim.Adam:
    """The nested optimizer with ngp_comp.py's values (`optim = dict(type='Adam', lr=1e-1, eps=1e-15, betas=(0.9, 0.99))`)."""
    return torch.optim.Adam(list(params), lr=lr, eps=eps, betas=betas)


class NGPExpDecay:
    """`ExpDecay` (optims/expdecay.py): before each nested step, once `steps >= decay_start` and every `decay_interval` steps from there (while
    `steps <= decay_end`), the learning-rate factor is multiplied by `decay_base`."""

    def __init__(self, nested_optimizer: torch.optim.Optimizer, decay_start: int = 20000, decay_interval: int = 10000, decay_base: float = 0.33,
                 decay_end: Optional[int] = None):
        self._nested_optimizer = nested_optimizer
        self.base_lr = nested_optimizer.param_groups[0]["lr"]
        self.decay_start, self.decay_interval, self.decay_base = decay_start, decay_interval, decay_base
        self.decay_end = 10000000 if decay_end is None else decay_end
        self.steps = 0
        self.m_learning_rate_factor = 1

    @property
    def lr(self) -> float:
        return self.base_lr * self.m_learning_rate_factor

    def step(self) -> None:
        if self.steps >= self.decay_start and (self.steps - self.decay_start) % self.decay_interval == 0 and self.steps <= self.decay_end:
            self.m_learning_rate_factor *= self.decay_base
        for pg in self._nested_optimizer.param_groups:
            pg["lr"] = self.base_lr * self.m_learning_rate_factor
        self._nested_optimizer.step()
        self.steps += 1

    def zero_grad(self) -> None:
        self._nested_optimizer.zero_grad(set_to_none=True)


class NGPEma:
    """`EMA` (optims/ema.py): after each optimizer step the parameters are REWRITTEN IN PLACE with their debiased exponential moving average,
    p <- ((1 - decay) p + decay v (1 - decay^(t-1))) / (1 - decay^t), v <- p — as the reference does (training continues from the averaged values).  The
    in-place write bumps the parameters' version, so `NGPNetworks.packed()` repacks on its next use."""

    def __init__(self, params, decay: float = 0.95):
        self.params = list(params)
        self.decay, self.steps = decay, 0
        self.values = [p.detach().clone() for p in self.params]

    @torch.no_grad()
    def ema_step(self) -> None:
        self.steps += 1
        ema_debias_old = 1 - self.decay ** (self.steps - 1)
        ema_debias_new = 1 / (1 - self.decay ** self.steps)
        for p, v in zip(self.params, self.values):
            p.copy_(((1 - self.decay) * p + self.decay * v * ema_debias_old) * ema_debias_new)
            v.copy_(p)


# ------------------------------------------------------------------------------------------------------------------ data
class NGPTrainData:
    """Training views: images [n,H,W,4] (RGBA, float in [0,1]), camera matrices [n,3,4] in the NGP convention (`ngp.matrix_nerf2ngp`) and focal lengths
    [n,2] (or one pair for all).  `next_batch` draws pixels uniformly over all images; ray r of an image is row r of `ngp.generate_rays` for its camera and
    is paired with pixel r of the image in row-major order.  `generate_rays` (the reference's `generate_rays_total_test`) numbers its rays so that this pairing
    holds for SQUARE images only, so other shapes are refused."""

    def __init__(self, images, transforms, focal_lengths, principal: Sequence[float] = (0.5, 0.5), device=None):
        self.images = torch.as_tensor(images, dtype=torch.float32).to(device)
        if self.images.dim() != 4 or self.images.shape[-1] != 4:
            raise ValueError(f"images must be [n,H,W,4] RGBA, got {tuple(self.images.shape)}")
        self.device = self.images.device
        self.n_images, self.H, self.W = (int(v) for v in self.images.shape[:3])
        if self.H != self.W:
            raise ValueError(f"images are {self.W}x{self.H}: ray r and pixel r agree for square images only (generate_rays' numbering)")
        self.transforms = torch.as_tensor(np.asarray(transforms, np.float32).reshape(-1, 3, 4)).to(self.device)
        f = np.asarray(focal_lengths, np.float32).reshape(-1, 2)
        self.focal_lengths = torch.as_tensor(np.tile(f, (self.n_images, 1)) if f.shape[0] == 1 else f).to(self.device)
        if self.transforms.shape[0] != self.n_images or self.focal_lengths.shape[0] != self.n_images:
            raise ValueError(f"{self.n_images} images, {self.transforms.shape[0]} cameras, {self.focal_lengths.shape[0]} focal lengths")
        self.principal = torch.tensor([float(principal[0]), float(principal[1])], device=self.device)
        self.resolution = (self.W, self.H)

    def rays_of(self, img_ids: torch.Tensor, pix: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """rays_o, rays_d [n,3] of ray index `pix` in image `img_ids`: `ngp.generate_rays`, one row at a time."""
        H, W = self.H, self.W
        xy = torch.stack([((pix % H).to(torch.float32) + 0.5) / H, ((pix // H).to(torch.float32) + 0.5) / W], -1)
        res = torch.tensor([W, H], dtype=torch.float32, device=self.device)
        d = torch.cat([(xy - self.principal) * res / self.focal_lengths[img_ids], torch.ones(pix.shape[0], 1, device=self.device)], -1)
        x = self.transforms[img_ids]
        d = (x[:, :, :3] @ d[:, :, None])[:, :, 0]
        d = d / torch.clamp(torch.sqrt((d * d).sum(-1, keepdim=True)), min=1e-12)
        return x[:, :, 3].contiguous(), d.contiguous()

    def next_batch(self, n_rays: int, generator: Optional[torch.Generator] = None):
        """(img_ids [n], rays_o [n,3], rays_d [n,3], rgba [n,4]) for `n_rays` uniformly drawn pixels."""
        gdev = generator.device if generator is not None else self.device
        img_ids = torch.randint(self.n_images, (n_rays,), generator=generator, device=gdev).to(self.device)
        pix = torch.randint(self.H * self.W, (n_rays,), generator=generator, device=gdev).to(self.device)
        o, d = self.rays_of(img_ids, pix)
        return img_ids, o, d, self.images.reshape(self.n_images, -1, 4)[img_ids, pix]

    def training_views(self):
        """(focal_lengths [n,2], transforms [n,3,4], (W, H)): the arguments of `DensityGridSampler.mark_untrained_density_grid`."""
        return self.focal_lengths.cpu().numpy(), self.transforms.cpu().numpy(), self.resolution

    @classmethod
    def from_blender(cls, root: str, split: str = "train", aabb_scale: Optional[int] = None, device=None) -> "NGPTrainData":
        """`transforms_<split>.json` of the NeRF synthetic format and its PNGs (RGBA)."""
        import json
        import os
        from PIL import Image
        views = ngp.NerfRays(root, mode=split, aabb_scale=aabb_scale)
        with open(os.path.join(root, f"transforms_{split}.json")) as f:
            frames = json.load(f)["frames"]
        imgs = []
        for fr in frames:
            path = os.path.join(root, fr["file_path"])
            if not os.path.exists(path):
                path += ".png"
            imgs.append(np.asarray(Image.open(path).convert("RGBA"), np.float32) / 255.0)
        images = np.stack(imgs)
        H, W = images.shape[1:3]
        scale = (W / views.W, H / views.H)                               # focal lengths given for another resolution
        data = cls(images, np.stack(views.transforms), [views.focal[0] * scale[0], views.focal[1] * scale[1]], views.principal, device=device)
        data.aabb_scale = views.aabb_scale
        return data


# ------------------------------------------------------------------------------------------------------------------ trainer
class NGPTrainer:
    """`Runner.train` (runner.py:62-86), one `step()` per iteration: a random background per ray, the target blended over it, sample (training branch),
    network, `rays2rgb`, Huber, the optimizer step on the SUM of the elementwise loss (Jittor's `optimizer.step(loss)` differentiates the sum of a non-scalar),
    the EMA step.  `mark_untrained_density_grid` runs once from the data's cameras; the sampler refreshes the occupancy grid and its ray count on its own
    schedule from `training_step`.  `network` and `composite` are the two calls a subclass may replace (the tests' torch yardstick does)."""

    def __init__(self, model: "ngp.NGPNetworks", sampler: "ngp.DensityGridSampler", data: NGPTrainData, n_rays_per_batch: Optional[int] = None,
                 huber_delta: float = 0.1, lr: float = 1e-1, eps: float = 1e-15, betas: Tuple[float, float] = (0.9, 0.99), ema_decay: float = 0.95,
                 decay_start: int = 20000, decay_interval: int = 10000, decay_base: float = 0.33, decay_end: Optional[int] = None,
                 generator: Optional[torch.Generator] = None):
        self.model, self.sampler, self.data = model, sampler, data
        model.hip_training = True
        if n_rays_per_batch is not None:
            sampler.n_rays_per_batch = int(n_rays_per_batch)
        self.huber_delta = huber_delta
        params = list(model.parameters())
        self.optimizer = NGPExpDecay(ngp_adam(params, lr, eps, betas), decay_start, decay_interval, decay_base, decay_end)
        self.ema_optimizer = NGPEma(params, ema_decay)
        self.generator = generator
        self.global_step = 0
        sampler.mark_untrained_density_grid(*data.training_views())

    def network(self, pos: torch.Tensor, dirs: torch.Tensor) -> torch.Tensor:
        return self.model(pos, dirs)

    def composite(self, net_out: torch.Tensor, bg: torch.Tensor) -> torch.Tensor:
        return self.sampler.rays2rgb(net_out, bg)

    def step(self) -> torch.Tensor:
        """One training step; returns the mean loss as a device scalar (no host read)."""
        s = self.sampler
        s.training_step = self.global_step
        img_ids, rays_o, rays_d, rgba = self.data.next_batch(s.n_rays_per_batch, self.generator)
        gdev = self.generator.device if self.generator is not None else rgba.device
        bg = torch.rand(rgba.shape[0], 3, generator=self.generator, device=gdev).to(rgba.device)
        target = (rgba[:, :3] * rgba[:, 3:] + bg * (1 - rgba[:, 3:])).detach()
        with torch.enable_grad():
            pos, dirs = s.sample(img_ids, rays_o, rays_d, is_training=True)
            rgb = self.composite(self.network(pos, dirs), bg)
            loss = huber_loss(rgb, target, self.huber_delta)
            self.optimizer.zero_grad()
            loss.sum().backward()
        self.optimizer.step()
        self.ema_optimizer.ema_step()
        self.global_step += 1
        return loss.detach().mean()

    def train(self, n_steps: int, log_every: int = 0) -> list:
        """`n_steps` steps; returns the mean loss of each (read back once, at the end)."""
        losses = []
        for i in range(n_steps):
            losses.append(self.step())
            if log_every and (i + 1) % log_every == 0:
                print(f"STEP={self.global_step} | LOSS={float(losses[-1]):.6f} | rays/batch={self.sampler.n_rays_per_batch}", flush=True)
        return [float(v) for v in torch.stack(losses).cpu()] if losses else []


def save_jnerf_checkpoint(path: str, model: "ngp.NGPNetworks", sampler: Optional["ngp.DensityGridSampler"], step: int) -> None:
    """`Runner.save_ckpt` (runner.py:127-135) as `jt.save` stores it: a pickle of `{'global_step', 'model': state_dict, 'sampler': state_dict}` with every
    array a numpy array — the file `ngp.load_jnerf_checkpoint` reads.  Optimizer states are not written."""
    import pickle

    def arr(t):
        return t.detach().cpu().numpy().copy()
    ckpt = {"global_step": int(step),
            "model": {"pos_encoder.m_grid": arr(model.pos_encoder.m_grid), "density_mlp.0.weight": arr(model.density_mlp[0].weight),
                      "density_mlp.2.weight": arr(model.density_mlp[2].weight), "rgb_mlp.0.weight": arr(model.rgb_mlp[0].weight),
                      "rgb_mlp.2.weight": arr(model.rgb_mlp[2].weight), "rgb_mlp.4.weight": arr(model.rgb_mlp[4].weight)}}
    if sampler is not None:
        ckpt["sampler"] = {k: arr(getattr(sampler, k)) for k in ("density_grid", "density_grid_bitfield", "density_grid_mean")}
    with open(path, "wb") as f:
        pickle.dump(ckpt, f, protocol=4)


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(description="Train an Instant-NGP field on a NeRF-synthetic scene and write a JNeRF-format checkpoint.")
    ap.add_argument("--data", required=True, help="scene directory holding transforms_train.json")
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--out", required=True, help="checkpoint to write (params.pkl)")
    ap.add_argument("--aabb_scale", type=int, default=None, help="overrides the value in the scene's json (default 1)")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    data = NGPTrainData.from_blender(a.data, aabb_scale=a.aabb_scale, device=a.device)
    model = ngp.NGPNetworks(data.aabb_scale).to(a.device)
    sampler = ngp.DensityGridSampler(model, data.aabb_scale).to(a.device)
    trainer = NGPTrainer(model, sampler, data)
    losses = trainer.train(a.steps, log_every=max(1, a.steps // 20))
    save_jnerf_checkpoint(a.out, model, sampler, trainer.global_step)
    print(f"{a.steps} steps, last mean loss {losses[-1] if losses else float('nan'):.6f}, wrote {a.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
