"""Host side of the alt path (BASELINE configs[4]): JNeRF's Instant-NGP inference surface on the HIP kernels of
csrc/tvr_ngp.hip (C-ABI: include/tvr_ngp.h).  No CPU fallback: every op raises if libtvr.so is missing or a call fails.

Mirrors, under jnerf-myc/python/jnerf/:
  HashEncoder          models/position_encoders/hash_encoder/hash_encoder.py:9-30 (+ grid_encode.py:17-39 level table)
  SHEncoder            models/position_encoders/sh_encoder/sh_encoder.py:9-53
  NGPNetworks          models/networks/ngp_network.py:41-96 (plain-Linear branch, the fp32 configs Car.py / Easyship.py)
  DensityGridSampler   models/samplers/density_grid_sampler/density_grid_sampler.py:17-267 (inference: sample / rays2rgb / bitfield; the occupancy grid
                       from the network: mark_untrained_density_grid / update_density_grid_nerf / update_density_grid, csrc/tvr_ngp_grid.hip; training, opt-in:
                       sample(is_training=True) / rays2rgb(inference=False) / update_batch_rays, csrc/tvr_ngp_train.hip — the trainer is ngp_train.py)
  render_img           runner/runner.py:195-228 (the 4096-ray slab loop) — and render_frame, the same image in one pass
  NerfRays             dataset/dataset.py:267-292,313-320 (ray generation for one camera in the NGP convention)
State-dict keys are the reference's (`pos_encoder.m_grid`, `density_mlp.0.weight`, ..., `density_grid`, `density_grid_bitfield`).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

NERF_GRIDSIZE, NERF_CASCADES, MAX_STEP = 128, 5, 1024
NERF_SCALE = 0.33                                   # dataset.py:14
_PCG_MULT = 0x5851F42D4C957F2D
_M64 = (1 << 64) - 1


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _need_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise L.TvrError(f"{what}: tensors must live on the GPU (there is no CPU fallback)")


# ------------------------------------------------------------------------------------------------------------------ RNG
class Pcg32:
    """The process-global `pcg32 rng{1337}` of the reference (ops/code_ops/global_vars.py:14-17, pcg32.h): the sampling kernel is
    handed its state and the host advances it by 2^32 after every sampling call (ray_sampler.py:61)."""

    def __init__(self, initstate: int = 1337, initseq: int = 1):
        self.state, self.inc = 0, ((initseq << 1) | 1) & _M64
        self._next()
        self.state = (self.state + initstate) & _M64
        self._next()

    def _next(self) -> int:
        old = self.state
        self.state = (old * _PCG_MULT + self.inc) & _M64
        xs = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
        rot = old >> 59
        return ((xs >> rot) | (xs << ((-rot) & 31))) & 0xFFFFFFFF

    def next_uint(self) -> int:
        return self._next()

    def advance(self, delta: int = 1 << 32) -> None:
        cur_mult, cur_plus, acc_mult, acc_plus = _PCG_MULT, self.inc, 1, 0
        delta &= _M64
        while delta > 0:
            if delta & 1:
                acc_mult = (acc_mult * cur_mult) & _M64
                acc_plus = (acc_plus * cur_mult + cur_plus) & _M64
            cur_plus = ((cur_mult + 1) * cur_plus) & _M64
            cur_mult = (cur_mult * cur_mult) & _M64
            delta >>= 1
        self.state = (acc_mult * self.state + acc_plus) & _M64


global_rng = Pcg32(1337)


# ------------------------------------------------------------------------------------------------------------------ encoders
def grid_levels(aabb_scale: int, n_levels: int = 16, base_resolution: int = 16, log2_hashmap_size: int = 19,
                desired_resolution: float = 2048.0) -> Tuple[np.ndarray, np.ndarray, float]:
    """`GridEncode.__init__` (grid_encode.py:17-39): per-level first entry and the kernel's per-level scale, in fp32 like the
    reference (`jt.exp(jt.log(..))`, `jt.pow(2, ..)`; `exp2f(level * log2_per_level_scale) * base_resolution - 1`)."""
    f32 = np.float32
    per_level_scale = float(np.exp(np.log(f32(desired_resolution * aabb_scale / base_resolution)) / f32(n_levels - 1)))
    log2s = float(np.log2(f32(per_level_scale)))
    offsets = np.zeros(n_levels + 1, np.uint32)
    scale = np.zeros(n_levels, np.float32)
    off = 0
    for i in range(n_levels):
        s = np.power(f32(2), f32(i * log2s)) * f32(base_resolution) - f32(1.0)
        res = int(np.ceil(s)) + 1
        n = min((res ** 3 + 7) // 8 * 8, 1 << log2_hashmap_size)
        offsets[i] = off
        off += n
        scale[i] = np.exp2(f32(i) * f32(np.log2(per_level_scale))) * f32(base_resolution) - f32(1.0)
    offsets[n_levels] = off
    return offsets, scale, per_level_scale


def _grid_cfg(offsets, scale) -> L.NgpGridCfg:
    g = L.NgpGridCfg()
    for i in range(17):
        g.offsets[i] = int(offsets[i])
    for i in range(16):
        g.scale[i] = float(scale[i])
    return g


class HashEncoder(torch.nn.Module):
    def __init__(self, aabb_scale: int = 1, n_pos_dims: int = 3, n_features_per_level: int = 2, n_levels: int = 16, base_resolution: int = 16,
                 log2_hashmap_size: int = 19):
        super().__init__()
        if (n_pos_dims, n_features_per_level, n_levels) != (3, 2, 16):
            raise NotImplementedError("the kernels are built for 3-D positions, 16 levels x 2 features (hash_encoder.py:18-19)")
        self.aabb_scale = aabb_scale
        self.offsets, self.scale, self.per_level_scale = grid_levels(aabb_scale, n_levels, base_resolution, log2_hashmap_size)
        self.m_n_params = int(self.offsets[-1]) * n_features_per_level
        self.m_grid = torch.nn.Parameter(torch.empty(self.m_n_params).uniform_(-1e-4, 1e-4))          # hash_encoder.py:23-24
        self.out_dim = n_features_per_level * n_levels
        self.cfg = _grid_cfg(self.offsets, self.scale)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _need_gpu(self.m_grid, "HashEncoder")
        x = x.detach().to(self.m_grid.device, torch.float32)
        if x.stride(-1) != 1:
            x = x.contiguous()
        n = x.shape[0]
        out = torch.empty(n, self.out_dim, device=x.device)
        L.check(L.lib().tvr_ngp_hash_encode(C.byref(self.cfg), self.m_grid.data_ptr(), x.data_ptr(), x.stride(0) if n else 3, n, out.data_ptr(),
                                            _stream(x.device)), "tvr_ngp_hash_encode")
        return out

    execute = forward


class SHEncoder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.m_sh_degree, self.out_dim = 4, 16

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _need_gpu(x, "SHEncoder")
        x = x.detach().to(torch.float32)
        if x.stride(-1) != 1:
            x = x.contiguous()
        n = x.shape[0]
        out = torch.empty(n, 16, device=x.device)
        L.check(L.lib().tvr_ngp_sh_encode(x.data_ptr(), x.stride(0) if n else 3, n, out.data_ptr(), _stream(x.device)), "tvr_ngp_sh_encode")
        return out

    execute = forward


class NGPNetworks(torch.nn.Module):
    """`NGPNetworks` (ngp_network.py:41-96), plain-Linear branch.  `forward(pos, dir)` is ONE fused kernel (hash grid + SH + both
    MLPs on fp32 MFMAs); the encoders stay available as separate modules, as in the reference."""

    def __init__(self, aabb_scale: int = 1, use_fully: bool = True, density_hidden_layer: int = 1, density_n_neurons: int = 64, rgb_hidden_layer: int = 2,
                 rgb_n_neurons: int = 64):
        super().__init__()
        if (density_hidden_layer, density_n_neurons, rgb_hidden_layer, rgb_n_neurons) != (1, 64, 2, 64):
            raise NotImplementedError("the fused kernel is built for the 32-64-16 / 32-64-64-3 networks (ngp_network.py:43)")
        self.use_fully, self.using_fp16 = use_fully, False
        self.pos_encoder = HashEncoder(aabb_scale)
        self.dir_encoder = SHEncoder()
        Lin = torch.nn.Linear
        self.density_mlp = torch.nn.Sequential(Lin(32, 64, bias=False), torch.nn.ReLU(), Lin(64, 16, bias=False))
        self.rgb_mlp = torch.nn.Sequential(Lin(32, 64, bias=False), torch.nn.ReLU(), Lin(64, 64, bias=False), torch.nn.ReLU(), Lin(64, 3, bias=False))
        self._packed: Optional[torch.Tensor] = None
        self._sig = None
        self.hip_training = False                                       # opt-in: forward() under grad mode builds the training graph (forward_train)

    def _weights(self):
        return [self.density_mlp[0].weight, self.density_mlp[2].weight, self.rgb_mlp[0].weight, self.rgb_mlp[2].weight, self.rgb_mlp[4].weight]

    def packed(self, force: bool = False) -> torch.Tensor:
        ws = self._weights()
        _need_gpu(ws[0], "NGPNetworks")
        sig = tuple((w.data_ptr(), w._version) for w in ws)
        if force or self._packed is None or sig != self._sig:
            dev = ws[0].device
            cs = [w.detach().to(torch.float32).contiguous() for w in ws]
            p = L.NgpNetParams(*[c.data_ptr() for c in cs])
            nbytes = L.lib().tvr_ngp_net_packed_bytes()
            if self._packed is None or self._packed.device != dev:
                self._packed = torch.empty(nbytes // 4, device=dev)
            L.check(L.lib().tvr_ngp_net_pack(C.byref(p), self._packed.data_ptr(), nbytes, _stream(dev)), "tvr_ngp_net_pack")
            self._sig = sig
        return self._packed

    def _run(self, pos: torch.Tensor, dirs: torch.Tensor, n_dev: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        grid = self.pos_encoder.m_grid
        _need_gpu(grid, "NGPNetworks")
        n = pos.shape[0]
        if out is None:
            out = torch.empty(n, 4, device=grid.device)
        if n:
            L.check(L.lib().tvr_ngp_network(C.byref(self.pos_encoder.cfg), grid.data_ptr(), self.packed().data_ptr(), pos.data_ptr(), pos.stride(0),
                                            dirs.data_ptr(), dirs.stride(0), n, None if n_dev is None else n_dev.data_ptr(), out.data_ptr(),
                                            _stream(grid.device)), "tvr_ngp_network")
        return out

    @staticmethod
    def _rows(x: torch.Tensor, device) -> torch.Tensor:
        x = x.detach().to(device, torch.float32)
        return x if (x.dim() == 2 and x.stride(1) == 1 and x.shape[1] >= 3) else x.contiguous()

    def forward(self, pos_input: torch.Tensor, dir_input: torch.Tensor) -> torch.Tensor:
        """[n,3] positions in [0,1] and directions warped to [0,1] -> [n,4] = (rgb raw, density raw) (`execute_`, ngp_network.py:78-85).
        Row-strided views (the sampler's `coords[:, :3]`, `coords[:, 4:]`) are read in place."""
        dev = self.pos_encoder.m_grid.device
        if self.hip_training and torch.is_grad_enabled():
            return self.forward_train(pos_input, dir_input)
        return self._run(self._rows(pos_input, dev), self._rows(dir_input, dev))

    def forward_train(self, pos_input: torch.Tensor, dir_input: torch.Tensor) -> torch.Tensor:
        """`execute_` under autograd, at row level: `tvr_ngp_hash_encode` (backward: `tvr_ngp_hash_encode_backward` into a zeroed buffer, the gradient of
        `m_grid`), the five bias-free Linears through `autograd_ops._LinearFn` (fp32-input MFMAs forward and dX, `tvr_gemm_tn` for the weight gradients), SH
        without a gradient.  Positions and directions are detached, as in the reference.  Returns [n,4] = (rgb raw, density raw)."""
        from .ngp_train import network_train
        dev = self.pos_encoder.m_grid.device
        return network_train(self, self._rows(pos_input, dev), self._rows(dir_input, dev))

    execute = forward

    def density(self, pos_input: torch.Tensor) -> torch.Tensor:
        """`density` (ngp_network.py:87-90): [n,3] -> [n,1]."""
        p = self._rows(pos_input, self.pos_encoder.m_grid.device)
        return self._run(p, p)[:, 3:4]

    def density_raw(self, pos_input: torch.Tensor) -> torch.Tensor:
        """[n,3] -> [n]: the raw density through the hash gather and `density_mlp` only (`tvr_ngp_density`: no SH, no colour layers) —
        bit-equal to `forward(pos, pos)[:, 3]`.  Row-strided views are read in place."""
        grid = self.pos_encoder.m_grid
        _need_gpu(grid, "NGPNetworks")
        p = self._rows(pos_input, grid.device)
        _need_gpu(p, "NGPNetworks.density_raw")
        n = p.shape[0]
        out = torch.empty(n, device=grid.device)
        if n:
            L.check(L.lib().tvr_ngp_density(C.byref(self.pos_encoder.cfg), grid.data_ptr(), self.packed().data_ptr(), p.data_ptr(), p.stride(0), n, None,
                                            out.data_ptr(), _stream(grid.device)), "tvr_ngp_density")
        return out

    def density_gradient(self, pos_input: torch.Tensor, n_dev: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """[n,3] -> (raw [n], grad [n,3]): the raw density (bit-equal to `density_raw`) and its analytic gradient with respect to the unit-cube position the
        kernels take (`tvr_ngp_density_gradient`, include/tvr_ngp.h: per hash cell a constant times a bilinear function — no smoothing, no finite difference).
        Row-strided views are read in place.  `n_dev` (uint32 [1] on the device) cuts the rows; rows behind it are left as allocated."""
        grid = self.pos_encoder.m_grid
        _need_gpu(grid, "NGPNetworks")
        p = self._rows(pos_input, grid.device)
        _need_gpu(p, "NGPNetworks.density_gradient")
        n = p.shape[0]
        raw, grad = torch.empty(n, device=grid.device), torch.empty(n, 3, device=grid.device)
        if n:
            L.check(L.lib().tvr_ngp_density_gradient(C.byref(self.pos_encoder.cfg), grid.data_ptr(), self.packed().data_ptr(), p.data_ptr(), p.stride(0), n,
                                                     None if n_dev is None else n_dev.data_ptr(), raw.data_ptr(), grad.data_ptr(), _stream(grid.device)),
                    "tvr_ngp_density_gradient")
        return raw, grad

    def surface_normals(self, pos_input: torch.Tensor) -> torch.Tensor:
        """[n,3] -> [n,3]: -grad raw / |grad raw| (out of the dense side), in the axes of the positions; exactly zero where the gradient is zero."""
        _, g = self.density_gradient(pos_input)
        norm = torch.sqrt((g * g).sum(-1, keepdim=True))
        return torch.where(norm > 0, -g / norm.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(g))

    def set_fp16(self):
        pass                                                            # fp16 = False in the shipped scene configs


# ------------------------------------------------------------------------------------------------------------------ occupancy grid from the network
N_GRID_CELLS = NERF_CASCADES * NERF_GRIDSIZE ** 3
NERF_MIN_OPTICAL_THICKNESS = 0.01


def _f3(v) -> "C.Array":
    return (C.c_float * 3)(*[float(x) for x in v])


def _box(aabb_range):
    return _f3([aabb_range[0]] * 3), _f3([aabb_range[1]] * 3)


def _grid_tensor(t: torch.Tensor, what: str, dtype=torch.float32, numel: Optional[int] = N_GRID_CELLS) -> torch.Tensor:
    _need_gpu(t, what)
    if t.dtype != dtype or not t.is_contiguous() or (numel is not None and t.numel() != numel):
        raise L.TvrError(f"{what}: expected a contiguous {dtype} tensor" + (f" of {numel} elements" if numel is not None else ""))
    return t


def grid_mark_untrained(density_grid: torch.Tensor, focal_lengths, transforms, resolution: Sequence[int]) -> None:
    """`tvr_ngp_grid_mark_untrained` in place: cells no camera sees become -1, negative cells a camera sees become 0.  `focal_lengths` [n,2],
    `transforms` [n,3,4] in the NGP convention (`matrix_nerf2ngp`), `resolution` = (W, H)."""
    g = _grid_tensor(density_grid, "grid_mark_untrained")
    f = torch.as_tensor(np.asarray(focal_lengths, np.float32).reshape(-1, 2)).to(g.device).contiguous()
    x = torch.as_tensor(np.asarray(transforms, np.float32).reshape(-1, 3, 4)).to(g.device).contiguous()
    if f.shape[0] != x.shape[0]:
        raise L.TvrError(f"grid_mark_untrained: {f.shape[0]} focal lengths for {x.shape[0]} cameras")
    L.check(L.lib().tvr_ngp_grid_mark_untrained(g.data_ptr(), x.shape[0], f.data_ptr(), x.data_ptr(), int(resolution[0]), int(resolution[1]), _stream(g.device)),
            "tvr_ngp_grid_mark_untrained")


def grid_samples(density_grid: torch.Tensor, n: int, ema_step: int, n_cascades: int, thresh: float, rng: Pcg32, aabb_range) -> Tuple[torch.Tensor, torch.Tensor]:
    """`tvr_ngp_grid_samples`: (positions [n,3] warped to the aabb, cell indices [n] as int32 holding the uint32 bits).  `rng` is read, not advanced."""
    g = _grid_tensor(density_grid, "grid_samples")
    pos = torch.empty(max(n, 0), 3, device=g.device)
    idx = torch.empty(max(n, 0), dtype=torch.int32, device=g.device)
    lo, hi = _box(aabb_range)
    L.check(L.lib().tvr_ngp_grid_samples(n, ema_step & 0xFFFFFFFF, n_cascades, thresh, rng.state, rng.inc, C.byref(lo), C.byref(hi), g.data_ptr(), pos.data_ptr(),
                                         idx.data_ptr(), _stream(g.device)), "tvr_ngp_grid_samples")
    return pos, idx


def grid_splat(indices: torch.Tensor, raw: torch.Tensor, grid_tmp: torch.Tensor) -> None:
    """`tvr_ngp_grid_splat`: grid_tmp[indices[i]] = max(., exp(raw[i]) * MIN_CONE_STEPSIZE) (atomic, on the bits)."""
    t = _grid_tensor(grid_tmp, "grid_splat")
    i = _grid_tensor(indices, "grid_splat", torch.int32, None)
    r = _grid_tensor(raw, "grid_splat", torch.float32, None)
    if i.numel() != r.numel():
        raise L.TvrError(f"grid_splat: {i.numel()} indices for {r.numel()} densities")
    L.check(L.lib().tvr_ngp_grid_splat(i.data_ptr(), r.data_ptr(), i.numel(), t.data_ptr(), _stream(t.device)), "tvr_ngp_grid_splat")


def grid_ema(grid_tmp: torch.Tensor, density_grid: torch.Tensor, decay: float) -> None:
    """`tvr_ngp_grid_ema` in place on `density_grid`."""
    t, g = _grid_tensor(grid_tmp, "grid_ema"), _grid_tensor(density_grid, "grid_ema")
    L.check(L.lib().tvr_ngp_grid_ema(t.data_ptr(), g.data_ptr(), decay, _stream(g.device)), "tvr_ngp_grid_ema")


def grid_update(model: NGPNetworks, density_grid: torch.Tensor, grid_tmp: torch.Tensor, bitfield: torch.Tensor, mean: torch.Tensor, aabb_range, n_uniform: int,
                n_nonuniform: int, ema_step: int, n_cascades: int, decay: float, rng: Pcg32) -> None:
    """`tvr_ngp_grid_update`: one whole `update_density_grid_nerf` (zero tmp, ONE kernel that draws, evaluates and splats both populations, ema, bitfield and
    mean) without a host read.  `grid_tmp` is scratch of at least 5 * 128^3 floats; `rng` is read, not advanced."""
    g = _grid_tensor(density_grid, "grid_update")
    t = _grid_tensor(grid_tmp, "grid_update", torch.float32, None)
    b = _grid_tensor(bitfield, "grid_update", torch.uint8, N_GRID_CELLS // 8)
    m = _grid_tensor(mean, "grid_update", torch.float32, None)
    hashgrid = model.pos_encoder.m_grid
    _need_gpu(hashgrid, "grid_update")
    lo, hi = _box(aabb_range)
    L.check(L.lib().tvr_ngp_grid_update(C.byref(lo), C.byref(hi), C.byref(model.pos_encoder.cfg), hashgrid.data_ptr(), model.packed().data_ptr(), g.data_ptr(),
                                        t.data_ptr(), L.nbytes(t), b.data_ptr(), m.data_ptr(), n_uniform, n_nonuniform, ema_step & 0xFFFFFFFF, n_cascades, decay,
                                        rng.state, rng.inc, _stream(g.device)), "tvr_ngp_grid_update")


# ------------------------------------------------------------------------------------------------------------------ sampler
class DensityGridSampler(torch.nn.Module):
    """`DensityGridSampler` (density_grid_sampler.py): `sample` -> `model` -> `rays2rgb(inference=True)`, the occupancy grid built and refreshed from the
    network (`update_density_grid`, `build_density_grid`), and — opt-in, for `ngp_train.NGPTrainer` — the training branch of `sample` with its row capacity
    `target_batch_size` and `rays2rgb(out, background)` under autograd.  Buffers keep the reference's names so a converted
    `ckpt['sampler']` loads with `load_state_dict`; the update's step counter and scratch are plain attributes, not buffers."""

    def __init__(self, model: NGPNetworks, aabb_scale: int = 1, n_rays_per_batch: int = 4096, near_distance: float = 0.2,
                 cone_angle_constant: float = 0.00390625, const_dt: bool = True, background_color: Sequence[float] = (1.0, 1.0, 1.0),
                 rng: Optional[Pcg32] = None, target_batch_size: int = 1 << 18):
        super().__init__()
        if aabb_scale > (1 << (NERF_CASCADES - 1)):
            raise ValueError(f"NeRF dataset's aabb_scale must <= {1 << (NERF_CASCADES - 1)}, but now is {aabb_scale}")     # :55-58
        self.__dict__["model"] = model                                  # not a sub-module (the reference reaches it through the config)
        self.aabb_scale, self.n_rays_per_batch = aabb_scale, n_rays_per_batch
        self.aabb_range = (0.5 - aabb_scale / 2, 0.5 + aabb_scale / 2)  # dataset.py:214-215
        self.near_distance, self.cone_angle_constant, self.const_dt = near_distance, cone_angle_constant, const_dt
        self.background_color = [float(c) for c in background_color]
        self.rng = rng if rng is not None else global_rng
        self.MAX_STEP = MAX_STEP
        n = NERF_CASCADES * NERF_GRIDSIZE ** 3
        self.register_buffer("density_grid", torch.zeros(n))
        self.register_buffer("density_grid_bitfield", torch.zeros(n // 8, dtype=torch.uint8))
        self.register_buffer("density_grid_mean", torch.zeros(1))
        self._coords = self._rays_numsteps = self._counter = None
        self._scratch: Optional[torch.Tensor] = None
        self.max_cascade = 0                                            # :59-61
        while (1 << self.max_cascade) < aabb_scale:
            self.max_cascade += 1
        self.density_grid_decay = 0.95                                  # :66
        self.density_grid_ema_step = 0                                  # a plain int (the reference keeps a one-element Var); not part of the state dict
        self.density_grid_tmp: Optional[torch.Tensor] = None            # allocated by the first update
        # training-time sampling (:76-78, :131): the row capacity, the step the trainer sets, and the rows seen since the last update_batch_rays
        self.target_batch_size = int(target_batch_size)
        self.max_train_samples = n_rays_per_batch * MAX_STEP            # the training branch's row buffer, fixed like the reference's (ray_sampler.py:15)
        self.update_den_freq = 16
        self.training_step = 0
        self.measured_batch_size = 0
        self._rays_numsteps_compacted = None

    # -- maintenance
    def update_bitfield(self) -> None:
        """`update_bitfield` (update_bitfield.py:14-31) from `density_grid`."""
        _need_gpu(self.density_grid, "DensityGridSampler")
        dev = self.density_grid.device
        L.check(L.lib().tvr_ngp_update_bitfield(self.density_grid.data_ptr(), self.density_grid_bitfield.data_ptr(), self.density_grid_mean.data_ptr(),
                                                None, 0, _stream(dev)), "tvr_ngp_update_bitfield")

    def mark_untrained_density_grid(self, focal_lengths, transforms, resolution: Sequence[int]) -> None:
        """`mark_untrained_density_grid` (density_grid_sampler.py:208-211): the grid is zeroed (the reference's wrapper starts from zeros), then every cell
        that no camera sees is set to -1 — such a cell is never sampled, updated or marched.  Arguments as `NerfRays.training_views()` returns them."""
        self.density_grid.zero_()
        grid_mark_untrained(self.density_grid, focal_lengths, transforms, resolution)

    def _tmp(self) -> torch.Tensor:
        dev = self.density_grid.device
        if self.density_grid_tmp is None or self.density_grid_tmp.device != dev:
            self.density_grid_tmp = L.dev_empty(N_GRID_CELLS, torch.float32, dev, what="density_grid_tmp")
        return self.density_grid_tmp

    def update_density_grid_nerf(self, decay: float, n_uniform: int, n_nonuniform: int, fused: bool = True) -> None:
        """`update_density_grid_nerf` (density_grid_sampler.py:200-247): `n_uniform` samples over every cell that is not marked untrained (thresh -0.01)
        and `n_nonuniform` over the occupied ones (thresh 0.01) go through the density network; each cell keeps the largest optical thickness
        exp(raw) * MIN_CONE_STEPSIZE it received, the grid becomes max(grid * decay, that), then bitfield and mean are refreshed.
        `fused=True` is one `tvr_ngp_grid_update`; `fused=False` runs the stand-alone calls (positions, indices and densities in memory) — the same bits.
        QUIRK kept from the reference: `decay` is accepted and ignored, the ema uses the fixed `density_grid_decay` = 0.95
        (`ema_grid_samples_nerf(..., decay=0.95)`, :108-109).  The generator is advanced by 2^32 after each of the two generate calls, also when a
        count is 0."""
        _need_gpu(self.density_grid, "DensityGridSampler")
        n_cascades, step, tmp = self.max_cascade + 1, self.density_grid_ema_step, self._tmp()
        if fused:
            grid_update(self.model, self.density_grid, tmp, self.density_grid_bitfield, self.density_grid_mean, self.aabb_range, n_uniform, n_nonuniform, step,
                        n_cascades, self.density_grid_decay, self.rng)
            self.rng.advance()
            self.rng.advance()
        else:
            tmp.zero_()
            pos_u, idx_u = grid_samples(self.density_grid, n_uniform, step, n_cascades, -0.01, self.rng, self.aabb_range)
            self.rng.advance()
            pos_n, idx_n = grid_samples(self.density_grid, n_nonuniform, step, n_cascades, NERF_MIN_OPTICAL_THICKNESS, self.rng, self.aabb_range)
            self.rng.advance()
            raw = self.model.density_raw(torch.cat([pos_u, pos_n]))
            grid_splat(torch.cat([idx_u, idx_n]), raw, tmp)
            grid_ema(tmp, self.density_grid, self.density_grid_decay)
            self.update_bitfield()
        self.density_grid_ema_step += 1

    def update_density_grid(self, training_step: int, n_training_steps: int = 40000, fused: bool = True) -> None:
        """`update_density_grid` (density_grid_sampler.py:252-259): every cell of the cascades in use once below step 256, afterwards a quarter of that
        uniformly and a quarter among the occupied cells."""
        n = NERF_GRIDSIZE ** 3 * (self.max_cascade + 1)
        alpha = self.density_grid_decay ** (n_training_steps / 16)     # computed and passed as in the reference; see update_density_grid_nerf
        if training_step < 256:
            self.update_density_grid_nerf(alpha, n, 0, fused=fused)
        else:
            self.update_density_grid_nerf(alpha, n // 4, n // 4, fused=fused)

    def build_density_grid(self, n_updates: int = 16, focal_lengths=None, transforms=None, resolution=None) -> float:
        """Occupancy for a network that came without a sampler state (or whose weights changed): the grid is zeroed — or marked, when cameras are given —
        the step counter reset, and `n_updates` updates of the early policy run.  Returns the fraction of set bits in cascade 0."""
        _need_gpu(self.density_grid, "DensityGridSampler")
        if focal_lengths is not None:
            self.mark_untrained_density_grid(focal_lengths, transforms, resolution)
        else:
            self.density_grid.zero_()
        self.density_grid_ema_step = 0
        for _ in range(n_updates):
            self.update_density_grid(0)
        if n_updates == 0:
            self.update_bitfield()
        bits0 = self.density_grid_bitfield[:NERF_GRIDSIZE ** 3 // 8].to(torch.int32)
        set_bits = sum(int(((bits0 >> k) & 1).sum()) for k in range(8))
        return set_bits / NERF_GRIDSIZE ** 3

    # -- sampling
    def _cfg(self, slab_rays: int) -> L.NgpMarchCfg:
        c = L.NgpMarchCfg()
        c.aabb_lo[:] = [self.aabb_range[0]] * 3
        c.aabb_hi[:] = [self.aabb_range[1]] * 3
        c.near_distance, c.cone_angle, c.const_dt = self.near_distance, self.cone_angle_constant, int(self.const_dt)
        c.rng_state, c.rng_inc, c.slab_rays = self.rng.state, self.rng.inc, slab_rays
        return c

    def _sample_raw(self, rays_o: torch.Tensor, rays_d: torch.Tensor, max_samples: int, slab_rays: int = 0, want_index: bool = False):
        dev = self.density_grid_bitfield.device
        _need_gpu(self.density_grid_bitfield, "DensityGridSampler")
        o = rays_o.detach().to(dev, torch.float32).contiguous()
        d = rays_d.detach().to(dev, torch.float32).contiguous()
        R = o.shape[0]
        coords = torch.empty(max_samples, 7, device=dev)
        numsteps = torch.empty(R, 2, dtype=torch.int32, device=dev)
        index = torch.empty(R, dtype=torch.int32, device=dev) if want_index else None
        counter = torch.zeros(2, dtype=torch.int32, device=dev)
        need = L.lib().tvr_ngp_sample_scratch_bytes(R)
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != dev:
            self._scratch = L.dev_bytes(need, dev, what="tvr_ngp scratch")
        cfg = self._cfg(slab_rays)
        L.check(L.lib().tvr_ngp_sample(C.byref(cfg), o.data_ptr(), d.data_ptr(), R, self.density_grid_bitfield.data_ptr(), coords.data_ptr(), max_samples,
                                       numsteps.data_ptr(), None if index is None else index.data_ptr(), counter.data_ptr(), self._scratch.data_ptr(),
                                       self._scratch.numel(), _stream(dev)), "tvr_ngp_sample")
        n_slabs = 1 if slab_rays == 0 else (R + slab_rays - 1) // slab_rays
        for _ in range(n_slabs):
            self.rng.advance()                                          # ray_sampler.py:61, once per reference call
        return coords, index, numsteps, counter

    def sample(self, img_ids, rays_o: torch.Tensor, rays_d: torch.Tensor, rgb_target=None, is_training: bool = False):
        """`sample` (density_grid_sampler.py:133-164): returns (coords_pos [n,3], coords_dir [n,3]) — views of the sampler's [n,7] rows.  Like the
        reference this reads the sample count back (`.item()`, ray_sampler.py:69).
        `is_training=True` is the training branch: the SAME sampling call (there is no training-time jitter of its own, :138-140), then the compaction to
        the row capacity `target_batch_size`.  The reference's `compacted_coord` keeps every step of every ray until the capacity is reached (its
        `T < EPSILON` break is commented out, op_header/compacted_coord.h:40-43), so the network forward it runs first (:154) feeds a loop whose result is
        unused: that forward is NOT run here.  Bases are the prefix sum in ray order, so a ray's compacted base is its sampled base and the compaction is
        the slice `coords[:min(total, cap)]` plus `steps_c = min(cap - min(cap, base), steps)` (`_rays_numsteps_compacted`); the reference's arrival-order
        atomics give another layout with the same per-ray content.  Only the used rows are returned (the reference returns all `cap` rows, zero-padded).
        Around it, as in the reference: `update_density_grid(step)` when `training_step % update_den_freq == 0`, `update_batch_rays()` when it is
        `update_den_freq - 1`; `measured_batch_size` grows by the uncapped total.
        Opt-in like the rest of training: the branch (and `rays2rgb(inference=False)`) needs `model.hip_training` set (`NGPTrainer` does it); without it the call raises, as before."""
        if is_training and not self.model.hip_training:
            raise NotImplementedError("training-time sampling is opt-in: set model.hip_training = True (ngp_train.NGPTrainer does) before sample(is_training=True)")
        if is_training and self.training_step % self.update_den_freq == 0:
            self.update_density_grid(self.training_step)
        R = rays_o.shape[0]
        # training: `update_batch_rays` may raise the ray count up to the row capacity, so the buffer keeps the size the reference fixes at construction
        # (n_rays_per_batch * MAX_STEP rows); a ray whose steps would cross it gets (0, base), as in the reference
        max_samples = min(R * self.MAX_STEP, self.max_train_samples) if is_training else R * self.MAX_STEP
        coords, index, numsteps, counter = self._sample_raw(rays_o, rays_d, max_samples, want_index=True)
        samples = int(counter[1].item())
        if is_training:
            cap = self.target_batch_size
            self.measured_batch_size += samples
            coords = coords[:min(samples, cap)]
            n, base = numsteps[:, 0], numsteps[:, 1]
            steps_c = torch.minimum(cap - torch.clamp(base, max=cap), n)
            self._rays_numsteps_compacted = torch.stack([steps_c, base], 1).contiguous()
            if self.training_step % self.update_den_freq == self.update_den_freq - 1:
                self.update_batch_rays()
        else:
            coords = coords[:samples]
        self._coords, self._rays_numsteps, self._counter, self._rays_index = coords, numsteps, counter, index
        return coords[:, :3], coords[:, 4:]

    @staticmethod
    def batch_rays(n_rays_per_batch: int, target_batch_size: int, measured_batch_size: int, update_den_freq: int = 16) -> int:
        """`update_batch_rays` (density_grid_sampler.py:262-267), the same arithmetic: rays per batch so that a batch fills the row capacity."""
        measured = max(measured_batch_size / update_den_freq, 1)
        rays_per_batch = int(n_rays_per_batch * target_batch_size / measured)
        return int(min((int(rays_per_batch) + 127) // 128 * 128, target_batch_size))

    def update_batch_rays(self) -> None:
        self.n_rays_per_batch = self.batch_rays(self.n_rays_per_batch, self.target_batch_size, self.measured_batch_size, 16)   # the reference divides by 16
        self.measured_batch_size = 0

    def rays2rgb(self, network_outputs: torch.Tensor, training_background_color=None, inference: bool = False) -> torch.Tensor:
        """`rays2rgb` (density_grid_sampler.py:163-190).  `inference=True`: `CalcRgb.inference` (calc_rgb.py:118-150).  `inference=False`: `CalcRgb.execute`
        (:35-78) under autograd over `tvr_ngp_composite_train` / `tvr_ngp_composite_backward`, on the rows of the last `sample(is_training=True)`;
        `training_background_color` is [n_rays,3]."""
        assert network_outputs.shape[0] == self._coords.shape[0]
        if not inference:
            if not self.model.hip_training:
                raise NotImplementedError("the training compositor is opt-in: set model.hip_training = True (ngp_train.NGPTrainer does)")
            from .ngp_train import composite_train
            if training_background_color is None:
                training_background_color = torch.tensor(self.background_color, device=self._coords.device).expand(self._rays_numsteps.shape[0], 3)
            return composite_train(network_outputs, self._coords, self._rays_numsteps, training_background_color)
        return self._composite(network_outputs, self._coords, self._rays_numsteps,
                               self.background_color if training_background_color is None else training_background_color)

    def _composite(self, net_out, coords, numsteps, bg) -> torch.Tensor:
        dev = numsteps.device
        R = numsteps.shape[0]
        rgb = torch.empty(R, 3, device=dev)
        o = net_out.detach().to(dev, torch.float32).contiguous()
        bgc = (C.c_float * 3)(*[float(b) for b in bg])
        L.check(L.lib().tvr_ngp_composite(o.data_ptr(), coords.data_ptr(), numsteps.data_ptr(), R, C.byref(bgc), rgb.data_ptr(), _stream(dev)), "tvr_ngp_composite")
        return rgb

    # -- one frame without the slab loop
    def render_frame(self, rays_o: torch.Tensor, rays_d: torch.Tensor, stats: Optional[dict] = None, profile: Optional[dict] = None) -> torch.Tensor:
        """The image `render_img` produces, in two launches and no host read (`tvr_ngp_render`): the march over all rays (each ray draws
        the jitter it would get in its 4096-ray slab), then one kernel that walks every ray's steps through the encoders and networks
        and composites them in order, stopping where `compute_rgbs_inference` breaks (T < 1e-4).  Nothing in between is materialised.
        `profile` (a dict) switches to the measuring entry point: per-kernel milliseconds, at the price of waiting for the frame."""
        dev = self.density_grid_bitfield.device
        _need_gpu(self.density_grid_bitfield, "DensityGridSampler")
        o = rays_o.detach().to(dev, torch.float32).contiguous()
        d = rays_d.detach().to(dev, torch.float32).contiguous()
        R = o.shape[0]
        rgb = torch.empty(R, 3, device=dev)
        need = L.lib().tvr_ngp_render_scratch_bytes(R)
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != dev:
            self._scratch = L.dev_bytes(need, dev, what="tvr_ngp scratch")
        st = torch.zeros(2, dtype=torch.int64, device=dev) if stats is not None else None
        cfg = self._cfg(self.n_rays_per_batch)
        bgc = (C.c_float * 3)(*self.background_color)
        m = self.model
        args = (C.byref(cfg), C.byref(m.pos_encoder.cfg), m.pos_encoder.m_grid.data_ptr(), m.packed().data_ptr(), o.data_ptr(), d.data_ptr(),
                R, self.density_grid_bitfield.data_ptr(), C.byref(bgc), rgb.data_ptr(), None if st is None else st.data_ptr(),
                self._scratch.data_ptr(), self._scratch.numel(), _stream(dev))
        if profile is None:
            L.check(L.lib().tvr_ngp_render(*args), "tvr_ngp_render")
        else:                                                           # HIP events around the two kernels; waits for completion
            ms = (C.c_float * 2)()
            L.check(L.lib().tvr_ngp_render_profiled(*args, C.byref(ms)), "tvr_ngp_render_profiled")
            profile.update(march_ms=float(ms[0]), render_ms=float(ms[1]))
        for _ in range((R + self.n_rays_per_batch - 1) // self.n_rays_per_batch):
            self.rng.advance()                                          # as many advances as the slab loop would make
        if stats is not None:
            ev, tot = (int(v) for v in st.tolist())
            stats.update(evaluated=ev, samples=tot)
        return rgb

    def render_frame_rows(self, rays_o: torch.Tensor, rays_d: torch.Tensor, samples_per_ray_hint: int = 256, stats: Optional[dict] = None) -> torch.Tensor:
        """The same image through the three stand-alone entry points over the whole frame (rows of every step, network outputs of every
        row, compositing): what `render_img` does without the slabs.  The only host read is the total at the end, to detect that the row
        buffer was too small (then it is re-rendered larger).  Kept as the cross-check of `render_frame` and as the bulk user of the
        row-level ABI."""
        R = rays_o.shape[0]
        state0 = (self.rng.state, self.rng.inc)
        cap = max(1, min(R * self.MAX_STEP, R * samples_per_ray_hint))
        while True:
            coords, _, numsteps, counter = self._sample_raw(rays_o, rays_d, cap, slab_rays=self.n_rays_per_batch)
            out = torch.empty(cap, 4, device=coords.device)
            self.model._run(coords[:, :3], coords[:, 4:], n_dev=counter[1:], out=out)
            rgb = self._composite(out, coords, numsteps, self.background_color)
            total = int(counter[1].item())
            if total <= cap:
                if stats is not None:
                    stats.update(samples=total, capacity=cap)
                return rgb
            del coords, out
            self.rng.state, self.rng.inc = state0                       # same jitter on the retry
            cap = min(R * self.MAX_STEP, int(total * 1.05) + 1024)


def render_img(sampler: DensityGridSampler, model: NGPNetworks, rays_o: torch.Tensor, rays_d: torch.Tensor) -> torch.Tensor:
    """`Runner.render_img` (runner.py:209-222): slabs of n_rays_per_batch rays, the last one padded with rays of ones."""
    R, B = rays_o.shape[0], sampler.n_rays_per_batch
    imgs = torch.empty(R + B, 3, device=rays_o.device)
    for pixel in range(0, R, B):
        o, d = rays_o[pixel:pixel + B], rays_d[pixel:pixel + B]
        if o.shape[0] < B:
            pad = torch.ones(B - o.shape[0], 3, dtype=o.dtype, device=o.device)
            o, d = torch.cat([o, pad]), torch.cat([d, pad])
        pos, dirs = sampler.sample(None, o, d)
        out = model(pos, dirs)
        imgs[pixel:pixel + B] = sampler.rays2rgb(out, inference=True)
    return imgs[:R]


# ------------------------------------------------------------------------------------------------------------------ the density on a lattice
DENSITY_FLOOR = -1.0e4              # what `empty_value = -inf` becomes: exp() of it is 0 in fp32 (empty space), and marching cubes can still interpolate against it


def unit_spacing(n: int) -> float:
    """The largest fp32 spacing s <= 1 / (n - 1) whose last lattice point fma(n - 1, s, 0) still lies inside [0, 1] (1 for n == 1)."""
    if n <= 1:
        return 1.0
    s = np.float32(1.0 / (n - 1))
    while float(np.float32(float(n - 1) * float(s))) > 1.0:             # the product is exact in fp64: one rounding, like the kernel's fma
        s = np.nextafter(s, np.float32(0))
    return float(s)


def density_volume(model: NGPNetworks, sampler: Optional["DensityGridSampler"] = None, resolution: Optional[int] = None, dims: Optional[Sequence[int]] = None,
                   origin: Sequence[float] = (0.0, 0.0, 0.0), spacing: Optional[Sequence[float]] = None, empty_value: float = -math.inf) -> torch.Tensor:
    """The RAW density on a lattice -> volume [nx, ny, nz] fp32 on the device, laid out as `mesh.marching_cubes` reads it (`tvr_ngp_density_grid`).  Lattice point
    (i, j, k) is the unit-cube position fma((i, j, k), spacing, origin), formed in the kernel; no point tensor exists.  `resolution` = R is short for dims (R, R, R);
    without `spacing` the lattice spans the unit cube from `origin` = 0 (`unit_spacing`).  With a `sampler`, a point whose occupancy cell (the march's lookup:
    the cascade of the position, that cascade's cell) is not set in `density_grid_bitfield` receives `empty_value` without being evaluated, and so does every point
    outside [0,1]^3; evaluated points are bit-equal to `NGPNetworks.density_raw`.  `empty_value` = -inf (the default) is stored as DENSITY_FLOOR.  The level set
    sigma = s of the density is `raw = log(s)`."""
    grid = model.pos_encoder.m_grid
    _need_gpu(grid, "density_volume")
    if (resolution is None) == (dims is None):
        raise ValueError("density_volume: give either resolution or dims")
    dims = [int(resolution)] * 3 if dims is None else [int(d) for d in dims]
    if len(dims) != 3 or not all(0 < d < (1 << 31) for d in dims):
        raise ValueError(f"density_volume: dims {dims} must be three positive int32 values")
    if spacing is None:
        spacing = [unit_spacing(d) for d in dims]
    empty = float(empty_value)
    if math.isnan(empty):
        raise ValueError("density_volume: empty_value is NaN")
    empty = DENSITY_FLOOR if empty == -math.inf else empty
    bits = None
    if sampler is not None:
        bits = sampler.density_grid_bitfield
        _need_gpu(bits, "density_volume")
    lo, hi = _box(sampler.aabb_range) if sampler is not None else (None, None)
    vol = L.dev_empty(tuple(max(d, 0) for d in dims), torch.float32, grid.device, what="density volume")
    L.check(L.lib().tvr_ngp_density_grid(C.byref(model.pos_encoder.cfg), grid.data_ptr(), model.packed().data_ptr(), None if bits is None else bits.data_ptr(),
                                         lo, hi, (C.c_int32 * 3)(*dims), _f3(origin), _f3(spacing), empty, vol.data_ptr() if vol.numel() else None,
                                         _stream(grid.device)), "tvr_ngp_density_grid")
    return vol


# ------------------------------------------------------------------------------------------------------------------ rays
def matrix_nerf2ngp(matrix, scale: float = NERF_SCALE, offset=(0.5, 0.5, 0.5), correct_pose=(-1, -1, 1)) -> np.ndarray:
    """dataset.py:313-320: Blender camera-to-world [3or4,4] -> NGP convention [3,4]."""
    m = np.array(matrix, np.float32)[:3].copy()
    for k in range(3):
        m[:, k] *= correct_pose[k]
    m[:, 3] = m[:, 3] * np.float32(scale) + np.asarray(offset, np.float32)
    return m[[1, 2, 0]]


def generate_rays(xform, W: int, H: int, focal: Sequence[float], principal=(0.5, 0.5), device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`generate_rays_total_test` (dataset.py:267-292) for one camera: rays_o, rays_d [H*W,3] fp32."""
    x = torch.as_tensor(np.asarray(xform, np.float32), device=device)
    gx = (torch.linspace(0, H - 1, H, device=device) + 0.5) / H
    gy = (torch.linspace(0, W - 1, W, device=device) + 0.5) / W
    a, b = torch.meshgrid(gx, gy, indexing="ij")
    xy = torch.stack([a, b], -1).permute(1, 0, 2).reshape(-1, 2)
    res = torch.tensor([W, H], dtype=torch.float32, device=device)
    d = torch.cat([(xy - torch.tensor(principal, dtype=torch.float32, device=device)) * res / torch.tensor(list(focal), dtype=torch.float32, device=device),
                   torch.ones(H * W, 1, device=device)], -1)
    d = (x[:, :3] @ d[:, :, None])[:, :, 0]
    d = d / torch.clamp(torch.sqrt((d * d).sum(-1, keepdim=True)), min=1e-12)
    return x[:, 3].expand_as(d).contiguous(), d.contiguous()


def fov_to_focal_length(resolution: int, degrees: float) -> float:
    return 0.5 * resolution / math.tan(0.5 * degrees * math.pi / 180)      # dataset.py:17-18


def load_scene_arrays(model: NGPNetworks, sampler: Optional[DensityGridSampler], arrs: Dict[str, np.ndarray]) -> None:
    """Fill a model / sampler from a flat dict keyed like the reference's state dicts (`synthetic.make_ngp_scene_arrays`, or a
    converted `ckpt['model']` / `ckpt['sampler']`)."""
    with torch.no_grad():
        model.pos_encoder.m_grid.copy_(torch.as_tensor(arrs["grid" if "grid" in arrs else "pos_encoder.m_grid"]).reshape(-1))
        for name, mod in (("density_mlp.0", model.density_mlp[0]), ("density_mlp.2", model.density_mlp[2]), ("rgb_mlp.0", model.rgb_mlp[0]),
                          ("rgb_mlp.2", model.rgb_mlp[2]), ("rgb_mlp.4", model.rgb_mlp[4])):
            mod.weight.copy_(torch.as_tensor(arrs[name + ".weight"]))
        model._sig = None
        if sampler is not None:
            if "density_grid" in arrs:
                sampler.density_grid.copy_(torch.as_tensor(arrs["density_grid"]))
            if "density_grid_bitfield" in arrs:
                sampler.density_grid_bitfield.copy_(torch.as_tensor(arrs["density_grid_bitfield"]))
            elif sampler.density_grid.is_cuda:
                sampler.update_bitfield()


# ------------------------------------------------------------------------------------------------------------------ formats either side
def load_jnerf_checkpoint(path: str, model: NGPNetworks, sampler: Optional[DensityGridSampler] = None) -> int:
    """`Runner.load_ckpt` (runner/runner.py:137-144) for inference: the file `Runner.save_ckpt` (:127-135) writes with `jt.save` is a pickle
    of `{'global_step', 'model': state_dict, 'sampler': state_dict, optimizer states...}` with every jt.Var turned into a numpy array
    (Jittor's published behaviour, restated; Jittor itself is absent here).  Fills `model` from `ckpt['model']` (`pos_encoder.m_grid`,
    `density_mlp.{0,2}.weight`, `rgb_mlp.{0,2,4}.weight`) and `sampler` from `ckpt['sampler']` (`density_grid`, `density_grid_bitfield`,
    `density_grid_mean`); fp16 checkpoints (`fp16 = True` configs) are widened to fp32.  Returns `global_step`."""
    from .field import _ArrayUnpickler                       # numpy arrays + builtin containers only: a downloaded checkpoint is untrusted input
    with open(path, "rb") as f:
        ckpt = _ArrayUnpickler.load(f)
    m = {k: np.asarray(v) for k, v in ckpt["model"].items()}
    # `fp16 = True` configs (ngp_comp.py:100) build the networks as FMLP (ngp_network.py:9-39): each keeps ONE flat `con_weights` =
    # concat_i(dweights[i].T.reshape(-1)) with dweights[i] of shape (in, out) and the last layer zero-padded to 16 outputs.  dweights[i].T is
    # the [out, in] matrix of the equivalent bias-free Linear; they are evaluated here in fp32 (the FMLP kernels themselves ship without
    # source, so their fp16 rounding is not reproduced).
    for prefix, shapes, names in (("density_mlp", [(64, 32), (16, 64)], ["0", "2"]), ("rgb_mlp", [(64, 32), (64, 64), (16, 64)], ["0", "2", "4"])):
        key = prefix + ".con_weights"
        if key in m and prefix + ".0.weight" not in m:
            flat, off = m[key].astype(np.float32).reshape(-1), 0
            if flat.size != sum(a * b for a, b in shapes):
                raise ValueError(f"{path}: {key} has {flat.size} entries, expected {sum(a * b for a, b in shapes)}")
            for (o, i), nm in zip(shapes, names):
                m[f"{prefix}.{nm}.weight"] = flat[off:off + o * i].reshape(o, i)
                off += o * i
            if prefix == "rgb_mlp":
                m["rgb_mlp.4.weight"] = m["rgb_mlp.4.weight"][:3]          # drop the zero padding rows
    want = {"pos_encoder.m_grid": (model.pos_encoder.m_n_params,), "density_mlp.0.weight": (64, 32), "density_mlp.2.weight": (16, 64),
            "rgb_mlp.0.weight": (64, 32), "rgb_mlp.2.weight": (64, 64), "rgb_mlp.4.weight": (3, 64)}
    for k, shape in want.items():
        if k not in m:
            raise KeyError(f"{path}: 'model' has no '{k}'")
        if tuple(m[k].shape) != shape:
            raise ValueError(f"{path}: {k} has shape {tuple(m[k].shape)}, this model (aabb_scale {model.pos_encoder.aabb_scale}) needs {shape}")
    load_scene_arrays(model, None, {k: m[k].astype(np.float32) for k in want})
    if sampler is not None and "sampler" in ckpt:
        s = {k: np.asarray(v) for k, v in ckpt["sampler"].items()}
        with torch.no_grad():
            for k in ("density_grid", "density_grid_bitfield", "density_grid_mean"):
                if k in s:
                    buf = getattr(sampler, k)
                    buf.copy_(torch.as_tensor(s[k].reshape(-1)[:buf.numel()].astype(np.uint8 if k.endswith("bitfield") else np.float32)).reshape(buf.shape))
    return int(ckpt.get("global_step", 0))


class NerfRays:
    """Test-set rays of a `NerfDataset` (dataset/dataset.py:82-228, mode 'test', `have_img=False`): `transforms_test.json` in the NeRF
    synthetic format -> NGP-convention camera matrices (`matrix_nerf2ngp`: `correct_pose`, `scale`, `offset`, axis cycle) and focal
    lengths (`fl_x` / `camera_angle_x`, :187-203); `rays(i)` is `generate_rays_total_test` for image i."""

    def __init__(self, root_dir: str, mode: str = "test", H: int = 800, W: int = 800, correct_pose=(1, -1, -1), aabb_scale: Optional[int] = None,
                 scale: Optional[float] = None, offset=None, device=None):
        import json
        import os
        with open(os.path.join(root_dir, f"transforms_{mode}.json")) as f:
            meta = json.load(f)
        self.H, self.W, self.device = int(meta.get("h", H)), int(meta.get("w", W)), device
        self.scale = NERF_SCALE if scale is None else scale
        self.offset = [0.5, 0.5, 0.5] if offset is None else offset
        self.aabb_scale = meta.get("aabb_scale", 1) if aabb_scale is None else aabb_scale
        self.aabb_range = (0.5 - self.aabb_scale / 2, 0.5 + self.aabb_scale / 2)

        def focal(res, axis):
            if "fl_" + axis in meta:
                return float(meta["fl_" + axis])
            if "camera_angle_" + axis in meta:
                return fov_to_focal_length(res, meta["camera_angle_" + axis] * 180 / math.pi)
            return 0.0
        fx, fy = focal(self.W, "x"), focal(self.H, "y")
        if fx == 0 and fy == 0:
            raise RuntimeError("Couldn't read fov.")
        self.focal = (fx or fy, fy or fx)
        self.principal = (meta.get("cx", self.W / 2) / self.W, meta.get("cy", self.H / 2) / self.H)
        self.transforms = [matrix_nerf2ngp(np.asarray(fr["transform_matrix"], np.float32), self.scale, self.offset, correct_pose) for fr in meta["frames"]]
        self.n_images = len(self.transforms)

    def rays(self, img_id: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return generate_rays(self.transforms[img_id], self.W, self.H, self.focal, self.principal, device=self.device)

    def training_views(self) -> Tuple[np.ndarray, np.ndarray, Tuple[int, int]]:
        """(focal_lengths [n,2], transforms [n,3,4] in the NGP convention, (W, H)): the arguments of `DensityGridSampler.mark_untrained_density_grid` /
        `build_density_grid` (the reference's `dataset.focal_lengths`, `dataset.transforms_gpu`, `dataset.resolution`)."""
        focal = np.tile(np.asarray(self.focal, np.float32), (self.n_images, 1))
        return focal, np.stack(self.transforms).astype(np.float32).reshape(self.n_images, 3, 4), (self.W, self.H)
