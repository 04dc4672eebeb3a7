"""TensorCP (reference tensorf-myc/models/tensoRF.py:317-447): a CP-decomposed field — three lines per factor, no planes —

    sigma_feature(p) = sum_r L0[r](p_z) L1[r](p_y) L2[r](p_x),    features(p) = basis_mat(A0[r](p_z) A1[r](p_y) A2[r](p_x))

behind TensorBase's march, MLPRender_Fea and compositing.  Constructed, loaded (our checkpoints and the reference's `.th` files), queried, masked, filtered, shrunk,
upsampled and RENDERED through the HIP path (tvr_cp_scene_create, csrc/tvr_cp.hip); up to 96 density and 288 appearance components (configs/*.txt: n_lamb_sigma = [96],
n_lamb_sh = [288]).

Training is OPT-IN: `model.cp_training = True` (reconstruct.py: --cp_training 1).  render_rays_autograd is then TensorBase's eager chain on the CP backward kernels
(csrc/tvr_cp_train.hip): tvr_cp_march_forward / _backward for the density lines (autograd_ops._CpMarchFn), tvr_app_feature / tvr_cp_app_backward for the appearance lines
and basis_mat (_CpAppFn), the network through MLPRender_Fea.forward_autograd (_LinearFn), compositing as an index_add_.  The line and basis gradients are summed with
float atomics: two runs agree to rounding, not bit for bit.  Not built for CP: the fused two-call step and its hipGraph capture, the MFMA network kernels, the reduced
arithmetics, the data-parallel helper.  With the default, cp_training = False, a CP model refuses to train exactly as before."""
from __future__ import annotations

import torch

from . import _lib as L
from .autograd_ops import _CpAppFn, _CpMarchFn, _f32c
from .field import AlphaGridMask, TensorBase

_NO_TRAINING = ("CP training is not built into the default path: TensorCP renders and answers field queries through the HIP kernels, and trains only after "
                "the opt-in `model.cp_training = True` (reconstruct.py: --cp_training 1), which routes render_rays_autograd through the CP backward kernels")


class TensorCP(TensorBase):
    """tensoRF.py:317-447."""

    _cp = True
    _ARITH = {"f32": 0}           # CP scenes compute in the default arithmetic only (include/tvr.h)

    def __init__(self, aabb, gridSize, device, **kargs):
        super().__init__(aabb, gridSize, device, **kargs)

    def init_svd_volume(self, res, device):                                                   # :322-325
        self.density_line = self.init_one_svd(self.density_n_comp[0], self.gridSize, 0.2, device)
        self.app_line = self.init_one_svd(self.app_n_comp[0], self.gridSize, 0.2, device)
        self.basis_mat = torch.nn.Linear(self.app_n_comp[0], self.app_dim, bias=False)

    def init_one_svd(self, n_component, gridSize, scale, device):                             # :328-334
        line_coef = []
        for i in range(len(self.vecMode)):
            vec_id = self.vecMode[i]
            line_coef.append(torch.nn.Parameter(scale * torch.randn((1, int(n_component), int(gridSize[vec_id]), 1))))
        return torch.nn.ParameterList(line_coef)

    def get_optparam_groups(self, lr_init_spatialxyz=0.02, lr_init_network=0.001):            # :337-343
        grad_vars = [{'params': self.density_line, 'lr': lr_init_spatialxyz}, {'params': self.app_line, 'lr': lr_init_spatialxyz},
                     {'params': self.basis_mat.parameters(), 'lr': lr_init_network}]
        grad_vars += [{'params': self.renderModule.parameters(), 'lr': lr_init_network}]
        return grad_vars

    # compute_densityfeature (:345-360) and compute_appfeature (:362-376) are TensorBase's entry points: tvr_density_feature / tvr_app_feature on the CP scene handle.

    # ---- training: opt-in -------------------------------------------------------------------------------------------------------------------------
    cp_training = False           # True: render_rays_autograd runs the CP backward kernels; False: it refuses, as it always did

    def render_rays_autograd(self, rays_chunk, white_bg=True, N_samples=-1, jitter=None):
        """TensorBase.execute with gradients (train.py:225-261) for the CP field: TensorBase.render_rays_autograd's eager chain with the CP march and feature Functions."""
        if not self.cp_training:
            raise NotImplementedError(_NO_TRAINING)
        rays = _f32c(rays_chunk, self.device)
        S = int(N_samples) if N_samples > 0 else self.nSamples
        eps_T = self.eps_T if self.eps_T is not None else float(self.rayMarch_weight_thres)
        w, acc, xyz, ray_id, depth = _CpMarchFn.apply(self, rays, jitter, S, eps_T, *self.density_line)
        features = _CpAppFn.apply(self, xyz, *self.app_line, self.basis_mat.weight)           # tensoRF.py:362-376
        rgb = self.renderModule.forward_autograd(rays[ray_id, 3:6], features)                 # tensorBase.py:517
        rgb_map = torch.zeros((rays.shape[0], 3), device=self.device).index_add_(0, ray_id, w[:, None] * rgb)   # :521
        if white_bg:
            rgb_map = rgb_map + (1.0 - acc[:, None])                                          # :524
        return rgb_map.clamp(0, 1), depth                                                     # :527

    def _get_cp_grad_scratch(self) -> torch.Tensor:
        nbytes = L.lib().tvr_cp_grad_scratch_bytes(self._ensure_scene(settle=False))
        if getattr(self, "_cp_grad_scratch", None) is None or self._cp_grad_scratch.numel() < nbytes:
            self._cp_grad_scratch = L.dev_bytes(nbytes, self.device, what="tvr_cp_grad_scratch")
        return self._cp_grad_scratch

    # ---- what a CP scene does not have -----------------------------------------------------------------------------------------------------------

    def _fused_step_ok(self) -> bool:
        return False

    def fp16_range_report(self):
        """No host-side range proof for CP: the kernels' own fp16-range check stays on."""
        return dict(proven=False, why="TensorCP: the features are not bounded on the host; the in-kernel check stays on")

    def _settle_arith(self, rays, S, white_bg, eps_T):
        if self.mlp_arith != "f32":
            raise ValueError(f"mlp_arith must be 'f32' for a TensorCP scene, got {self.mlp_arith!r}")
        self.arith_in_effect = "f32"

    # ---- grid maintenance ------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def up_sampling_Vector(self, density_line_coef, app_line_coef, res_target):               # :380-391
        F = torch.nn.functional
        for i in range(len(self.vecMode)):
            vec_id = self.vecMode[i]
            density_line_coef[i] = torch.nn.Parameter(F.interpolate(density_line_coef[i].data, size=(int(res_target[vec_id]), 1), mode='bilinear',
                                                                    align_corners=True))
            app_line_coef[i] = torch.nn.Parameter(F.interpolate(app_line_coef[i].data, size=(int(res_target[vec_id]), 1), mode='bilinear',
                                                                align_corners=True))
        return density_line_coef, app_line_coef

    @torch.no_grad()
    def upsample_volume_grid(self, res_target):                                               # :394-398
        self.density_line, self.app_line = self.up_sampling_Vector(self.density_line, self.app_line, res_target)
        self.update_stepSize(res_target)

    @torch.no_grad()
    def shrink(self, new_aabb):                                                               # :401-429
        new_aabb = torch.as_tensor(new_aabb, dtype=torch.float32).cpu()
        xyz_min, xyz_max = new_aabb
        t_l, b_r = (xyz_min - self.aabb[0]) / self.units, (xyz_max - self.aabb[0]) / self.units
        t_l, b_r = torch.round(torch.round(t_l)).long(), torch.round(b_r).long() + 1
        b_r = torch.stack([b_r, self.gridSize.long()]).amin(0)
        for i in range(len(self.vecMode)):
            mode0 = self.vecMode[i]
            self.density_line[i] = torch.nn.Parameter(self.density_line[i].data[..., int(t_l[mode0]):int(b_r[mode0]), :].contiguous())
            self.app_line[i] = torch.nn.Parameter(self.app_line[i].data[..., int(t_l[mode0]):int(b_r[mode0]), :].contiguous())
        if not torch.all(self.alphaMask.gridSize == self.gridSize):
            t_l_r, b_r_r = t_l / (self.gridSize - 1), (b_r - 1) / (self.gridSize - 1)
            correct_aabb = torch.zeros_like(new_aabb)
            correct_aabb[0] = (1 - t_l_r) * self.aabb[0] + t_l_r * self.aabb[1]
            correct_aabb[1] = (1 - b_r_r) * self.aabb[0] + b_r_r * self.aabb[1]
            new_aabb = correct_aabb
        newSize = b_r - t_l
        self.aabb = new_aabb
        self.update_stepSize((int(newSize[0]), int(newSize[1]), int(newSize[2])))

    # ---- regularisers (:431-447), plain torch on the parameters ------------------------------------------------------------------------------------
    def density_L1(self):
        total = 0
        for idx in range(len(self.density_line)):
            total = total + torch.mean(torch.abs(self.density_line[idx]))
        return total

    def TV_loss_density(self, reg):
        total = 0
        for idx in range(len(self.density_line)):
            total = total + reg(self.density_line[idx]) * 1e-3
        return total

    def TV_loss_app(self, reg):
        total = 0
        for idx in range(len(self.app_line)):
            total = total + reg(self.app_line[idx]) * 1e-3
        return total

    def load_arrays(self, arrs):
        """Copy a flat CP array dict (synthetic.make_cp_scene_arrays) into the parameters."""
        with torch.no_grad():
            for i in range(3):
                self.density_line[i].copy_(torch.as_tensor(arrs[f"density_line.{i}"]))
                self.app_line[i].copy_(torch.as_tensor(arrs[f"app_line.{i}"]))
            self.basis_mat.weight.copy_(torch.as_tensor(arrs["basis_mat"]))
            m = self.renderModule.mlp
            for idx, (w, b) in zip((0, 2, 4), (("W1", "b1"), ("W2", "b2"), ("W3", "b3"))):
                m[idx].weight.copy_(torch.as_tensor(arrs[w]))
                m[idx].bias.copy_(torch.as_tensor(arrs[b]))
        if "alpha_volume" in arrs:
            self.alphaMask = AlphaGridMask(self.device, arrs["alpha_aabb"], torch.as_tensor(arrs["alpha_volume"]))
        return self
