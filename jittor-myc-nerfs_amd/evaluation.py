"""Callers and data formats either side of the render path: Blender-format datasets in, PNG + metrics out.

  * BlenderRays            — the ray side of `BlenderDataset` (tensorf-myc/dataLoader/blender.py:13-161): reads `transforms_{split}.json`,
                             builds `all_rays [n_img, H*W, 6]`, loads ground-truth PNGs when they exist (alpha blended to white, :105-108)
  * evaluation             — tensorf-myc/renderer.py:29-91: per-image render (chunk 1024), clamp, PSNR / SSIM, `*_r_{idx}.png`, `rgbd/*.png`, `mean.txt`
  * evaluation_path        — tensorf-myc/renderer.py:93-148 without the mp4 writers (imageio is not available here)
  * normal_map_to_rgb8     — (no reference counterpart) the picture of TensorBase.render_normals' output; `evaluation(..., normal_maps=True)` writes `normal/{idx:03d}.png`
  * rgb_ssim, visualize_depth_numpy — tensorf-myc/utils.py:73-119, :11-26 (the depth colour map is a numpy jet ramp standing in for cv2's LUT)
Everything here is host-side plumbing around `renderer(rays, tensorf, …)`; the rendering itself is the HIP path.
"""
from __future__ import annotations

import json
import os
from typing import List, Optional

import numpy as np
import torch

from . import rays as R


class BlenderRays:
    def __init__(self, datadir: str, split: str = "test", downsample: float = 1.0, is_stack: bool = True, N_vis: int = -1,
                 near: Optional[float] = None, far: Optional[float] = None, bbox=None, white_bg: bool = True):
        self.root_dir, self.split, self.is_stack, self.white_bg = datadir, split, is_stack, white_bg
        self.img_wh = (int(800 / downsample), int(800 / downsample))                                    # blender.py:19
        self.near_far = [5.0, 40.0] if near is None or far is None else [near, far]                     # blender.py:50-53
        self.scene_bbox = torch.tensor([[-5.0] * 3, [5.0] * 3] if bbox is None else bbox, dtype=torch.float32).view(2, 3)
        name = f"transforms_{split}.json"
        path = os.path.join(datadir, name)
        if not os.path.exists(path) and split == "test":            # data_refine/Easyship ships it as transform_test.json
            path = os.path.join(datadir, "transform_test.json")
        with open(path) as f:
            self.meta = json.load(f)
        w, h = self.img_wh
        self.camera_angle_x = float(self.meta["camera_angle_x"])
        self.focal = R.focal_from_angle(self.camera_angle_x, w)
        frames = self.meta["frames"]
        interval = 1 if N_vis < 0 else max(len(frames) // N_vis, 1)
        self.poses, rays, rgbs = [], [], []
        for fr in frames[::interval]:
            M = np.asarray(fr["transform_matrix"], dtype=np.float64)
            self.poses.append(torch.tensor(M @ R.BLENDER2OPENCV, dtype=torch.float32))
            rays.append(R.frame_rays(M, h, w, self.camera_angle_x))
            img_path = os.path.join(datadir, f"{fr['file_path']}.png")
            if os.path.exists(img_path):
                from PIL import Image
                img = Image.open(img_path)
                if img.size != (w, h):
                    img = img.resize((w, h), Image.LANCZOS)
                a = (np.asarray(img).astype(np.float32) / 255.0).reshape(h * w, -1)
                if a.shape[1] == 4:
                    a = a[:, :3] * a[:, 3:] + (1 - a[:, 3:])                                              # blender.py:108
                rgbs.append(torch.from_numpy(np.ascontiguousarray(a[:, :3])))
        self.all_rays = torch.stack(rays, 0) if is_stack else torch.cat(rays, 0)
        self.all_rgbs = (torch.stack(rgbs, 0).reshape(-1, h, w, 3) if is_stack else torch.cat(rgbs, 0)) if len(rgbs) == len(rays) else []


def rgb_ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
    """utils.py:73-119 (mip-NeRF SSIM): separable 11-tap Gaussian, 'valid' convolution, per channel."""
    import scipy.signal
    img0, img1 = np.asarray(img0, np.float64), np.asarray(img1, np.float64)
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    filt = np.exp(-0.5 * ((np.arange(filter_size) - hw + shift) / filter_sigma) ** 2)
    filt /= filt.sum()
    conv = lambda z, f: scipy.signal.convolve2d(z, f, mode="valid")
    blur = lambda z: np.stack([conv(conv(z[..., i], filt[:, None]), filt[None, :]) for i in range(z.shape[-1])], -1)
    mu0, mu1 = blur(img0), blur(img1)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    s00 = np.maximum(0.0, blur(img0 ** 2) - mu00)
    s11 = np.maximum(0.0, blur(img1 ** 2) - mu11)
    s01 = blur(img0 * img1) - mu01
    s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    return float(np.mean(((2 * mu01 + c1) * (2 * s01 + c2)) / ((mu00 + mu11 + c1) * (s00 + s11 + c2))))


def rgb_ssim_torch(img0: torch.Tensor, img1: torch.Tensor, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03) -> float:
    """`rgb_ssim` on the tensors' device: the same separable 11-tap Gaussian, 'valid' window, float64 — two depthwise conv2d calls per
    blur instead of 30 scipy convolutions per frame (0.4 s per 800x800 frame on the host, the render itself takes 23 ms)."""
    return float(_rgb_ssim_dev(img0, img1, max_val, filter_size, filter_sigma, k1, k2))


def _rgb_ssim_dev(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03) -> torch.Tensor:
    """The 0-dim result of rgb_ssim_torch, left on the device (no host synchronisation: the evaluation loop fetches it with the frame)."""
    x0 = img0.to(torch.float64).permute(2, 0, 1).unsqueeze(1)          # [3,1,H,W]: channels as a batch
    x1 = img1.to(device=x0.device, dtype=torch.float64).permute(2, 0, 1).unsqueeze(1)
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    f = torch.exp(-0.5 * ((torch.arange(filter_size, dtype=torch.float64, device=x0.device) - hw + shift) / filter_sigma) ** 2)
    f = f / f.sum()
    blur = lambda z: torch.nn.functional.conv2d(torch.nn.functional.conv2d(z, f.view(1, 1, -1, 1)), f.view(1, 1, 1, -1))
    mu0, mu1 = blur(x0), blur(x1)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    s00 = torch.clamp(blur(x0 * x0) - mu00, min=0.0)
    s11 = torch.clamp(blur(x1 * x1) - mu11, min=0.0)
    s01 = blur(x0 * x1) - mu01
    s01 = torch.sign(s01) * torch.minimum(torch.sqrt(s00 * s11), torch.abs(s01))
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    return torch.mean(((2 * mu01 + c1) * (2 * s01 + c2)) / ((mu00 + mu11 + c1) * (s00 + s11 + c2)))


class _ImageWriter:
    """PNG encoding off the render loop: a few worker threads (zlib releases the GIL); `close()` waits for the files."""

    def __init__(self, workers: int = 0):
        from concurrent.futures import ThreadPoolExecutor
        workers = workers or max(4, min(12, (os.cpu_count() or 8) // 2))
        self.pool, self.jobs = ThreadPoolExecutor(max_workers=workers), []

    def write(self, path, arr):
        self.jobs.append(self.pool.submit(_imwrite, path, arr))

    def close(self):
        for j in self.jobs:
            j.result()
        self.pool.shutdown()


_PNG_LEVEL = int(os.environ.get("TVR_PNG_LEVEL", "1"))
_LOOKAHEAD = os.environ.get("TVR_EVAL_LOOKAHEAD", "1") != "0"     # 0: finish every frame on the host before the next is enqueued (the A/B of scripts/eval_loop_timing.py)


class _FrameFetch:
    """Device -> host copies of a finished frame on a SIDE stream into pinned memory, so that the loop can enqueue frame k + 1 before it touches frame k on the host
    (round 5: a plain `.cpu()` is ordered behind everything queued on the render stream, the next frame included; the reference synchronises per 1024-ray chunk,
    renderer.py:23-25).  On a CPU device `start` is a plain conversion."""

    def __init__(self, device):
        self.cuda = torch.device(device).type == "cuda" and torch.cuda.is_available()
        self.stream = torch.cuda.Stream(device) if self.cuda else None

    def start(self, *tensors):
        if not self.cuda:
            return [t.detach().cpu().numpy() for t in tensors], None
        ready = torch.cuda.Event()
        ready.record()                                              # behind the frame's kernels (and metrics) on the render stream
        host = []
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            for t in tensors:
                h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                h.copy_(t, non_blocking=True)
                t.record_stream(self.stream)
                host.append(h)
            done = torch.cuda.Event()
            done.record(self.stream)
        return host, done

    @staticmethod
    def finish(handle):
        host, done = handle
        if done is None:
            return host
        done.synchronize()
        return [h.numpy() for h in host]


def visualize_depth_numpy(depth, minmax=None):
    """utils.py:11-26 with a numpy jet ramp instead of cv2.applyColorMap (returns BGR-ordered uint8 like cv2 does)."""
    x = np.nan_to_num(depth)
    mi, ma = (np.min(x[x > 0]) if (x > 0).any() else 0.0, np.max(x)) if minmax is None else minmax
    x = np.clip((x - mi) / (ma - mi + 1e-8), 0, 1)
    x = (255 * x).astype(np.uint8).astype(np.float32) / 255.0
    r = np.clip(1.5 - np.abs(4 * x - 3), 0, 1)
    g = np.clip(1.5 - np.abs(4 * x - 2), 0, 1)
    b = np.clip(1.5 - np.abs(4 * x - 1), 0, 1)
    return (np.stack([b, g, r], -1) * 255).astype(np.uint8), [mi, ma]


def normal_map_to_rgb8(normal: torch.Tensor, acc: torch.Tensor, white_bg: bool = True) -> torch.Tensor:
    """uint8 [..., 3] picture of a normal map (TensorBase.render_normals: normal [..., 3] = sum of weight x unit normal, acc [...] = sum of the weights):
    round(255 * clamp(0.5 * normal + 0.5 * acc + (1 - acc) * bg, 0, 1)), bg = 1 (white) or 0.  The usual 0.5 n + 0.5 colouring of a unit normal, composited over the
    background with the colour's own opacity: a ray that hits nothing shows the background, a silhouette pixel blends as the colour image does.  Pure; either device."""
    a = acc.to(torch.float32).unsqueeze(-1)
    x = 0.5 * normal.to(torch.float32) + 0.5 * a + (1.0 - a) * (1.0 if white_bg else 0.0)
    return torch.round(255.0 * x.clamp(0.0, 1.0)).to(torch.uint8)


def _normal_frame(tensorf, rays, N_samples, white_bg, H, W):
    normal, acc, _ = tensorf.render_normals(rays, N_samples=N_samples)
    return normal_map_to_rgb8(normal, acc, white_bg).reshape(H, W, 3)


def _imwrite(path, arr):
    from PIL import Image
    # compress_level 1: the same pixels (PNG is lossless), files ~ 15 % larger, encoding 3 - 4 x faster than Pillow's default 6 — the encoder, not the renderer, sets the pace of
    # an evaluation loop (scripts/eval_loop_timing.py: 48 ms per 800 x 800 frame with the default level against 20 ms of kernels)
    Image.fromarray(arr).save(path, compress_level=_PNG_LEVEL)


@torch.no_grad()
def evaluation(test_dataset, tensorf, args, renderer, savePath=None, N_vis=5, prtx='', N_samples=-1, white_bg=False, ndc_ray=False,
               compute_extra_metrics=True, device='cuda', normal_maps=False) -> List[float]:
    """normal_maps (not a reference option): with savePath, also write normal/{idx:03d}.png per frame — tensorf.render_normals on the frame's rays (not `renderer`),
    encoded by normal_map_to_rgb8."""
    PSNRs, ssims = [], []
    normal_maps = bool(normal_maps) and savePath is not None
    if savePath is not None:
        os.makedirs(savePath + "/rgbd", exist_ok=True)
    if normal_maps:
        os.makedirs(savePath + "/normal", exist_ok=True)
    near_far = test_dataset.near_far
    n = test_dataset.all_rays.shape[0]
    interval = 1 if N_vis < 0 else max(n // N_vis, 1)
    idxs = list(range(0, n, interval))
    W, H = test_dataset.img_wh
    expname = getattr(args, "expname", "render") if args is not None else "render"
    writer = _ImageWriter() if savePath is not None else None
    fetch = _FrameFetch(device)

    def finish(idx, handle, n_metrics):
        arrs = fetch.finish(handle)
        rgb, depth, metrics = arrs[0], arrs[1], arrs[2:2 + n_metrics]
        if n_metrics >= 1:
            PSNRs.append(-10.0 * np.log(float(metrics[0])) / np.log(10.0))
        if n_metrics >= 2:
            ssims.append(float(metrics[1]))
        img = (rgb * 255).astype('uint8')
        if savePath is not None:
            depth_vis, _ = visualize_depth_numpy(depth, near_far)
            writer.write(f'{savePath}/{expname}_r_{idx}.png', img)
            writer.write(f'{savePath}/rgbd/{prtx}{idx:03d}.png', np.concatenate((img, depth_vis), axis=1))
            if normal_maps:
                writer.write(f'{savePath}/normal/{prtx}{idx:03d}.png', arrs[2 + n_metrics])

    pending = None                                                   # one frame of lookahead: frame k is post-processed on the host while frame k + 1 renders
    for idx, samples in enumerate(test_dataset.all_rays[0::interval]):
        rays = samples.view(-1, samples.shape[-1]).to(device)
        rgb_map, _, depth_map, _, _ = renderer(rays, tensorf, chunk=1024, N_samples=N_samples, ndc_ray=ndc_ray, white_bg=white_bg, device=device)
        rgb_dev = rgb_map.clamp(0.0, 1.0).reshape(H, W, 3)
        metrics = []
        if len(test_dataset.all_rgbs):
            gt = test_dataset.all_rgbs[idxs[idx]].view(H, W, 3).to(rgb_dev.device)
            metrics.append(torch.mean((rgb_dev - gt) ** 2))
            if compute_extra_metrics:
                metrics.append(_rgb_ssim_dev(rgb_dev, gt, 1))                # utils.py:73-119 on the device
        extra = [_normal_frame(tensorf, rays, N_samples, white_bg, H, W)] if normal_maps else []
        handle = fetch.start(rgb_dev, depth_map.reshape(H, W), *metrics, *extra)
        if pending is not None:
            finish(*pending)
        pending = (idx, handle, len(metrics))
        if not _LOOKAHEAD:
            finish(*pending)
            pending = None
    if pending is not None:
        finish(*pending)
    if writer is not None:
        writer.close()
    if PSNRs and savePath is not None:
        vals = [np.mean(PSNRs)] + ([np.mean(ssims), 0.0, 0.0] if compute_extra_metrics else [])
        np.savetxt(f'{savePath}/{prtx}mean.txt', np.asarray(vals))
    return PSNRs


@torch.no_grad()
def evaluation_path(test_dataset, tensorf, c2ws, renderer, savePath=None, N_vis=5, prtx='', N_samples=-1, white_bg=False, ndc_ray=False,
                    compute_extra_metrics=True, device='cuda', normal_maps=False):
    """normal_maps: as in evaluation."""
    normal_maps = bool(normal_maps) and savePath is not None
    if savePath is not None:
        os.makedirs(savePath + "/rgbd", exist_ok=True)
    if normal_maps:
        os.makedirs(savePath + "/normal", exist_ok=True)
    W, H = test_dataset.img_wh
    focal = test_dataset.focal
    dirs = R.get_ray_directions(H, W, [focal, focal])
    dirs = dirs / np.sqrt((dirs * dirs).sum(-1, keepdims=True))
    frames = []
    writer = _ImageWriter() if savePath is not None else None
    fetch = _FrameFetch(device)

    def finish(idx, handle):
        arrs = fetch.finish(handle)
        rgb, depth = arrs[0], arrs[1]
        img = (rgb * 255).astype('uint8')
        frames.append(img)
        if savePath is not None:
            depth_vis, _ = visualize_depth_numpy(depth, test_dataset.near_far)
            writer.write(f'{savePath}/{prtx}{idx:03d}.png', img)
            writer.write(f'{savePath}/rgbd/{prtx}{idx:03d}.png', np.concatenate((img, depth_vis), axis=1))
            if normal_maps:
                writer.write(f'{savePath}/normal/{prtx}{idx:03d}.png', arrs[2])

    pending = None
    for idx, c2w in enumerate(c2ws):
        o, d = R.get_rays(dirs, np.asarray(c2w, dtype=np.float32))
        rays = torch.from_numpy(np.ascontiguousarray(np.concatenate([o, d], 1), dtype=np.float32)).to(device)
        rgb_map, _, depth_map, _, _ = renderer(rays, tensorf, chunk=8192, N_samples=N_samples, ndc_ray=ndc_ray, white_bg=white_bg, device=device)
        extra = [_normal_frame(tensorf, rays, N_samples, white_bg, H, W)] if normal_maps else []
        handle = fetch.start(rgb_map.clamp(0.0, 1.0).reshape(H, W, 3), depth_map.reshape(H, W), *extra)
        if pending is not None:
            finish(*pending)
        pending = (idx, handle)
        if not _LOOKAHEAD:
            finish(*pending)
            pending = None
    if pending is not None:
        finish(*pending)
    if writer is not None:
        writer.close()
    return frames


# ---- mesh views beside the rendered views (mesh.render_mesh) ------------------------------------------------------------------------------------------
def mesh_agreement(mesh_depth, mesh_hit, field_depth, field_acc, voxel) -> dict:
    """How well a mesh view (mesh.render_mesh) and a field view (TensorBase.render_normals' depth and acc) of one camera agree, in image space:
      iou               intersection over union of mesh_hit with field_acc > 0.5 (1.0 when both are empty)
      depth_median_vox  over the pixels with mesh_hit and field_acc > 0.99: median of |mesh depth - field depth| / voxel
      depth_p95_vox     their 95th percentile
      depth_pixels      how many such pixels there are (the two depth entries are NaN when there is none)
    voxel: the edge of one export voxel in world units (a number, or three whose mean is taken).  Pure; tensors on either device or arrays."""
    def host(a, dt):
        return np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=dt).reshape(-1)
    md, fd, fa = host(mesh_depth, np.float64), host(field_depth, np.float64), host(field_acc, np.float64)
    mh = host(mesh_hit, bool)
    if not (md.shape == mh.shape == fd.shape == fa.shape):
        raise ValueError(f"mesh_agreement: the four maps hold {md.size}, {mh.size}, {fd.size} and {fa.size} pixels")
    vox = float(np.mean(np.asarray(voxel, dtype=np.float64)))
    if not (np.isfinite(vox) and vox > 0):
        raise ValueError(f"voxel = {voxel!r}: a positive finite edge length")
    solid = fa > 0.5
    union = int((mh | solid).sum())
    both = mh & (fa > 0.99)
    err = np.abs(md[both] - fd[both]) / vox
    return {"iou": float((mh & solid).sum() / union) if union else 1.0,
            "depth_median_vox": float(np.median(err)) if err.size else float("nan"),
            "depth_p95_vox": float(np.percentile(err, 95)) if err.size else float("nan"),
            "depth_pixels": int(err.size)}


def mesh_color_psnr(mesh_rgb8, mesh_hit, field_rgb, field_acc):
    """PSNR in dB of a mesh view's colour (uint8 [H,W,3], mesh.mesh_view_to_rgb8) against the field's rendered colour (float [H*W,3] in 0 .. 1) over the pixels with
    mesh_hit and field_acc > 0.99: -10 log10(mean squared difference of the colours in 0 .. 1).  None when there is no such pixel, +inf for equal colours.
    Pure; tensors on either device or arrays."""
    def host(a):
        return np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    m = host(mesh_hit).astype(bool).reshape(-1) & (host(field_acc).astype(np.float64).reshape(-1) > 0.99)
    if not m.any():
        return None
    d = host(mesh_rgb8).astype(np.float64).reshape(-1, 3)[m] / 255.0 - np.clip(host(field_rgb).astype(np.float64).reshape(-1, 3)[m], 0.0, 1.0)
    mse = float(np.mean(d * d))
    return float("inf") if mse == 0 else float(-10.0 * np.log10(mse))


@torch.no_grad()
def evaluation_mesh(test_dataset, tensorf, verts, faces, savePath, normals=None, colors=None, N_vis=-1, white_bg=True, device="cuda", voxel=None, N_samples=-1,
                    texture=None, texture_layout=None, color_psnr=False):
    """Views of a mesh from the test poses, beside the rendered views: writes `{savePath}/mesh/{idx:03d}.png` per pose (H, W, focal and poses are the ones the dataset's
    rays were made from, so pixel p of the picture is ray p of the frame) and returns the per-frame mesh_agreement against tensorf.render_normals' depth and acc.

    verts [V,3] / faces [F,3]: tensors or arrays (a PLY read by mesh.read_ply_attributes).  colors [V,3] uint8 -> the colour view; else normals [V,3] -> the normal
    view; with neither a flat-shaded view from the face normals (mesh.mesh_view_to_rgb8).  voxel: the export voxel in world units (default: extent / (gridSize - 1)
    of the field, the voxel of export_mesh(spacing="samples") at the field's own grid).  The agreement means something for meshes exported with spacing="samples":
    the reference's convention shrinks the mesh by (N - 1) / N about aabb[0], and a PLY does not record which was used.
    texture [Ha,Wa,3] uint8 with texture_layout = (P, C): the per-triangle atlas of TensorBase.bake_texture (a textured OBJ read by mesh.read_obj; the layout from
    mesh.atlas_layout_from_uv) -> the colour view through mesh.sample_texture; it takes precedence over colors and normals.
    color_psnr=True adds "color_psnr" to every frame: mesh_color_psnr of the colour view (texture or vertex colours) against the field's rendered colour
    (tensorf.render_rays on the frame's rays) over the pixels with a hit and acc > 0.99; None when the view has no colours.  Off by default: the frames are then
    what they were.
    NerfPlusPlus has no normal pass: the pictures are written and None is returned.  Nothing here is called by evaluation() / evaluation_path()."""
    from . import mesh as M
    dev = torch.device(device)
    v = torch.as_tensor(np.asarray(verts) if not torch.is_tensor(verts) else verts).to(device=dev, dtype=torch.float32)
    f = torch.as_tensor(np.asarray(faces) if not torch.is_tensor(faces) else faces).to(device=dev, dtype=torch.int32)
    attr, mode, atlas = None, "normal", None
    if texture is not None:
        if texture_layout is None:
            raise ValueError("evaluation_mesh with a texture takes texture_layout = (P, C) (mesh.atlas_layout_from_uv)")
        atlas, mode = torch.as_tensor(np.asarray(texture) if not torch.is_tensor(texture) else texture).to(device=dev, dtype=torch.uint8).contiguous(), "color"
        tex_P, tex_C = (int(x) for x in texture_layout)
    elif colors is not None:
        attr, mode = torch.as_tensor(np.asarray(colors) if not torch.is_tensor(colors) else colors).to(device=dev, dtype=torch.float32), "color"
    elif normals is not None:
        attr = torch.as_tensor(np.asarray(normals) if not torch.is_tensor(normals) else normals).to(device=dev, dtype=torch.float32)
    fn = M.face_normals(v, f) if attr is None and atlas is None else None
    from .variants import NerfPlusPlus
    has_normal_pass = not isinstance(tensorf, NerfPlusPlus)               # its render_normals refuses: the samples lie at explicit depths
    if voxel is None:
        ext = (tensorf.aabb[1] - tensorf.aabb[0]).detach().cpu().numpy().astype(np.float64)
        voxel = ext / (np.asarray([int(g) for g in tensorf.gridSize], dtype=np.float64) - 1.0)
    os.makedirs(savePath + "/mesh", exist_ok=True)
    W, H = test_dataset.img_wh
    n = test_dataset.all_rays.shape[0]
    interval = 1 if N_vis < 0 else max(n // N_vis, 1)
    writer = _ImageWriter()
    out = []
    for idx, k in enumerate(range(0, n, interval)):
        depth, tri, bary, a = M.render_mesh(v, f, test_dataset.poses[k], H, W, test_dataset.focal, attributes=attr)
        if atlas is not None:
            a = M.sample_texture(tri, bary, atlas, tex_P, tex_C, f.shape[0])
        img = M.mesh_view_to_rgb8(tri, a, mode, white_bg=white_bg, face_normal=fn)
        writer.write(f"{savePath}/mesh/{idx:03d}.png", img.cpu().numpy())
        if has_normal_pass:
            rays = test_dataset.all_rays[k].view(-1, 6).to(dev)
            _, acc, fdepth = tensorf.render_normals(rays, N_samples=N_samples)
            out.append(mesh_agreement(depth, tri >= 0, fdepth, acc, voxel))
            if color_psnr:
                rgb = tensorf.render_rays(rays, white_bg=white_bg, N_samples=N_samples)[0] if mode == "color" else None
                out[-1]["color_psnr"] = None if rgb is None else mesh_color_psnr(img, tri >= 0, rgb, acc)
    writer.close()
    return out if has_normal_pass else None


def mesh_agreement_summary(frames) -> dict:
    """{"frames": [...], "mean": {...}} of evaluation_mesh's list: the mean of each entry over the frames where it is a number."""
    mean = {}
    for key in ("iou", "depth_median_vox", "depth_p95_vox", "depth_pixels"):
        vals = [fr[key] for fr in frames if np.isfinite(fr[key])]
        mean[key] = float(np.mean(vals)) if vals else float("nan")
    if any("color_psnr" in fr for fr in frames):                      # evaluation_mesh(color_psnr=True): None (null in the file) where the view has no colours
        vals = [fr["color_psnr"] for fr in frames if fr.get("color_psnr") is not None and np.isfinite(fr["color_psnr"])]
        mean["color_psnr"] = float(np.mean(vals)) if vals else None
    return {"frames": list(frames), "mean": mean}
