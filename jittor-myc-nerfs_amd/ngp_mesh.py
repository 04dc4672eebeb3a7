"""The surface of an Instant-NGP scene as a PLY mesh: `ngp.density_volume` (csrc/tvr_ngp_geom.hip) -> `mesh.marching_cubes` -> the mesh pipeline of
`TensorBase.export_mesh` (component filter, clustering, Taubin smoothing, in that order and with its defaults) -> normals from the field's analytic density
gradient (`NGPNetworks.surface_normals`) and colours from the field seen head-on -> `mesh.write_ply`.  No CPU fallback.

Coordinates.  The kernels take positions in the UNIT CUBE of the scene's aabb: u = (x_ngp - aabb_lo) / (aabb_hi - aabb_lo) with aabb = 0.5 -+ aabb_scale / 2
(`DensityGridSampler.aabb_range`).  NGP coordinates come from world (Blender / NeRF-synthetic) coordinates as `ngp.matrix_nerf2ngp` maps a camera origin:
x_ngp = cycle(x_world * NERF_SCALE + 0.5) with cycle(a, b, c) = (b, c, a).  The written vertices are WORLD coordinates (`unit_to_world`):
x_world = (uncycle(u * (aabb_hi - aabb_lo) + aabb_lo) - 0.5) / NERF_SCALE, uncycle(a, b, c) = (c, a, b).  The cycle is a rotation and the scale uniform, so triangle
orientation is kept and a normal is carried by `uncycle` alone.

Everything else a mesh can go through (`--mesh_ao`, `--mesh_check`, `--mesh_compare`, `--mesh_watertight`, `--render_mesh` of reconstruct.py) works on the written
file through `--mesh_file`; nothing of that is wired a second time here.

  python -m jittor_myc_nerfs_amd.ngp_mesh --ckpt params.pkl --out x.ply [--resolution R --density_level S --normals 1 --colors 1 --min_faces N --keep_largest K
                                           --simplify S --smooth N --aabb_scale A]
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import mesh, ngp

DEFAULT_DENSITY_LEVEL = 10.0        # sigma of the level set; the volume holds log sigma, so marching cubes runs at log(density_level)


def _cycle(x: torch.Tensor, back: bool) -> torch.Tensor:
    return x[:, [2, 0, 1]] if back else x[:, [1, 2, 0]]


def unit_to_world(u: torch.Tensor, aabb_range: Sequence[float], scale: float = ngp.NERF_SCALE) -> torch.Tensor:
    """[n,3] unit-cube positions -> world coordinates (the module docstring's convention)."""
    lo, hi = float(aabb_range[0]), float(aabb_range[1])
    return (_cycle(u * (hi - lo) + lo, back=True) - 0.5) / scale


def world_to_unit(x: torch.Tensor, aabb_range: Sequence[float], scale: float = ngp.NERF_SCALE) -> torch.Tensor:
    """The inverse of `unit_to_world`."""
    lo, hi = float(aabb_range[0]), float(aabb_range[1])
    return (_cycle(x * scale + 0.5, back=False) - lo) / (hi - lo)


def occupied_bbox(sampler: ngp.DensityGridSampler) -> Optional[Tuple[np.ndarray, np.ndarray]]:
    """(lo [3], hi [3]) in unit-cube coordinates of the tight box around the occupied cells of cascade 0, or None when no cell is occupied."""
    G = ngp.NERF_GRIDSIZE
    bits = sampler.density_grid_bitfield[:G ** 3 // 8].to(torch.int64)
    occ = torch.stack([(bits >> k) & 1 for k in range(8)], 1).reshape(-1).nonzero().reshape(-1)          # Morton indices of the set cells
    if occ.numel() == 0:
        return None
    lo, hi = [], []
    for axis in range(3):
        x = (occ >> axis) & 0x49249249
        x = (x | (x >> 2)) & 0xC30C30C3
        x = (x | (x >> 4)) & 0x0F00F00F
        x = (x | (x >> 8)) & 0xFF0000FF
        x = (x | (x >> 16)) & 0x0000FFFF
        lo.append(int(x.min()))
        hi.append(int(x.max()) + 1)
    a, b = float(sampler.aabb_range[0]), float(sampler.aabb_range[1])
    return (np.asarray(lo, np.float64) / G - a) / (b - a), (np.asarray(hi, np.float64) / G - a) / (b - a)


def export_lattice(sampler: Optional[ngp.DensityGridSampler], resolution: int, bbox=None):
    """(dims [3], origin [3], spacing [3]) of export_mesh's lattice.  `bbox` = (lo [3], hi [3]) in unit-cube coordinates; None: the tight box of the occupied
    cascade-0 cells (the unit cube without a sampler or without an occupied cell).  The voxel is the box's longest edge / (resolution - 1), the same on every axis;
    the default box is then padded by one voxel per side and every box is clipped to the unit cube."""
    resolution = int(resolution)
    if resolution < 2:
        raise ValueError(f"resolution = {resolution}: at least 2 lattice points per axis")
    pad = bbox is None
    if bbox is None:
        bbox = occupied_bbox(sampler) if sampler is not None else None
    lo, hi = (np.zeros(3), np.ones(3)) if bbox is None else (np.asarray(bbox[0], np.float64).reshape(3), np.asarray(bbox[1], np.float64).reshape(3))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise ValueError(f"bbox {lo.tolist()} .. {hi.tolist()}: needs hi > lo on every axis")
    voxel = float((hi - lo).max()) / (resolution - 1)
    if pad:
        lo, hi = lo - voxel, hi + voxel
    lo, hi = np.clip(lo, 0.0, 1.0), np.clip(hi, 0.0, 1.0)
    v32 = np.float32(voxel)
    dims = [max(2, int(math.floor(float(e) / voxel + 1e-4)) + 1) for e in (hi - lo)]
    origin = [float(np.float32(x)) for x in lo]
    # the last lattice point of an axis, fma(n - 1, voxel, origin) rounded once, must not leave the unit cube by the rounding of the voxel: a few ulps less if so
    while any(float(np.float32(float(n - 1) * float(v32) + o)) > 1.0 for n, o in zip(dims, origin)):
        v32 = np.nextafter(v32, np.float32(0))
    return dims, origin, [float(v32)] * 3


@torch.no_grad()
def export_mesh(model: ngp.NGPNetworks, sampler: Optional[ngp.DensityGridSampler], path, density_level: float = DEFAULT_DENSITY_LEVEL, resolution: int = 256, bbox=None,
                normals: bool = False, colors: bool = False, min_component_faces: int = 0, keep_largest: int = 0, simplify: float = 0, smooth: int = 0,
                aabb_range: Optional[Sequence[float]] = None, stats: Optional[dict] = None):
    """An NGP scene's surface {density == density_level} as a PLY file.  Returns (verts [V,3] in WORLD coordinates as written, faces [F,3]) on the device.

      1. `ngp.density_volume` over `export_lattice(sampler, resolution, bbox)`: the raw density, empty space skipped through the sampler's bitfield;
      2. `mesh.marching_cubes` at log(density_level) — inside is raw >= level, triangles face out of the dense side;
      3. `mesh.filter_components(min_component_faces, keep_largest)`, `mesh.simplify_clustering` (cell = simplify x the voxel, lattice corner = the lattice's
         origin; 0 = off, else >= 1), `mesh.smooth_taubin(smooth iterations, SMOOTH_LAMBDA, SMOOTH_MU, boundary pinned)`: TensorBase.export_mesh's order and defaults;
      4. normals=True: `model.surface_normals` at the final vertices (the analytic gradient; not the faces' normals);
      5. colors=True: logistic(rgb raw) of `model.forward(v, dir)` with dir the warped direction (d + 1) / 2 of d = -normal: the surface seen head-on;
      6. vertices (and normals) go to world coordinates — the module docstring's convention; `aabb_range` defaults to the sampler's, or 0.5 -+ aabb_scale / 2;
      7. `mesh.write_ply`.
    `stats` (a dict) receives dims / origin / spacing and the entries of the mesh steps."""
    if not density_level > 0 or not math.isfinite(density_level):
        raise ValueError(f"density_level = {density_level}: a finite density > 0 (the volume holds its logarithm)")
    if min_component_faces < 0 or keep_largest < 0:
        raise ValueError(f"min_component_faces = {min_component_faces} / keep_largest = {keep_largest}: negative values mean nothing (0 switches an option off)")
    simplify = float(simplify)
    if not np.isfinite(simplify) or simplify < 0 or 0 < simplify < 1:
        raise ValueError(f"simplify = {simplify}: the cluster cell's edge in marching-cubes voxels, 0 (off) or a finite value >= 1")
    if isinstance(smooth, bool) or not isinstance(smooth, (int, np.integer)) or not 0 <= int(smooth) <= mesh.SMOOTH_MAX_ITERATIONS:
        raise ValueError(f"smooth = {smooth!r}: Taubin iterations, an integer in 0 .. {mesh.SMOOTH_MAX_ITERATIONS} (0 = off)")
    if aabb_range is None:
        s = model.pos_encoder.aabb_scale
        aabb_range = sampler.aabb_range if sampler is not None else (0.5 - s / 2, 0.5 + s / 2)
    st = stats if stats is not None else {}
    dims, origin, spacing = export_lattice(sampler, resolution, bbox)
    st.update(dims=dims, origin=origin, spacing=spacing)
    vol = ngp.density_volume(model, sampler, dims=dims, origin=origin, spacing=spacing)
    verts, faces = mesh.marching_cubes(vol, math.log(density_level), spacing=spacing, origin=origin)
    del vol
    verts, faces, _ = mesh.filter_components(verts, faces, min_faces=min_component_faces, keep_largest=keep_largest, stats=st)
    if simplify:
        verts, faces, _ = mesh.simplify_clustering(verts, faces, [simplify * x for x in spacing], origin=origin, stats=st)
    if smooth:
        verts = mesh.smooth_taubin(verts, faces, int(smooth), lam=mesh.SMOOTH_LAMBDA, mu=mesh.SMOOTH_MU, pin_boundary=True, stats=st)
    n_unit = c8 = None
    if (normals or colors) and verts.shape[0]:
        n_unit = model.surface_normals(verts)
        if colors:
            rgb = torch.sigmoid(model.forward(verts, (1.0 - n_unit) * 0.5)[:, :3])
            c8 = torch.round(255.0 * rgb.clamp(0.0, 1.0)).to(torch.uint8)
    elif normals or colors:
        n_unit = torch.zeros(0, 3, device=verts.device)
        c8 = torch.zeros(0, 3, dtype=torch.uint8, device=verts.device) if colors else None
    world = unit_to_world(verts, aabb_range) if verts.shape[0] else verts
    mesh.write_ply(path, world, faces, normals=_cycle(n_unit, back=True) if normals else None, colors=c8)
    return world, faces


def _aabb_scale_of(n_params: int) -> int:
    for s in (1, 2, 4, 8, 16):
        if int(ngp.grid_levels(s)[0][-1]) * 2 == n_params:
            return s
    raise ValueError(f"pos_encoder.m_grid has {n_params} entries: not the hash grid of an aabb_scale in 1, 2, 4, 8, 16 (give --aabb_scale)")


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(description="Export the surface of an Instant-NGP checkpoint (JNeRF format) as a PLY mesh.")
    ap.add_argument("--ckpt", required=True, help="params.pkl as Runner.save_ckpt / ngp_train.save_jnerf_checkpoint write it")
    ap.add_argument("--out", required=True, help="the PLY file to write")
    ap.add_argument("--resolution", type=int, default=256, help="lattice points along the longest edge of the meshed box")
    ap.add_argument("--density_level", type=float, default=DEFAULT_DENSITY_LEVEL, help="the density sigma whose level set is meshed")
    ap.add_argument("--normals", type=int, default=0)
    ap.add_argument("--colors", type=int, default=0)
    ap.add_argument("--min_faces", type=int, default=0, help="drop connected components with fewer triangles")
    ap.add_argument("--keep_largest", type=int, default=0, help="keep only the K largest components")
    ap.add_argument("--simplify", type=float, default=0.0, help="vertex clustering: the cell's edge in voxels (0 = off)")
    ap.add_argument("--smooth", type=int, default=0, help="Taubin iterations (0 = off)")
    ap.add_argument("--aabb_scale", type=int, default=None, help="default: read off the size of the checkpoint's hash grid")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    from .field import _ArrayUnpickler
    with open(a.ckpt, "rb") as f:
        ckpt = _ArrayUnpickler.load(f)
    scale = a.aabb_scale if a.aabb_scale is not None else _aabb_scale_of(int(np.asarray(ckpt["model"]["pos_encoder.m_grid"]).size))
    model = ngp.NGPNetworks(scale).to(a.device)
    sampler = ngp.DensityGridSampler(model, scale).to(a.device)
    ngp.load_jnerf_checkpoint(a.ckpt, model, sampler)
    if "sampler" not in ckpt or "density_grid_bitfield" not in ckpt["sampler"]:
        if "sampler" in ckpt and "density_grid" in ckpt["sampler"]:
            sampler.update_bitfield()
        else:
            sampler.build_density_grid(16)                           # a checkpoint without sampler state: occupancy from the network
    st = {}
    verts, faces = export_mesh(model, sampler, a.out, density_level=a.density_level, resolution=a.resolution, normals=bool(a.normals), colors=bool(a.colors),
                               min_component_faces=a.min_faces, keep_largest=a.keep_largest, simplify=a.simplify, smooth=a.smooth, stats=st)
    print(f"lattice {st['dims']}: {verts.shape[0]} vertices, {faces.shape[0]} triangles -> {a.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
