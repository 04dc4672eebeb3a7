"""The callers of the render path in the reference's own shape (tensorf-myc/train.py, tensorf-myc/opt.py): option parser for the shipped
`configs/*.txt` files, `reconstruction` (train.py:113-371) `render_test` (train.py:62-110) and `export_mesh` (train.py:41-59), on the HIP field and renderer.

    python -m jittor_myc_nerfs_amd.reconstruct --config configs/Scar.txt [--datadir ...]

What differs from the reference, on purpose:
  * the optimizer is torch.optim.Adam (fused); the per-group lr decay, the lr reset after upsampling, the regulariser schedule and the
    checkpoint contents (`kwargs`, `state_dict`, packed alpha mask, `lr`, `global_step`) are the reference's;
  * no TensorBoard writer, no `ndc_ray` datasets (the reference ships only the Blender loader); `set_nerfplusplus` is called for NerfPlusPlus only
    (train.py:172 calls it unconditionally and fails for the others);
  * `--export_mesh 1` (train.py:41-59) extracts the surface with the HIP marching cubes (mesh.py) instead of skimage and writes the PLY without plyfile; the
    level and the grid are options (`mesh_level`, `mesh_grid`), `--mesh_min_faces N` / `--mesh_keep_largest K` drop connected components (floaters), `--mesh_simplify S` merges the vertices of every cell of S voxels (vertex clustering), `--mesh_smooth N` runs N Taubin smoothing iterations, `--mesh_refine N` projects the vertices back onto the iso-surface with N Newton iterations, `--mesh_texture P` bakes a per-triangle texture atlas of P texels per patch side and writes a textured OBJ beside the PLY, `--mesh_normals 1` / `--mesh_colors 1` add per-vertex normals / colours (the reference writes bare
    geometry), `--render_mesh 1` (with `--render_only 1 --render_test 1`) draws the exported mesh from every test pose beside the rendered views and reports how well the two agree, and the command ends after the export instead of falling through into a training run;
  * progress is a plain print every `progress_refresh_rate` iterations.
Host-side plumbing only: every pixel comes from the HIP kernels through `OctreeRender_trilinear_fast`.
"""
from __future__ import annotations

import argparse
import ast
import datetime
import os
import sys
from typing import Dict, List, Optional

import numpy as np
import torch

from .evaluation import BlenderRays, evaluation, evaluation_mesh, evaluation_path, mesh_agreement_summary
from .cp import TensorCP
from .field import TensorVMSplit, load_checkpoint
from .losses import TVLoss
from .render import N_to_reso, OctreeRender_trilinear_fast, cal_n_samples
from .variants import NerfPlusPlus, REFTensoRF

MODELS = {"TensorVMSplit": TensorVMSplit, "TensorCP": TensorCP, "REFTensoRF": REFTensoRF, "NerfPlusPlus": NerfPlusPlus}
RENDER_ONLY_MODELS = ("TensorCP",)       # constructed, loaded and rendered (render_test) by default; TensorCP trains with --cp_training 1


def parse_config_file(path: str) -> Dict[str, object]:
    """The `key = value` files the reference feeds to configargparse (configs/Scar.txt): `#` comments, blank lines, `[a, b, c]` lists."""
    out: Dict[str, object] = {}
    with open(path) as f:
        for raw in f:
            line = raw.split("#", 1)[0].strip()
            if not line or "=" not in line:
                continue
            key, val = [t.strip() for t in line.split("=", 1)]
            if val.startswith("["):
                out[key] = list(ast.literal_eval(val))
            else:
                out[key] = val
    return out


def config_parser(cmd: Optional[List[str]] = None) -> argparse.Namespace:
    """tensorf-myc/opt.py:4-155 — same option names, types and defaults; `--config` values are defaults that the command line overrides."""
    p = argparse.ArgumentParser()
    p.add_argument("--config", type=str, default=None)
    for name, typ, default in (("bg_freq", int, 4), ("bg_view_freq", int, 2), ("bg_D", int, 4), ("radii", float, 20.0),
                               ("normal_vector_penalty_weight", float, 0.0), ("near", float, None), ("far", float, None), ("gc_every", int, 20),
                               ("expname", str, None), ("basedir", str, "./log"), ("add_timestamp", int, 0), ("datadir", str, "./data/llff/fern"),
                               ("progress_refresh_rate", int, 10), ("downsample_train", float, 1.0), ("downsample_test", float, 1.0),
                               ("batch_size", int, 4096), ("n_iters", int, 30000), ("lr_init", float, 0.02), ("lr_basis", float, 1e-3),
                               ("lr_decay_iters", int, -1), ("lr_decay_target_ratio", float, 0.1), ("lr_upsample_reset", int, 1),
                               ("L1_weight_inital", float, 0.0), ("L1_weight_rest", float, 0.0), ("Ortho_weight", float, 0.0),
                               ("TV_weight_density", float, 0.0), ("TV_weight_app", float, 0.0), ("data_dim_color", int, 27),
                               ("rm_weight_mask_thre", float, 1e-4), ("alpha_mask_thre", float, 1e-4), ("distance_scale", float, 25.0),
                               ("density_shift", float, -10.0), ("shadingMode", str, "MLP_PE"), ("pos_pe", int, 6), ("view_pe", int, 6),
                               ("fea_pe", int, 6), ("featureC", int, 128), ("ckpt", str, None), ("render_only", int, 0), ("render_test", int, 0),
                               ("render_train", int, 0), ("render_path", int, 0), ("export_mesh", int, 0), ("perturb", float, 1.0),
                               ("accumulate_decay", float, 0.998), ("fea2denseAct", str, "softplus"), ("ndc_ray", int, 0), ("nSamples", float, 1e6),
                               ("step_ratio", float, 0.5), ("N_voxel_init", int, 100 ** 3), ("N_voxel_final", int, 300 ** 3), ("idx_view", int, 0),
                               ("N_vis", int, 5), ("vis_every", int, 10000)):
        p.add_argument("--" + name, type=typ, default=default)
    p.add_argument("--model_name", type=str, default="TensorVMSplit", choices=["TensorVMSplit", "TensorCP", "NerfPlusPlus", "REFTensoRF"])
    # (not a reference option) arithmetic of the appearance network in the evaluation renders: field.py `mlp_arith`, include/tvr.h TVR_ARITH_*; training is fp32-class always
    p.add_argument("--mlp_arith", type=str, default="f32", choices=["f32", "f16act", "f16"])
    # (not a reference option) 1 = train a TensorCP model through the CP backward kernels (cp.TensorCP.cp_training); 0 = TensorCP only renders, as before
    p.add_argument("--cp_training", type=int, default=0)
    p.add_argument("--dataset_name", type=str, default="blender", choices=["blender", "llff", "nsvf", "dtu", "tankstemple", "own_data"])
    for name in ("with_depth", "lindisp", "white_bkgd"):
        p.add_argument("--" + name, action="store_true")
    # (not reference options) export_mesh: the iso-level train.py:59 hard-codes (its comment: 0.005 for Scarf, 0.0005 for Coffee) and an optional [nx, ny, nz] grid for the
    # dense alpha volume (default: the checkpoint's gridSize, as the reference)
    p.add_argument("--mesh_level", type=float, default=0.0005)
    # (not reference options) per-vertex normals (nx ny nz) / colours (red green blue) in the exported PLY; 0 = the reference's bare geometry
    p.add_argument("--mesh_normals", type=int, default=0)
    p.add_argument("--mesh_colors", type=int, default=0)
    # drop floaters from the mesh (mesh.filter_components): components below N triangles, then all but the K largest; 0 = off
    p.add_argument("--mesh_min_faces", type=int, default=0)
    p.add_argument("--mesh_keep_largest", type=int, default=0)
    # shrink the mesh by vertex clustering (mesh.simplify_clustering): the cluster cell's edge in marching-cubes voxels; 0 = off, 2 = about a quarter of the triangles
    p.add_argument("--mesh_simplify", type=float, default=0.0)
    # smooth the mesh (mesh.smooth_taubin, lam 0.5 / mu -0.53, boundaries pinned): Taubin iterations, after the clustering and before the attributes; 0 = off
    p.add_argument("--mesh_smooth", type=int, default=0)
    # put the vertices back on the iso-surface (TensorBase.project_to_isosurface): Newton iterations, after the smoothing and before the attributes; 0 = off
    p.add_argument("--mesh_refine", type=int, default=0)
    # texture the mesh (TensorBase.bake_texture): the patch side P in texels (5 .. 64) of a per-triangle atlas baked from the field after every other step; writes
    # <ckpt minus .th>.obj / .mtl / .png beside the PLY; 0 = off
    p.add_argument("--mesh_texture", type=int, default=0)
    # shade the mesh by ambient occlusion (mesh.build_bvh / mesh.ambient_occlusion): K directions per vertex after every geometry step, the grey round(255 * AO) written as
    # the PLY's red green blue (--render_mesh 1 then draws it as vertex colours); --mesh_ao_radius R ends the rays after R export voxels (0 = unlimited); 0 = off
    p.add_argument("--mesh_ao", type=int, default=0)
    p.add_argument("--mesh_ao_radius", type=float, default=0.0)
    # measure how far a mesh is from another (mesh.mesh_distance): REF.ply or REF.obj; with --export_mesh 1 the mesh just written is compared, without it --mesh_file
    # (no checkpoint needed); writes <mesh minus extension>_distance.json in world units and, when a --ckpt is loaded, in export voxels; unset = off
    p.add_argument("--mesh_compare", type=str, default=None)
    # with --mesh_compare: 1 = also say in which direction the meshes differ (mesh.signed_mesh_distance): per direction signed_mean (positive: outside the target)
    # and inside_fraction, and under "closedness" each target's degenerate / open / non-manifold / inconsistent counters; a target that is not closed gets null for
    # both keys and "signed_reason"; 0 = the JSON as it always was
    p.add_argument("--mesh_compare_signed", type=int, default=0)
    # make a mesh watertight (mesh.remesh_watertight): R > 0 = the 0.5 level set of the mesh's winding-number field on a lattice of R voxels along the longest edge of its
    # bounding box — one closed, outward-oriented surface whatever the input's holes, overlaps and unwelded corners; with --export_mesh 1 the mesh just written is taken,
    # without it --mesh_file (no checkpoint needed); writes <mesh minus extension>_watertight.ply and _watertight.json; --mesh_watertight_beta B is the accuracy of the
    # winding walk (>= 1, inf = exact); 0 = off
    p.add_argument("--mesh_watertight", type=int, default=0)
    p.add_argument("--mesh_watertight_beta", type=float, default=2.0)
    # say whether a mesh is usable for printing, simulation or boolean operations (mesh.mesh_check): 1 = counts, closedness counters, components and the triangle pairs
    # that cut through each other (mesh.self_intersections); with --export_mesh 1 the mesh just written is checked, without it --mesh_file (no checkpoint needed);
    # writes <mesh minus extension>_check.json, lengths in world units and, when a --ckpt is loaded, in export voxels; --mesh_check_curves 1 also writes the pairs'
    # intersection segments as <mesh minus extension>_crossings.obj (v and l records); 0 = off
    p.add_argument("--mesh_check", type=int, default=0)
    p.add_argument("--mesh_check_curves", type=int, default=0)
    # (not a reference option) normal maps beside the colour images of render_test / render_path: normal/{idx:03d}.png (TensorBase.render_normals, evaluation.normal_map_to_rgb8)
    p.add_argument("--render_normals", type=int, default=0)
    # (not a reference option) views of an exported mesh beside the rendered test views (mesh.render_mesh): with --render_only 1 --render_test 1, read --mesh_file
    # (default: <ckpt minus .th>.ply), write imgs_test_all/mesh/{idx:03d}.png per pose and imgs_test_all/mesh_agreement.json
    p.add_argument("--render_mesh", type=int, default=0,
                   help="1: also draw the exported mesh from every test pose and report how well it agrees with the rendered depth and opacity (silhouette IoU, depth "
                        "error in export voxels).  The agreement is meaningful for meshes exported with spacing='samples': the reference's voxel-size convention shrinks "
                        "the mesh by (N - 1) / N about aabb[0], and the PLY does not record which was used.")
    p.add_argument("--mesh_file", type=str, default=None, help="the PLY, or the textured OBJ of --mesh_texture, that --render_mesh 1 reads (default: <ckpt minus .th>.ply)")
    for name, typ in (("bbox", float), ("n_lamb_sigma", int), ("n_lamb_sh", int), ("upsamp_list", int), ("update_AlphaMask_list", int), ("mesh_grid", int)):
        p.add_argument("--" + name, type=typ, action="append")
    argv = sys.argv[1:] if cmd is None else list(cmd)
    pre, _ = p.parse_known_args(argv)
    if pre.config:
        cfg = parse_config_file(pre.config)
        defaults = {}
        for k, v in cfg.items():
            act = next((a for a in p._actions if a.dest == k), None)
            if act is None:
                raise SystemExit(f"{pre.config}: unknown option {k!r}")
            if isinstance(act, argparse._StoreTrueAction):
                defaults[k] = str(v).lower() in ("1", "true", "yes")
            elif isinstance(v, list):
                defaults[k] = [act.type(x) for x in v]
            else:
                defaults[k] = act.type(v) if act.type is not None else v
        p.set_defaults(**defaults)
    return p.parse_args(argv)


class SimpleSampler:
    """train.py:21-36: a fresh random permutation per epoch, consecutive batches of it.  `device`: where the permutation lives — with the training set on the
    GPU a batch's indices are then a device slice (a host permutation costs one pageable host-to-device copy per step, which waits for the stream)."""

    def __init__(self, total, batch, device=None):
        self.total, self.batch, self.curr, self.ids, self.device = total, batch, total, None, device

    def nextids(self):
        self.curr += self.batch
        if self.curr + self.batch > self.total:
            self.ids = torch.randperm(self.total, device=self.device)
            self.curr = 0
        return self.ids[self.curr:self.curr + self.batch]


def _bbox(args):
    return None if not args.bbox else [args.bbox[:3], args.bbox[3:6]]


def _build_from_ckpt(args, ckpt, device):
    kwargs = dict(ckpt["kwargs"])
    kwargs.update({"device": device})
    bg = {k: kwargs.pop(k) for k in ("bg_D", "bg_freq", "radii", "bg_view_freq") if k in kwargs}       # train.py:45-54
    tensorf = MODELS[args.model_name](**kwargs)
    if bg:
        tensorf.set_nerfplusplus(bg["bg_freq"], bg["bg_view_freq"], bg["bg_D"], bg["radii"])
    tensorf.load(ckpt)
    tensorf.mlp_arith = getattr(args, "mlp_arith", "f32")
    return tensorf, kwargs


def _normal_maps_wanted(args) -> bool:
    """--render_normals 1, refused where the model has no normal pass (NerfPlusPlus places its samples itself: TensorBase.render_normals)."""
    if not getattr(args, "render_normals", 0):
        return False
    if args.model_name == "NerfPlusPlus":
        raise NotImplementedError("--render_normals 1: normal maps are not built for NerfPlusPlus (its samples lie at explicit depths; the normal pass marches uniform steps)")
    return True


@torch.no_grad()
def render_test(args, device="cuda"):
    """train.py:62-110."""
    if args.dataset_name != "blender":
        raise NotImplementedError("only the Blender loader exists in the reference (dataLoader/__init__.py)")
    test_dataset = BlenderRays(args.datadir, split="test", downsample=args.downsample_train, is_stack=True, bbox=_bbox(args), near=args.near,
                               far=args.far, white_bg=args.white_bkgd)
    if not args.ckpt or not os.path.exists(args.ckpt):
        print("the ckpt path does not exists!!")
        return None
    tensorf, _ = _build_from_ckpt(args, load_checkpoint(args.ckpt), device)
    normal_maps = _normal_maps_wanted(args)
    logfolder = os.path.dirname(args.ckpt)
    out = {}
    if args.render_test:
        out["test"] = evaluation(test_dataset, tensorf, args, OctreeRender_trilinear_fast, f"{logfolder}/imgs_test_all/", N_vis=-1, N_samples=-1,
                                 white_bg=test_dataset.white_bg, ndc_ray=args.ndc_ray, device=device, normal_maps=normal_maps)
        print(f"======> {args.expname} test all psnr: {np.mean(out['test'])} <========================")
        if getattr(args, "render_mesh", 0):
            out["mesh"] = render_mesh_views(args, test_dataset, tensorf, f"{logfolder}/imgs_test_all/", device)
    if args.render_path:
        out["path"] = evaluation_path(test_dataset, tensorf, [p.numpy() for p in test_dataset.poses], OctreeRender_trilinear_fast,
                                      f"{logfolder}/imgs_path_all/", N_vis=-1, N_samples=-1, white_bg=test_dataset.white_bg, ndc_ray=args.ndc_ray,
                                      device=device, normal_maps=normal_maps)
    return out


def mesh_export_voxel(tensorf, mesh_grid=None):
    """The export voxel [3] in world units that --render_mesh measures depth differences in: extent / (N - 1), N = --mesh_grid when given (the grid the PLY was exported
    on), else the field's own gridSize — export_mesh's default grid.  A PLY does not record its grid: the value used goes into mesh_agreement.json."""
    grid = [int(g) for g in (mesh_grid if mesh_grid else tensorf.gridSize)]
    if len(grid) != 3 or min(grid) < 2:
        raise ValueError(f"mesh_grid takes three sizes [nx, ny, nz] of at least 2; got {grid}")
    ext = (tensorf.aabb[1] - tensorf.aabb[0]).detach().cpu().numpy().astype(np.float64)
    return ext / (np.asarray(grid, dtype=np.float64) - 1.0)


def render_mesh_views(args, test_dataset, tensorf, savePath, device="cuda"):
    """--render_mesh 1: the PLY (--mesh_file, default <ckpt minus .th>.ply) drawn from every test pose into {savePath}/mesh/, and {savePath}/mesh_agreement.json with
    evaluation.mesh_agreement per frame and its mean (no agreement for NerfPlusPlus, which has no normal pass: the file then says so).  A --mesh_file that ends in
    .obj is the textured mesh of --mesh_texture: it is read with its PNG (mesh.read_obj) and drawn through mesh.sample_texture.  Every frame and the mean carry
    color_psnr, the PSNR of the mesh view's colour against the field's rendered colour over the pixels with a hit and acc > 0.99 — for a textured OBJ and for a PLY with
    vertex colours alike, so the two can be compared; null without colours or for NerfPlusPlus."""
    import json
    from .mesh import atlas_layout_from_uv, read_obj, read_ply_attributes, read_texture_png
    path = getattr(args, "mesh_file", None) or f"{args.ckpt[:-3]}.ply"
    if not os.path.exists(path):
        raise FileNotFoundError(f"--render_mesh 1 needs a mesh: {path!r} does not exist (write it with --export_mesh 1, or name one with --mesh_file)")
    kw = {}
    if path.endswith(".obj"):
        verts, faces, uv, png = read_obj(path)
        atlas = read_texture_png(png)
        kw = dict(texture=atlas, texture_layout=atlas_layout_from_uv(uv, atlas.shape[0], atlas.shape[1]))
    else:
        verts, faces, attrs = read_ply_attributes(path)
        kw = dict(normals=attrs.get("normals"), colors=attrs.get("colors"))
    voxel = mesh_export_voxel(tensorf, getattr(args, "mesh_grid", None))
    frames = evaluation_mesh(test_dataset, tensorf, verts, faces, savePath.rstrip("/"), N_vis=-1, white_bg=test_dataset.white_bg, device=device, voxel=voxel,
                             color_psnr=True, **kw)
    report = {"mesh_file": path, "voxel": [float(x) for x in voxel],
              "voxel_from": "--mesh_grid" if getattr(args, "mesh_grid", None) else "the field's gridSize (pass the export's --mesh_grid if it was made on another grid)",
              "note": "meaningful for meshes exported with spacing='samples' (the reference convention shrinks the mesh by (N - 1) / N about aabb[0])"}
    report.update(mesh_agreement_summary(frames) if frames is not None else {"frames": None, "mean": None, "color_psnr": None})
    with open(os.path.join(savePath, "mesh_agreement.json"), "w") as fjson:
        json.dump(report, fjson, indent=1)
    if frames:
        m = report["mean"]
        print(f"mesh views of {path}: silhouette IoU {m['iou']:.4f}, depth error median {m['depth_median_vox']:.3f} / 95 % {m['depth_p95_vox']:.3f} export voxels")
        if m.get("color_psnr") is not None:
            print(f"mesh views of {path}: colour against the rendered views, PSNR {m['color_psnr']:.2f} dB")
    return report


@torch.no_grad()
def export_mesh(args, device="cuda"):
    """train.py:41-59: the checkpoint's field -> getDenseAlpha -> iso-surface at `mesh_level` -> `<ckpt minus .th>.ply` (TensorBase.export_mesh: the reference's
    voxel-size convention, utils.py:166-179).  Returns the path written.
    Departure from the reference: train.py:402-409 calls export_mesh and then FALLS THROUGH into render_test or a full reconstruction; here main() returns after the
    export unless `--render_only 1` with a render flag asks for the renders as well."""
    if not args.ckpt or not os.path.exists(args.ckpt):
        raise FileNotFoundError(f"export_mesh needs a checkpoint: --ckpt {args.ckpt!r} does not exist")
    grid = list(args.mesh_grid) if getattr(args, "mesh_grid", None) else None
    if grid is not None and len(grid) != 3:
        raise ValueError(f"mesh_grid takes three sizes [nx, ny, nz]; got {grid}")
    tensorf, _ = _build_from_ckpt(args, load_checkpoint(args.ckpt), device)
    path = f"{args.ckpt[:-3]}.ply"
    verts, faces = tensorf.export_mesh(path, level=getattr(args, "mesh_level", 0.0005), gridSize=grid, normals=bool(getattr(args, "mesh_normals", 0)),
                                       colors=bool(getattr(args, "mesh_colors", 0)), min_component_faces=int(getattr(args, "mesh_min_faces", 0)),
                                       keep_largest=int(getattr(args, "mesh_keep_largest", 0)), simplify=float(getattr(args, "mesh_simplify", 0.0)),
                                       smooth=int(getattr(args, "mesh_smooth", 0)), refine=int(getattr(args, "mesh_refine", 0)),
                                       **({"texture": int(args.mesh_texture)} if getattr(args, "mesh_texture", 0) else {}),
                                       **({"ao": int(args.mesh_ao), "ao_radius": float(args.mesh_ao_radius) if getattr(args, "mesh_ao_radius", 0.0) else None}
                                          if getattr(args, "mesh_ao", 0) else {}))
    st = getattr(tensorf, "mesh_export_stats", None) or {}
    dropped = f"; dropped {st['components'] - st['components_kept']} of {st['components']} components, {st['triangles_dropped']} triangles" if "components" in st else ""
    merged = f"; simplified from {st['vertices_in']} vertices, {st['triangles_in']} triangles" if "triangles_in" in st else ""
    smoothed = f"; smoothed {st['smooth_iterations']} iterations, {st['boundary_edges']} boundary / {st['nonmanifold_edges']} non-manifold edges" \
        if "smooth_iterations" in st else ""
    refined = f"; refined {st['refine_iterations']} iterations, {st['refine_converged']} vertices converged, median |residual| " \
        f"{st['refine_residual_median_before']:.3g} -> {st['refine_residual_median_after']:.3g}" if "refine_iterations" in st else ""
    textured = f"; textured at {st['atlas_patch']} texels per patch side, atlas {st['atlas_width']} x {st['atlas_height']} in {path[:-4]}.obj / .mtl / .png" \
        if "atlas_patch" in st else ""
    shaded = f"; ambient occlusion from {st['ao_directions']} directions, mean openness {st['ao_mean']:.3f}" if st.get("ao_mean") is not None else ""
    print(f"saving mesh to {path} ({verts.shape[0]} vertices, {faces.shape[0]} triangles{dropped}{merged}{smoothed}{refined}{textured}{shaded})")
    return path


def _read_mesh_geometry(path):
    """(verts [V,3] float32, faces [F,3] int32) of a PLY that write_ply wrote or of the OBJ of --mesh_texture (its texture is not read)."""
    from .mesh import read_ply_attributes
    if not os.path.exists(path):
        raise FileNotFoundError(f"--mesh_compare: {path!r} does not exist")
    if path.endswith(".obj"):
        verts, faces = [], []
        with open(path) as f:
            for line in f:
                tok = line.split()
                if tok[:1] == ["v"]:
                    verts.append([float(x) for x in tok[1:4]])
                elif tok[:1] == ["f"]:
                    if len(tok) != 4:
                        raise ValueError(f"{path}: a face is not a triangle")
                    faces.append([int(c.split("/")[0]) - 1 for c in tok[1:4]])
        return np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    return read_ply_attributes(path)[:2]


@torch.no_grad()
def mesh_compare(args, path, device="cuda"):
    """--mesh_compare REF: mesh.mesh_distance of the mesh at `path` (A) against REF (B), written to <path minus extension>_distance.json — the figures in world units,
    both file names and the vertex and triangle counts; with a --ckpt also the same figures in export voxels, the unit being the smallest edge of
    mesh_export_voxel(tensorf, --mesh_grid), which the file records (a mesh file does not say on which grid it was made).  Returns the path of the JSON."""
    import json
    from .mesh import CLOSEDNESS_COUNTERS, build_bvh, mesh_distance, signed_mesh_distance
    ref = args.mesh_compare
    va, fa = _read_mesh_geometry(path)
    vb, fb = _read_mesh_geometry(ref)
    ta, tfa, tb, tfb = (torch.from_numpy(np.ascontiguousarray(x)).to(device) for x in (va, fa, vb, fb))
    bvh_a, bvh_b = build_bvh(ta, tfa), build_bvh(tb, tfb)
    signed, st = bool(getattr(args, "mesh_compare_signed", 0)), {}
    distance = signed_mesh_distance if signed else mesh_distance
    report = {"mesh_file": path, "reference_file": ref, "vertices": int(len(va)), "triangles": int(len(fa)), "reference_vertices": int(len(vb)),
              "reference_triangles": int(len(fb)), "a_is": "mesh_file", "b_is": "reference_file", "subdiv": 2,
              "world": distance(ta, tfa, tb, tfb, bvh_a=bvh_a, bvh_b=bvh_b, stats=st)}
    if signed:                                                       # per direction the TARGET's counters: a_to_b is measured against the reference
        report["closedness"] = {side: {k: c[k] for k in CLOSEDNESS_COUNTERS + ("closed",)} for side, c in st["closedness"].items()}
    if args.ckpt and os.path.exists(args.ckpt):
        tensorf, _ = _build_from_ckpt(args, load_checkpoint(args.ckpt), device)
        voxel = mesh_export_voxel(tensorf, getattr(args, "mesh_grid", None))
        report["voxel"] = [float(x) for x in voxel]
        report["voxel_unit"] = float(voxel.min())
        report["voxel_from"] = "--mesh_grid" if getattr(args, "mesh_grid", None) else "the field's gridSize (pass the export's --mesh_grid if it was made on another grid)"
        report["voxels"] = distance(ta, tfa, tb, tfb, unit=float(voxel.min()), bvh_a=bvh_a, bvh_b=bvh_b)
    out = os.path.splitext(path)[0] + "_distance.json"
    with open(out, "w") as fjson:
        json.dump(report, fjson, indent=1)
    w = report["world"]
    print(f"distance of {path} to {ref}: hausdorff {w['hausdorff']:.6g}, chamfer {w['chamfer']:.6g}, to the reference mean {w['a_to_b']['mean']:.6g} / 95 % "
          f"{w['a_to_b']['p95']:.6g} (world units)" + (f"; hausdorff {report['voxels']['hausdorff']:.3f} export voxels" if "voxels" in report else ""))
    if signed:
        for side in ("a_to_b", "b_to_a"):
            x = w[side]
            print(f"  {side}: " + (x["signed_reason"] if x["signed_mean"] is None else f"signed mean {x['signed_mean']:.6g}, inside fraction {x['inside_fraction']:.4f}"))
    return out


@torch.no_grad()
def mesh_watertight(args, path, device="cuda"):
    """--mesh_watertight R: mesh.remesh_watertight of the mesh at `path` on R voxels along its longest box edge -> <path minus extension>_watertight.ply, and
    <path minus extension>_watertight.json with the lattice (dims, voxel, origin), the closedness counters of the input and of the result, the result's component
    count and mesh.mesh_distance of the result (A) against the input (B) in world units and in voxels of the remesh.  Returns the path of the JSON."""
    import json
    from .mesh import mesh_distance, remesh_watertight, write_ply
    v, f = _read_mesh_geometry(path)
    tv, tf = (torch.from_numpy(np.ascontiguousarray(x)).to(device) for x in (v, f))
    st = {}
    ov, of = remesh_watertight(tv, tf, resolution=int(args.mesh_watertight), beta=float(args.mesh_watertight_beta), stats=st)
    base = os.path.splitext(path)[0]
    write_ply(base + "_watertight.ply", ov, of)
    report = {"mesh_file": path, "watertight_file": base + "_watertight.ply", "vertices": int(len(v)), "triangles": int(len(f)), "watertight_vertices": int(ov.shape[0]),
              "watertight_triangles": int(of.shape[0]), "resolution": int(args.mesh_watertight), "beta": float(args.mesh_watertight_beta), "level": 0.5, **st,
              "a_is": "watertight_file", "b_is": "mesh_file", "subdiv": 2}
    if int(of.shape[0]):
        report["world"] = mesh_distance(ov, of, tv, tf)
        report["voxels"] = mesh_distance(ov, of, tv, tf, unit=st["voxel"])
    out = base + "_watertight.json"
    with open(out, "w") as fjson:
        json.dump(report, fjson, indent=1)
    print(f"watertight remesh of {path}: {report['watertight_triangles']} triangles on {st['dims']} grid points, voxel {st['voxel']:.6g}, "
          f"{st['components']} component(s), closed: {st['result']['closed']} (the input: {st['input']['closed']})"
          + (f"; hausdorff to the input {report['voxels']['hausdorff']:.3f} voxels" if "voxels" in report else ""))
    return out


@torch.no_grad()
def mesh_check_report(args, path, device="cuda"):
    """--mesh_check 1: mesh.mesh_check of the mesh at `path`, written to <path minus extension>_check.json — the file name, the counts, the closedness counters, the
    component count and the crossings (pairs, triangles involved, the summed length of the intersection segments, the histogram of n_pierce); crossing_length is in world
    units; with a --ckpt also crossing_length_voxels, the unit being the smallest edge of mesh_export_voxel(tensorf, --mesh_grid), which the file records as
    _distance.json does.  --mesh_check_curves 1 also writes <path minus extension>_crossings.obj.  Returns the path of the JSON."""
    import json
    from .mesh import build_bvh, mesh_check, self_intersections, write_obj_segments
    v, f = _read_mesh_geometry(path)
    tv, tf = (torch.from_numpy(np.ascontiguousarray(x)).to(device) for x in (v, f))
    bvh = build_bvh(tv, tf)
    report = {"mesh_file": path, **mesh_check(tv, tf, bvh=bvh), "crossing_length_unit": "world"}
    base = os.path.splitext(path)[0]
    if getattr(args, "mesh_check_curves", 0):
        report["crossings_file"] = base + "_crossings.obj"
        write_obj_segments(report["crossings_file"], self_intersections(bvh, points=True)[2])
    if args.ckpt and os.path.exists(args.ckpt):
        tensorf, _ = _build_from_ckpt(args, load_checkpoint(args.ckpt), device)
        voxel = mesh_export_voxel(tensorf, getattr(args, "mesh_grid", None))
        report["voxel"] = [float(x) for x in voxel]
        report["voxel_unit"] = float(voxel.min())
        report["voxel_from"] = "--mesh_grid" if getattr(args, "mesh_grid", None) else "the field's gridSize (pass the export's --mesh_grid if it was made on another grid)"
        report["crossing_length_voxels"] = report["crossing_length"] / float(voxel.min())
    out = base + "_check.json"
    with open(out, "w") as fjson:
        json.dump(report, fjson, indent=1)
    print(f"check of {path}: {report['triangles']} triangles, {report['components']} component(s), closed: {report['closed']}, {report['crossing_pairs']} crossing pairs "
          f"on {report['crossing_faces']} triangles, intersection length {report['crossing_length']:.6g} (world units)"
          + (f" = {report['crossing_length_voxels']:.3f} export voxels" if "crossing_length_voxels" in report else ""))
    return out


FAULT_POLL_EVERY = 16       # iterations between two reads of the training-fault accumulator (field.check_training_faults)


def reconstruction(args, device="cuda", log=print, train_dataset=None, val_dataset=None):
    """train.py:113-371.  Returns (tensorf, logfolder, PSNRs_test of the last visualisation or final test).
    `train_dataset` / `val_dataset`: ready-made datasets (objects with all_rays, all_rgbs, scene_bbox, white_bg, near_far as BlenderRays has them) instead of the
    Blender folder under args.datadir — synthetic training sets (scripts/reconstruction_timing.py)."""
    cp_training = bool(int(getattr(args, "cp_training", 0) or 0))
    if getattr(args, "model_name", None) in RENDER_ONLY_MODELS and not cp_training:          # before any data is touched
        raise NotImplementedError(f"model_name {args.model_name!r}: CP training is not built into the default path (the CP backward kernels are opt-in: pass "
                                  "--cp_training 1); a CP checkpoint renders through --render_only 1 --ckpt ...")
    if getattr(args, "model_name", None) == "TensorCP" and float(getattr(args, "Ortho_weight", 0.0) or 0.0) > 0:
        raise ValueError("Ortho_weight > 0 with TensorCP: the class has no vector_comp_diffs (tensoRF.py:317-447); set Ortho_weight to 0")
    if args.dataset_name != "blender":
        raise NotImplementedError("only the Blender loader exists in the reference (dataLoader/__init__.py)")
    if args.model_name not in MODELS:
        raise NotImplementedError(f"model_name {args.model_name!r} is outside the accelerated path (TensorVMSplit, REFTensoRF, NerfPlusPlus)")
    if args.ndc_ray:
        raise NotImplementedError("ndc_ray datasets are not part of the reference's loaders")
    normal_maps = _normal_maps_wanted(args)                              # (refused before any training, not after it)
    if train_dataset is None:
        train_dataset = BlenderRays(args.datadir, split="train", downsample=args.downsample_train, is_stack=False, bbox=_bbox(args), near=args.near,
                                    far=args.far, white_bg=args.white_bkgd)
    if val_dataset is None:
        val_split = "val" if os.path.exists(os.path.join(args.datadir, "transforms_val.json")) else "train"
        val_dataset = BlenderRays(args.datadir, split=val_split, downsample=args.downsample_train, is_stack=True, bbox=_bbox(args), near=args.near,
                                  far=args.far, white_bg=args.white_bkgd)
    white_bg, near_far = train_dataset.white_bg, train_dataset.near_far
    upsamp_list = list(args.upsamp_list or [])
    update_AlphaMask_list = list(args.update_AlphaMask_list or [])
    logfolder = f"{args.basedir}/{args.expname}" + (datetime.datetime.now().strftime("-%Y%m%d-%H%M%S") if args.add_timestamp else "")
    for sub in ("", "/imgs_vis", "/imgs_rgba", "/rgba"):
        os.makedirs(logfolder + sub, exist_ok=True)

    aabb = train_dataset.scene_bbox
    reso_cur = N_to_reso(args.N_voxel_init, aabb)
    nSamples = int(min(args.nSamples, cal_n_samples(reso_cur, args.step_ratio)))
    global_step = 0
    ckpt = None
    if args.ckpt is not None:
        ckpt = load_checkpoint(args.ckpt)
        if "global_step" in ckpt:
            global_step = int(ckpt["global_step"]) + 1
        tensorf, kwargs = _build_from_ckpt(args, ckpt, device)
        nSamples = int(min(args.nSamples, cal_n_samples(kwargs["gridSize"], args.step_ratio)))
        reso_cur = [int(g) for g in kwargs["gridSize"]]
    else:
        tensorf = MODELS[args.model_name](aabb, reso_cur, device, density_n_comp=args.n_lamb_sigma, appearance_n_comp=args.n_lamb_sh,
                                          app_dim=args.data_dim_color, near_far=near_far, shadingMode=args.shadingMode,
                                          alphaMask_thres=args.alpha_mask_thre, density_shift=args.density_shift,
                                          distance_scale=args.distance_scale, pos_pe=args.pos_pe, view_pe=args.view_pe, fea_pe=args.fea_pe,
                                          featureC=args.featureC, step_ratio=args.step_ratio, fea2denseAct=args.fea2denseAct)
        if isinstance(tensorf, NerfPlusPlus):
            tensorf.set_nerfplusplus(bg_freq=args.bg_freq, bg_view_freq=args.bg_view_freq, bg_D=args.bg_D, radii=args.radii)
        tensorf.mlp_arith = getattr(args, "mlp_arith", "f32")            # (the evaluation renders of the run; the training steps compute fp32-class whatever it says)
    if cp_training and isinstance(tensorf, TensorCP):
        tensorf.cp_training = True                                       # opt in to the CP backward kernels (cp.py); the eager chain, no fused step

    if args.lr_decay_iters > 0:
        lr_factor = args.lr_decay_target_ratio ** (1 / args.lr_decay_iters)
    else:
        args.lr_decay_iters = args.n_iters
        lr_factor = args.lr_decay_target_ratio ** (1 / args.n_iters)

    def make_optimizer(lr_xyz, lr_net):
        return torch.optim.Adam(tensorf.get_optparam_groups(lr_xyz, lr_net), betas=(0.9, 0.99), fused=(torch.device(device).type == "cuda"))

    optimizer = make_optimizer(args.lr_init, args.lr_basis)
    if ckpt is not None and "lr" in ckpt:
        for pg, lr in zip(optimizer.param_groups, ckpt["lr"]):
            pg["lr"] = lr
    N_voxel_list = [int(v) for v in torch.round(torch.exp(torch.linspace(np.log(args.N_voxel_init), np.log(args.N_voxel_final),
                                                                          len(upsamp_list) + 1))).long().tolist()][1:]
    PSNRs, PSNRs_test = [], [0]
    allrays, allrgbs = train_dataset.all_rays, train_dataset.all_rgbs
    allrays, allrgbs = allrays.to(device), allrgbs.to(device)              # 288 GB of HBM: the whole training set lives on the device
    allrays, allrgbs = tensorf.filtering_rays(allrays, allrgbs, bbox_only=True)
    sampler = SimpleSampler(allrays.shape[0], args.batch_size, device=allrays.device)
    Ortho_w, L1_w = args.Ortho_weight, args.L1_weight_inital
    TV_d, TV_a = args.TV_weight_density, args.TV_weight_app
    tvreg = TVLoss()
    pen_w = args.normal_vector_penalty_weight
    reso_mask = reso_cur

    fused_adam = torch.device(device).type == "cuda"
    loss_hist = []
    for iteration in range(global_step, args.n_iters):
        optimizer.zero_grad()
        idx = sampler.nextids().to(device)
        rays_train, rgb_train = allrays[idx], allrgbs[idx]
        rgb_map, _, depth_map, _, _ = OctreeRender_trilinear_fast(rays_train, tensorf, chunk=args.batch_size, N_samples=nSamples, white_bg=white_bg,
                                                                  ndc_ray=False, device=device, is_train=True)
        loss = torch.mean((rgb_map - rgb_train) ** 2)
        total_loss = loss
        if Ortho_w > 0:
            total_loss = total_loss + Ortho_w * tensorf.vector_comp_diffs()
        if L1_w > 0:
            total_loss = total_loss + L1_w * tensorf.density_L1()
        if TV_d > 0:
            TV_d *= lr_factor
            total_loss = total_loss + tensorf.TV_loss_density(tvreg) * TV_d
        if TV_a > 0:
            TV_a *= lr_factor
            total_loss = total_loss + tensorf.TV_loss_app(tvreg) * TV_a
        if pen_w > 0 and hasattr(tensorf, "penalty"):                                              # train.py:253-257
            total_loss = total_loss + pen_w * tensorf.penalty
            tensorf.penalty = torch.zeros((), device=device)
        total_loss.backward()
        # No host read per step (train.py:262 takes `loss.item()` here; on this GPU that wait is 1.5 ms of a 3.9 ms step): the fused Adam kernel itself skips an
        # update whose step raised a fault flag (workspace overflow / fp16-range saturation inside the fused step, field.training_fault_flag), and the
        # losses stay on the device until the next log line.
        if fused_adam:
            optimizer.found_inf = tensorf.training_fault_flag()
            optimizer.step()
        else:
            fault = tensorf.check_training_faults()
            if fault is not None:
                log(f"Iteration {iteration:05d}: training step dropped ({fault})")
                optimizer.zero_grad(set_to_none=True)
            else:
                optimizer.step()
        loss_hist.append(loss.detach())
        for pg in optimizer.param_groups:
            pg["lr"] = pg["lr"] * lr_factor
        # the fault accumulator is polled on its own short cadence, not at the log rate: every step between a first fault and the adjustment of capacity / scale
        # is dropped on the device while the learning-rate decay keeps running (one host read per FAULT_POLL_EVERY steps: <= 0.1 ms per step)
        if fused_adam and (iteration % FAULT_POLL_EVERY == 0 or iteration % args.progress_refresh_rate == 0):
            fault = tensorf.check_training_faults()
            if fault is not None:                      # the flagged steps were skipped on the device; capacity / scale are adjusted now
                log(f"Iteration {iteration:05d}: training step(s) dropped since the last poll ({fault}); samples per ray "
                    f"{tensorf.train_app_samples_per_ray}, scale {tensorf.grad_scale_target:g}")
        if iteration % args.progress_refresh_rate == 0:
            hist = torch.stack(loss_hist)
            PSNRs = (-10.0 * torch.log10(hist)).tolist()
            log(f"Iteration {iteration:05d}: train_psnr = {float(np.mean(PSNRs)):.2f} test_psnr = {float(np.mean(PSNRs_test)):.2f} mse = {float(hist[-1]):.6f}")
            PSNRs, loss_hist = [], []
        if iteration % args.vis_every == args.vis_every - 1 and args.N_vis != 0 and len(val_dataset.all_rgbs):
            with torch.no_grad():
                PSNRs_test = evaluation(val_dataset, tensorf, args, OctreeRender_trilinear_fast, f"{logfolder}/imgs_vis/", N_vis=args.N_vis,
                                        prtx=f"{iteration:06d}_", N_samples=nSamples, white_bg=white_bg, ndc_ray=False, compute_extra_metrics=False,
                                        device=device)
        if iteration in update_AlphaMask_list:                                                     # train.py:292-313
            if reso_cur[0] * reso_cur[1] * reso_cur[2] < 256 ** 3:
                reso_mask = reso_cur
            new_aabb = tensorf.updateAlphaMask(tuple(reso_mask))
            if iteration == update_AlphaMask_list[0]:
                tensorf.shrink(new_aabb)
                L1_w = args.L1_weight_rest
            if len(update_AlphaMask_list) > 1 and iteration == update_AlphaMask_list[1]:
                allrays, allrgbs = tensorf.filtering_rays(allrays, allrgbs)
                sampler = SimpleSampler(allrgbs.shape[0], args.batch_size, device=allrays.device)
        if iteration in upsamp_list:                                                               # train.py:316-330
            reso_cur = N_to_reso(N_voxel_list.pop(0), tensorf.aabb)
            nSamples = int(min(args.nSamples, cal_n_samples(reso_cur, args.step_ratio)))
            tensorf.upsample_volume_grid(reso_cur)
            lr_scale = 1 if args.lr_upsample_reset else args.lr_decay_target_ratio ** (iteration / args.n_iters)
            optimizer = make_optimizer(args.lr_init * lr_scale, args.lr_basis * lr_scale)
        if iteration % (5 * args.vis_every) == 0 and iteration > 0:                                # train.py:337-345
            tensorf.save(f"{logfolder}/{args.expname}{iteration}.th",
                         {"lr": [pg["lr"] for pg in optimizer.param_groups], "global_step": iteration})
    tensorf.save(f"{logfolder}/{args.expname}.th", {"lr": [pg["lr"] for pg in optimizer.param_groups], "global_step": args.n_iters})
    if args.render_test:
        test_dataset = BlenderRays(args.datadir, split="test", downsample=args.downsample_train, is_stack=True, bbox=_bbox(args), near=args.near,
                                   far=args.far, white_bg=args.white_bkgd)
        if len(test_dataset.all_rgbs):
            with torch.no_grad():
                PSNRs_test = evaluation(test_dataset, tensorf, args, OctreeRender_trilinear_fast, f"{logfolder}/imgs_test_all/", N_vis=-1,
                                        N_samples=-1, white_bg=white_bg, ndc_ray=False, device=device, normal_maps=normal_maps)
            log(f"======> {args.expname} test all psnr: {np.mean(PSNRs_test)} <========================")
    return tensorf, logfolder, PSNRs_test


def main(cmd: Optional[List[str]] = None):
    torch.manual_seed(20211202)                                                                    # train.py:396-397
    np.random.seed(20211202)
    args = config_parser(cmd)
    if getattr(args, "render_mesh", 0) and not (args.render_only and args.render_test):
        raise SystemExit("--render_mesh 1 draws the mesh beside the test renders: it needs --render_only 1 --render_test 1 (and --ckpt); nothing was done")
    if getattr(args, "mesh_compare", None) and not args.export_mesh:
        if not getattr(args, "mesh_file", None):
            raise SystemExit("--mesh_compare REF compares the mesh of --export_mesh 1, or the one --mesh_file names: neither was given; nothing was done")
        out = mesh_compare(args, args.mesh_file)
        if getattr(args, "mesh_watertight", 0):
            mesh_watertight(args, args.mesh_file)
        if getattr(args, "mesh_check", 0):
            mesh_check_report(args, args.mesh_file)
        return out
    if getattr(args, "mesh_watertight", 0) and not args.export_mesh:
        if not getattr(args, "mesh_file", None):
            raise SystemExit("--mesh_watertight R remeshes the mesh of --export_mesh 1, or the one --mesh_file names: neither was given; nothing was done")
        out = mesh_watertight(args, args.mesh_file)
        if getattr(args, "mesh_check", 0):
            mesh_check_report(args, args.mesh_file)
        return out
    if getattr(args, "mesh_check", 0) and not args.export_mesh:
        if not getattr(args, "mesh_file", None):
            raise SystemExit("--mesh_check 1 checks the mesh of --export_mesh 1, or the one --mesh_file names: neither was given; nothing was done")
        return mesh_check_report(args, args.mesh_file)
    if args.export_mesh:
        path = export_mesh(args)
        if getattr(args, "mesh_compare", None):
            mesh_compare(args, path)
        if getattr(args, "mesh_watertight", 0):
            mesh_watertight(args, path)
        if getattr(args, "mesh_check", 0):
            mesh_check_report(args, path)
        if not (args.render_only and (args.render_test or args.render_path)):
            return path
    if args.render_only and (args.render_test or args.render_path):
        return render_test(args)
    return reconstruction(args)


if __name__ == "__main__":
    main()
