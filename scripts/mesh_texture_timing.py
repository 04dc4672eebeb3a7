#!/usr/bin/env python3
"""What the per-triangle texture atlas costs and what it buys, on the meshes export_mesh makes of scene A:

  * tvr_mesh_atlas_points alone (the whole atlas in one call into buffers allocated beforehand; GB/s counts the 16 B written per texel),
  * TensorBase.bake_texture as a whole and the share of its time spent in the existing field calls (surface_normals, the colour evaluation), from one pass with events
    around every stage,
    for the simplify=4 export at P = 8 and P = 16 and for the full 300^3 export at P = 5;
  * mesh.sample_texture per 800 x 800 view (uint8 atlas), beside the render_mesh call that feeds it;
  * the PSNR of mesh views against the field's render (pixels with a hit and acc > 0.99, evaluation.mesh_color_psnr) over the benchmark's eight poses, for the simplify=4
    export with vertex colours and with textures at P = 8 and P = 16: the number that says whether the feature does what it is for.

Timed by events on the stream after warm-up; the candidates of a comparison alternate within every round and the median of --runs rounds is reported with min and max.
The parent commit has no atlas and neither has the reference: a record for the next reader, not a gate.

    python scripts/mesh_texture_timing.py [--runs 7] [--json profiles/mesh_texture_timing.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def summary(v):
    v = sorted(v)
    return {"ms_median": v[len(v) // 2], "ms_min": v[0], "ms_max": v[-1]}


def points_alone(verts, faces, P, runs):
    from jittor_myc_nerfs_amd import _lib as L, mesh
    from jittor_myc_nerfs_amd.autograd_ops import _stream_ptr
    F = int(faces.shape[0])
    Ha, Wa, C = mesh.atlas_shape(F, P)
    n, dev = Ha * Wa, verts.device
    pos, tri = torch.empty((n, 3), device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    lib, stream = L.lib(), _stream_ptr(dev)

    def call():
        L.check(lib.tvr_mesh_atlas_points(verts.data_ptr(), verts.shape[0], faces.data_ptr(), F, P, C, 0, n, pos.data_ptr(), 12 * n, tri.data_ptr(), 4 * n, flag.data_ptr(),
                                          stream), "tvr_mesh_atlas_points")
    ms = [timed(call)[0] for r in range(-3, runs)][3:]
    assert int(flag.item()) == 0
    s = summary(ms)
    s.update(texels=n, atlas=[Ha, Wa], columns=C, owned_texels=int((tri >= 0).sum()), gb_per_s_written=16.0 * n / (s["ms_median"] * 1e-3) / 1e9)
    return s


@torch.no_grad()
def bake_stages(model, verts, faces, P, chunk=1 << 20):
    """one bake with events around every stage of TensorBase.bake_texture's loop (the same calls in the same order, without autograd as there)"""
    from jittor_myc_nerfs_amd import mesh
    Ha, Wa, C = mesh.atlas_shape(int(faces.shape[0]), P)
    aabb = model.aabb.to(device=model.device, dtype=torch.float32)
    out = torch.zeros((Ha * Wa, 3), dtype=torch.uint8, device=model.device)
    ms = dict(atlas_points=0.0, select_and_clamp=0.0, surface_normals=0.0, colours=0.0, scatter=0.0)
    for t0 in range(0, Ha * Wa, chunk):
        dt, (pos, tri) = timed(lambda: mesh.atlas_points(verts, faces, P, C, t0, min(chunk, Ha * Wa - t0)))
        ms["atlas_points"] += dt

        def select():
            idx = (tri >= 0).nonzero().view(-1)
            return idx, torch.maximum(torch.minimum(pos[idx], aabb[1]), aabb[0])
        dt, (idx, p) = timed(select)
        ms["select_and_clamp"] += dt
        if idx.numel() == 0:
            continue
        dt, nrm = timed(lambda: model.surface_normals(p))
        ms["surface_normals"] += dt
        dt, col = timed(lambda: model._vertex_colors(p, nrm))
        ms["colours"] += dt

        def scatter():
            out[idx + t0] = col
        ms["scatter"] += timed(scatter)[0]
    total = sum(ms.values())
    return {"ms": ms, "ms_total": total, "share_of_existing_field_calls": (ms["surface_normals"] + ms["colours"]) / total}, out.view(Ha, Wa, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--json", default="profiles/mesh_texture_timing.json")
    args = ap.parse_args()
    from jittor_myc_nerfs_amd import mesh, rays as R
    from jittor_myc_nerfs_amd.evaluation import mesh_color_psnr
    dev = torch.device("cuda:0")
    vm, _, A = bench.build_model(dev, "TensorVMSplit")
    W, H = A["img_wh"]
    focal = R.focal_from_angle(A["camera_angle_x"], W)
    raw = R.sphere_poses(bench.N_POSES, A["cam_radius"])
    poses = [(M @ R.BLENDER2OPENCV).astype(np.float32) for M in raw]
    vs, fs = vm.export_mesh(os.devnull, level=0.0005, spacing="samples", keep_largest=1, simplify=4.0)
    vf, ff = vm.export_mesh(os.devnull, level=0.0005, spacing="samples", keep_largest=1)
    rows = {}
    atlases = {}
    for label, v, f, P in (("simplify=4, P=8", vs, fs, 8), ("simplify=4, P=16", vs, fs, 16), ("full 300^3 export, P=5", vf, ff, 5)):
        row = {"vertices": int(v.shape[0]), "triangles": int(f.shape[0]), "P": P, "atlas_points_alone": points_alone(v, f, P, args.runs)}
        vm.bake_texture(v, f, P)                                                       # warm-up: allocator, scene state
        runs = max(3, args.runs // 2)
        row["bake_texture"] = summary([timed(lambda: vm.bake_texture(v, f, P))[0] for _ in range(runs)])
        row["bake_texture"]["runs"] = runs
        row["bake_stages_one_pass"], atlas = bake_stages(vm, v, f, P)
        row["stage_pass_equals_bake_texture"] = bool(torch.equal(atlas, vm.bake_texture(v, f, P)))
        if "simplify" in label:
            atlases[P] = atlas
        rows[label] = row
        print(label, json.dumps(row), flush=True)
    # sampling one 800 x 800 view, and the views' PSNR against the field's render
    colors = vm.mesh_vertex_attributes(vs, normals=False, colors=True)["colors"].to(torch.float32)
    F = int(fs.shape[0])
    layouts = {P: mesh.atlas_shape(F, P) for P in atlases}
    depth, tri, bary, _ = mesh.render_mesh(vs, fs, poses[0], H, W, focal)
    sample = {}
    for r in range(-3, args.runs):
        for P in (sorted(atlases) if r % 2 == 0 else sorted(atlases)[::-1]):
            dt = timed(lambda: mesh.sample_texture(tri, bary, atlases[P], P, layouts[P][2], F))[0]
            if r >= 0:
                sample.setdefault(P, []).append(dt)
    raster = [timed(lambda: mesh.render_mesh(vs, fs, poses[0], H, W, focal))[0] for _ in range(-3, args.runs)][3:]
    view = {"pixels_hit_pose0": int((tri >= 0).sum()), "render_mesh": summary(raster), "sample_texture": {f"P={P}": summary(v) for P, v in sample.items()}}
    psnr = {"vertex colours": [], **{f"texture P={P}": [] for P in sorted(atlases)}}
    for k, pose in enumerate(poses):
        rays = R.frame_rays(raw[k], H, W, A["camera_angle_x"]).to(dev)
        rgb = vm.render_rays(rays, white_bg=True)[0]
        _, acc, _ = vm.render_normals(rays)
        depth, tri, bary, attr = mesh.render_mesh(vs, fs, pose, H, W, focal, attributes=colors)
        psnr["vertex colours"].append(mesh_color_psnr(mesh.mesh_view_to_rgb8(tri, attr, "color"), tri >= 0, rgb, acc))
        for P in sorted(atlases):
            col = mesh.sample_texture(tri, bary, atlases[P], P, layouts[P][2], F)
            psnr[f"texture P={P}"].append(mesh_color_psnr(mesh.mesh_view_to_rgb8(tri, col, "color"), tri >= 0, rgb, acc))
    out = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "image": [H, W], "bakes": rows, "view_800x800": view,
           "psnr_db_against_the_field_render": {k: {"per_pose": v, "mean": float(np.mean(v))} for k, v in psnr.items()},
           "note": "atlas_points alone: events around the C call, buffers allocated beforehand, the whole atlas in one call; bake_texture: events around the Python call "
                   "(chunks of 2^20 texels, allocation and one host read of the fault flag per chunk included); the stage pass adds a synchronisation per stage, so its "
                   "total exceeds bake_texture's; PSNR over pixels with a mesh hit and field acc > 0.99, colours rounded to uint8 as the written views are; "
                   "not measured: the kernels under a profiler, atlases above 2^20 texels per chunk, fp32 atlases"}
    print(json.dumps(out), flush=True)
    if args.json:
        path = args.json if os.path.isabs(args.json) else os.path.join(ROOT, args.json)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as fjson:
            json.dump(out, fjson, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
