"""GPU: the texture atlas kernels (csrc/tvr_mesh_texture.hip, include/tvr.h tvr_mesh_atlas_points / tvr_mesh_texture_sample; mesh.atlas_points, mesh.sample_texture)
against the numpy fp32 restatement of tests/mesh_texture_common.py (owners equal, points and samples within 2 ulp; 0 observed), range chunking, the affine field end
to end against the fp64 oracle's hit points, TensorBase.bake_texture on the tiny scene, the bad-index convention, F = 0, and export -> OBJ -> evaluation_mesh -> the
command line.  Every case is a handful of launches on at most a few thousand texels or pixels."""
import json

import numpy as np
import pytest
import torch

import mesh_raster_common as RC
import mesh_texture_common as TC
from conftest import TINY, make_model

pytestmark = pytest.mark.gpu

_cache = {}


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def sphere():
    """(verts, faces, camera, numpy raster restatement, fp64 oracle) of the 960-triangle sphere at 48 x 64, computed once"""
    if "sphere" not in _cache:
        v, f, cam = RC.sphere_fixture("sphere960")
        _cache["sphere"] = (v, f, cam, RC.restate(v, f, cam), RC.oracle(v, f, cam))
    return _cache["sphere"]


def meshes():
    if "meshes" not in _cache:
        v, f = sphere()[:2]
        _cache["meshes"] = {"F1": TC.small_mesh(1), "F2": TC.small_mesh(2), "F7": TC.small_mesh(7), "sphere960": (v, f)}
    return _cache["meshes"]


def columns(F, which):
    """C = 1, the default, and one that leaves the last row partial (S % C != 0 where S allows it)"""
    S = (F + 1) // 2
    if which == "one":
        return 1
    if which == "default":
        return TC.default_columns(F)
    c = next((c for c in range(2, S + 2) if S % c), 2)
    return c


# ---- atlas_points ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["one", "default", "partial"])
@pytest.mark.parametrize("P", [5, 6, 8])
@pytest.mark.parametrize("name", ["F1", "F2", "F7", "sphere960"])
def test_atlas_points_against_the_restatement(name, P, which):
    from jittor_myc_nerfs_amd import mesh
    v, f = meshes()[name]
    C_ = columns(len(f), which)
    Ha, Wa, _ = mesh.atlas_shape(len(f), P, C_)
    assert (Ha, Wa) == TC.layout(len(f), P, C_)
    pos, tri = mesh.atlas_points(_dev(v, np.float32), _dev(f, np.int32), P, C_, 0, Ha * Wa)
    rpos, rtri = TC.restate_points(v, f, P, C_)
    assert torch.equal(tri.cpu(), torch.from_numpy(rtri))
    d = RC.ulp_diff(_np(pos), rpos)
    print(f"    {name} P={P} C={C_}: {Ha}x{Wa} texels, {int((rtri >= 0).sum())} owned, points {d} ulp from the restatement")
    assert d <= 2
    assert (_np(pos)[rtri < 0] == 0).all()


def test_atlas_points_ranges_equal_the_one_call():
    from jittor_myc_nerfs_amd import mesh
    v, f = meshes()["sphere960"]
    P, C_ = 6, 7                                                 # 480 squares in rows of 7: Wa = 42, the last row partial
    Ha, Wa, _ = mesh.atlas_shape(len(f), P, C_)
    tv, tf = _dev(v, np.float32), _dev(f, np.int32)
    pos, tri = mesh.atlas_points(tv, tf, P, C_, 0, Ha * Wa)
    ranges = [(Wa * 2 + 5, Wa * 2 + 5 + 17),                     # starts and ends inside one atlas row of a square row
              (Wa * 3 + 11, Wa * 4 + 9),                         # crosses an atlas row inside a square row
              (Wa * (P - 1) + 30, Wa * (P + 1) + 3),             # crosses from one square row into the next
              (Wa * 7 + 13, Wa * 7 + 14),                        # n = 1
              (Ha * Wa - 1, Ha * Wa), (0, 1), (Ha * Wa, Ha * Wa)]
    for a, b in ranges:
        p2, t2 = mesh.atlas_points(tv, tf, P, C_, a, b - a)
        assert torch.equal(p2, pos[a:b]) and torch.equal(t2, tri[a:b]), (a, b)
    parts = [mesh.atlas_points(tv, tf, P, C_, a, min(1000, Ha * Wa - a)) for a in range(0, Ha * Wa, 1000)]
    assert len(parts) == -(-Ha * Wa // 1000) > 10
    assert torch.equal(torch.cat([p for p, _ in parts]), pos) and torch.equal(torch.cat([t for _, t in parts]), tri)


# ---- sample_texture -------------------------------------------------------------------------------------------------------------------------------------------------------------
def _atlases(F, P, C_):
    Ha, Wa = TC.layout(F, P, C_)
    rng = np.random.default_rng(17)
    return {"uint8": rng.integers(0, 256, (Ha, Wa, 3), dtype=np.uint8), "fp32": (rng.random((Ha, Wa, 3)) * 2 - 1).astype(np.float32)}


@pytest.mark.parametrize("fmt", ["uint8", "fp32"])
@pytest.mark.parametrize("P", [5, 8])
def test_sample_texture_on_a_rendered_sphere(P, fmt):
    from jittor_myc_nerfs_amd import mesh
    v, f, cam, _, _ = sphere()
    C_ = TC.default_columns(len(f))
    atlas = _atlases(len(f), P, C_)[fmt]
    depth, tri, bary, _ = mesh.render_mesh(_dev(v, np.float32), _dev(f, np.int32), cam["c2w"], cam["H"], cam["W"], (cam["fx"], cam["fy"]), center=(cam["cx"], cam["cy"]))
    got = mesh.sample_texture(tri, bary, torch.from_numpy(atlas).cuda(), P, C_, len(f))
    assert got.shape == (cam["H"], cam["W"], 3) and got.dtype == torch.float32
    want = TC.restate_sample(_np(tri), _np(bary), atlas, P, C_, len(f))
    d = RC.ulp_diff(_np(got), want)
    hit = _np(tri) >= 0
    print(f"    P={P} {fmt}: {int(hit.sum())} pixels hit, samples {d} ulp from the restatement")
    assert hit.sum() > 500 and d <= 2
    assert (_np(got)[~hit] == 0).all()


@pytest.mark.parametrize("fmt", ["uint8", "fp32"])
def test_sample_texture_on_hand_made_hits(fmt):
    from jittor_myc_nerfs_amd import mesh
    F, P, C_ = 7, 6, 2
    atlas = _atlases(F, P, C_)[fmt]
    b = TC.probe_barycentrics(50, seed=9)                        # random points, corners, edge points, points an ulp outside
    tri = np.concatenate([np.full(len(b), t, np.int32) for t in (0, 1, 5, 6, -1, F, F + 100)])      # both halves, the last (odd) triangle, no hit, indices past the mesh
    bary = np.concatenate([b] * 7)
    bary[3] = [np.nan, np.nan, np.nan]                           # a NaN weight reads the corner texel
    got = mesh.sample_texture(_dev(tri, np.int32), _dev(bary, np.float32), torch.from_numpy(atlas).cuda(), P, C_, F)
    want = TC.restate_sample(tri, bary, atlas, P, C_, F)
    d = RC.ulp_diff(_np(got), want)
    print(f"    hand-made hits, {fmt}: {d} ulp from the restatement")
    assert d <= 2
    assert (_np(got)[tri < 0] == 0).all() and (_np(got)[tri >= F] == 0).all()
    if fmt == "uint8":                                           # corners read their own texel as it is
        e, _, _ = TC.tap_texels(np.array([0, 0, 0]), np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32), P, C_, F)
        corner = mesh.sample_texture(_dev(np.zeros(3), np.int32), _dev(np.eye(3), np.float32), torch.from_numpy(atlas).cuda(), P, C_, F)
        assert np.array_equal(_np(corner), atlas.reshape(-1, 3)[e[:, 0]].astype(np.float32))


def test_affine_field_end_to_end_against_the_oracle():
    """An affine colour field baked into an fp32 atlas on the sphere (the GPU's own atlas_points), drawn by render_mesh and read by sample_texture, against the field at
    the fp64 oracle's hit points.  The bound is 4 x the error of the numpy restatement (numpy raster, numpy atlas, numpy sampling) on the same pixels."""
    from jittor_myc_nerfs_amd import mesh
    v, f, cam, res, orc = sphere()
    P, C_ = 8, TC.default_columns(len(f))
    Ha, Wa = TC.layout(len(f), P, C_)
    tv, tf = _dev(v, np.float32), _dev(f, np.int32)
    pos, owner = mesh.atlas_points(tv, tf, P, C_, 0, Ha * Wa)
    atlas = np.where((_np(owner) >= 0)[:, None], TC.affine(_np(pos)), 0.0).astype(np.float32).reshape(Ha, Wa, 3)
    depth, tri, bary, _ = mesh.render_mesh(tv, tf, cam["c2w"], cam["H"], cam["W"], (cam["fx"], cam["fy"]), center=(cam["cx"], cam["cy"]))
    got = _np(mesh.sample_texture(tri, bary, torch.from_numpy(atlas).cuda(), P, C_, len(f))).reshape(-1, 3).astype(np.float64)
    ref = TC.restate_sample(res["tri"], res["bary"], TC.affine_atlas(v, f, P, C_), P, C_, len(f)).reshape(-1, 3).astype(np.float64)
    want = TC.affine(TC.oracle_hit_points(cam, orc))
    m = ((orc["tri"] >= 0) & ~orc["ambiguous"] & (orc["tri"] == res["tri"]) & (orc["tri"] == _np(tri))).reshape(-1)
    own, err = float(np.abs(ref[m] - want[m]).max()), float(np.abs(got[m] - want[m]).max())
    print(f"    affine end to end over {int(m.sum())} pixels: kernels {err:.3g}, restatement's own error {own:.3g}")
    assert m.sum() > 500 and own > 0
    assert err <= 4 * own


# ---- the bad-index convention, F = 0 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_a_bad_face_index_raises_the_flag_and_writes_nothing():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    from jittor_myc_nerfs_amd.autograd_ops import _stream_ptr
    v, f = meshes()["sphere960"]
    P, C_ = 5, TC.default_columns(len(f))
    Ha, Wa = TC.layout(len(f), P, C_)
    dev = torch.device("cuda")
    for wrong in (len(v), -1):
        fb = f.copy()
        fb[777, 1] = wrong
        tv, tf = _dev(v, np.float32), _dev(fb, np.int32)
        with pytest.raises(L.TvrError, match="fault flag"):
            mesh.atlas_points(tv, tf, P, C_, 0, Ha * Wa)
        n = Ha * Wa
        outs = [torch.full((k,), 0x5A, dtype=torch.uint8, device=dev) for k in (12 * n, 4 * n)]
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        L.check(L.lib().tvr_mesh_atlas_points(tv.data_ptr(), len(v), tf.data_ptr(), len(fb), P, C_, 0, n, outs[0].data_ptr(), 12 * n, outs[1].data_ptr(), 4 * n,
                                              flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_atlas_points")
        assert int(flag.item()) == 1
        assert all(bool((o == 0x5A).all()) for o in outs)                                 # points and owners: no byte changed


def test_a_mesh_without_triangles():
    from jittor_myc_nerfs_amd import mesh
    tv, tf = torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    assert mesh.atlas_shape(0, 5) == (5, 5, 1)
    pos, tri = mesh.atlas_points(tv, tf, 5, 1, 0, 25)
    assert bool((tri == -1).all()) and bool((pos == 0).all()) and pos.shape == (25, 3)
    out = mesh.sample_texture(torch.full((4, 4), -1, dtype=torch.int32, device="cuda"), torch.zeros((4, 4, 3), device="cuda"),
                              torch.full((5, 5, 3), 200, dtype=torch.uint8, device="cuda"), 5, 1, 0)
    assert bool((out == 0).all())


# ---- the field's bake -------------------------------------------------------------------------------------------------------------------------------------------------------------
def _tiny(tiny_arrays):
    from jittor_myc_nerfs_amd import synthetic
    if "tiny" not in _cache:
        hyper = dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=TINY["step_ratio"])
        m = make_model(tiny_arrays, hyper)
        alpha = m.getDenseAlpha()[0]
        _cache["tiny"] = (m, 0.5 * (float(alpha.min()) + float(alpha.max())))
    return _cache["tiny"]


def test_bake_texture_on_a_simplified_export(tiny_arrays, tmp_path):
    from jittor_myc_nerfs_amd import mesh
    m, level = _tiny(tiny_arrays)
    verts, faces = m.export_mesh(str(tmp_path / "tiny.ply"), level=level, spacing="samples", simplify=2.0)
    F, P = int(faces.shape[0]), 6
    assert F > 50
    stats = {}
    atlas = m.bake_texture(verts, faces, P, stats=stats)
    Ha, Wa, C_ = mesh.atlas_shape(F, P)
    assert atlas.shape == (Ha, Wa, 3) and atlas.dtype == torch.uint8 and atlas.is_cuda
    _, owner, = TC.restate_points(_np(verts), _np(faces), P, C_)
    assert stats == dict(atlas_texels=Ha * Wa, atlas_owned_texels=int((owner >= 0).sum()), atlas_chunks=1)
    assert bool((atlas.view(-1, 3)[torch.from_numpy(owner < 0).cuda()] == 0).all())         # unowned texels stay 0
    assert int((atlas.view(-1, 3)[torch.from_numpy(owner >= 0).cuda()] != 0).sum()) > 0
    # corner texels hold the vertex colours (the same definition at the same point): equal is expected, one level of 255 is allowed
    colors = _np(m.mesh_vertex_attributes(verts, normals=False, colors=True)["colors"]).astype(np.int64)
    uv = mesh.atlas_uv(F, P, C_)
    X, Y = np.rint(uv[..., 0] * Wa - 0.5).astype(np.int64), np.rint((1 - uv[..., 1]) * Ha - 0.5).astype(np.int64)
    corner = _np(atlas).astype(np.int64)[Y, X]                                              # [F,3 corners,3]
    worst = int(np.abs(corner - colors[_np(faces).astype(np.int64)]).max())
    print(f"    {F} triangles, atlas {Ha}x{Wa}: corner texels differ from the vertex colours by at most {worst} levels")
    assert worst <= 1
    # chunking and repetition change nothing
    st2 = {}
    assert torch.equal(m.bake_texture(verts, faces, P, chunk=1000, stats=st2), atlas) and st2["atlas_chunks"] == -(-Ha * Wa // 1000) > 1
    assert torch.equal(m.bake_texture(verts, faces, P), atlas)
    with pytest.raises(ValueError):
        m.bake_texture(verts, faces, 4)


def test_reftensorf_does_not_bake(tiny_ref_arrays):
    from jittor_myc_nerfs_amd import synthetic
    hyper = dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=TINY["step_ratio"])
    m = make_model(tiny_ref_arrays, hyper)
    v, f = TC.small_mesh(2)
    with pytest.raises(NotImplementedError, match="REFTensoRF"):
        m.bake_texture(_dev(v * 0.5, np.float32), _dev(f, np.int32), 5)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_export_with_a_texture_then_the_command_line(tiny_arrays, tmp_path):
    from PIL import Image
    from jittor_myc_nerfs_amd import BlenderRays, mesh, rays as R, reconstruct
    from jittor_myc_nerfs_amd.evaluation import evaluation_mesh
    m, level = _tiny(tiny_arrays)
    plain = tmp_path / "plain.ply"
    m.export_mesh(str(plain), level=level, spacing="samples", simplify=2.0, colors=True)
    ply = tmp_path / "tiny.ply"
    verts, faces = m.export_mesh(str(ply), level=level, spacing="samples", simplify=2.0, colors=True, texture=5)
    assert open(ply, "rb").read() == open(plain, "rb").read()                              # the PLY is what it is without the option
    assert not (tmp_path / "plain.obj").exists()
    for ext in (".obj", ".mtl", ".png"):
        assert (tmp_path / ("tiny" + ext)).exists()
    F = int(faces.shape[0])
    Ha, Wa, C_ = mesh.atlas_shape(F, 5)
    st = m.mesh_export_stats
    assert (st["atlas_patch"], st["atlas_columns"], st["atlas_height"], st["atlas_width"], st["atlas_texels"]) == (5, C_, Ha, Wa, Ha * Wa)
    v2, f2, uv, png = mesh.read_obj(str(tmp_path / "tiny.obj"))
    atlas = mesh.read_texture_png(png)
    assert np.array_equal(v2, _np(verts)) and np.array_equal(f2, _np(faces)) and atlas.shape == (Ha, Wa, 3)
    assert mesh.atlas_layout_from_uv(uv, Ha, Wa) == (5, C_)
    assert np.array_equal(atlas, _np(m.bake_texture(verts, faces, 5)))
    meta = {"camera_angle_x": 0.6911, "frames": [{"file_path": f"./test/r_{i}", "transform_matrix": M.tolist()} for i, M in enumerate(R.sphere_poses(2, 4.0))]}
    with open(tmp_path / "transforms_test.json", "w") as fjson:
        json.dump(meta, fjson)
    near, far = TINY["near_far"]
    ds = BlenderRays(str(tmp_path), split="test", downsample=25.0, near=near, far=far)
    frames = evaluation_mesh(ds, m, v2, f2, str(tmp_path / "view"), white_bg=True, device="cuda", texture=atlas, texture_layout=(5, C_), color_psnr=True)
    assert len(frames) == 2
    for idx, fr in enumerate(frames):
        img = np.asarray(Image.open(tmp_path / "view" / "mesh" / f"{idx:03d}.png"))
        assert img.shape == (32, 32, 3) and (img != 255).any() and (img[0, 0] == 255).all()
        assert set(fr) == {"iou", "depth_median_vox", "depth_p95_vox", "depth_pixels", "color_psnr"} and np.isfinite(fr["color_psnr"])
        print(f"    textured view {idx}: {fr}")
    # without colours the key is null; without the option it is absent
    bare = evaluation_mesh(ds, m, v2, f2, str(tmp_path / "bare"), white_bg=True, device="cuda", color_psnr=True)
    assert [fr["color_psnr"] for fr in bare] == [None, None]
    # the command line on the OBJ, and on the PLY with vertex colours: both reports carry the PSNR
    ckpt = tmp_path / "tiny.th"
    m.save(str(ckpt))
    common = ["--render_only", "1", "--render_test", "1", "--render_mesh", "1", "--ckpt", str(ckpt), "--datadir", str(tmp_path), "--downsample_train", "25",
              "--model_name", "TensorVMSplit", "--expname", "tiny", "--near", repr(near), "--far", repr(far), "--white_bkgd"]
    psnr = {}
    for kind, path in (("obj", tmp_path / "tiny.obj"), ("ply", ply)):
        report = reconstruct.main(common + ["--mesh_file", str(path)])["mesh"]
        saved = json.load(open(tmp_path / "imgs_test_all" / "mesh_agreement.json"))
        assert saved["mesh_file"] == str(path) and len(saved["frames"]) == 2 and saved["mean"] == report["mean"]
        assert all(np.isfinite(fr["color_psnr"]) for fr in saved["frames"]) and np.isfinite(saved["mean"]["color_psnr"])
        assert (tmp_path / "imgs_test_all" / "mesh" / "001.png").exists()
        psnr[kind] = saved["mean"]["color_psnr"]
    assert abs(psnr["obj"] - float(np.mean([fr["color_psnr"] for fr in frames]))) < 1e-9
    print(f"    command line: PSNR against the rendered views, textured OBJ {psnr['obj']:.2f} dB, PLY with vertex colours {psnr['ply']:.2f} dB")
