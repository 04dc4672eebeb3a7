"""No GPU: what of the z-buffer rasteriser (include/tvr.h tvr_mesh_raster, mesh.render_mesh, evaluation.mesh_agreement / evaluation_mesh, reconstruct --render_mesh) can
be checked without one — the definition restated in numpy fp32 (tests/mesh_raster_common.py) against an fp64 ray-casting oracle that shares none of its formulation,
the shared-edge rule on an exact-arithmetic quad, every argument error of the C call (they come before any launch), the pure Python helpers and the option parser."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mesh_raster_common as RC
from conftest import ROOT

# largest relative depth error of the fp32 restatement against the fp64 oracle on the two sphere fixtures, as this test measures it (and asserts it is no larger):
# 2.93e-6 (sphere960) and 9.26e-7 (sphere6240); an earlier numpy prototype saw 3.6e-6 / 5.8e-7.  tests/test_gpu_mesh_raster.py takes its allowance against the oracle from
# the value it measures itself, by the same call.
RESTATEMENT_DEPTH_ERROR_BOUND = 2.0 ** -17       # 7.6e-6 = 64 ulp: twice the 4e-6 the plane form of the depth kept in the prototype at a camera distance of 4
                                                 # (camera-space coordinates of size 4 carry 2.4e-7 each, an edge of 0.1 therefore 2.4e-6 relative, and so does pn)


@pytest.fixture(scope="module", params=sorted(RC.SPHERES))
def sphere(request):
    v, f, cam = RC.sphere_fixture(request.param)
    return request.param, v, f, cam, RC.restate(v, f, cam), RC.oracle(v, f, cam)


def test_restatement_matches_the_oracle(sphere):
    name, v, f, cam, res, orc = sphere
    cmp = RC.compare_with_oracle(res["depth"], res["tri"], orc)
    print(f"    {name}: {cmp}, counts {res['counts']}")
    assert cmp["hit"] > 500                                             # the fixture shows the sphere
    assert cmp["ambiguous"] <= 0.01 * cmp["hit"]                        # a condition on the fixture
    assert cmp["mask_diff"] == 0 and cmp["tri_diff"] == 0 and cmp["ties"] == 0
    assert cmp["max_rel_depth"] <= RESTATEMENT_DEPTH_ERROR_BOUND
    assert res["counts"][0] == int((res["tri"] >= 0).sum()) and res["counts"][1] == 0
    # barycentrics: positive, sum to one within rounding, zero off the mesh
    hit = res["tri"] >= 0
    assert (res["bary"][hit] >= 0).all() and np.abs(res["bary"][hit].sum(-1) - 1).max() <= 4e-7 and (res["bary"][~hit] == 0).all()
    assert np.isinf(res["depth"][~hit]).all()


def test_restatement_culls_the_far_side_only(sphere):
    name, v, f, cam, res, orc = sphere
    culled = RC.restate(v, f, dict(cam, cull=True))
    assert np.array_equal(culled["tri"], res["tri"]) and np.array_equal(culled["depth"], res["depth"])        # the near side of a closed surface is all one sees
    assert culled["counts"][2] > res["counts"][2]                                                                # the far side no longer covers pixels
    o2 = RC.oracle(v, f, dict(cam, cull=True))
    assert RC.compare_with_oracle(culled["depth"], culled["tri"], o2)["tri_diff"] == 0
    # the reverse orientation shows the far side instead: deeper everywhere it hits
    flipped = RC.restate(v, f[:, ::-1].copy(), dict(cam, cull=True))
    both = (flipped["tri"] >= 0) & (res["tri"] >= 0)
    assert both.sum() > 400 and (flipped["depth"][both] > res["depth"][both]).all()


def test_interpolated_attributes_of_the_restatement():
    v, f, cam = RC.sphere_fixture("sphere960")
    res = RC.restate(v, f, cam, attr=v)                                  # interpolating the positions gives the hit point
    hit = res["tri"] >= 0
    dist = np.linalg.norm(res["attr"][hit].astype(np.float64) - cam["c2w"][:, 3].astype(np.float64), axis=-1)
    assert np.abs(dist - res["depth"][hit]).max() <= 1e-5 * 4.0
    assert (res["attr"][~hit] == 0).all()


@pytest.mark.parametrize("swap_labels", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
def test_shared_edge_rule_on_the_exact_quad(swap_labels, reverse):
    verts, faces, cam, diag = RC.exact_quad(swap_labels, reverse)
    res = RC.restate(verts, faces, cam)
    inside = np.zeros((16, 16), bool)
    inside[4:12, 4:12] = True
    assert np.array_equal(res["tri"] >= 0, inside)                      # every pixel centre inside the quad is hit, none outside
    owner = RC.quad_owner(faces, verts, diag)
    assert [int(res["tri"][15 - i, i]) for i in range(4, 12)] == [owner] * 8
    # exact arithmetic: the depth of pixel (j, i) is 4 |dir| with every operation but the square root exact; the ray through the diagonal has one E_k == 0
    dx, dy = RC.pixel_dirs32(cam)
    want = (np.float32(4) * np.sqrt((dx * dx + dy * dy) + np.float32(1))).reshape(16, 16)
    assert np.array_equal(res["depth"][inside], want[inside])
    assert all((res["bary"][15 - i, i] == 0).sum() == 1 for i in range(4, 12))
    off = inside.copy()
    off[[15 - i for i in range(4, 12)], list(range(4, 12))] = False
    assert (res["bary"][off] > 0).all()
    orc = RC.oracle(verts, faces, cam)
    assert orc["ambiguous"][[15 - i for i in range(4, 12)], list(range(4, 12))].all()          # the oracle calls exactly such rays ambiguous
    assert np.array_equal(orc["tri"] >= 0, inside)


def test_numbering_decides_the_owner():
    a = RC.quad_owner(*[RC.exact_quad(False, False)[k] for k in (1, 0, 3)])
    b = RC.quad_owner(*[RC.exact_quad(True, False)[k] for k in (1, 0, 3)])
    assert {a, b} == {0, 1}


def test_box_is_conservative_on_the_fixtures():
    """no pixel the oracle hits lies outside the winning triangle's box: the box changes no result"""
    for name in RC.SPHERES:
        v, f, cam = RC.sphere_fixture(name)
        S = RC.setup32(v, f, cam)
        orc = RC.oracle(v, f, cam)
        jj, ii = np.nonzero(orc["tri"] >= 0)
        t = orc["tri"][jj, ii]
        assert ((S["i0"][t] <= ii) & (ii <= S["i1"][t]) & (S["j0"][t] <= jj) & (jj <= S["j1"][t])).all()
        # and with a margin: a pixel the oracle hits is never on the box's rim unless the rim is the image's
        rim = ((S["i0"][t] == ii) & (ii > 0)) | ((S["i1"][t] == ii) & (ii < cam["W"] - 1)) | ((S["j0"][t] == jj) & (jj > 0)) | ((S["j1"][t] == jj) & (jj < cam["H"] - 1))
        assert not rim.any()


# ---- the C call's argument errors -------------------------------------------------------------------------------------------------------------------------------------------
def _aligned(nbytes):
    buf = C.create_string_buffer(nbytes + 256)
    base = C.addressof(buf)
    return buf, (base + 255) // 256 * 256


def _call(lib, L, **kw):
    """tvr_mesh_raster with host pointers that are never followed: every case below is refused before any launch"""
    H, W, F, V, A = kw.get("H", 4), kw.get("W", 4), kw.get("F", 2), kw.get("V", 4), kw.get("A", 0)
    cam = L.MeshCamera()
    cam.c2w[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    cam.H, cam.W, cam.fx, cam.fy, cam.cx, cam.cy, cam.near_, cam.cull, cam.large_bbox = H, W, 4.0, 4.0, 2.0, 2.0, 0.0, 0, 0
    for k, val in kw.get("cam", {}).items():
        if k == "c2w0":
            cam.c2w[0] = val
        else:
            setattr(cam, k, val)
    keep, p = _aligned(1 << 16)
    n = max(H * W, 1) if H * W < 1 << 20 else 1
    args = dict(verts=p, V=V, faces=p, F=F, cam=C.byref(cam), attr=p if A else None, A=A, depth=p, depth_bytes=4 * n, tri=p, tri_bytes=4 * n, bary=p, bary_bytes=12 * n,
                attr_out=p if A else None, attr_out_bytes=4 * n * max(A, 0), scratch=p, scratch_bytes=1 << 16, counts=p, flag=p)
    args.update(kw.get("args", {}))
    rc = lib.tvr_mesh_raster(args["verts"], args["V"], args["faces"], args["F"], args["cam"], args["attr"], args["A"], args["depth"], args["depth_bytes"], args["tri"],
                             args["tri_bytes"], args["bary"], args["bary_bytes"], args["attr_out"], args["attr_out_bytes"], args["scratch"], args["scratch_bytes"],
                             args["counts"], args["flag"], None)
    return rc, lib.tvr_last_error().decode()


INVALID, SCRATCH, UNSUPPORTED = -1, -3, -4


@pytest.mark.parametrize("kw, code, word", [
    (dict(args=dict(cam=None)), INVALID, "cam"),
    (dict(args=dict(depth=None)), INVALID, "depth"),
    (dict(args=dict(tri=None)), INVALID, "tri"),
    (dict(args=dict(bary=None)), INVALID, "bary"),
    (dict(args=dict(scratch=None)), INVALID, "scratch"),
    (dict(args=dict(counts=None)), INVALID, "counts_dev"),
    (dict(args=dict(flag=None)), INVALID, "fault_flag_dev"),
    (dict(args=dict(faces=None)), INVALID, "faces"),
    (dict(args=dict(verts=None)), INVALID, "verts"),
    (dict(F=-1), INVALID, "n_triangles"),
    (dict(V=-1), INVALID, "n_vertices"),
    (dict(H=0), INVALID, "H"),
    (dict(W=0), INVALID, "W"),
    (dict(cam=dict(c2w0=float("nan"))), INVALID, "c2w"),
    (dict(cam=dict(c2w0=float("inf"))), INVALID, "c2w"),
    (dict(cam=dict(fx=0.0)), INVALID, "fx"),
    (dict(cam=dict(fy=-1.0)), INVALID, "fy"),
    (dict(cam=dict(fx=float("inf"))), INVALID, "fx"),
    (dict(cam=dict(cx=float("nan"))), INVALID, "cx"),
    (dict(cam=dict(near_=-0.5)), INVALID, "near"),
    (dict(cam=dict(near_=float("nan"))), INVALID, "near"),
    (dict(cam=dict(near_=float("inf"))), INVALID, "near"),
    (dict(cam=dict(cull=2)), INVALID, "cull"),
    (dict(cam=dict(large_bbox=-1)), INVALID, "large_bbox"),
    (dict(A=-1), INVALID, "n_attr"),
    (dict(A=9), INVALID, "n_attr"),
    (dict(A=3, args=dict(attr=None)), INVALID, "attr"),
    (dict(A=3, args=dict(attr_out=None)), INVALID, "attr_out"),
    (dict(H=65536, W=32768), UNSUPPORTED, "2^31"),
    (dict(F=1 << 31), UNSUPPORTED, "2^31"),
    (dict(H=(1 << 24) + 1, W=1), UNSUPPORTED, "2^24"),
    (dict(H=1, W=(1 << 24) + 1), UNSUPPORTED, "2^24"),
    (dict(V=1 << 31), UNSUPPORTED, "n_vertices"),
    (dict(args=dict(depth_bytes=63)), SCRATCH, "depth"),
    (dict(args=dict(tri_bytes=63)), SCRATCH, "tri"),
    (dict(args=dict(bary_bytes=191)), SCRATCH, "bary"),
    (dict(A=3, args=dict(attr_out_bytes=191)), SCRATCH, "attr_out"),
    (dict(args=dict(scratch_bytes=256 + 256 + 255)), SCRATCH, "scratch"),
])
def test_c_argument_errors_come_before_any_launch(kw, code, word):
    from jittor_myc_nerfs_amd import _lib as L
    rc, msg = _call(L.lib(), L, **kw)
    assert rc == code, (rc, msg)
    assert word in msg and "tvr_mesh_raster" in msg, msg


def test_misaligned_scratch_and_scratch_bytes():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    keep, p = _aligned(1 << 16)
    rc, msg = _call(lib, L, args=dict(scratch=p + 8))
    assert rc == INVALID and "aligned" in msg
    up = lambda x: (x + 255) // 256 * 256
    for F, H, W in ((0, 1, 1), (2, 4, 4), (960, 48, 64), (6240, 37, 53), (2_700_000, 800, 800)):
        assert lib.tvr_mesh_raster_scratch_bytes(F, H, W) == 256 + up(8 * H * W) + up(4 * F)
    assert lib.tvr_mesh_raster_scratch_bytes(1, 1 << 24, 1) == 256 + up(8 << 24) + 256          # the largest side that is taken
    for F, H, W in ((-1, 4, 4), (4, 0, 4), (4, 4, -2), (1 << 31, 4, 4), (4, 65536, 32768), (4, (1 << 24) + 1, 1), (4, 1, (1 << 24) + 1)):
        assert lib.tvr_mesh_raster_scratch_bytes(F, H, W) == 0


def test_export_is_additive():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    lib = L.lib()
    assert lib.tvr_version() == 141
    assert len(L.SYMBOLS["tvr_mesh_raster"][1]) == 20 and len(L.SYMBOLS["tvr_mesh_raster_scratch_bytes"][1]) == 3
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tvr.h")).read(), flags=re.S)
    assert re.search(r"#define\s+TVR_MESH_RASTER_LARGE_BBOX\s+64\b", src) and re.search(r"#define\s+TVR_MESH_RASTER_MAX_ATTR\s+8\b", src)
    assert re.search(r"#define\s+TVR_MESH_RASTER_MAX_SIDE\s+16777216\b", src)
    assert mesh.RASTER_LARGE_BBOX == 64 and mesh.RASTER_MAX_ATTR == 8
    # the ctypes struct has the header's fields in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} tvr_mesh_camera;", src).group(1)
    names = re.findall(r"\b([A-Za-z_][A-Za-z_0-9]*)\s*(?:\[\d+\])?\s*[,;]", body)
    assert names == [n for n, _ in L.MeshCamera._fields_]
    assert C.sizeof(L.MeshCamera) == 12 * 4 + 9 * 4


# ---- Python side ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_render_mesh_has_no_cpu_fallback():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    v, f, cam = RC.sphere_fixture("sphere960")
    with pytest.raises(L.TvrError, match="no CPU fallback"):
        mesh.render_mesh(torch.from_numpy(v), torch.from_numpy(f), cam["c2w"], cam["H"], cam["W"], cam["fx"])
    c = mesh.mesh_camera(cam["c2w"], 48, 64, 70.0)
    assert (c.cx, c.cy, c.fx, c.fy, c.near_, c.cull, c.large_bbox) == (32.0, 24.0, 70.0, 70.0, 0.0, 0, 0)
    c = mesh.mesh_camera(torch.eye(4), 48, 64, (70.0, 71.0), center=(30.0, 20.0), near=0.5, cull=True, large_bbox=9)
    assert (c.cx, c.cy, c.fx, c.fy, c.near_, c.cull, c.large_bbox) == (30.0, 20.0, 70.0, 71.0, 0.5, 1, 9) and list(c.c2w) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    with pytest.raises(ValueError):
        mesh.mesh_camera(np.eye(3), 4, 4, 1.0)
    # focal as a 0-d tensor, a numpy scalar, a tensor pair
    for focal, want in ((torch.tensor(70.0), (70.0, 70.0)), (np.float32(70.0), (70.0, 70.0)), (torch.tensor([70.0, 71.0]), (70.0, 71.0)), ([70.0, 71.0], (70.0, 71.0))):
        c = mesh.mesh_camera(np.eye(4), 4, 4, focal)
        assert (c.fx, c.fy) == want


def test_mesh_view_to_rgb8():
    from jittor_myc_nerfs_amd import mesh
    from jittor_myc_nerfs_amd.evaluation import normal_map_to_rgb8
    tri = torch.tensor([[0, -1], [1, 1]], dtype=torch.int32)
    n = torch.tensor([[[0.0, 0.0, 2.0], [0.0, 0.0, 0.0]], [[3.0, 0.0, 4.0], [0.0, -0.5, 0.0]]])
    img = mesh.mesh_view_to_rgb8(tri, n, "normal")
    assert img.dtype == torch.uint8 and img.shape == (2, 2, 3)
    assert img[0, 0].tolist() == [128, 128, 255] and img[0, 1].tolist() == [255, 255, 255]            # renormalised; the background is white
    assert img[1, 1].tolist() == [128, 0, 128]
    assert mesh.mesh_view_to_rgb8(tri, n, "normal", white_bg=False)[0, 1].tolist() == [0, 0, 0]
    # the same picture normal_map_to_rgb8 makes of unit normals with the hit mask as acc
    unit = n / n.norm(dim=-1, keepdim=True).clamp_min(1e-30)
    hit = (tri >= 0).float()
    assert torch.equal(img, normal_map_to_rgb8(unit * hit.unsqueeze(-1), hit))
    col = torch.tensor([[[255.0, 0.0, 127.6], [9.0, 9.0, 9.0]], [[12.0, 13.0, 14.0], [300.0, -4.0, 0.4]]])
    img = mesh.mesh_view_to_rgb8(tri, col, "color")
    assert img[0, 0].tolist() == [255, 0, 128] and img[0, 1].tolist() == [255, 255, 255] and img[1, 0].tolist() == [12, 13, 14] and img[1, 1].tolist() == [255, 0, 0]
    # no attributes: flat shading from the face normals
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    f = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    fn = mesh.face_normals(v, f)
    assert torch.equal(fn, torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]))
    img = mesh.mesh_view_to_rgb8(tri, None, "normal", face_normal=fn)
    assert img[0, 0].tolist() == [128, 128, 255] and img[1, 0].tolist() == [255, 128, 128] and img[0, 1].tolist() == [255, 255, 255]
    with pytest.raises(ValueError):
        mesh.mesh_view_to_rgb8(tri, None, "normal")
    # a mesh without faces: render_mesh takes it and hits nothing; its flat view is the background
    none = torch.full((2, 3), -1, dtype=torch.int32)
    empty = mesh.mesh_view_to_rgb8(none, None, "normal", face_normal=mesh.face_normals(torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int32)))
    assert empty.shape == (2, 3, 3) and bool((empty == 255).all())
    with pytest.raises(ValueError):
        mesh.mesh_view_to_rgb8(tri, n, "depth")


def test_mesh_agreement_on_hand_made_maps():
    from jittor_myc_nerfs_amd.evaluation import mesh_agreement, mesh_agreement_summary
    mesh_hit = np.array([[1, 1, 1, 0], [0, 0, 1, 0]], bool)
    mesh_depth = np.where(mesh_hit, np.array([[2.0, 2.5, 3.0, 0], [0, 0, 4.0, 0]]), np.inf)
    acc = np.array([[1.0, 0.995, 0.6, 0.7], [0.0, 0.4, 1.0, 0.0]])
    fdepth = np.array([[2.1, 2.5, 9.0, 3.0], [0.0, 1.0, 3.7, 0.0]])
    a = mesh_agreement(mesh_depth, mesh_hit, fdepth, acc, 0.1)
    # solid = acc > 0.5: 5 pixels; mesh 4; intersection 4 -> union 5
    assert a["iou"] == pytest.approx(4 / 5) and a["depth_pixels"] == 3
    assert a["depth_median_vox"] == pytest.approx(1.0) and a["depth_p95_vox"] == pytest.approx(np.percentile([1.0, 0.0, 3.0], 95))
    b = mesh_agreement(torch.from_numpy(mesh_depth), torch.from_numpy(mesh_hit), torch.from_numpy(fdepth), torch.from_numpy(acc), [0.1, 0.1, 0.1])
    assert b == pytest.approx(a, rel=1e-12)
    empty = mesh_agreement(np.full((2, 2), np.inf), np.zeros((2, 2), bool), np.zeros((2, 2)), np.zeros((2, 2)), 1.0)
    assert empty["iou"] == 1.0 and empty["depth_pixels"] == 0 and np.isnan(empty["depth_median_vox"])
    s = mesh_agreement_summary([a, empty])
    assert s["mean"]["iou"] == pytest.approx(0.9) and s["mean"]["depth_median_vox"] == pytest.approx(1.0) and len(s["frames"]) == 2
    with pytest.raises(ValueError):
        mesh_agreement(mesh_depth, mesh_hit, fdepth, acc, 0.0)
    with pytest.raises(ValueError):
        mesh_agreement(mesh_depth, mesh_hit[:1], fdepth, acc, 0.1)


def test_argument_parser():
    from jittor_myc_nerfs_amd import reconstruct
    a = reconstruct.config_parser([])
    assert a.render_mesh == 0 and a.mesh_file is None
    a = reconstruct.config_parser(["--render_mesh", "1", "--mesh_file", "x.ply"])
    assert a.render_mesh == 1 and a.mesh_file == "x.ply"
    # the flag alone draws nothing: that is said, not passed over
    for cmd in (["--render_mesh", "1"], ["--render_mesh", "1", "--render_only", "1"], ["--render_mesh", "1", "--render_test", "1"],
                ["--render_mesh", "1", "--export_mesh", "1"]):
        with pytest.raises(SystemExit, match="render_test"):
            reconstruct.main(cmd)


def test_export_voxel_follows_mesh_grid(tiny_arrays):
    from conftest import TINY, make_model
    from jittor_myc_nerfs_amd import reconstruct, synthetic
    m = make_model(tiny_arrays, dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=TINY["step_ratio"]), device="cpu")
    ext = np.asarray(TINY["aabb"][1]) - np.asarray(TINY["aabb"][0])
    assert np.allclose(reconstruct.mesh_export_voxel(m), ext / (np.asarray(TINY["gridSize"]) - 1.0), rtol=1e-6)
    assert np.allclose(reconstruct.mesh_export_voxel(m, [31, 41, 51]), ext / np.asarray([30.0, 40.0, 50.0]), rtol=1e-6)
    for bad in ([8, 8], [8, 8, 1]):
        with pytest.raises(ValueError):
            reconstruct.mesh_export_voxel(m, bad)
