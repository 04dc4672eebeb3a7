"""GPU: the z-buffer rasteriser (csrc/tvr_mesh_raster.hip, include/tvr.h tvr_mesh_raster, mesh.render_mesh) against the two references of tests/mesh_raster_common.py —
the definition restated in numpy fp32 (triangle indices equal everywhere, depth and barycentrics within 2 ulp) and the fp64 ray-casting oracle (masks and indices equal
outside its ambiguous pixels, depth within 4 x the restatement's own error) — on the smallest shapes at which each path of the kernels can go wrong, the independence
of the result from runs, large_bbox, face order and vertex labels, watertightness along shared edges, the bad-index convention, and evaluation_mesh end to end.
Every test is a few calls on a healthy mesh; images are at most 64 x 64."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import mesh_raster_common as RC
from conftest import TINY, make_model

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
_refs = {}


def _np(t):
    return t.detach().cpu().numpy()


def gpu(v, f, cam, attr=None, large_bbox=0, stats=None):
    from jittor_myc_nerfs_amd import mesh
    dev = "cuda"
    a = None if attr is None else torch.from_numpy(np.ascontiguousarray(attr, np.float32)).to(dev)
    depth, tri, bary, out = mesh.render_mesh(torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev),
                                             cam["c2w"], cam["H"], cam["W"], (cam["fx"], cam["fy"]), center=(cam["cx"], cam["cy"]), near=cam["near"], cull=cam["cull"],
                                             attributes=a, large_bbox=large_bbox, stats=stats)
    return dict(depth=_np(depth), tri=_np(tri), bary=_np(bary), attr=None if out is None else _np(out))


def refs(name, cull=False):
    """(verts, faces, camera, restatement, oracle) of a sphere fixture, computed once"""
    key = (name, cull)
    if key not in _refs:
        v, f, cam = RC.sphere_fixture(name, cull=cull)
        _refs[key] = (v, f, cam, RC.restate(v, f, cam, attr=v), RC.oracle(v, f, cam))
    return _refs[key]


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("depth", "tri", "bary")) and \
        (a["attr"] is None or np.array_equal(a["attr"], b["attr"], equal_nan=True))


def check_against_restatement(got, res, stats=None, what=""):
    assert np.array_equal(got["tri"], res["tri"]), what
    du, bu = RC.ulp_diff(got["depth"], res["depth"]), RC.ulp_diff(got["bary"], res["bary"])
    print(f"    {what}: depth {du} ulp, bary {bu} ulp from the restatement; {int((res['tri'] >= 0).sum())} pixels hit")
    assert du <= 2 and bu <= 2, what
    hit = res["tri"] >= 0
    assert np.isinf(got["depth"][~hit]).all() and (got["depth"][~hit] > 0).all() and (got["bary"][~hit] == 0).all()
    if stats is not None:
        assert [stats["pixels_hit"], stats["triangles_skipped"], stats["triangles_without_pixel"]] == res["counts"], what
    return du, bu


def check_against_oracle(got, res, orc, what="", crossing=False):
    """crossing: the mesh has triangles that cross each other — the one case where pixels whose two nearest hits tie are left out of the index comparison besides the
    ambiguous ones (tests/mesh_raster_common.py compare_with_oracle); everywhere else there must be no tie and nothing but ambiguous pixels is left out"""
    own = RC.compare_with_oracle(res["depth"], res["tri"], orc)["max_rel_depth"]          # the restatement's own error on this fixture
    cmp = RC.compare_with_oracle(got["depth"], got["tri"], orc)
    print(f"    {what}: {cmp}; restatement's own depth error {own:.3g}")
    assert cmp["mask_diff"] == 0, what
    if crossing:
        assert cmp["tri_diff_outside_ties"] == 0, what
    else:
        assert cmp["ties"] == 0 and cmp["tri_diff"] == 0, what
    assert cmp["max_rel_depth"] <= max(4 * own, 2 * ULP), what


# ---- against both references ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RC.SPHERES))          # sphere6240 is the W = 53, H = 37 image: no multiple of a wave or of a workgroup, several workgroups
def test_spheres_against_restatement_and_oracle(name):
    v, f, cam, res, orc = refs(name)
    st = {}
    got = gpu(v, f, cam, attr=v, stats=st)
    check_against_restatement(got, res, st, name)
    check_against_oracle(got, res, orc, name)
    if RC.ulp_diff(got["bary"], res["bary"]) == 0:
        assert np.array_equal(got["attr"], res["attr"])
    assert np.allclose(got["attr"], res["attr"], rtol=0, atol=4 * ULP * 1.0)          # |attribute| <= 1 here and the weights differ by 2 ulp at most
    assert st["triangles_large"] == int((RC.box_pixels(res["setup"]) > 64).sum())
    # every triangle with a box through the queue: more entries than the image has pixels (6 240 against 37 x 53 rounded up to 2 048 lanes) takes the resolve
    # kernel's count of the entries that covered nothing through more than one pass
    st1 = {}
    large = gpu(v, f, cam, attr=v, large_bbox=1, stats=st1)
    assert same(got, large)
    assert [st1["pixels_hit"], st1["triangles_skipped"], st1["triangles_without_pixel"]] == res["counts"]
    assert st1["triangles_large"] == int((RC.box_pixels(res["setup"]) > 1).sum())
    if name == "sphere6240":
        assert st1["triangles_large"] > 2 * 2048


# ---- the shared-edge rule in the kernels --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swap_labels", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
def test_shared_edge_rule_on_the_exact_quad(swap_labels, reverse):
    """The quad whose arithmetic is exact: its diagonal passes through pixel centres, so those rays have E_k == 0 on the shared edge and only the owner rule decides.
    Through the lane's walk (large_bbox = H * W), the default (the boxes hold 100 pixels: the queue) and large_bbox = 1."""
    verts, faces, cam, diag = RC.exact_quad(swap_labels, reverse)
    res = RC.restate(verts, faces, cam)
    owner = RC.quad_owner(faces, verts, diag)
    inside = np.zeros((16, 16), bool)
    inside[4:12, 4:12] = True
    assert int(RC.box_pixels(res["setup"]).min()) > 64
    for large_bbox, n_large in ((16 * 16, 0), (0, 2), (1, 2)):
        st = {}
        got = gpu(verts, faces, cam, attr=verts, large_bbox=large_bbox, stats=st)
        assert st["triangles_large"] == n_large
        assert np.array_equal(got["tri"], res["tri"]) and np.array_equal(got["depth"], res["depth"]) and np.array_equal(got["bary"], res["bary"])        # exact: 0 ulp
        assert np.array_equal(got["tri"] >= 0, inside)                                            # every pixel centre inside is hit: no pinhole on the diagonal
        assert [int(got["tri"][15 - i, i]) for i in range(4, 12)] == [owner] * 8                 # and by the triangle the rule names: no double claim decided by index
        assert all((got["bary"][15 - i, i] == 0).sum() == 1 for i in range(4, 12))
        assert [st["pixels_hit"], st["triangles_skipped"], st["triangles_without_pixel"]] == res["counts"] == [64, 0, 0]
    # each triangle alone: the owner takes the diagonal, the other leaves it — the rule, not the depth tie-break, decided above
    for t in (0, 1):
        alone = gpu(verts, faces[t:t + 1], cam)
        on_diag = [int(alone["tri"][15 - i, i]) for i in range(4, 12)]
        assert on_diag == ([0] * 8 if t == owner else [-1] * 8)


def test_one_triangle_at_16x12():
    v = np.array([[-0.7, -0.5, 0.1], [0.8, -0.4, -0.2], [0.1, 0.7, 0.3]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    cam = RC.sphere_camera(12, 16, fill=1.0)
    st = {}
    got = gpu(v, f, cam, stats=st)
    res = RC.restate(v, f, cam)
    assert 10 < res["counts"][0] < 16 * 12
    check_against_restatement(got, res, st, "one triangle")
    check_against_oracle(got, res, RC.oracle(v, f, cam), "one triangle")


def test_box_of_exactly_large_bbox_and_one_more():
    v = np.array([[-0.7, -0.5, 0.1], [0.8, -0.4, -0.2], [0.1, 0.7, 0.3]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    cam = RC.sphere_camera(37, 53)
    res = RC.restate(v, f, cam)
    n = int(RC.box_pixels(res["setup"])[0])
    assert 64 < n < 37 * 53
    a, b = {}, {}
    at = gpu(v, f, cam, large_bbox=n, stats=a)            # the box holds exactly large_bbox pixels: the lane walks it
    above = gpu(v, f, cam, large_bbox=n - 1, stats=b)     # one more than large_bbox: the queue and a workgroup
    assert (a["triangles_large"], b["triangles_large"]) == (0, 1)
    assert same(at, above)
    check_against_restatement(at, res, a, "box == large_bbox")
    check_against_restatement(above, res, b, "box == large_bbox + 1")


def _big_triangle_behind(v, f, cam):
    """the mesh plus one triangle in the plane through the origin that faces the camera, large enough to fill the image"""
    c2w = cam["c2w"].astype(np.float64)
    right, up = c2w[:, 0], c2w[:, 1]
    big = np.stack([-40 * right - 30 * up, 40 * right - 30 * up, 50 * up]).astype(np.float32)
    return np.concatenate([v, big]), np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)


def test_a_screen_filling_triangle_plus_960_small_ones():
    v0, f0, _ = RC.sphere_fixture("sphere960")
    cam = RC.sphere_camera(64, 64)
    v, f = _big_triangle_behind(v0, f0, cam)
    st = {}
    got = gpu(v, f, cam, stats=st)
    res = RC.restate(v, f, cam)
    assert res["counts"][0] == 64 * 64 and (res["tri"] == 960).sum() > 1000 and (res["tri"] < 960).sum() > 1000
    assert st["triangles_large"] >= 1 and RC.box_pixels(res["setup"])[960] == 64 * 64
    check_against_restatement(got, res, st, "screen-filling triangle")
    check_against_oracle(got, res, RC.oracle(v, f, cam), "screen-filling triangle")


@pytest.mark.parametrize("near", [0.0, 2.0])
def test_a_corner_behind_the_camera(near):
    cam = RC.sphere_camera(32, 40, near=near)
    c2w = cam["c2w"].astype(np.float64)
    o, right, up, back = c2w[:, 3], c2w[:, 0], c2w[:, 1], c2w[:, 2]            # the camera looks along -back
    v = np.stack([o - 6 * back - 1.2 * right - 0.9 * up, o - 5 * back + 1.4 * right - 0.3 * up, o + 2 * back + 0.2 * right + 0.6 * up]).astype(np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    st = {}
    got = gpu(v, f, cam, stats=st)
    res = RC.restate(v, f, cam)
    assert RC.box_pixels(res["setup"])[0] == 32 * 40                            # a corner behind the camera plane: the whole image is offered
    assert 50 < res["counts"][0] < 32 * 40
    check_against_restatement(got, res, st, f"corner behind, near {near}")
    hit = got["tri"] >= 0
    assert (got["depth"][hit] > near).all()
    check_against_oracle(got, res, RC.oracle(v, f, cam), f"corner behind, near {near}")


def test_behind_and_off_screen():
    cam = RC.sphere_camera(32, 40)
    c2w = cam["c2w"].astype(np.float64)
    o, right, up, back = c2w[:, 3], c2w[:, 0], c2w[:, 1], c2w[:, 2]
    tri_at = lambda c, s: [c - s * right - s * up, c + s * right - s * up, c + s * up]
    centre = o - 4 * back
    v = np.stack(tri_at(o + 3 * back, 1.0)                 # wholly behind the camera
                 + tri_at(centre + 9 * right, 0.5)         # wholly off screen
                 + tri_at(centre + 1.0 * right, 0.6)       # partly off screen
                 + tri_at(centre - 0.3 * up, 0.4)).astype(np.float32)
    f = np.arange(12, dtype=np.int32).reshape(4, 3)
    st = {}
    got = gpu(v, f, cam, stats=st)
    res = RC.restate(v, f, cam)
    assert list(res["setup"]["state"]) == [2, 2, 0, 0] and res["counts"][2] == 2
    seen = set(np.unique(res["tri"]).tolist())
    assert seen == {-1, 2, 3} and (res["tri"][:, 0] == 2).any()                 # the third triangle runs off the image's edge (camera +x is screen left)
    check_against_restatement(got, res, st, "behind / off screen")
    check_against_oracle(got, res, RC.oracle(v, f, cam), "behind / off screen")
    # wholly behind alone: nothing
    st = {}
    got = gpu(v[:3], f[:1], cam, stats=st)
    assert (got["tri"] == -1).all() and np.isinf(got["depth"]).all() and (st["pixels_hit"], st["triangles_without_pixel"]) == (0, 1)


def test_coplanar_duplicates_go_to_the_smaller_index():
    v, f, cam, res, _ = refs("sphere960")
    twice = np.concatenate([f, f])
    for large_bbox in (0, 1):
        got = gpu(v, twice, cam, large_bbox=large_bbox)
        assert np.array_equal(got["tri"], res["tri"]) and np.array_equal(got["depth"], res["depth"])         # never 960 + t


def test_two_crossing_triangles():
    cam = RC.sphere_camera(32, 40)
    v = np.array([[-1.0, -0.8, -0.6], [1.0, -0.7, 0.7], [0.0, 0.9, 0.0], [-1.0, -0.7, 0.6], [1.0, -0.8, -0.7], [0.1, 0.9, 0.1]], np.float32)
    f = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    got = gpu(v, f, cam)
    res = RC.restate(v, f, cam)
    assert (res["tri"] == 0).sum() > 30 and (res["tri"] == 1).sum() > 30
    check_against_restatement(got, res, None, "crossing triangles")
    orc = RC.oracle(v, f, cam)
    check_against_oracle(got, res, orc, "crossing triangles", crossing=True)
    # per pixel the nearer of the two: where both are hit, the other one alone is farther
    for t in (0, 1):
        alone = gpu(v, f[t:t + 1], cam)
        both = (alone["tri"] >= 0) & (got["tri"] >= 0)
        assert (got["depth"][both] <= alone["depth"][both]).all()


def test_cull_on_a_closed_sphere():
    v, f, cam, res, _ = refs("sphere960")
    _, _, cam_c, res_c, orc_c = refs("sphere960", cull=True)
    a, b = {}, {}
    plain, culled = gpu(v, f, cam, stats=a), gpu(v, f, cam_c, stats=b)
    assert same(plain, culled)                                                    # the front hits are identical
    assert a["pixels_hit"] == b["pixels_hit"] and b["triangles_without_pixel"] > a["triangles_without_pixel"]
    check_against_restatement(culled, res_c, b, "cull")
    check_against_oracle(culled, res_c, orc_c, "cull")


def test_a_non_finite_vertex():
    v, f, cam, res, _ = refs("sphere960")
    bad = int(f[res["tri"][cam["H"] // 2, cam["W"] // 2], 0])                    # a corner of the triangle in the middle of the picture
    using = (f == bad).any(1)
    for value in (np.nan, np.inf):
        vb = v.copy()
        vb[bad, 1] = value
        st = {}
        got = gpu(vb, f, cam, stats=st)
        assert st["triangles_skipped"] == int(using.sum()) >= 3
        assert np.isin(res["tri"], np.nonzero(using)[0]).sum() >= 3             # they were seen
        rb = RC.restate(vb, f, cam)
        check_against_restatement(got, rb, st, f"vertex with {value}")
        keep = ~np.isin(res["tri"], np.nonzero(using)[0])                         # pixels the skipped triangles did not win are unchanged
        assert keep.sum() > 1000 and np.array_equal(got["tri"][keep], res["tri"][keep]) and np.array_equal(got["depth"][keep], res["depth"][keep])
        assert not np.isin(got["tri"], np.nonzero(using)[0]).any()


def test_no_triangles():
    cam = RC.sphere_camera(12, 16)
    st = {}
    got = gpu(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), cam, stats=st)
    assert (got["tri"] == -1).all() and np.isinf(got["depth"]).all() and (got["bary"] == 0).all()
    assert st == dict(pixels_hit=0, triangles_skipped=0, triangles_without_pixel=0, triangles_large=0)
    got = gpu(np.zeros((5, 3), np.float32), np.zeros((0, 3), np.int32), cam, attr=np.ones((5, 2), np.float32))
    assert got["attr"].shape == (12, 16, 2) and (got["attr"] == 0).all()
    # no vertices either, attributes of shape [0, A]; and the picture of nothing
    from jittor_myc_nerfs_amd import mesh
    got = gpu(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), cam, attr=np.zeros((0, 3), np.float32))
    assert got["attr"].shape == (12, 16, 3) and (got["attr"] == 0).all() and (got["tri"] == -1).all()
    img = mesh.mesh_view_to_rgb8(torch.from_numpy(got["tri"]), None, face_normal=mesh.face_normals(torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int32)))
    assert bool((img == 255).all())


# ---- independence -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_independent_of_runs_large_bbox_face_order_and_labels():
    v0, f0, _ = RC.sphere_fixture("sphere960")
    cam = RC.sphere_camera(48, 64)
    v, f = _big_triangle_behind(v0, f0, cam)                                      # both paths are in use at the default large_bbox
    base = gpu(v, f, cam, attr=v)
    assert same(base, gpu(v, f, cam, attr=v))                                     # two runs
    counts = []
    for lb in (1, 0, 48 * 64):
        st = {}
        assert same(base, gpu(v, f, cam, attr=v, large_bbox=lb, stats=st)), lb
        counts.append(st)
    assert counts[0]["triangles_large"] > 900 and counts[2]["triangles_large"] == 0 and 1 <= counts[1]["triangles_large"] < 100
    assert len({(c["pixels_hit"], c["triangles_skipped"], c["triangles_without_pixel"]) for c in counts}) == 1
    # permuted face order (no two triangles of this mesh tie in depth at a pixel: the restatement's winners are unique by more than an ulp — checked on the oracle's ties)
    assert not RC.oracle(v, f, cam)["tie"].any()
    perm = np.random.default_rng(5).permutation(len(f))
    got = gpu(v, f[perm], cam, attr=v)
    assert np.array_equal(got["depth"], base["depth"]) and np.array_equal(got["bary"], base["bary"]) and np.array_equal(got["attr"], base["attr"])
    hit = base["tri"] >= 0
    assert np.array_equal(got["tri"] >= 0, hit) and np.array_equal(perm[got["tri"][hit]], base["tri"][hit])
    # relabelled vertices: no ray of this view passes through an edge (every barycentric weight of every winner is > 0), so no owner rule is consulted
    assert (base["bary"][hit] > 0).all()
    relabel = np.random.default_rng(6).permutation(len(v))                        # new index of old vertex k
    v2 = np.empty_like(v)
    v2[relabel] = v
    got = gpu(v2, relabel[f].astype(np.int32), cam, attr=v2)
    assert same(base, got)


# ---- watertightness ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_marching_cubes_sphere_has_no_pinholes():
    verts, faces = RC.mc_sphere("cuda")
    v, f = _np(verts), _np(faces)
    assert 2000 < len(f) < 20000
    cam = RC.sphere_camera(64, 64)
    got = gpu(v, f, cam)
    orc = RC.oracle(v, f, cam)
    must = (orc["tri"] >= 0) & ~orc["ambiguous"]
    assert must.sum() > 1500
    assert (got["tri"][must] >= 0).all()                                          # every pixel the oracle hits and does not call ambiguous is hit
    res = RC.restate(v, f, cam)
    check_against_restatement(got, res, None, "marching-cubes sphere")
    cmp = RC.compare_with_oracle(got["depth"], got["tri"], orc)
    print(f"    marching-cubes sphere: {len(f)} triangles, {cmp}")
    assert cmp["mask_diff"] == 0
    # and the silhouette is one piece without holes: inside the hit mask's rows, hits are contiguous
    for row in got["tri"] >= 0:
        idx = np.nonzero(row)[0]
        assert idx.size == 0 or row[idx[0]:idx[-1] + 1].all()


# ---- a bad face index -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_bad_face_index_raises_the_flag_and_writes_nothing():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    from jittor_myc_nerfs_amd.autograd_ops import _stream_ptr
    v, f, cam, _, _ = refs("sphere960")
    dev = torch.device("cuda")
    for wrong in (len(v), -1):
        fb = f.copy()
        fb[777, 1] = wrong
        tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(fb).to(dev)
        with pytest.raises(L.TvrError, match="fault flag"):
            mesh.render_mesh(tv, tf, cam["c2w"], cam["H"], cam["W"], cam["fx"])
        lib = L.lib()
        c = mesh.mesh_camera(cam["c2w"], cam["H"], cam["W"], cam["fx"])
        n = cam["H"] * cam["W"]
        outs = [torch.full((k,), 0x5A, dtype=torch.uint8, device=dev) for k in (4 * n, 4 * n, 12 * n, 12 * n, 16)]
        scratch = torch.zeros(lib.tvr_mesh_raster_scratch_bytes(len(fb), cam["H"], cam["W"]), dtype=torch.uint8, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        attr = tv.clone()
        L.check(lib.tvr_mesh_raster(tv.data_ptr(), len(v), tf.data_ptr(), len(fb), C.byref(c), attr.data_ptr(), 3, outs[0].data_ptr(), 4 * n, outs[1].data_ptr(), 4 * n,
                                    outs[2].data_ptr(), 12 * n, outs[3].data_ptr(), 12 * n, scratch.data_ptr(), scratch.numel(), outs[4].data_ptr(), flag.data_ptr(),
                                    _stream_ptr(dev)), "tvr_mesh_raster")
        assert int(flag.item()) == 1
        assert all(bool((o == 0x5A).all()) for o in outs)                          # depth, tri, bary, attr_out and the counts: no byte changed


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_export_then_evaluation_mesh(tiny_arrays, tmp_path):
    from PIL import Image
    from jittor_myc_nerfs_amd import BlenderRays, mesh, rays as R, reconstruct, synthetic
    from jittor_myc_nerfs_amd.evaluation import evaluation_mesh
    hyper = dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=TINY["step_ratio"])
    m = make_model(tiny_arrays, hyper)
    alpha = m.getDenseAlpha()[0]
    level = 0.5 * (float(alpha.min()) + float(alpha.max()))
    ply = tmp_path / "tiny.ply"
    m.export_mesh(str(ply), level=level, spacing="samples", normals=True, colors=True)
    verts, faces, attrs = mesh.read_ply_attributes(str(ply))
    meta = {"camera_angle_x": 0.6911, "frames": [{"file_path": f"./test/r_{i}", "transform_matrix": M.tolist()} for i, M in enumerate(R.sphere_poses(2, 4.0))]}
    with open(tmp_path / "transforms_test.json", "w") as fjson:
        json.dump(meta, fjson)
    ds = BlenderRays(str(tmp_path), split="test", downsample=25.0, near=TINY["near_far"][0], far=TINY["near_far"][1])
    assert ds.img_wh == (32, 32) and ds.all_rays.shape == (2, 1024, 6)
    near, far = TINY["near_far"]
    for kind, kw in (("color", dict(normals=attrs["normals"], colors=attrs["colors"])), ("normal", dict(normals=attrs["normals"])), ("flat", {})):
        out = tmp_path / kind
        frames = evaluation_mesh(ds, m, verts, faces, str(out), white_bg=True, device="cuda", **kw)
        assert len(frames) == 2
        for idx, fr in enumerate(frames):
            img = np.asarray(Image.open(out / "mesh" / f"{idx:03d}.png"))
            assert img.shape == (32, 32, 3) and img.dtype == np.uint8
            assert (img != 255).any() and (img[0, 0] == 255).all()                # the object shows, the corner is background
            assert set(fr) == {"iou", "depth_median_vox", "depth_p95_vox", "depth_pixels"}
            assert all(np.isfinite(x) for x in fr.values()) and 0 <= fr["iou"] <= 1 and fr["depth_pixels"] > 0
            print(f"    {kind} view {idx}: {fr}")
    # the depths where the mesh is hit lie between near and far, and pixel p of the picture is ray p of the frame
    depth, tri, _, _ = mesh.render_mesh(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda(), ds.poses[0], 32, 32, ds.focal)
    d = _np(depth)[_np(tri) >= 0]
    assert d.size > 50 and (d > near).all() and (d < far).all()
    d2 = mesh.render_mesh_frame(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda(), np.asarray(meta["frames"][0]["transform_matrix"]), 32, 32, 0.6911)[0]
    assert torch.equal(depth, d2)
    # the command line: --render_only 1 --render_test 1 --render_mesh 1 writes the views and the report beside the rendered views
    ckpt = tmp_path / "tiny.th"
    m.save(str(ckpt))
    report = reconstruct.main(["--render_only", "1", "--render_test", "1", "--render_mesh", "1", "--ckpt", str(ckpt), "--datadir", str(tmp_path), "--downsample_train", "25",
                               "--model_name", "TensorVMSplit", "--expname", "tiny", "--near", repr(near), "--far", repr(far), "--white_bkgd"])["mesh"]
    folder = tmp_path / "imgs_test_all"
    assert (folder / "mesh" / "000.png").exists() and (folder / "mesh" / "001.png").exists()
    saved = json.load(open(folder / "mesh_agreement.json"))
    assert saved["mean"] == report["mean"] and len(saved["frames"]) == 2 and saved["mesh_file"] == str(ply)
    ext = np.asarray(TINY["aabb"][1]) - np.asarray(TINY["aabb"][0])
    assert np.allclose(saved["voxel"], ext / (np.asarray(TINY["gridSize"]) - 1.0), rtol=1e-6) and "gridSize" in saved["voxel_from"]      # the voxel used is on record
    print(f"    command line: mean {saved['mean']}")
