"""No GPU: what of the per-triangle texture atlas (include/tvr.h tvr_mesh_atlas_points / tvr_mesh_texture_sample, mesh.atlas_* / sample_texture / write_obj / read_obj,
TensorBase.bake_texture, reconstruct --mesh_texture) can be checked without a device: the definition's restatement (tests/mesh_texture_common.py) against its own
properties and against fp64, the layout helpers, the OBJ / PNG round trip, the C calls' argument errors (host pointers that are never followed), the ABI, the parser."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mesh_texture_common as TC
from conftest import ROOT

F32 = np.float32


# ---- the definition -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [5, 6, 7, 8, 9])
def test_every_texel_of_a_used_square_has_exactly_one_owner(P):
    for F, C_ in ((1, 1), (2, 1), (7, 2), (8, 2), (9, 3)):
        Ha, Wa = TC.layout(F, P, C_)
        tri, x, y = TC.owners(F, P, C_, np.arange(Ha * Wa))
        tri, x, y = tri.reshape(Ha, Wa), x.reshape(Ha, Wa), y.reshape(Ha, Wa)
        S = (F + 1) // 2
        for s in range(Ha // P * C_):
            X0, Y0 = (s % C_) * P, (s // C_) * P
            sq = tri[Y0:Y0 + P, X0:X0 + P]
            lx, ly = x[Y0:Y0 + P, X0:X0 + P], y[Y0:Y0 + P, X0:X0 + P]
            if s >= S:
                assert (sq == -1).all()
                continue
            upper = np.add.outer(np.arange(P), np.arange(P)) <= P - 1                     # [b, a]: a + b <= P - 1
            assert (sq[upper] == 2 * s).all()
            assert (sq[~upper] == (2 * s + 1 if 2 * s + 1 < F else -1)).all()
            # local coordinates: each half holds every (x, y) of its own range exactly once
            for h, m in ((0, upper), (1, ~upper)):
                pairs = sorted(zip(lx[m].tolist(), ly[m].tolist()))
                bound = P - 1 if h == 0 else P - 2
                assert pairs == sorted((a, b) for a in range(P) for b in range(P) if a + b <= bound)
        assert int((tri >= 0).sum()) == (F // 2) * P * P + (F % 2) * (P * (P + 1) // 2)


@pytest.mark.parametrize("P", [5, 6, 7, 8, 9, 10, 11])
def test_taps_stay_on_texels_of_their_own_triangle(P):
    F, C_ = 7, 2
    Ha, Wa = TC.layout(F, P, C_)
    owner, _, _ = TC.owners(F, P, C_, np.arange(Ha * Wa))
    b = TC.probe_barycentrics(2000, seed=P)
    for t in (0, 1, 4, 5, 6):                                                             # both halves, several squares, the last (odd) triangle
        e, fx, fy = TC.tap_texels(np.full(len(b), t), b, P, C_, F)
        assert e.min() >= 0 and e.max() < Ha * Wa
        assert (owner[e] == t).all(), (P, t)
        assert (fx >= 0).all() and (fx < 1).all() and (fy >= 0).all() and (fy < 1).all()


def test_affine_field_is_reproduced_through_bake_and_sample():
    """The restatement against fp64: an affine field baked into the restatement's fp32 atlas and read back by the sampling rule at random points, corners, edge points
    and points an ulp outside, both halves.  The bound is 4 x the error the numpy prototype of the definition observed (7.8e-7 for values of order 1), scaled by the
    field's largest magnitude on the atlas.  Observed: 1.11e-7 x the magnitude (the test prints it)."""
    worst = 0.0
    for P in (5, 6, 7, 8, 9, 10, 11):
        v, f = TC.small_mesh(7, seed=P)
        C_ = TC.default_columns(len(f))
        atlas = TC.affine_atlas(v, f, P, C_)
        scale = float(np.abs(atlas).max())
        b = TC.probe_barycentrics(2000, seed=100 + P)
        for t in range(len(f)):
            tri = np.full(len(b), t)
            got = TC.restate_sample(tri, b, atlas, P, C_, len(f)).astype(np.float64)
            # the sampling rule clamps x = b1 L and y = b2 L into 0 .. L: the fp64 truth is the field at the clamped weights
            b1, b2 = np.clip(b[:, 1].astype(np.float64), 0, 1), np.clip(b[:, 2].astype(np.float64), 0, 1)
            want = TC.affine(TC.true_points(v, f, tri, np.stack([1 - b1 - b2, b1, b2], -1)))
            err = float(np.abs(got - want).max())
            worst = max(worst, err / scale)
            assert err <= 4 * TC.PROTOTYPE_AFFINE_ERROR * scale, (P, t, err, scale)
    print(f"    affine reproduction: worst error / field magnitude {worst:.3g} (bound {4 * TC.PROTOTYPE_AFFINE_ERROR:.3g})")


@pytest.mark.parametrize("P", [5, 6, 8, 13])
def test_corner_texels_are_the_vertices_bit_for_bit(P):
    v, f = TC.small_mesh(7, seed=P)
    C_ = 2
    Ha, Wa = TC.layout(len(f), P, C_)
    pos, tri = TC.restate_points(v, f, P, C_)
    L = P - 4
    for t in range(len(f)):
        s, h = t >> 1, t & 1
        X0, Y0 = (s % C_) * P, (s // C_) * P
        for k, (x, y) in enumerate(((0, 0), (L, 0), (0, L))):
            a, b = (P - 1 - x, P - 1 - y) if h else (x, y)
            e = (Y0 + b) * Wa + X0 + a
            assert tri[e] == t
            assert pos[e].view(np.int32).tolist() == v[f[t, k]].view(np.int32).tolist(), (t, k)


# ---- layout helpers -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_atlas_shape():
    from jittor_myc_nerfs_amd import mesh
    assert mesh.atlas_shape(0, 5) == (5, 5, 1)                 # Ha >= P even without a triangle
    assert mesh.atlas_shape(1, 5) == (5, 5, 1)
    assert mesh.atlas_shape(2, 5) == (5, 5, 1)
    assert mesh.atlas_shape(3, 5) == (5, 10, 2) and mesh.atlas_shape(5, 5) == (10, 10, 2)
    assert mesh.atlas_shape(8, 6, 2) == (12, 12, 2)            # 4 squares, 2 per row: the last row is exactly full
    assert mesh.atlas_shape(9, 6, 2) == (18, 12, 2)            # one more triangle opens a row
    assert mesh.atlas_shape(7, 8, 1) == (32, 8, 1)
    assert mesh.atlas_shape(960, 8) == (22 * 8, 22 * 8, 22)    # S = 480, ceil(sqrt) = 22
    assert mesh.atlas_shape(2 * 49, 5)[2] == 7 and mesh.atlas_shape(2 * 49 + 1, 5)[2] == 8
    for F in (0, 1, 2, 7, 8, 9, 960):
        for P in (5, 8):
            for C_ in (1, 2, 3, None):
                Ha, Wa, cc = mesh.atlas_shape(F, P, C_)
                assert (Ha, Wa) == TC.layout(F, P, cc) and (C_ is None and cc == TC.default_columns(F) or cc == C_)
    for bad in (dict(F=-1, P=5), dict(F=1, P=4), dict(F=1, P=65), dict(F=1, P=5, C=0)):
        with pytest.raises(ValueError):
            mesh.atlas_shape(**bad)
    assert (mesh.ATLAS_MIN_P, mesh.ATLAS_MAX_P) == (5, 64)


def test_atlas_uv_against_the_layout():
    from jittor_myc_nerfs_amd import mesh
    for F, P, C_ in ((1, 5, 1), (7, 6, 2), (8, 8, 3), (9, 5, None)):
        Ha, Wa, cc = mesh.atlas_shape(F, P, C_)
        uv = mesh.atlas_uv(F, P, C_)
        assert uv.shape == (F, 3, 2) and uv.dtype == np.float64
        owner, lx, ly = TC.owners(F, P, cc, np.arange(Ha * Wa))
        X = np.rint(uv[..., 0] * Wa - 0.5).astype(np.int64)
        Y = np.rint((1.0 - uv[..., 1]) * Ha - 0.5).astype(np.int64)
        assert np.allclose(uv[..., 0], (X + 0.5) / Wa, rtol=0, atol=1e-15) and np.allclose(uv[..., 1], 1 - (Y + 0.5) / Ha, rtol=0, atol=1e-15)
        e = Y * Wa + X
        L = P - 4
        for t in range(F):
            assert owner[e[t]].tolist() == [t, t, t]
            assert list(zip(lx[e[t]].tolist(), ly[e[t]].tolist())) == [(0, 0), (L, 0), (0, L)]
        assert mesh.atlas_layout_from_uv(uv, Ha, Wa) == (P, cc)
    with pytest.raises(ValueError):
        mesh.atlas_layout_from_uv(mesh.atlas_uv(7, 6, 2) * 0.9, 24, 12)
    assert mesh.atlas_uv(0, 5).shape == (0, 3, 2)


def test_obj_and_png_round_trip(tmp_path):
    from jittor_myc_nerfs_amd import mesh
    v, f = TC.small_mesh(7)
    P = 6
    Ha, Wa, C_ = mesh.atlas_shape(len(f), P)
    atlas = np.random.default_rng(5).integers(0, 256, (Ha, Wa, 3), dtype=np.uint8)
    normals = np.random.default_rng(6).standard_normal(v.shape).astype(F32)
    uv = mesh.atlas_uv(len(f), P)
    for name, nr in (("plain", None), ("withn", normals)):
        obj, png = tmp_path / f"{name}.obj", tmp_path / f"{name}.png"
        mesh.write_texture_png(str(png), torch.from_numpy(atlas))
        mesh.write_obj(str(obj), torch.from_numpy(v), f, uv, str(png), normals=nr)
        text = open(obj).read().split("\n")
        assert text[0] == f"mtllib {name}.mtl" and text[1] == "usemtl atlas"
        kinds = [ln.split()[0] for ln in text if ln]
        assert kinds.count("v") == len(v) and kinds.count("vt") == 3 * len(f) and kinds.count("f") == len(f) and kinds.count("vn") == (len(v) if nr is not None else 0)
        face = next(ln for ln in text if ln.startswith("f "))
        assert face == ("f 1/1 2/2 3/3" if nr is None else "f 1/1/1 2/2/2 3/3/3")
        assert f"map_Kd {name}.png" in open(tmp_path / f"{name}.mtl").read().split("\n")
        v2, f2, uv2, tex = mesh.read_obj(str(obj))
        assert v2.dtype == np.float32 and np.array_equal(v2, v) and f2.dtype == np.int32 and np.array_equal(f2, f)
        assert uv2.shape == (len(f), 3, 2) and np.abs(uv2 - uv).max() <= 0.5e-10         # ten decimals: far below a texel (1 / Wa) of any atlas that is taken
        assert os.path.samefile(tex, png) and np.array_equal(mesh.read_texture_png(tex), atlas)
        assert mesh.atlas_layout_from_uv(uv2, Ha, Wa) == (P, C_)
    with pytest.raises(ValueError):
        mesh.write_obj(str(tmp_path / "x.ply"), v, f, uv, "x.png")
    with pytest.raises(ValueError):
        mesh.write_obj(str(tmp_path / "x.obj"), v, f, uv[:-1], "x.png")
    bad = tmp_path / "bad.obj"
    bad.write_text("mtllib plain.mtl\nv 0 0 0\nf 1 1 1\n")
    with pytest.raises(ValueError, match="write_obj"):
        mesh.read_obj(str(bad))


# ---- the C calls' argument errors ---------------------------------------------------------------------------------------------------------------------------------------------
INVALID, SCRATCH, UNSUPPORTED = -1, -3, -4


def _host_pointer():
    buf = C.create_string_buffer(1 << 12)
    return buf, C.addressof(buf)


def _points(lib, **kw):
    """tvr_mesh_atlas_points with host pointers that are never followed: every case below is refused before any launch"""
    keep, p = _host_pointer()
    a = dict(verts=p, V=4, faces=p, F=2, P=5, C=1, texel0=0, n=25, pos=p, pos_bytes=300, tri=p, tri_bytes=100, flag=p)
    a.update(kw)
    rc = lib.tvr_mesh_atlas_points(a["verts"], a["V"], a["faces"], a["F"], a["P"], a["C"], a["texel0"], a["n"], a["pos"], a["pos_bytes"], a["tri"], a["tri_bytes"],
                                   a["flag"], None)
    return rc, lib.tvr_last_error().decode()


def _sample(lib, **kw):
    keep, p = _host_pointer()
    a = dict(tri=p, bary=p, n_pix=16, atlas=p, fmt=0, Ha=5, Wa=5, P=5, C=1, F=2, out=p, out_bytes=192)
    a.update(kw)
    rc = lib.tvr_mesh_texture_sample(a["tri"], a["bary"], a["n_pix"], a["atlas"], a["fmt"], a["Ha"], a["Wa"], a["P"], a["C"], a["F"], a["out"], a["out_bytes"], None)
    return rc, lib.tvr_last_error().decode()


@pytest.mark.parametrize("kw, code, word", [
    (dict(flag=None), INVALID, "fault_flag_dev"),
    (dict(verts=None), INVALID, "verts"),
    (dict(faces=None), INVALID, "faces"),
    (dict(pos=None), INVALID, "pos_out"),
    (dict(tri=None), INVALID, "tri_out"),
    (dict(V=-1), INVALID, "n_vertices"),
    (dict(F=-1), INVALID, "n_triangles"),
    (dict(P=4), INVALID, "P"),
    (dict(P=65), INVALID, "P"),
    (dict(C=0), INVALID, "C"),
    (dict(texel0=-1), INVALID, "texel0"),
    (dict(n=-1), INVALID, "n"),
    (dict(texel0=1, n=25), INVALID, "range"),
    (dict(texel0=26, n=0), INVALID, "range"),
    (dict(F=3, n=51), INVALID, "range"),                         # F = 3 at C = 1: 2 squares, 50 texels
    (dict(pos_bytes=299), SCRATCH, "pos_out"),
    (dict(tri_bytes=99), SCRATCH, "tri_out"),
    (dict(F=1 << 31), UNSUPPORTED, "n_triangles"),
    (dict(V=1 << 31), UNSUPPORTED, "n_vertices"),
    (dict(F=(1 << 31) - 1, P=64, C=1, n=0), UNSUPPORTED, "2^31"),
    (dict(F=2_000_000, P=64, C=1000, n=0), UNSUPPORTED, "2^31"),
    (dict(F=2, P=64, C=(1 << 31) - 1, n=0), UNSUPPORTED, "2^31"),
])
def test_atlas_points_argument_errors_come_before_any_launch(kw, code, word):
    from jittor_myc_nerfs_amd import _lib as L
    rc, msg = _points(L.lib(), **kw)
    assert rc == code, (rc, msg)
    assert word in msg and "tvr_mesh_atlas_points" in msg, msg


@pytest.mark.parametrize("kw, code, word", [
    (dict(tri=None), INVALID, "tri"),
    (dict(bary=None), INVALID, "bary"),
    (dict(atlas=None), INVALID, "atlas"),
    (dict(out=None), INVALID, "out"),
    (dict(n_pix=-1), INVALID, "n_pix"),
    (dict(fmt=2), INVALID, "fmt"),
    (dict(fmt=-1), INVALID, "fmt"),
    (dict(P=4), INVALID, "P"),
    (dict(P=65), INVALID, "P"),
    (dict(C=0), INVALID, "C"),
    (dict(F=-1), INVALID, "n_triangles"),
    (dict(Ha=10), INVALID, "Ha"),
    (dict(Wa=10), INVALID, "Wa"),
    (dict(F=3), INVALID, "Ha"),                                  # three triangles at C = 1 make 10 x 5
    (dict(out_bytes=191), SCRATCH, "out"),
    (dict(n_pix=1 << 31), UNSUPPORTED, "n_pix"),
    (dict(F=2_000_000, P=64, C=1000, Ha=64000, Wa=64000), UNSUPPORTED, "2^31"),
])
def test_texture_sample_argument_errors_come_before_any_launch(kw, code, word):
    from jittor_myc_nerfs_amd import _lib as L
    rc, msg = _sample(L.lib(), **kw)
    assert rc == code, (rc, msg)
    assert word in msg and "tvr_mesh_texture_sample" in msg, msg


def test_empty_calls_are_valid_without_a_device():
    """n == 0 and n_pix == 0 launch nothing: they return TVR_OK with arrays that may be NULL"""
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    assert _points(lib, n=0, pos=None, tri=None, pos_bytes=0, tri_bytes=0)[0] == 0
    assert _points(lib, F=0, faces=None, verts=None, V=0, n=0, texel0=25)[0] == 0
    assert _sample(lib, n_pix=0, tri=None, bary=None, out=None, out_bytes=0)[0] == 0


def test_export_is_additive():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    lib = L.lib()
    assert lib.tvr_version() == 141
    assert len(L.SYMBOLS["tvr_mesh_atlas_points"][1]) == 14 and len(L.SYMBOLS["tvr_mesh_texture_sample"][1]) == 13
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tvr.h")).read(), flags=re.S)
    assert re.search(r"#define\s+TVR_MESH_ATLAS_MIN_P\s+5\b", src) and re.search(r"#define\s+TVR_MESH_ATLAS_MAX_P\s+64\b", src)
    for name in ("tvr_mesh_atlas_points", "tvr_mesh_texture_sample"):
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(proto.split(",")) == len(L.SYMBOLS[name][1]), name
    assert not re.search(r"tvr_mesh_atlas_points_scratch_bytes|tvr_mesh_texture_sample_scratch_bytes", src)       # neither needs scratch


# ---- Python side ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_no_cpu_fallback():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    v, f = TC.small_mesh(7)
    with pytest.raises(L.TvrError, match="no CPU fallback"):
        mesh.atlas_points(torch.from_numpy(v), torch.from_numpy(f), 5, 2, 0, 10)
    with pytest.raises(L.TvrError, match="no CPU fallback"):
        mesh.sample_texture(torch.zeros((4, 4), dtype=torch.int32), torch.zeros((4, 4, 3)), torch.zeros((10, 10, 3), dtype=torch.uint8), 5, 2, 7)


def test_argument_parser_and_signatures():
    from jittor_myc_nerfs_amd import TensorBase, reconstruct
    from jittor_myc_nerfs_amd.evaluation import evaluation_mesh
    assert reconstruct.config_parser([]).mesh_texture == 0
    assert reconstruct.config_parser(["--mesh_texture", "8"]).mesh_texture == 8
    assert reconstruct.config_parser(["--render_mesh", "1", "--mesh_file", "x.obj"]).mesh_file == "x.obj"
    sig = inspect.signature(TensorBase.export_mesh).parameters
    assert sig["texture"].default == 0
    assert [sig[k].default for k in ("normals", "colors", "simplify", "smooth", "refine")] == [False, False, 0.0, 0, 0]       # the other defaults are what they were
    bake = inspect.signature(TensorBase.bake_texture).parameters
    assert list(bake)[1:] == ["verts", "faces", "P", "C", "chunk", "half_width", "stats"] and bake["chunk"].default == 1 << 20 and bake["C"].default is None
    ev = inspect.signature(evaluation_mesh).parameters
    assert ev["texture"].default is None and ev["color_psnr"].default is False


def test_mesh_color_psnr_and_summary():
    from jittor_myc_nerfs_amd.evaluation import mesh_agreement_summary, mesh_color_psnr
    img = np.full((2, 2, 3), 128, np.uint8)
    hit = np.array([[True, True], [False, True]])
    acc = np.array([1.0, 0.5, 1.0, 1.0])
    rgb = np.full((4, 3), 128 / 255.0)
    assert mesh_color_psnr(img, hit, rgb, acc) == float("inf")
    rgb[0] += 0.1                                                # pixel 0 counts (hit, solid); pixel 1 (acc 0.5) and pixel 2 (no hit) do not
    rgb[1] += 0.5
    rgb[2] += 0.5
    want = -10 * np.log10(0.01 / 2)
    assert abs(mesh_color_psnr(torch.from_numpy(img), torch.from_numpy(hit), torch.from_numpy(rgb), torch.from_numpy(acc)) - want) < 1e-9
    assert mesh_color_psnr(img, np.zeros((2, 2), bool), rgb, acc) is None
    base = {"iou": 1.0, "depth_median_vox": 0.1, "depth_p95_vox": 0.2, "depth_pixels": 3}
    s = mesh_agreement_summary([dict(base, color_psnr=30.0), dict(base, color_psnr=None), dict(base, color_psnr=20.0)])
    assert s["mean"]["color_psnr"] == 25.0
    assert mesh_agreement_summary([dict(base, color_psnr=None)])["mean"]["color_psnr"] is None
    assert "color_psnr" not in mesh_agreement_summary([base])["mean"]                     # without the option the summary is what it was
