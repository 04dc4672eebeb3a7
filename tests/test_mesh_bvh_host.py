"""No GPU: what of the ray queries (include/tvr.h tvr_mesh_bvh_*, mesh.build_bvh / cast_rays / ambient_occlusion / fibonacci_sphere, TensorBase.export_mesh(ao=),
reconstruct --mesh_ao) can be checked without a device: the C calls' argument errors (host pointers that are never followed), the layout query, the parser and the
signatures, and the restatement of the definition (tests/mesh_bvh_common.py) against the fp64 oracle on the fixtures the GPU tests use."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mesh_bvh_common as BC
import mesh_raster_common as RC
from conftest import ROOT

INVALID, SCRATCH, UNSUPPORTED = -1, -3, -4
MAX_F = 1 << 30


def _aligned(n):
    buf = (C.c_uint8 * (n + 256))()
    a = C.addressof(buf)
    return buf, (a + 255) // 256 * 256


def _up(x):
    return (x + 255) // 256 * 256


def _blob_bytes(F):
    return 256 + _up(24 * (2 * F - 1 if F else 0)) + _up(8 * max(F - 1, 0)) + _up(4 * F)


def _scratch_bytes(F):
    return 256 + _up(4 * max(F - 1, 0)) + _up(4 * ((F + 31) // 32))


def _call(lib, fn, **kw):
    keep, p = _aligned(1 << 16)
    F, V, N, M, K = kw.pop("F", 4), kw.pop("V", 6), kw.pop("N", 5), kw.pop("M", 5), kw.pop("K", 8)
    a = dict(verts=p, faces=p, keys=p, keys_bytes=8 * max(F, 0), bvh=p, bvh_bytes=_blob_bytes(max(F, 0)) if F <= 1000 else 1 << 16, scratch=p,
             scratch_bytes=_scratch_bytes(max(F, 0)) if F <= 1000 else 1 << 16, counts=p, flag=p, origins=p, dirs=p, t_min=0.0, t_max=float("inf"), mode=0, cull=0, t=p,
             t_bytes=4 * N, tri=p, tri_bytes=4 * N, bary=p, bary_bytes=12 * N, hit=p, hit_bytes=N, points=p, normals=p, bias=1e-3, out=p, out_bytes=4 * M)
    a.update(kw)
    if fn == "keys":
        rc = lib.tvr_mesh_bvh_keys(a["verts"], V, a["faces"], F, a["keys"], a["keys_bytes"], a["scratch"], a["scratch_bytes"], a["flag"], None)
    elif fn == "build":
        rc = lib.tvr_mesh_bvh_build(a["verts"], V, a["faces"], F, a["keys"], a["bvh"], a["bvh_bytes"], a["scratch"], a["scratch_bytes"], a["counts"], a["flag"], None)
    elif fn == "cast":
        rc = lib.tvr_mesh_bvh_cast(a["verts"], V, a["faces"], F, a["bvh"], a["bvh_bytes"], a["origins"], a["dirs"], N, a["t_min"], a["t_max"], a["mode"], a["cull"],
                                   a["t"], a["t_bytes"], a["tri"], a["tri_bytes"], a["bary"], a["bary_bytes"], a["hit"], a["hit_bytes"], a["counts"], a["flag"], None)
    else:
        rc = lib.tvr_mesh_bvh_occlusion(a["verts"], V, a["faces"], F, a["bvh"], a["bvh_bytes"], a["points"], a["normals"], M, a["dirs"], K, a["bias"], a["t_max"],
                                        a["out"], a["out_bytes"], a["counts"], a["flag"], None)
    return rc, lib.tvr_last_error().decode()


@pytest.mark.parametrize("fn, kw, code, word", [
    ("keys", dict(verts=None), INVALID, "verts"),
    ("keys", dict(faces=None), INVALID, "faces"),
    ("keys", dict(keys=None), INVALID, "keys_out"),
    ("keys", dict(scratch=None), INVALID, "scratch"),
    ("keys", dict(flag=None), INVALID, "fault_flag_dev"),
    ("keys", dict(F=-1), INVALID, "n_triangles"),
    ("keys", dict(V=-1), INVALID, "n_vertices"),
    ("keys", dict(F=MAX_F + 1), UNSUPPORTED, "TVR_MESH_BVH_MAX_TRIANGLES"),
    ("keys", dict(V=1 << 31), UNSUPPORTED, "n_vertices"),
    ("keys", dict(keys_bytes=31), SCRATCH, "keys_out"),
    ("keys", dict(scratch_bytes=_scratch_bytes(4) - 1), SCRATCH, "scratch"),
    ("build", dict(verts=None), INVALID, "verts"),
    ("build", dict(keys=None), INVALID, "sorted_keys"),
    ("build", dict(bvh=None), INVALID, "bvh"),
    ("build", dict(scratch=None), INVALID, "scratch"),
    ("build", dict(flag=None), INVALID, "fault_flag_dev"),
    ("build", dict(F=MAX_F + 1), UNSUPPORTED, "TVR_MESH_BVH_MAX_TRIANGLES"),
    ("build", dict(bvh_bytes=_blob_bytes(4) - 1), SCRATCH, "bvh"),
    ("build", dict(scratch_bytes=_scratch_bytes(4) - 1), SCRATCH, "scratch"),
    ("cast", dict(verts=None), INVALID, "verts"),
    ("cast", dict(bvh=None), INVALID, "bvh"),
    ("cast", dict(origins=None), INVALID, "origins"),
    ("cast", dict(dirs=None), INVALID, "dirs"),
    ("cast", dict(t=None), INVALID, "t / tri / bary"),
    ("cast", dict(tri=None), INVALID, "t / tri / bary"),
    ("cast", dict(bary=None), INVALID, "t / tri / bary"),
    ("cast", dict(mode=1, hit=None), INVALID, "hit"),
    ("cast", dict(flag=None), INVALID, "fault_flag_dev"),
    ("cast", dict(N=-1), INVALID, "n_rays"),
    ("cast", dict(N=1 << 31), UNSUPPORTED, "n_rays"),
    ("cast", dict(mode=2), INVALID, "mode"),
    ("cast", dict(cull=2), INVALID, "cull"),
    ("cast", dict(t_min=float("nan")), INVALID, "t_min"),
    ("cast", dict(t_max=float("nan")), INVALID, "t_max"),
    ("cast", dict(F=MAX_F + 1), UNSUPPORTED, "TVR_MESH_BVH_MAX_TRIANGLES"),
    ("cast", dict(bvh_bytes=_blob_bytes(4) - 1), SCRATCH, "bvh"),
    ("cast", dict(t_bytes=19), SCRATCH, "t [n_rays]"),
    ("cast", dict(tri_bytes=19), SCRATCH, "tri"),
    ("cast", dict(bary_bytes=59), SCRATCH, "bary"),
    ("cast", dict(mode=1, hit_bytes=4), SCRATCH, "hit"),
    ("occlusion", dict(bvh=None), INVALID, "bvh"),
    ("occlusion", dict(points=None), INVALID, "points"),
    ("occlusion", dict(normals=None), INVALID, "normals"),
    ("occlusion", dict(out=None), INVALID, "out"),
    ("occlusion", dict(dirs=None), INVALID, "dirs"),
    ("occlusion", dict(flag=None), INVALID, "fault_flag_dev"),
    ("occlusion", dict(M=-1), INVALID, "n_points"),
    ("occlusion", dict(K=-1), INVALID, "n_dirs"),
    ("occlusion", dict(K=65537), INVALID, "TVR_MESH_BVH_MAX_DIRS"),
    ("occlusion", dict(bias=float("inf")), INVALID, "bias"),
    ("occlusion", dict(t_max=float("nan")), INVALID, "t_max"),
    ("occlusion", dict(out_bytes=19), SCRATCH, "out"),
    ("occlusion", dict(bvh_bytes=_blob_bytes(4) - 1), SCRATCH, "bvh"),
])
def test_c_argument_errors_come_before_any_launch(fn, kw, code, word):
    from jittor_myc_nerfs_amd import _lib as L
    rc, msg = _call(L.lib(), fn, **kw)
    assert rc == code, (rc, msg)
    assert word in msg and "tvr_mesh_bvh_" + fn in msg, msg


def test_misaligned_buffers_are_refused():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    keep, p = _aligned(1 << 16)
    for fn, kw in (("keys", dict(scratch=p + 8)), ("build", dict(scratch=p + 8)), ("build", dict(bvh=p + 128)), ("cast", dict(bvh=p + 4)), ("occlusion", dict(bvh=p + 4)),
                   ("keys", dict(keys=p + 4)), ("build", dict(keys=p + 4))):
        rc, msg = _call(lib, fn, **kw)
        assert rc == INVALID and "aligned" in msg, (fn, kw, rc, msg)


def test_empty_mesh_is_accepted_without_a_launch():
    from jittor_myc_nerfs_amd import _lib as L
    rc, msg = _call(L.lib(), "cast", F=0, N=0, verts=None, faces=None, origins=None, dirs=None, t=None, tri=None, bary=None, counts=None)
    assert rc == 0, msg
    rc, msg = _call(L.lib(), "occlusion", F=0, M=0, verts=None, faces=None, points=None, normals=None, out=None, counts=None)
    assert rc == 0, msg


def test_sizes_and_describe_agree():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    lib = L.lib()
    for F in (0, 1, 2, 3, 960, 6240, 2_700_000, MAX_F):
        assert lib.tvr_mesh_bvh_bytes(F) == _blob_bytes(F)
        assert lib.tvr_mesh_bvh_scratch_bytes(F) == _scratch_bytes(F)
        lay = mesh.bvh_layout(F)
        assert lay["total"] == _blob_bytes(F) and lay["header"] == 0 and lay["boxes"] == 256
        assert lay["children"] == lay["boxes"] + _up(lay["box_stride"] * lay["n_nodes"])
        assert lay["leaf_order"] == lay["children"] + _up(lay["child_stride"] * lay["n_internal"])
        assert lay["total"] == lay["leaf_order"] + _up(lay["leaf_stride"] * F)
        assert (lay["n_nodes"], lay["n_internal"]) == ((2 * F - 1, F - 1) if F else (0, 0))
        assert all(lay[k] % 256 == 0 for k in ("boxes", "children", "leaf_order", "total"))
    for F in (-1, MAX_F + 1):
        assert lib.tvr_mesh_bvh_bytes(F) == 0 and lib.tvr_mesh_bvh_scratch_bytes(F) == 0
        assert lib.tvr_mesh_bvh_describe(F, C.byref(L.MeshBvhLayout())) < 0
    assert lib.tvr_mesh_bvh_describe(4, None) == INVALID
    assert 2 * MAX_F - 1 < 2 ** 31                                   # the limit's reason: every node number fits int32


def test_export_is_additive():
    import jittor_myc_nerfs_amd as pkg
    from jittor_myc_nerfs_amd import _lib as L, mesh
    assert L.lib().tvr_version() == 141
    assert [len(L.SYMBOLS["tvr_mesh_bvh_" + n][1]) for n in ("bytes", "scratch_bytes", "describe", "keys", "build", "cast", "occlusion")] == [1, 1, 2, 10, 12, 24, 18]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tvr.h")).read(), flags=re.S)
    assert re.search(r"#define\s+TVR_MESH_BVH_MAX_TRIANGLES\s+1073741824\b", src) and re.search(r"#define\s+TVR_MESH_BVH_MAX_DIRS\s+65536\b", src)
    assert mesh.BVH_MAX_TRIANGLES == MAX_F and mesh.BVH_MAX_DIRS == 65536
    for name in ("MeshBVH", "build_bvh", "cast_rays", "ambient_occlusion", "fibonacci_sphere"):
        assert getattr(pkg, name) is getattr(mesh, name)


def test_parser_signatures_and_value_errors():
    from jittor_myc_nerfs_amd import TensorBase, mesh, reconstruct
    a = reconstruct.config_parser([])
    assert a.mesh_ao == 0 and a.mesh_ao_radius == 0.0
    a = reconstruct.config_parser(["--mesh_ao", "64", "--mesh_ao_radius", "12.5"])
    assert a.mesh_ao == 64 and a.mesh_ao_radius == 12.5
    sig = inspect.signature(TensorBase.export_mesh).parameters
    assert list(sig)[-2:] == ["ao", "ao_radius"] and sig["ao"].default == 0 and sig["ao_radius"].default is None
    assert [sig[k].default for k in ("level", "gridSize", "spacing", "flip", "normals", "colors", "min_component_faces", "keep_largest", "simplify", "smooth", "refine",
                                     "texture")] == [0.0005, None, "reference", False, False, False, 0, 0, 0.0, 0, 0, 0]
    assert list(inspect.signature(mesh.build_bvh).parameters) == ["verts", "faces", "stats"]
    p = inspect.signature(mesh.cast_rays).parameters
    assert list(p) == ["bvh", "rays_or_origins", "dirs", "t_min", "t_max", "any_hit", "cull", "stats"]
    assert (p["t_min"].default, p["t_max"].default, p["any_hit"].default, p["cull"].default) == (0.0, float("inf"), False, False)
    p = inspect.signature(mesh.ambient_occlusion).parameters
    assert list(p)[:7] == ["bvh", "normals", "n_dirs", "bias", "t_max", "points", "dirs"] and p["n_dirs"].default == 64 and p["t_max"].default == float("inf")


class _Field:
    """export_mesh's argument checks run before the field is touched"""
    PROJECT_MAX_ITERATIONS = 64
    _mesh_simplify_factor = staticmethod(lambda s: float(s))


@pytest.mark.parametrize("kw, word", [(dict(ao=8, colors=True), "colors"), (dict(ao=8, texture=8), "texture"), (dict(ao=-1), "ao"), (dict(ao=65537), "ao"),
                                      (dict(ao=True), "ao"), (dict(ao=2.5), "ao"), (dict(ao=8, ao_radius=0.0), "ao_radius"), (dict(ao=8, ao_radius=float("nan")), "ao_radius")])
def test_export_mesh_refuses_before_anything_runs(kw, word):
    from jittor_myc_nerfs_amd import TensorBase
    with pytest.raises(ValueError, match=word):
        TensorBase.export_mesh.__wrapped__(_Field(), "x.ply", **kw)


def test_no_cpu_fallback():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    v, f = RC.latlong_sphere(4, 6)
    with pytest.raises(L.TvrError, match="no CPU fallback"):
        mesh.build_bvh(torch.from_numpy(v), torch.from_numpy(f))
    bvh = mesh.MeshBVH(torch.zeros(256, dtype=torch.uint8, device="meta"), torch.from_numpy(v), torch.from_numpy(f), 0, 0)
    with pytest.raises(L.TvrError, match="no CPU fallback"):
        mesh.cast_rays(bvh, torch.zeros((4, 6)))
    with pytest.raises(L.TvrError, match="no CPU fallback"):
        mesh.ambient_occlusion(bvh, torch.zeros((len(v), 3)))
    with pytest.raises(L.TvrError, match="MeshBVH"):
        mesh.cast_rays(None, torch.zeros((4, 6)))


def test_fibonacci_sphere():
    from jittor_myc_nerfs_amd import mesh
    for K in (1, 7, 64, 1000):
        d = mesh.fibonacci_sphere(K)
        assert d.dtype == torch.float32 and tuple(d.shape) == (K, 3) and d.device.type == "cpu"
        assert torch.equal(d, mesh.fibonacci_sphere(K))                                    # deterministic
        assert np.array_equal(d.numpy(), BC.fibonacci_sphere(K))                           # the definition
        assert np.abs(np.linalg.norm(d.numpy().astype(np.float64), axis=1) - 1).max() < 2e-7
        if K >= 64:
            assert np.linalg.norm(d.numpy().astype(np.float64).mean(0)) < 1.0 / K           # the mean direction: z cancels exactly in pairs, the spiral's rest is O(1/K)
    with pytest.raises(ValueError):
        mesh.fibonacci_sphere(0)


# ---- the restatement against the oracle: the figures the issue was written with, asserted ---------------------------------------------------------------------------------------
N_RAYS = 20000
_cache = {}


def references(name, kind):
    """(origins, dirs, restate, oracle) of one fixture and ray set, computed once per process"""
    key = (name, kind)
    if key not in _cache:
        v, f, _ = RC.sphere_fixture(name)
        if kind == "interior":
            o, d = BC.rays_interior(N_RAYS, seed=len(f))
        elif kind == "exterior":
            o, d = BC.rays_exterior(N_RAYS, seed=len(f) + 1)
        else:
            o, d, _ = BC.edge_midpoint_rays(v, f)
        _cache[key] = (v, f, o, d, BC.restate(v, f, o, d), BC.oracle(v, f, o, d))
    return _cache[key]


@pytest.mark.parametrize("name", ["sphere960", "sphere6240"])
def test_restatement_agrees_with_the_oracle(name):
    for kind in ("interior", "exterior"):
        v, f, o, d, ref, orc = references(name, kind)
        c = BC.compare(ref["t"], ref["tri"], orc)
        print(f"    {name} {kind}: {c}, hit share {ref['hit'].mean():.3f}")
        assert c["mask_diff"] == 0 and c["tri_diff"] == 0
        assert c["ambiguous"] <= 0.005                               # (0.03 - 0.11 % when the issue was written)
        assert c["max_rel_t"] <= 1e-5                                # (2.6e-7)
        if kind == "interior":
            assert ref["hit"].all()                                  # watertight from inside: no ray finds a pinhole
        else:
            assert 0.05 < 1 - ref["hit"].mean() < 0.2                # "about 10 % miss"
        b = ref["bary"][ref["hit"]]
        assert np.abs(b.sum(1) - 1).max() < 1e-6 and b.min() >= 0


@pytest.mark.parametrize("name", ["sphere960", "sphere6240"])
def test_no_edge_midpoint_ray_finds_a_gap(name):
    v, f, o, d, ref, orc = references(name, "edges")
    assert len(d) == 3 * len(f) // 2 and ref["hit"].all()
    assert orc["ambiguous"].mean() > 0.99                            # they are what the ambiguity rule is about: only the restatement can be asked


def test_quad_diagonal_goes_to_the_owner():
    for swap, rev in ((False, False), (True, False), (False, True), (True, True)):
        v, f, _, diag = RC.exact_quad(swap_labels=swap, reverse=rev)
        o, d = BC.quad_diagonal_rays()
        ref = BC.restate(v, f, o, d)
        inside = np.abs(d[:, 0]) < 2
        assert inside.sum() >= 5
        assert (ref["tri"][inside] == RC.quad_owner(f, v, diag)).all() and (ref["tri"][~inside] == -1).all()
        assert (ref["t"][inside] == 1.0).all()


def test_ranges_refusals_and_cull_of_the_restatement():
    v, f, _ = RC.sphere_fixture("sphere960")
    o, d = BC.rays_exterior(500, seed=3)
    ref = BC.restate(v, f, o, d)
    hit = ref["hit"]
    t0 = ref["t"][hit]
    sel = np.flatnonzero(hit)
    # t_max exactly at the hit keeps it, the float below drops it for the far side; t_min exactly at the hit drops it
    keep = BC.restate(v, f, o[sel], d[sel], t_max=np.inf)
    assert np.array_equal(keep["t"], t0)
    for i in sel[:20]:
        t = ref["t"][i]
        assert BC.restate(v, f, o[i], d[i:i + 1], t_max=t)["t"][0] == t
        assert BC.restate(v, f, o[i], d[i:i + 1], t_max=np.nextafter(t, np.float32(0)))["tri"][0] == -1
        assert BC.restate(v, f, o[i], d[i:i + 1], t_min=t)["t"][0] > t                      # the far side of the sphere
    culled = BC.restate(v, f, o, d, cull=True)
    assert np.array_equal(culled["tri"], ref["tri"])                 # from outside the nearest hit faces the ray
    oi, di = BC.rays_interior(200, seed=4)
    assert not BC.restate(v, f, oi, di, cull=True)["hit"].any()      # from inside every triangle faces away
    bad = d[:6].copy()
    bad[0, 0], bad[1, 1], bad[2] = np.nan, np.inf, 0.0
    ob = o[:6].copy()
    ob[3, 2] = np.nan
    r = BC.restate(v, f, ob, bad)
    assert (r["tri"][:4] == -1).all() and BC.refused(ob, bad).tolist() == [True, True, True, True, False, False]


def test_the_comparison_can_fail():
    """The power of the bar: a reference that pretends one triangle of the sphere is absent must fail the comparison with the oracle."""
    v, f, o, d, ref, orc = references("sphere960", "interior")
    victim = int(np.bincount(ref["tri"][ref["hit"]]).argmax())
    broken = BC.restate(v, f, o, d, drop_triangle=victim)
    c = BC.compare(broken["t"], broken["tri"], orc)
    print(f"    without triangle {victim}: {c}")
    assert c["mask_diff"] + c["tri_diff"] > 0
    assert BC.equal_to_restate(broken["t"], broken["tri"], ref, orc) > 0


def test_occlusion_restatement_on_the_convex_sphere():
    v, f, _ = RC.sphere_fixture("sphere960")
    n = v / np.linalg.norm(v, axis=1, keepdims=True)
    sel = np.arange(0, len(v), 37)
    ao, amb, _ = BC.occlusion_oracle(v, f, v[sel], n[sel], BC.fibonacci_sphere(64), 1e-3)
    assert (ao == 1.0).all() and amb.sum() == 0
