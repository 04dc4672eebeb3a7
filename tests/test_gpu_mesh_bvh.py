"""GPU: the linear BVH and its ray queries (csrc/tvr_mesh_bvh.hip, include/tvr.h tvr_mesh_bvh_*; mesh.build_bvh / cast_rays / ambient_occlusion) — the tree read back
through tvr_mesh_bvh_describe, closest hits against the numpy fp32 restatement (tri and t bit for bit) and the fp64 oracle of tests/mesh_bvh_common.py, watertightness,
the tie and owner rules, the rasteriser on the same camera, ranges and modes, the work the hierarchy saves, ambient occlusion, and export_mesh(ao=) end to end.
The references are computed once per process and shared."""
import numpy as np
import pytest
import torch

import mesh_bvh_common as BC
import mesh_raster_common as RC
from conftest import TINY, make_model

pytestmark = pytest.mark.gpu

N_RAYS = 20000
_cache = {}


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()                       # (a copy: broadcast views are read-only)


def built(name):
    """(verts, faces, MeshBVH, build stats) of a named mesh, built once"""
    from jittor_myc_nerfs_amd import mesh
    if ("bvh", name) not in _cache:
        if name == "mc96":
            vt, ft = RC.mc_sphere("cuda", n=96)
            v, f = _np(vt), _np(ft)
        elif name == "tripled960":
            v, f = BC.tripled(*RC.sphere_fixture("sphere960")[:2])
        else:
            v, f = RC.sphere_fixture(name)[:2]
        st = {}
        _cache[("bvh", name)] = (v, f, mesh.build_bvh(_dev(v), _dev(f, np.int32), stats=st), st)
    return _cache[("bvh", name)]


def ray_set(name, kind):
    """(origins [N,3] or [3], dirs) of a fixture's ray set"""
    v, f = built(name)[:2]
    if kind == "interior":
        return BC.rays_interior(N_RAYS if name != "mc96" else 2048, seed=len(f))
    if kind == "exterior":
        return BC.rays_exterior(N_RAYS if name != "mc96" else 2048, seed=len(f) + 1)
    return BC.edge_midpoint_rays(v, f)[:2]


def refs(name, kind):
    if ("ref", name, kind) not in _cache:
        v, f = built(name)[:2]
        o, d = ray_set(name, kind)
        _cache[("ref", name, kind)] = (o, d, BC.restate(v, f, o, d), BC.oracle(v, f, o, d))
    return _cache[("ref", name, kind)]


def cast(bvh, o, d, **kw):
    from jittor_myc_nerfs_amd import mesh
    o = np.broadcast_to(np.asarray(o, np.float32).reshape(-1, 3), d.shape)
    out = mesh.cast_rays(bvh, _dev(o), _dev(d), **kw)
    return _np(out) if kw.get("any_hit") else tuple(_np(x) for x in out)


# ---- the tree -------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _small(F):
    g = np.random.default_rng(F)
    return g.standard_normal((3 * F, 3)).astype(np.float32), np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def _nan_vertex():
    v, f = RC.sphere_fixture("sphere960")[:2]
    v = v.copy()
    v[17, 1] = np.nan
    return v, f


@pytest.mark.parametrize("name", ["sphere960", "sphere6240", "tripled960", "F1", "F2", "F3", "nan_vertex", "mc96"])
def test_tree_structure_and_determinism(name):
    from jittor_myc_nerfs_amd import mesh
    if name in ("F1", "F2", "F3"):
        v, f = _small(int(name[1]))
    elif name == "nan_vertex":
        v, f = _nan_vertex()
    else:
        v, f = built(name)[:2]
    st = {}
    a = mesh.build_bvh(_dev(v), _dev(f, np.int32), stats=st)
    b = mesh.build_bvh(_dev(v), _dev(f, np.int32))
    assert torch.equal(a.blob, b.blob)                               # two builds are byte-equal
    tree = BC.read_tree(_np(a.blob), a.layout(), len(f))
    height = BC.check_tree(tree, v, f)
    assert height <= 62 and st["height"] == height == a.height
    assert st["triangles_skipped"] == (0 if name != "nan_vertex" else int((f == 17).any(1).sum())) and st["internal_nodes"] == len(f) - 1
    if len(f) >= 960:
        assert height <= 4 * int(np.ceil(np.log2(len(f))))          # a tree, not a list
    print(f"    {name}: F = {len(f)}, height {height}, blob {st['blob_bytes']} B")


def test_empty_mesh():
    from jittor_myc_nerfs_amd import mesh
    bvh = mesh.build_bvh(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    assert bvh.n_triangles == 0 and BC.check_tree(BC.read_tree(_np(bvh.blob), bvh.layout(), 0), np.zeros((0, 3)), np.zeros((0, 3))) == 0
    o, d = BC.rays_exterior(100, 1)
    t, tri, bary = cast(bvh, o, d)
    assert np.isinf(t).all() and (tri == -1).all() and (bary == 0).all()
    assert not cast(bvh, o, d, any_hit=True).any()


def test_unsorted_keys_and_bad_indices_raise_the_flag():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    v, f = RC.sphere_fixture("sphere960")[:2]
    bad = f.copy()
    bad[5, 1] = len(v)
    with pytest.raises(L.TvrError, match="fault flag"):
        mesh.build_bvh(_dev(v), _dev(bad, np.int32))
    lib, F, V = L.lib(), len(f), len(v)
    vd, fd = _dev(v), _dev(f, np.int32)
    scratch = torch.zeros(lib.tvr_mesh_bvh_scratch_bytes(F), dtype=torch.uint8, device="cuda")
    blob = torch.zeros(lib.tvr_mesh_bvh_bytes(F), dtype=torch.uint8, device="cuda")
    keys = torch.zeros(F, dtype=torch.int64, device="cuda")
    for spoil in ("unsorted", "twice"):
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        L.check(lib.tvr_mesh_bvh_keys(vd.data_ptr(), V, fd.data_ptr(), F, keys.data_ptr(), 8 * F, scratch.data_ptr(), scratch.numel(), flag.data_ptr(), None))
        k = keys.clone() if spoil == "unsorted" else torch.sort(keys)[0]
        if spoil == "twice":
            k[7] = (k[7] >> 32 << 32) | (k[6] & 0xFFFFFFFF)          # ascending still, but triangle k[6] is named twice
        L.check(lib.tvr_mesh_bvh_build(vd.data_ptr(), V, fd.data_ptr(), F, k.data_ptr(), blob.data_ptr(), blob.numel(), scratch.data_ptr(), scratch.numel(), None,
                                       flag.data_ptr(), None))
        assert int(flag.item()) == 1, spoil
        # a cast through the refused blob raises the flag too and hits nothing
        bvh = mesh.MeshBVH(blob, vd, fd, 0, 0)
        with pytest.raises(L.TvrError, match="fault flag"):
            mesh.cast_rays(bvh, _dev(np.zeros((4, 3))), _dev(np.ones((4, 3))))


# ---- closest hit against both references ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["interior", "exterior"])
@pytest.mark.parametrize("name", ["sphere960", "sphere6240", "mc96"])
def test_closest_hit_against_restatement_and_oracle(name, kind):
    bvh = built(name)[2]
    o, d, ref, orc = refs(name, kind)
    st = {}
    t, tri, bary = cast(bvh, o, d, stats=st)
    c = BC.compare(t, tri, orc)
    diff = BC.equal_to_restate(t, tri, ref, orc)
    print(f"    {name} {kind}: {c}, bits differing from the restatement {diff}, tests per ray: {st['node_tests'] / len(d):.1f} nodes, {st['triangle_tests'] / len(d):.2f} triangles")
    assert diff == 0                                                 # tri and t bits equal the restatement on every unambiguous ray
    assert c["mask_diff"] == 0 and c["tri_diff"] == 0                # mask and tri equal the oracle on every unambiguous ray
    assert c["ambiguous"] <= 0.005
    assert c["max_rel_t"] <= 1e-5
    same = (tri == ref["tri"]) & (tri >= 0)
    assert np.array_equal(bary[same].view(np.uint32), ref["bary"][same].view(np.uint32))
    assert (bary[tri < 0] == 0).all() and np.isinf(t[tri < 0]).all()
    assert st["rays_hit"] == int((tri >= 0).sum()) and st["rays_refused"] == 0
    if kind == "interior":
        assert (tri >= 0).all()                                      # watertight: from the interior point no ray misses


@pytest.mark.parametrize("name", ["sphere960", "sphere6240"])
def test_no_edge_midpoint_ray_misses(name):
    bvh = built(name)[2]
    o, d, ref, _ = refs(name, "edges")
    t, tri, _ = cast(bvh, o, d)
    print(f"    {name}: {len(d)} edge rays, {int((tri != ref['tri']).sum())} differ from the restatement")
    assert (tri >= 0).all()


# ---- tie and owner rules ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swap_labels", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
def test_quad_diagonal_goes_to_the_owner(swap_labels, reverse):
    from jittor_myc_nerfs_amd import mesh
    v, f, _, diag = RC.exact_quad(swap_labels=swap_labels, reverse=reverse)
    o, d = BC.quad_diagonal_rays()
    t, tri, bary = cast(mesh.build_bvh(_dev(v), _dev(f, np.int32)), o, d)
    inside = np.abs(d[:, 0]) < 2
    assert (tri[inside] == RC.quad_owner(f, v, diag)).all() and (tri[~inside] == -1).all() and (t[inside] == 1.0).all()


def test_coincident_triangles_go_to_the_smallest_index():
    v, f, bvh, _ = built("tripled960")
    for kind in ("interior", "exterior"):
        o, d, ref, orc = refs("sphere960", kind)
        t, tri, _ = cast(bvh, o, d)
        assert (tri < 960).all()                                     # never t + 960 or t + 1920
        assert BC.equal_to_restate(t, tri, ref, orc) == 0            # and what the single sphere gives


# ---- the rasteriser on the same camera ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [False, True])
@pytest.mark.parametrize("name", ["sphere960", "sphere6240"])
def test_agrees_with_the_rasteriser(name, cull):
    from jittor_myc_nerfs_amd import mesh
    v, f, cam = RC.sphere_fixture(name, cull=cull)
    bvh = built(name)[2]
    depth, rtri, _, _ = mesh.render_mesh(_dev(v), _dev(f, np.int32), cam["c2w"], cam["H"], cam["W"], (cam["fx"], cam["fy"]), (cam["cx"], cam["cy"]), near=cam["near"], cull=cull)
    dx, dy = RC.pixel_dirs32(cam)
    dcam = np.stack([dx, dy, np.full_like(dx, -1.0)], -1)
    d = (dcam @ cam["c2w"][:, :3].T).astype(np.float32)              # rays.get_rays: rays_d = directions @ R^T
    t, tri, _ = cast(bvh, cam["c2w"][:, 3], d, cull=cull)
    clear = ~RC.oracle(v, f, cam)["ambiguous"].reshape(-1)
    rtri, depth = _np(rtri).reshape(-1), _np(depth).reshape(-1).astype(np.float64)
    assert clear.mean() > 0.99 and (rtri >= 0).sum() > 500
    assert np.array_equal(tri[clear], rtri[clear])
    both = clear & (tri >= 0)
    rel = np.abs(t[both].astype(np.float64) * np.linalg.norm(d[both].astype(np.float64), axis=1) - depth[both]) / depth[both]
    print(f"    {name} cull={cull}: {int(both.sum())} pixels, depth within {rel.max():.2e} relative")
    assert rel.max() <= 1e-5


# ---- ranges and modes -----------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_range_bounds_any_hit_refusals_and_batching():
    v, f, bvh, _ = built("sphere960")
    o, d, ref, orc = refs("sphere960", "exterior")
    o, d, t0, tri0 = o[:4000], d[:4000], ref["t"][:4000], ref["tri"][:4000]
    t, tri, bary = cast(bvh, o, d)
    assert BC.equal_to_restate(t, tri, dict(t=t0, tri=tri0), dict(ambiguous=orc["ambiguous"][:4000])) == 0
    # one common range: rays whose first hit lies inside it keep it, and exactly those
    lo, hi = np.float32(np.median(t[tri >= 0]) * 0.98), np.float32(np.median(t[tri >= 0]) * 1.02)
    r = BC.restate(v, f, o, d, t_min=lo, t_max=hi)
    t2, tri2, _ = cast(bvh, o, d, t_min=float(lo), t_max=float(hi))
    clear = ~orc["ambiguous"][:4000]
    assert np.array_equal(tri2[clear], r["tri"][clear]) and np.array_equal(t2[clear].view(np.uint32), r["t"][clear].view(np.uint32))
    assert 100 < (tri2 >= 0).sum() < 3900
    # exactly at the bounds: t_max == t keeps the hit, the float below loses it; t_min == t loses it (the far side answers)
    for i in np.flatnonzero((tri >= 0) & clear)[:12]:
        ti = t[i]
        assert cast(bvh, o[i], d[i:i + 1], t_max=float(ti))[0][0] == ti
        assert cast(bvh, o[i], d[i:i + 1], t_max=float(np.nextafter(ti, np.float32(0))))[1][0] == -1
        far = cast(bvh, o[i], d[i:i + 1], t_min=float(ti))
        assert far[0][0] > ti and far[1][0] != tri[i]
    # any hit == isfinite(closest t) on the same range
    for kw in (dict(), dict(t_min=float(lo), t_max=float(hi)), dict(cull=True)):
        tc = cast(bvh, o, d, **kw)[0]
        st = {}
        h = cast(bvh, o, d, any_hit=True, stats=st, **kw)
        assert h.dtype == np.uint8 and np.array_equal(h.astype(bool), np.isfinite(tc)) and st["rays_hit"] == int(h.sum())
    # refused rays are counted and miss
    ob, db = o[:64].copy(), d[:64].copy()
    db[0, 0], db[1, 2], db[2], ob[3, 1], ob[4, 0] = np.nan, np.inf, 0.0, np.nan, -np.inf
    st = {}
    tb, trib, bb = cast(bvh, ob, db, stats=st)
    assert st["rays_refused"] == 5 and (trib[:5] == -1).all() and np.isinf(tb[:5]).all() and (bb[:5] == 0).all()
    assert np.array_equal(trib[5:], tri[5:64])
    st = {}
    assert not cast(bvh, ob, db, any_hit=True, stats=st)[:5].any() and st["rays_refused"] == 5
    # permuted, and split into two calls
    perm = np.random.default_rng(5).permutation(len(d))
    tp, trip, bp = cast(bvh, o[perm], d[perm])
    assert np.array_equal(trip, tri[perm]) and np.array_equal(tp.view(np.uint32), t[perm].view(np.uint32)) and np.array_equal(bp.view(np.uint32), bary[perm].view(np.uint32))
    a, b = cast(bvh, o[:1777], d[:1777]), cast(bvh, o[1777:], d[1777:])
    assert np.array_equal(np.concatenate([a[1], b[1]]), tri) and np.array_equal(np.concatenate([a[0], b[0]]).view(np.uint32), t.view(np.uint32))
    # [N, 6] rows give what two [N, 3] tensors give
    from jittor_myc_nerfs_amd import mesh
    t6, tri6, _ = mesh.cast_rays(bvh, _dev(np.concatenate([o, d], 1)))
    assert np.array_equal(_np(tri6), tri) and np.array_equal(_np(t6).view(np.uint32), t.view(np.uint32))


def test_the_hierarchy_saves_work():
    """A tree that degenerated into a list would pass every correctness test: mean triangle tests per ray must stay below F / 10."""
    v, f, bvh, _ = built("sphere6240")
    o, d = ray_set("sphere6240", "exterior")
    st = {}
    cast(bvh, o, d, stats=st)
    per_ray = st["triangle_tests"] / len(d)
    print(f"    sphere6240 from outside: {per_ray:.2f} triangle tests and {st['node_tests'] / len(d):.1f} node tests per ray (F = {len(f)})")
    assert per_ray < len(f) / 10


# ---- ambient occlusion ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def test_occlusion_of_a_convex_sphere_is_exactly_one():
    from jittor_myc_nerfs_amd import mesh
    v, f, bvh, _ = built("sphere960")
    st = {}
    ao = mesh.ambient_occlusion(bvh, _dev(_unit(v)), n_dirs=64, bias=1e-3, stats=st)
    assert tuple(ao.shape) == (len(v),) and bool((ao == 1.0).all()) and st["rays_hit"] == 0
    assert torch.equal(ao, mesh.ambient_occlusion(bvh, _dev(_unit(v)), n_dirs=64, bias=1e-3))
    n = _unit(v)
    n[3], n[4, 0] = 0.0, np.nan
    assert bool((mesh.ambient_occlusion(bvh, _dev(n))[[3, 4]] == 1.0).all())


def test_occlusion_inside_a_larger_sphere():
    from jittor_myc_nerfs_amd import mesh
    v, f = RC.sphere_fixture("sphere960")[:2]
    v2 = np.concatenate([v, 3 * v]).astype(np.float32)
    f2 = np.concatenate([f, f + len(v)]).astype(np.int32)
    bvh = mesh.build_bvh(_dev(v2), _dev(f2, np.int32))
    p, n = _dev(v), _dev(_unit(v))
    assert bool((mesh.ambient_occlusion(bvh, n, points=p) == 0.0).all())                    # every ray ends on the outer sphere
    assert bool((mesh.ambient_occlusion(bvh, n, points=p, t_max=1.0) == 1.0).all())         # ... which is at least 1.9 away


def test_occlusion_against_the_oracle_on_two_overlapping_mc_spheres():
    from jittor_myc_nerfs_amd import mesh
    vt, ft = RC.mc_sphere("cuda", n=24)
    v, f = _np(vt), _np(ft)
    v2 = np.concatenate([v, v + np.float32([0.9, 0.3, -0.2])]).astype(np.float32)
    f2 = np.concatenate([f, f + len(v)]).astype(np.int32)
    bvh = mesh.build_bvh(_dev(v2), _dev(f2, np.int32))
    sel = np.arange(0, len(v2), 16)
    centre = np.where(sel[:, None] < len(v), np.float32([0.03, -0.02, 0.05]) / np.float32(0.42), np.float32([0.03, -0.02, 0.05]) / np.float32(0.42) + np.float32([0.9, 0.3, -0.2]))
    p, n = v2[sel], _unit(v2[sel] - centre)
    table = BC.fibonacci_sphere(64)
    bias = 0.02
    a = mesh.ambient_occlusion(bvh, _dev(n), points=_dev(p), dirs=_dev(table), bias=bias)
    b = mesh.ambient_occlusion(bvh, _dev(n), points=_dev(p), n_dirs=64, bias=bias)
    assert torch.equal(a, b)                                         # the default table is fibonacci_sphere(n_dirs); two runs are bit-equal
    want, n_amb, wmax = BC.occlusion_oracle(v2, f2, p, n, table, bias)
    err = np.abs(_np(a).astype(np.float64) - want)
    print(f"    {len(sel)} points: AO in {want.min():.3f} .. {want.max():.3f}, largest error {err.max():.2e}, {int(n_amb.sum())} ambiguous rays")
    assert want.min() < 0.7 and want.max() > 0.95                    # the overlap occludes, the far sides are open
    assert (err <= n_amb * wmax + 1e-5).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["vm", "ref"])
def test_export_mesh_with_ambient_occlusion(which, tiny_arrays, tiny_ref_arrays, tmp_path):
    from jittor_myc_nerfs_amd import mesh, synthetic
    hyper = dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=TINY["step_ratio"])
    m = make_model(tiny_arrays if which == "vm" else tiny_ref_arrays, hyper)
    alpha, _ = m.getDenseAlpha()
    level = 0.5 * (float(alpha.min()) + float(alpha.max()))
    plain, zero, shaded = (str(tmp_path / (n + ".ply")) for n in ("plain", "zero", "shaded"))
    m.export_mesh(plain, level=level, spacing="samples", normals=True)
    m.export_mesh(zero, level=level, spacing="samples", normals=True, ao=0)
    assert open(plain, "rb").read() == open(zero, "rb").read()       # ao = 0: the file is byte for byte today's export
    verts, faces = m.export_mesh(shaded, level=level, spacing="samples", ao=32, ao_radius=None)
    st = m.mesh_export_stats
    rv, rf, attrs = mesh.read_ply_attributes(shaded)
    assert "normals" not in attrs and np.array_equal(rf, _np(faces)) and np.array_equal(rv, _np(verts))
    c = attrs["colors"]
    assert c.dtype == np.uint8 and c.shape == (len(rv), 3) and (c[:, 0] == c[:, 1]).all() and (c[:, 1] == c[:, 2]).all()
    assert (c < 255).any() and (c == 255).any()
    assert st["ao_directions"] == 32 and st["ao_t_max"] is None and 0 < st["ao_mean"] <= 1 and st["bvh_height"] <= 62
    near = str(tmp_path / "near.ply")
    m.export_mesh(near, level=level, spacing="samples", normals=True, ao=32, ao_radius=2.0)
    a2 = mesh.read_ply_attributes(near)[2]
    assert "normals" in a2 and (a2["colors"].astype(int) >= c.astype(int)).all()         # shorter rays see no more than longer ones
