"""GPU (-m gpu): the baked density volume (include/tvr.h, BAKED DENSITY VOLUME) — the bake against an fp64 sum, the march that reads it against the golden
dumps and the oracle within the bounds test_gpu_parity.py holds for the factored march, the invariances that must stay bit for bit while a volume is attached, and
staleness (in-place edits, two streams, a captured render)."""
import numpy as np
import pytest
import torch

from conftest import TINY, make_model
from test_gpu_parity import RGB_TIGHT, _check_dense, _np

pytestmark = pytest.mark.gpu

ODD = dict(gridSize=[5, 7, 9], aabb=TINY["aabb"])          # non-cubic, smaller than a wave's chunk along every axis


def _volume(m):
    """The attached volume as a [gz+1, gy+1, gx+1] fp32 array (after a render: baked)."""
    assert m._dvol is not None, "no density volume attached"
    torch.cuda.synchronize()
    gx, gy, gz = [int(g) for g in m.gridSize]
    return _np(m._dvol.view(torch.float32)).reshape(gz + 1, gy + 1, gx + 1)


def _fp64_volume(m):
    """D[z,y,x] = sum_c P0[c,y,x] L0[c,z] + P1[c,z,x] L1[c,y] + P2[c,z,y] L2[c,x] in fp64 (matMode [[0,1],[0,2],[1,2]], vecMode [2,1,0])."""
    P = [_np(p)[0].astype(np.float64) for p in m.density_plane]
    Ln = [_np(v)[0, :, :, 0].astype(np.float64) for v in m.density_line]
    return (np.einsum("cyx,cz->zyx", P[0], Ln[0]) + np.einsum("czx,cy->zyx", P[1], Ln[1]) + np.einsum("czy,cx->zyx", P[2], Ln[2]))


def _oracle(arrs, hyper, grid, aabb):
    from oracle import c_oracle as CO, tensorf_oracle as TO
    a = dict(arrs, gridSize=np.asarray(grid, np.int32), aabb=np.asarray(aabb, np.float32).reshape(2, 3))
    sc = TO.scene_from_arrays(a, **hyper)
    return CO.COracle(a, step=float(sc.stepSize), **hyper)


def _check_against_oracle(m, orc, rays, S, white_bg=True, jitter=None):
    """One dense eps_T = 0 render with the volume attached against the oracle's dump: test_tiny_dense_bit_exact_indices_and_rgb's bounds."""
    ref = orc.render(_np(rays), S, white_bg=white_bg, jitter=None if jitter is None else _np(jitter), dump=True, nthreads=4)
    rgb, depth, d = m.render_rays(rays, white_bg=white_bg, N_samples=S, jitter=jitter, eps_T=0.0, dense=True)
    assert m._dvol is not None
    names = dict(t_min="tmin", z_vals="z", app_mask="app")
    _check_dense(d, lambda k: ref[names.get(k, k)])
    assert np.abs(_np(d["sigma_feature"]) - ref["sf"] * ref["valid"]).max() < 5e-5
    assert np.abs(_np(rgb) - ref["rgb_map"]).max() < RGB_TIGHT
    return d, ref


@pytest.mark.parametrize("which", ["tiny", "odd"])
def test_bake_equals_the_fp64_sum_to_one_ulp(tiny_arrays, hyper_tiny, tiny_dump, which):
    from jittor_myc_nerfs_amd import synthetic
    if which == "tiny":
        m = make_model(tiny_arrays, hyper_tiny)
    else:
        m = make_model(synthetic.make_scene_arrays(ODD["gridSize"], ODD["aabb"], seed=3), hyper_tiny)
    rays = torch.tensor(tiny_dump["rays"][:16], device="cuda")
    m.render_rays(rays, white_bg=True, N_samples=8)
    got = _volume(m)
    gx, gy, gz = [int(g) for g in m.gridSize]
    assert m._dvol.numel() == 4 * (gx + 1) * (gy + 1) * (gz + 1)
    assert np.isfinite(got).all()                                                      # the padding layer included
    assert not got[gz].any() and not got[:, gy].any() and not got[:, :, gx].any()      # ... which the bake derives from the packed images' zero padding: 0
    want = _fp64_volume(m).astype(np.float32)
    inner = got[:gz, :gy, :gx]
    ulp = np.spacing(np.maximum(np.abs(inner), np.abs(want)))
    worst = float((np.abs(inner.astype(np.float64) - want.astype(np.float64)) / ulp).max())
    print(f"    {which}: {inner.size} voxels, max |D| {np.abs(want).max():.3f}, worst difference {worst:g} ulp, bit-equal {np.array_equal(inner, want)}")
    assert worst <= 1.0


def test_attach_detach_leaves_the_factored_path_alone(tiny_dump, tiny_arrays, hyper_tiny):
    m = make_model(tiny_arrays, hyper_tiny)
    rays = torch.tensor(tiny_dump["rays"], device="cuda")
    S = TINY["N_samples"]

    def render():
        rgb, depth, d = m.render_rays(rays, white_bg=True, N_samples=S, eps_T=0.0, dense=True)
        return rgb, depth, d

    m.density_volume = False
    r1 = render()
    assert m._dvol is None
    m.density_volume = True
    rgb, depth, d = render()
    assert m._dvol is not None
    m.density_volume = False
    r3 = render()
    assert m._dvol is None
    assert torch.equal(r1[0], r3[0]) and torch.equal(r1[1], r3[1]) and all(torch.equal(r1[2][k], r3[2][k]) for k in r1[2])
    # the volume march against the golden dump: the bounds of test_tiny_dense_bit_exact_indices_and_rgb
    _check_dense(d, lambda k: tiny_dump[f"out.{k}"])
    err_sf = np.abs(_np(d["sigma_feature"]) - tiny_dump["out.sigma_feature"]).max()
    err_f = np.abs(_np(r1[2]["sigma_feature"]) - tiny_dump["out.sigma_feature"]).max()
    print(f"    feature against the dump: volume {err_sf:.3g}, factored {err_f:.3g}; weights {np.abs(_np(d['weight']) - tiny_dump['out.weight']).max():.3g}")
    assert err_sf < 5e-5
    assert np.abs(_np(d["alpha"]) - tiny_dump["out.alpha"]).max() < 2e-6
    assert np.abs(_np(d["acc"]) - tiny_dump["out.acc_map"]).max() < 1e-5
    assert np.abs(_np(rgb) - tiny_dump["out.rgb_map"]).max() < RGB_TIGHT
    assert np.abs(_np(depth) - tiny_dump["out.depth_map"]).max() < 1e-4
    # bit for bit what never depended on the density: positions, masks, cells
    for k in ("t_min", "z", "valid", "bbox_valid", "cell"):
        assert torch.equal(d[k], r1[2][k]), k


@pytest.mark.parametrize("name,wb,am,jit", [("wb1_am0", True, False, False), ("wb0_am0", False, False, False),
                                            ("wb1_am1", True, True, False), ("wb0_am1_jit", False, True, True)])
def test_edge_cases_with_the_volume(tiny_edge, tiny_arrays, hyper_tiny, name, wb, am, jit):
    """test_gpu_parity.py::test_edge_cases, asserting that the volume march ran."""
    arrs = dict(tiny_arrays)
    if am:
        arrs["alpha_volume"], arrs["alpha_aabb"] = tiny_edge["alpha_volume"], tiny_edge["alpha_aabb"]
    m = make_model(arrs, hyper_tiny)
    rays = torch.tensor(tiny_edge["rays"], device="cuda")
    jitter = torch.tensor(tiny_edge["jitter"], device="cuda") if jit else None
    g = lambda k: tiny_edge[f"{name}.{k}"]
    for eps in (0.0, None):
        rgb, depth, d = m.render_rays(rays, white_bg=wb, N_samples=TINY["N_samples"], jitter=jitter, eps_T=eps, dense=True)
        assert m._dvol is not None
        if eps == 0.0:
            _check_dense(d, g)
        assert np.abs(_np(rgb) - g("rgb_map")).max() < RGB_TIGHT
        assert np.abs(_np(depth) - g("depth_map")).max() < (1e-4 if eps == 0.0 else 1e-3)
    assert np.allclose(_np(rgb)[3], 1.0 if wb else 0.0) and _np(depth)[3] == tiny_edge["rays"][3, 5]   # ray missing the box


def _face_rays(aabb):
    """Rays that run INSIDE the upper faces of the box (a coordinate stays at aabb.hi for every sample: cell index grid - 1, weight 0, the +1 tap is the padding layer),
    along an upper edge, and through the upper corner."""
    lo, hi = np.asarray(aabb, np.float32)
    r = []
    for k in range(3):                                   # in the upper face of axis k, marching along axis (k + 1) % 3
        a = (k + 1) % 3
        o = 0.3 * hi
        o[k] = hi[k]
        o[a] = lo[a] - 2.5
        dvec = np.zeros(3, np.float32)
        dvec[a] = 1.0
        r.append(np.concatenate([o, dvec]))
    o = hi.copy()
    o[0] = lo[0] - 2.5
    r.append(np.concatenate([o, np.asarray([1, 0, 0], np.float32)]))            # the edge y = hi, z = hi
    dvec = (hi - lo) / np.linalg.norm(hi - lo)
    r.append(np.concatenate([hi - 3.0 * dvec, dvec]))                            # the diagonal, leaving through the upper corner
    return np.stack(r).astype(np.float32)


@pytest.mark.parametrize("which,S", [("tiny", 48), ("tiny", 65), ("odd", 65)])
def test_upper_faces_and_partial_chunks(tiny_arrays, tiny_dump, hyper_tiny, which, S):
    """Samples on the upper faces (f == grid - 1) and N_samples on both sides of a 64-sample chunk, against the oracle's per-sample dump."""
    from jittor_myc_nerfs_amd import synthetic
    arrs = tiny_arrays if which == "tiny" else synthetic.make_scene_arrays(ODD["gridSize"], ODD["aabb"], seed=3)
    grid = TINY["gridSize"] if which == "tiny" else ODD["gridSize"]
    m = make_model(arrs, hyper_tiny)
    orc = _oracle(arrs, hyper_tiny, grid, TINY["aabb"])
    rays = torch.tensor(np.concatenate([_face_rays(TINY["aabb"]), tiny_dump["rays"][:27]]), device="cuda")       # 32 rays: two tiles
    d, ref = _check_against_oracle(m, orc, rays, S)
    cell, valid = _np(d["cell"]), _np(d["valid"]).astype(bool)
    # the z axis of the tiny box is [-1, 1]: (hi - lo) * inv - 1 == 1 exactly in fp32, so ray 2 (in the face z = hi) sits in cell grid_z - 1 with weight 0
    assert valid[2].any() and (cell[2][valid[2]][:, 2] == grid[2] - 1).all()
    assert valid[3].any() and (cell[3][valid[3]][:, 2] == grid[2] - 1).all()
    assert torch.isfinite(d["sigma_feature"]).all() and torch.isfinite(d["weight"]).all()
    # default early termination too, and a jittered call (positions move off the faces' grid lines)
    jit = torch.rand(rays.shape[0], device="cuda", generator=torch.Generator(device="cuda").manual_seed(S))
    rgb, depth = m.render_rays(rays, white_bg=False, N_samples=S, jitter=jit)
    want = orc.render(_np(rays), S, white_bg=False, jitter=_np(jit), nthreads=4)
    assert np.abs(_np(rgb) - want["rgb_map"]).max() < RGB_TIGHT


@pytest.fixture(scope="module")
def scene_b(config1_golden):
    """The 128^3 scene of BASELINE.json configs[0] with ~2000 of its rays and the volume attached; the reference picture is computed once."""
    from jittor_myc_nerfs_amd import synthetic
    B = synthetic.SCENE_B
    arrs = synthetic.make_scene_arrays(B["gridSize"], B["aabb"])
    m = make_model(arrs, dict(synthetic.HYPER, near_far=B["near_far"], step_ratio=B["step_ratio"]))
    m.render_piece_rays = 0
    rays = torch.tensor(config1_golden["rays"][1000:3013], device="cuda")         # 2013 rays: 126 tiles, the last one ragged
    S = B["N_samples"]
    rgb, depth = m.render_rays(rays, white_bg=True, N_samples=S)
    assert m._dvol is not None
    torch.cuda.synchronize()
    return dict(m=m, rays=rays, S=S, rgb=rgb.clone(), depth=depth.clone(), golden=config1_golden["rgb_map"][1000:3013])


def test_invariances_bit_for_bit(scene_b):
    m, rays, S, rgb, depth = (scene_b[k] for k in ("m", "rays", "S", "rgb", "depth"))
    assert np.abs(_np(rgb) - scene_b["golden"]).max() < 3e-4                      # (default early termination: test_config1_against_golden's bound)
    # run to run
    again = m.render_rays(rays, white_bg=True, N_samples=S)
    assert torch.equal(again[0], rgb) and torch.equal(again[1], depth)
    # chunked calls equal the merged call
    parts = [m.render_rays(rays[a:a + 500], white_bg=True, N_samples=S) for a in range(0, rays.shape[0], 500)]
    assert torch.equal(torch.cat([p[0] for p in parts]), rgb) and torch.equal(torch.cat([p[1] for p in parts]), depth)
    # a permutation of the rays gives the permuted image
    perm = torch.randperm(rays.shape[0], device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    rp, dp = m.render_rays(rays[perm].contiguous(), white_bg=True, N_samples=S)
    assert torch.equal(rp, rgb[perm]) and torch.equal(dp, depth[perm])
    # pieces equal one launch set
    m.render_piece_rays = 256                                                     # 2013 rays: 8 pieces on the two library streams
    try:
        pieces = m.render_rays(rays, white_bg=True, N_samples=S)
        assert torch.equal(pieces[0], rgb) and torch.equal(pieces[1], depth)
    finally:
        m.render_piece_rays = 0
    # dense equals non-dense
    rd, dd, d = m.render_rays(rays, white_bg=True, N_samples=S, dense=True)
    assert torch.equal(rd, rgb) and torch.equal(dd, depth)
    # the normal pass runs the same march
    _, acc, depth_n = m.render_normals(rays, N_samples=S)
    assert torch.equal(acc, d["acc"]) and torch.equal(depth_n, depth)
    assert m._dvol is not None


def test_in_place_edit_is_followed(tiny_dump, tiny_arrays, hyper_tiny):
    """test_gpu_parity.py::test_parameter_update_repacks with the volume attached: the render behind an in-place edit re-bakes."""
    m = make_model(tiny_arrays, hyper_tiny)
    rays = torch.tensor(tiny_dump["rays"], device="cuda")
    rgb_a, _ = m(rays, N_samples=48)
    assert m._dvol is not None
    with torch.no_grad():
        for p in m.density_plane:
            p.mul_(0.0)
    rgb_b, _ = m(rays, N_samples=48)
    assert float((rgb_b - 1.0).abs().max()) < 1e-2 and float((rgb_a - rgb_b).abs().max()) > 0.1
    assert not _volume(m).any()                                                   # the volume of an all-zero field
    with torch.no_grad():
        m.density_plane[0].add_(0.25)
    rgb_c, _ = m(rays, N_samples=48)
    want = _fp64_volume(m).astype(np.float32)
    got = _volume(m)[:-1, :-1, :-1]
    assert np.abs(got.astype(np.float64) - want).max() <= np.spacing(np.abs(want).max())
    m.density_volume = False
    rgb_f, _ = m(rays, N_samples=48)
    assert float((rgb_c - rgb_f).abs().max()) < RGB_TIGHT and not torch.equal(rgb_c, rgb_b)


def test_frame_stream_after_an_update(scene_b):
    """An update between submits: the first frame behind it bakes on ITS stream, the next one (the other stream) reads the finished volume — every frame equals the serial
    render made with the parameters of its submit."""
    from jittor_myc_nerfs_amd import FrameStream
    m, rays, S = scene_b["m"], scene_b["rays"], scene_b["S"]
    w0 = [p.detach().clone() for p in m.density_plane]
    try:
        def schedule(render):
            out = []
            for k in range(5):
                if k in (1, 3):
                    with torch.no_grad():
                        m.density_plane[k % 3].mul_(1.0 + 0.1 * k)
                out.append(render())
            return out

        want = schedule(lambda: tuple(t.clone() for t in m.render_rays(rays, white_bg=True, N_samples=S)))
        assert not torch.equal(want[0][0], want[1][0]) and torch.equal(want[1][0], want[2][0]) and not torch.equal(want[2][0], want[3][0])
        with torch.no_grad():
            for p, w in zip(m.density_plane, w0):
                p.copy_(w)
        fs = FrameStream(m, white_bg=True, N_samples=S)
        got = []

        def submit():
            o = fs.submit(rays)
            if o is not None:
                got.append((o[0].clone(), o[1].clone()))

        schedule(submit)
        o = fs.flush()
        got.append((o[0].clone(), o[1].clone()))
        assert len(got) == len(want) and m._dvol is not None
        for k, ((a, b), (c, e)) in enumerate(zip(got, want)):
            assert torch.equal(a, c) and torch.equal(b, e), f"frame {k}"
    finally:
        with torch.no_grad():
            for p, w in zip(m.density_plane, w0):
                p.copy_(w)
        m.render_rays(rays, white_bg=True, N_samples=S)
        torch.cuda.synchronize()


def test_captured_render_replays_bit_equal(scene_b):
    """test_gpu_parity.py::test_render_is_hip_graph_capturable with the volume attached; each of two replays is compared on its own."""
    m, rays, S = scene_b["m"], scene_b["rays"], scene_b["S"]
    eager = m.render_rays(rays, white_bg=True, N_samples=S)
    assert torch.equal(eager[0], scene_b["rgb"]) and torch.equal(eager[1], scene_b["depth"])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.render_rays(rays, white_bg=True, N_samples=S)                          # warm-up on another stream: it waits on the bake's event
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap_rgb, cap_depth = m.render_rays(rays, white_bg=True, N_samples=S)
    assert m._dvol is not None
    for rep in range(2):
        cap_rgb.zero_(); cap_depth.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap_rgb, scene_b["rgb"]) and torch.equal(cap_depth, scene_b["depth"]), f"replay {rep}"
    del g
