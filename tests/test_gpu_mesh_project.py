"""GPU: tvr_mesh_project (csrc/tvr_mesh_project.hip), TensorBase.project_to_isosurface and export_mesh(refine=).

What is asserted is what include/tvr.h promises, and almost all of it is EXACT: the residuals are bit-equal to tvr_density_feature at the returned positions, no
vertex ends with a larger residual than it came with, none leaves its trust box or the aabb, the counters are the counts of the outputs, the result does not depend
on the run or on the vertex order.  The one-step test forms the Newton step in fp64 from tvr_density_gradient's own (f, g) and allows the forward error of the
step's rounded fp32 operations.  The converged share (>= 0.95) is a condition the definition itself meets in fp64 (tests/test_mesh_project_host.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cp_common as CC
import mesh_project_common as PC
from conftest import TINY, make_model

pytestmark = pytest.mark.gpu

SCENES = ["vm", "cp-16", "cp-1", "cp-96"]
FINE = [31, 39, 47]
CASES = [("own", PC.LEVELS[0]), ("own", PC.LEVELS[1]), ("fine", PC.LEVELS[0])]


def _hyper():
    from jittor_myc_nerfs_amd import synthetic
    return dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=TINY["step_ratio"])


def _bits(t):
    return t.contiguous().view(torch.int32)


_models, _verts = {}, {}


def _model(name, tiny_arrays):
    if name not in _models:
        kind, arrs = PC.scene(name, tiny_arrays)
        _models[name] = make_model(arrs, _hyper()) if kind == "vm" else CC.make_cp_model(arrs, _hyper())
    return _models[name]


def _surface(name, m, grid, level):
    """(marching-cubes vertices where the field was sampled, faces, one voxel of that grid [3]); computed once per case and never written to"""
    key = (name, grid, level)
    if key not in _verts:
        from jittor_myc_nerfs_amd import marching_cubes
        gs = PC.GRID if grid == "own" else FINE
        alpha = m.getDenseAlpha(gs)[0]
        aabb = m.aabb.float()
        voxel = (aabb[1] - aabb[0]) / (torch.tensor([float(g) for g in gs]) - 1)
        v, f = marching_cubes(alpha, level, spacing=voxel.tolist(), origin=aabb[0].tolist())
        assert 100 <= v.shape[0] <= 20000, (key, v.shape)            # enough for a share to mean something, small enough to stay quick
        _verts[key] = (v, f, voxel.tolist())
    return _verts[key]


def _project(m, verts, target, iterations, hw, mm, tol, pinned=None, want_in=True):
    """the C call itself: (out, residual_in, residual_out, counts [4] as a list)"""
    from jittor_myc_nerfs_amd import _lib as L
    sc = m._ensure_scene()
    V = verts.shape[0]
    out = torch.full((V, 3), -77.0, device="cuda")
    r_in, r_out = torch.full((V,), -77.0, device="cuda"), torch.full((V,), -77.0, device="cuda")
    counts = torch.full((4,), -5, dtype=torch.int64, device="cuda")
    h3, m3 = (C.c_float * 3)(*hw), (C.c_float * 3)(*mm)
    L.check(L.lib().tvr_mesh_project(sc, verts.data_ptr(), V, None if pinned is None else pinned.data_ptr(), float(target), iterations, C.byref(h3), C.byref(m3),
                                     float(tol), out.data_ptr(), L.nbytes(out), r_in.data_ptr() if want_in else None, L.nbytes(r_in), r_out.data_ptr(),
                                     L.nbytes(r_out), counts.data_ptr(), None), "tvr_mesh_project")
    torch.cuda.synchronize()
    return out, r_in, r_out, counts.tolist()


def _setup(name, tiny_arrays, grid, level):
    m = _model(name, tiny_arrays)
    verts, faces, voxel = _surface(name, m, grid, level)
    target = m.iso_feature_target(level)
    assert abs(target - PC.target_feature(level, float(m.stepSize), _hyper())) <= 1e-12 * abs(target)
    hw = PC.quarter_cell(PC.GRID).tolist()
    return m, verts, faces, voxel, target, hw, PC.default_tol(target)


def _t32(x):
    return torch.tensor(float(x), dtype=torch.float32, device="cuda")


# ---- one step ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_one_step_is_the_newton_step(tiny_arrays, name):
    for grid, level in CASES:
        m, p0, _, voxel, target, hw, tol = _setup(name, tiny_arrays, grid, level)
        f0, g0 = m.compute_density_gradient(m.normalize_coord(p0), half_width=hw)
        r0 = f0 - _t32(target)
        for mm in (voxel, [1e-4 * x for x in voxel]):                              # the export's box, and one so small that nearly every step is clamped
            out, r_in, r_out, counts = _project(m, p0, target, 1, hw, mm, tol)
            assert torch.equal(_bits(r_in), _bits(r0))                               # residual_in: bit-equal to f_0 - f*
            aabb = m.aabb.double().cuda()
            inv, P0, R0 = m.invaabbSize.double().cuda(), p0.double(), r0.double()
            gw = g0.double() * inv
            s = R0 / torch.clamp((gw * gw).sum(-1), min=1e-30)
            delta = -s[:, None] * gw
            mm64 = torch.tensor(mm, dtype=torch.float32).double().cuda()
            q = P0 + delta
            p1 = torch.minimum(torch.maximum(torch.minimum(torch.maximum(q, P0 - mm64), P0 + mm64), aabb[0]), aabb[1])
            stayed = (_bits(out) == _bits(p0)).all(-1)
            bound = 2.0 ** -20 * (delta.abs() + P0.abs())
            stepped = ((out.double() - p1).abs() <= bound).all(-1)
            assert bool((stayed | stepped).all()), f"{int((~(stayed | stepped)).sum())} vertices are neither p_0 nor within the bound of the fp64 step"
            assert torch.equal(_bits(r_out[stayed]), _bits(r0[stayed]))
            at0 = r0.abs() <= _t32(tol)
            assert bool(stayed[at0].all())                                           # converged at k = 0: no step is taken
            assert bool((r_out[~stayed].abs() < r0[~stayed].abs()).all())            # a step is kept only where it is better
            # clamped: decided in fp64 except where q lies within the bound of a face of the box or of the aabb
            lo_b, hi_b = torch.maximum(P0 - mm64, aabb[0]), torch.minimum(P0 + mm64, aabb[1])
            surely = ((q < lo_b - bound) | (q > hi_b + bound)).any(-1) & ~at0
            maybe = ((q < lo_b + bound) | (q > hi_b - bound)).any(-1) & ~at0
            print(f"    {name} {grid} level {level} box {mm[0]:.3g}: {p0.shape[0]} vertices, kept the step {int((~stayed).sum())}, counts {counts}, "
                  f"clamped in fp64 {int(surely.sum())} .. {int(maybe.sum())}")
            assert int(surely.sum()) <= counts[2] <= int(maybe.sum())
            assert counts[0] == int((r_out.abs() <= _t32(tol)).sum()) and counts[1] == int((~stayed).sum()) and counts[3] == 0
        assert counts[2] >= 0.9 * int((~at0).sum())                                  # (the small box did clamp)


# ---- eight steps ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_eight_steps_every_vertex(tiny_arrays, name):
    for grid, level in CASES:
        m, p0, _, voxel, target, hw, tol = _setup(name, tiny_arrays, grid, level)
        out, r_in, r_out, counts = _project(m, p0, target, PC.ITERATIONS, hw, voxel, tol)
        V = p0.shape[0]
        t32 = _t32(target)
        # the residual is the field's value at the result, bit for bit
        assert torch.equal(_bits(r_out), _bits(m.compute_densityfeature(m.normalize_coord(out)) - t32))
        assert torch.equal(_bits(r_in), _bits(m.compute_densityfeature(m.normalize_coord(p0)) - t32))
        # no vertex got worse; it is as good as it was iff it stayed
        stayed = (_bits(out) == _bits(p0)).all(-1)
        assert bool((r_out.abs() <= r_in.abs()).all())
        assert torch.equal(r_out.abs() == r_in.abs(), stayed)
        # the trust box (its rounded fp32 bounds) and the aabb
        mm = torch.tensor(voxel, dtype=torch.float32, device="cuda")
        assert bool((out >= p0 - mm).all()) and bool((out <= p0 + mm).all())
        aabb = m.aabb.float().cuda()
        assert bool((out >= aabb[0]).all()) and bool((out <= aabb[1]).all())
        # the counters are the counts of the outputs
        conv = r_out.abs() <= _t32(tol)
        at0 = r_in.abs() <= _t32(tol)
        assert counts[0] == int(conv.sum()) and counts[1] == int((~stayed).sum()) and counts[3] == 0
        on_box = ((out == p0 - mm) | (out == p0 + mm)).any(-1)
        assert int(on_box.sum()) <= counts[2] <= V - int(at0.sum())                 # a result ON a face of its box was clamped; a vertex converged at k = 0 never steps
        share = counts[0] / V
        move = ((out - p0).abs() / mm).amax(-1)
        print(f"    {name} {grid} level {level}: {V} vertices, converged {share:.4f}, moved {counts[1]}, clamped {counts[2]}; median |r| {float(r_in.abs().median()):.3g} -> "
              f"{float(r_out.abs().median()):.3g}, max |r| {float(r_in.abs().max()):.3g} -> {float(r_out.abs().max()):.3g}; movement median "
              f"{float(move.median()):.3g} / max {float(move.max()):.3g} voxel")
        assert share >= 0.95
        # the Python entry point: the same bits, and its stats
        st = {}
        pv, pr = m.project_to_isosurface(p0, level, iterations=PC.ITERATIONS, max_move=voxel, stats=st)
        assert torch.equal(_bits(pv), _bits(out)) and torch.equal(_bits(pr), _bits(r_out))
        assert st == dict(refine_iterations=8, refine_target_feature=float(np.float32(target)), refine_converged=counts[0], refine_moved=counts[1],
                          refine_clamped=counts[2], refine_nonfinite=0, refine_residual_median_before=float(r_in.abs().median()),
                          refine_residual_median_after=float(r_out.abs().median()))


# ---- behaviour --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vm", "cp-16"])
def test_reproducible_order_free_and_copy_through(tiny_arrays, name):
    m, p0, _, voxel, target, hw, tol = _setup(name, tiny_arrays, "fine", PC.LEVELS[0])
    V = p0.shape[0]
    out, r_in, r_out, counts = _project(m, p0, target, PC.ITERATIONS, hw, voxel, tol)
    out2, r_in2, r_out2, counts2 = _project(m, p0, target, PC.ITERATIONS, hw, voxel, tol)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(r_out), _bits(r_out2)) and torch.equal(_bits(r_in), _bits(r_in2)) and counts == counts2
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(3)).cuda()
    outp, r_inp, r_outp, countsp = _project(m, p0[perm].contiguous(), target, PC.ITERATIONS, hw, voxel, tol)
    assert torch.equal(_bits(outp), _bits(out[perm])) and torch.equal(_bits(r_outp), _bits(r_out[perm])) and countsp == counts
    # batches: 1, a ragged wave, the rest
    for a, b in ((0, 1), (1, 64), (64, V)):
        o, _, r, _ = _project(m, p0[a:b].contiguous(), target, PC.ITERATIONS, hw, voxel, tol)
        assert torch.equal(_bits(o), _bits(out[a:b])) and torch.equal(_bits(r), _bits(r_out[a:b]))
    # residual_in = NULL: the same result
    o, untouched, r, c = _project(m, p0, target, PC.ITERATIONS, hw, voxel, tol, want_in=False)
    assert torch.equal(_bits(o), _bits(out)) and c == counts and bool((untouched == -77.0).all())
    # N = 0 and all-pinned copy through bit for bit; the residual is still the field's
    at0 = int((r_in.abs() <= _t32(tol)).sum())
    o, ri, r, c = _project(m, p0, target, 0, hw, voxel, tol)
    assert torch.equal(_bits(o), _bits(p0)) and torch.equal(_bits(r), _bits(r_in)) and torch.equal(_bits(ri), _bits(r_in)) and c == [at0, 0, 0, 0]
    o, ri, r, c = _project(m, p0, target, PC.ITERATIONS, hw, voxel, tol, pinned=torch.ones(V, dtype=torch.uint8, device="cuda"))
    assert torch.equal(_bits(o), _bits(p0)) and torch.equal(_bits(r), _bits(r_in)) and c == [at0, 0, 0, 0]
    # every other vertex pinned: the pinned stay, the others are what they were
    pin = (torch.arange(V, device="cuda") % 2 == 0)
    o, _, r, _ = _project(m, p0, target, PC.ITERATIONS, hw, voxel, tol, pinned=pin.to(torch.uint8))
    assert torch.equal(_bits(o[pin]), _bits(p0[pin])) and torch.equal(_bits(o[~pin]), _bits(out[~pin])) and torch.equal(_bits(r[~pin]), _bits(r_out[~pin]))
    pv, _ = m.project_to_isosurface(p0, PC.LEVELS[0], max_move=voxel, pinned=pin)
    assert torch.equal(_bits(pv), _bits(o))
    # in place
    buf = p0.clone()
    from jittor_myc_nerfs_amd import _lib as L
    cnt = torch.empty(4, dtype=torch.int64, device="cuda")
    rr = torch.empty(V, device="cuda")
    h3, m3 = (C.c_float * 3)(*hw), (C.c_float * 3)(*voxel)
    L.check(L.lib().tvr_mesh_project(m._ensure_scene(), buf.data_ptr(), V, None, float(target), PC.ITERATIONS, C.byref(h3), C.byref(m3), float(tol), buf.data_ptr(),
                                     L.nbytes(buf), None, 0, rr.data_ptr(), L.nbytes(rr), cnt.data_ptr(), None), "tvr_mesh_project")
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(out)) and cnt.tolist() == counts


@pytest.mark.parametrize("name", ["vm", "cp-16"])
def test_nonfinite_and_zero_gradient_vertices_are_counted_not_faults(tiny_arrays, name):
    m, p0, _, voxel, target, hw, tol = _setup(name, tiny_arrays, "own", PC.LEVELS[0])
    out, _, r_out, counts = _project(m, p0, target, PC.ITERATIONS, hw, voxel, tol)
    nan, inf = float("nan"), float("inf")
    odd = torch.tensor([[nan, 0.0, 0.0], [0.1, inf, 0.2], [0.0, 0.0, -inf], [50.0, 50.0, 50.0], [-1e30, 0.0, 0.0]], device="cuda")
    both = torch.cat((p0[:100], odd, p0[100:])).contiguous()
    o, r_in, r, c = _project(m, both, target, PC.ITERATIONS, hw, voxel, tol)
    keep = torch.ones(both.shape[0], dtype=torch.bool, device="cuda")
    keep[100:105] = False
    assert torch.equal(_bits(o[keep]), _bits(out)) and torch.equal(_bits(r[keep]), _bits(r_out))      # the neighbours are untouched
    # the three non-finite vertices: frozen at p_0, counted
    # (their residual is whatever the field returns there: NaN on a VM scene, whose interpolation weights are NaN, and -f* on a CP scene, whose out-of-range taps
    # have weight zero — in both cases the value of tvr_density_feature at the frozen position)
    assert torch.equal(_bits(o[100:103]), _bits(odd[:3]))
    want = m.compute_densityfeature(m.normalize_coord(o[100:103])) - _t32(target)
    assert torch.equal(torch.isnan(r[100:103]), torch.isnan(want)) and torch.equal(torch.nan_to_num(r[100:103], nan=0.0), torch.nan_to_num(want, nan=0.0))
    assert c[3] == 3
    # far outside the box every tap is padding: f = 0 and g = 0 exactly, so the Newton step is zero and only the clamps move the vertex — the trust box keeps it
    # where it is, the aabb then takes it onto its nearest face (and (50, 50, 50) into the corner), from where the box lets no axis that was clamped move again
    aabb = m.aabb.float().cuda()
    mm = torch.tensor(voxel, device="cuda")
    assert float(r_in[103]) == float(-_t32(target)) and float(r_in[104]) == float(-_t32(target))
    assert bool(torch.isfinite(o[103:105]).all()) and bool(torch.isfinite(r[103:105]).all())
    assert torch.equal(o[103], both[103]) or torch.equal(o[103], aabb[1])
    assert torch.equal(o[104], both[104]) or (float(o[104][0]) == float(aabb[0][0]) and bool((o[104][1:].abs() <= mm[1:]).all()))
    assert bool((r[103:105].abs() <= r_in[103:105].abs()).all())
    # the counters, from the outputs
    assert c[0] == int((r.abs() <= _t32(tol)).sum()) and c[1] == int((_bits(o) != _bits(both)).any(-1).sum())
    assert c[2] == counts[2] + 2                                                     # both far vertices were clamped (into the aabb), no other count changed


def test_empty_input_and_error_codes(tiny_arrays):
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    for name in ("vm", "cp-16"):
        m, p0, _, voxel, target, hw, tol = _setup(name, tiny_arrays, "own", PC.LEVELS[0])
        sc = m._ensure_scene()
        V = 100
        x = p0[:V].contiguous()
        out = torch.full((V, 3), -7.0, device="cuda")
        r_in, r_out = torch.full((V,), -7.0, device="cuda"), torch.full((V,), -7.0, device="cuda")
        counts = torch.full((4,), -5, dtype=torch.int64, device="cuda")

        def call(scene=sc, xp=x.data_ptr(), n=V, tgt=target, it=8, h=hw, mm=voxel, tl=tol, op=out.data_ptr(), ob=None, ip=r_in.data_ptr(), ib=None,
                 rp=r_out.data_ptr(), rb=None, cp=counts.data_ptr()):
            h3 = None if h is None else C.byref((C.c_float * 3)(*h))
            m3 = None if mm is None else C.byref((C.c_float * 3)(*mm))
            return lib.tvr_mesh_project(scene, xp, n, None, float(tgt), it, h3, m3, float(tl), op, L.nbytes(out) if ob is None else ob, ip,
                                        L.nbytes(r_in) if ib is None else ib, rp, L.nbytes(r_out) if rb is None else rb, cp, None)

        INVALID, SCRATCH = -1, -3
        assert call(scene=None) == INVALID and call(xp=None) == INVALID and call(op=None) == INVALID and call(rp=None) == INVALID and call(cp=None) == INVALID
        assert call(n=-1) == INVALID
        assert call(it=-1) == INVALID and call(it=65) == INVALID and b"iterations" in lib.tvr_last_error()
        assert call(h=None) == INVALID and call(mm=None) == INVALID
        for bad in (0.0, -0.1, float("nan"), float("inf")):
            for k in range(3):
                v = list(hw)
                v[k] = bad
                assert call(h=v) == INVALID and b"half_width" in lib.tvr_last_error(), (bad, k)
                v = list(voxel)
                v[k] = bad
                assert call(mm=v) == INVALID and b"max_move" in lib.tvr_last_error(), (bad, k)
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(tgt=bad) == INVALID and b"target_feature" in lib.tvr_last_error()
        assert call(tl=-1e-6) == INVALID and call(tl=float("nan")) == INVALID and b"tol" in lib.tvr_last_error()
        assert call(ob=V * 12 - 4) == SCRATCH and b"verts_out" in lib.tvr_last_error()
        assert call(rb=V * 4 - 4) == SCRATCH and b"residual_out" in lib.tvr_last_error()
        assert call(ib=V * 4 - 4) == SCRATCH and b"residual_in" in lib.tvr_last_error()
        bare, packed = _scene_without_parameters(m)
        assert call(scene=bare) == INVALID and b"tvr_scene_update" in lib.tvr_last_error()
        lib.tvr_scene_destroy(bare)
        del packed
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((r_in == -7.0).all()) and bool((r_out == -7.0).all()) and counts.tolist() == [-5] * 4      # nothing was launched
        # V = 0: success, no kernel; the counters are zeroed by the call
        assert call(n=0) == 0 and call(n=0, xp=None, op=None, ip=None, rp=None) == 0
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((r_out == -7.0).all()) and counts.tolist() == [0, 0, 0, 0]
        e_v, e_r = m.project_to_isosurface(p0[:0], PC.LEVELS[0])
        assert e_v.shape == (0, 3) and e_r.shape == (0,)
        # and the same call with everything right runs
        assert call() == 0
        torch.cuda.synchronize()
        assert not bool((out == -7.0).any()) and not bool((r_out == -7.0).any()) and not bool((r_in == -7.0).any())


def _scene_without_parameters(m):
    """(handle, its packed buffer): a scene of m's shape that tvr_scene_update has not run on — what tvr_scene_create returns"""
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    m._ensure_scene()
    d = m._scene_desc
    packed_bytes, create = (lib.tvr_cp_scene_packed_bytes, lib.tvr_cp_scene_create) if m._cp else (lib.tvr_scene_packed_bytes, lib.tvr_scene_create)
    packed = torch.zeros(packed_bytes(C.byref(d)), dtype=torch.uint8, device="cuda")
    h = C.c_void_p()
    L.check(create(C.byref(d), packed.data_ptr(), packed.numel(), C.byref(h)), "scene create")
    return h, packed


# ---- export_mesh ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vm", "cp-16"])
def test_export_mesh_refine(tiny_arrays, tmp_path, name):
    from jittor_myc_nerfs_amd import read_ply, read_ply_attributes, reconstruct as R
    m = _model(name, tiny_arrays)
    level = PC.LEVELS[0]
    target = m.iso_feature_target(level)
    tol = _t32(PC.default_tol(target))
    for spacing in ("reference", "samples"):
        plain, off, on, sm, nr = [str(tmp_path / f"{name}_{spacing}_{k}.ply") for k in ("plain", "off", "on", "smooth", "normals")]
        pv, pf = m.export_mesh(plain, level=level, spacing=spacing)
        stats_plain = dict(m.mesh_export_stats)
        ov, of = m.export_mesh(off, level=level, spacing=spacing, refine=0)
        assert open(plain, "rb").read() == open(off, "rb").read() and torch.equal(pv, ov) and torch.equal(pf, of)
        assert m.mesh_export_stats == stats_plain and not any(k.startswith("refine_") for k in stats_plain)
        rv, rf = m.export_mesh(on, level=level, spacing=spacing, refine=8)
        st = dict(m.mesh_export_stats)
        assert torch.equal(rf, pf) and rv.shape == pv.shape and not torch.equal(rv, pv)
        v, f = read_ply(on)
        v0, f0 = read_ply(plain)
        assert np.array_equal(f, f0) and np.array_equal(v, rv.cpu().numpy()) and not np.array_equal(v, v0)
        V = v.shape[0]
        for k in ("refine_iterations", "refine_target_feature", "refine_converged", "refine_moved", "refine_clamped", "refine_nonfinite",
                  "refine_residual_median_before", "refine_residual_median_after"):
            assert k in st, k
        assert st["refine_iterations"] == 8 and st["refine_target_feature"] == float(np.float32(target)) and st["refine_nonfinite"] == 0
        assert 0.95 * V <= st["refine_converged"] <= V and 0 < st["refine_moved"] <= V
        # the positions in the file lie on the surface where the field was sampled
        at = m.mesh_sample_positions(torch.from_numpy(v).cuda(), m.gridSize.tolist(), spacing)
        r = m.compute_densityfeature(m.normalize_coord(at)) - _t32(target)
        r_before = m.compute_densityfeature(m.normalize_coord(m.mesh_sample_positions(pv, m.gridSize.tolist(), spacing))) - _t32(target)
        share = float((r.abs() <= tol).double().mean())
        print(f"    {name} / {spacing}: {V} vertices, within tol {float((r_before.abs() <= tol).double().mean()):.4f} -> {share:.4f}, stats {st}")
        assert share >= 0.95
        # after smoothing: the median residual does not grow (per vertex it cannot)
        m.export_mesh(sm, level=level, spacing=spacing, smooth=5, refine=8)
        s2 = dict(m.mesh_export_stats)
        assert s2["smooth_iterations"] == 5 and s2["refine_residual_median_after"] <= s2["refine_residual_median_before"]
        # normals are evaluated at the projected positions
        nv, nf = m.export_mesh(nr, level=level, spacing=spacing, refine=8, normals=True)
        assert torch.equal(nv, rv) and torch.equal(nf, rf)
        v2, f2, attrs = read_ply_attributes(nr)
        voxel = ((m.aabb[1] - m.aabb[0]).float() / (m.gridSize.float() - 1)).tolist()
        proj, _ = m.project_to_isosurface(m.mesh_sample_positions(pv, m.gridSize.tolist(), spacing), level, iterations=8, max_move=voxel)
        assert np.array_equal(v2, v) and np.array_equal(f2, f) and np.array_equal(attrs["normals"], m.surface_normals(proj).cpu().numpy())
        if spacing == "samples":
            assert torch.equal(proj, rv)
    # the command line
    ckpt = tmp_path / f"{name}.th"
    m.save(str(ckpt))
    cls = type(m).__name__
    out = R.main(["--export_mesh", "1", "--ckpt", str(ckpt), "--model_name", cls, "--mesh_level", repr(level), "--mesh_refine", "8"])
    assert open(out, "rb").read() == open(str(tmp_path / f"{name}_reference_on.ply"), "rb").read()
    out = R.main(["--export_mesh", "1", "--ckpt", str(ckpt), "--model_name", cls, "--mesh_level", repr(level)])
    assert open(out, "rb").read() == open(str(tmp_path / f"{name}_reference_plain.ply"), "rb").read()
