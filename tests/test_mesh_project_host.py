"""No GPU: what of the iso-surface projection (include/tvr.h tvr_mesh_project, TensorBase.project_to_isosurface, export_mesh(refine=)) can be checked without one —
iso_feature_target against compute_alpha's formula, the argument checks that come before any launch, the exports, and the restatement of
tests/mesh_project_common.py in fp64 on the scenes the GPU test uses: the Newton iteration AS DEFINED converges for at least 0.95 of the vertices, so the same
condition on the kernel's output (tests/test_gpu_mesh_project.py) asks nothing the definition does not deliver."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import cp_common as CC
import mesh_project_common as PC
from conftest import ROOT, TINY, make_model


def _hyper(**kw):
    from jittor_myc_nerfs_amd import synthetic
    return dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=TINY["step_ratio"], **kw)


# ---- iso_feature_target -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["softplus", "relu"])
def test_iso_feature_target_inverts_compute_alpha(tiny_arrays, act):
    hyper = _hyper()
    hyper["fea2denseAct"] = act
    m = make_model(tiny_arrays, hyper, device="cpu")
    step = float(m.stepSize)
    assert step == PC.step_size(TINY["aabb"], TINY["gridSize"], TINY["step_ratio"])
    for level in (1e-6, 0.0005, 0.005, 0.05, 0.5, 0.999):
        for length in (None, 0.01, 1.0, 37.5):
            ln = step if length is None else length
            t = m.iso_feature_target(level, length)
            assert isinstance(t, float) and math.isfinite(t)
            # compute_alpha's formula in fp64 at the target gives the level back
            # (1 - exp(-x) itself carries an absolute rounding error of 1.1e-16, i.e. 1.1e-16 / level relative: below 1e-12 from level = 1.1e-4 up.  The level
            # 1e-6 is therefore checked through -expm1(-x), the same function without the cancellation.)
            tt = torch.tensor(t, dtype=torch.float64)
            if level >= 1.1e-4:
                back = float(PC.alpha_of_feature(tt, ln, hyper))
            else:
                back = float(-torch.expm1(-(torch.nn.functional.softplus(tt + hyper["density_shift"]) if act == "softplus" else torch.relu(tt)) * ln))
            assert abs(back - level) <= 1e-12 * level, (act, level, length, back)
            assert abs(t - PC.target_feature(level, ln, hyper)) <= 1e-12 * max(1.0, abs(t))
    # a density beyond expm1's range (level -> 1 over a tiny length) still has a finite softplus target
    if act == "softplus":
        assert math.isfinite(m.iso_feature_target(0.999999, 1e-3))
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            m.iso_feature_target(bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            m.iso_feature_target(0.5, bad)


def test_relu_refuses_a_target_that_is_not_positive(tiny_arrays):
    hyper = _hyper()
    hyper["fea2denseAct"] = "relu"
    m = make_model(tiny_arrays, hyper, device="cpu")
    assert m.iso_feature_target(1e-300, 1.0) > 0.0
    with pytest.raises(ValueError, match="relu"):
        m.iso_feature_target(1e-300, 1e300)              # sigma* underflows to 0: relu has no inverse there


# ---- argument validation ------------------------------------------------------------------------------------------------------------------------------------------
def test_python_argument_checks_and_no_cpu_fallback(tiny_arrays, tiny_npp_arrays):
    from jittor_myc_nerfs_amd import _lib as L
    v = torch.zeros((5, 3))
    for m in (make_model(tiny_arrays, _hyper(), device="cpu"), CC.make_cp_model(CC.cp_arrays(5, 50), _hyper(), device="cpu")):
        for kw in (dict(iterations=-1), dict(iterations=65), dict(iterations=2.0), dict(iterations=True), dict(half_width=0.0), dict(half_width=[0.1, 0.1]),
                   dict(half_width=float("nan")), dict(max_move=-1.0), dict(max_move=[0.1, float("inf"), 0.1]), dict(tol=-1e-3), dict(tol=float("nan")),
                   dict(pinned=torch.zeros(4, dtype=torch.bool)), dict(pinned=torch.zeros(5))):
            with pytest.raises(ValueError):
                m.project_to_isosurface(v, 0.05, **kw)
        for level in (0.0, 1.0):
            with pytest.raises(ValueError):
                m.project_to_isosurface(v, level)
        with pytest.raises(ValueError):
            m.project_to_isosurface(torch.zeros((5, 2)), 0.05)
        with pytest.raises(L.TvrError, match="no CPU fallback"):
            m.project_to_isosurface(v, 0.05)
        for bad in (-1, 65, 1.5, True):
            with pytest.raises(ValueError, match="refine"):
                m.export_mesh("never_written.ply", refine=bad)
    npp = make_model(tiny_npp_arrays, _hyper(), device="cpu")
    assert type(npp).__name__ == "NerfPlusPlus"
    with pytest.raises(NotImplementedError, match="NerfPlusPlus"):
        npp.project_to_isosurface(v, 0.05)


def test_c_argument_checks_that_need_no_scene():
    """a NULL scene is refused before anything else is looked at, and nothing is launched (there is no device here to launch on)"""
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    h, mm = (C.c_float * 3)(0.1, 0.1, 0.1), (C.c_float * 3)(0.1, 0.1, 0.1)
    assert lib.tvr_mesh_project(None, None, 0, None, 0.0, 8, C.byref(h), C.byref(mm), 1e-3, None, 0, None, 0, None, 0, None, None) == -1
    assert b"scene" in lib.tvr_last_error()


# ---- exports --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_export_is_additive():
    from jittor_myc_nerfs_amd import _lib as L, reconstruct
    lib = L.lib()
    assert lib.tvr_version() == 141
    assert "tvr_mesh_project" in L.SYMBOLS and getattr(lib, "tvr_mesh_project") is not None and len(L.SYMBOLS["tvr_mesh_project"][1]) == 17
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tvr.h")).read(), flags=re.S)
    assert re.search(r"\btvr_mesh_project\s*\(", src) and re.search(r"#define\s+TVR_MESH_PROJECT_MAX_ITERATIONS\s+64\b", src)
    from jittor_myc_nerfs_amd import TensorBase
    assert TensorBase.PROJECT_MAX_ITERATIONS == 64
    args = reconstruct.config_parser(["--mesh_refine", "8"])
    assert args.mesh_refine == 8 and reconstruct.config_parser([]).mesh_refine == 0


# ---- the definition converges: fp64 restatement -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vm", "cp-16", "cp-5", "cp-96", "cp-1"])
def test_fp64_restatement_converges(tiny_arrays, name):
    kind, arrs = PC.scene(name, tiny_arrays)
    hyper = _hyper()
    f64 = PC.field(kind, arrs, hyper, torch.float64)
    length = PC.step_size(TINY["aabb"], TINY["gridSize"], TINY["step_ratio"])
    for level in PC.LEVELS:
        target = PC.target_feature(level, length, hyper)
        verts = PC.surface_vertices(f64, TINY["aabb"], PC.GRID, level, length, hyper)
        assert verts.shape[0] >= 100, (name, level, verts.shape)          # enough for a share to mean something
        tol = PC.default_tol(target)
        res = PC.project_restatement(f64, verts, TINY["aabb"], target, PC.ITERATIONS, PC.quarter_cell(PC.GRID), PC.units(TINY["aabb"], PC.GRID), tol, torch.float64)
        share = float(res["converged"].double().mean())
        before, after = float(res["residual_in"].abs().median()), float(res["residual_out"].abs().median())
        move = ((res["out"] - verts.double()).abs() / PC.units(TINY["aabb"], PC.GRID).double()).amax(-1)
        print(f"    {name} level {level}: {verts.shape[0]} vertices, f* = {target:.4f}, tol = {tol:.3g}; converged {share:.4f}; median |r| {before:.3g} -> {after:.3g}, "
              f"max |r| before {float(res['residual_in'].abs().max()):.3g}; movement median {float(move.median()):.3g} / max {float(move.max()):.3g} voxel; "
              f"clamped {int(res['clamped'].sum())}, non-finite {int(res['nonfinite'].sum())}")
        assert share >= 0.95
        assert int(res["nonfinite"].sum()) == 0
        # what the definition guarantees per vertex
        assert bool((res["residual_out"].abs() <= res["residual_in"].abs()).all())
        assert bool(((res["out"] - verts.double()).abs() <= PC.units(TINY["aabb"], PC.GRID).double() * (1 + 1e-12)).all())
        assert bool((res["converged"] == (res["residual_out"].abs() <= tol)).all())
