"""No GPU: the references of tests/ngp_geom_common.py checked against themselves, the inputs of the GPU tests checked for power, and the host side of
tvr_ngp_density_gradient / tvr_ngp_density_grid (exports, argument checks before any launch)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import ngp_geom_common as K  # noqa: E402

OK, INVALID, UNSUPPORTED, ERR_HIP = 0, -1, -4, -2
P = 1 << 20                                                                   # a fabricated, 256-byte aligned pointer: refused calls never dereference it


def test_status_codes_are_the_headers():
    text = open(os.path.join(ROOT, "include", "tvr.h")).read()
    for name, value in (("TVR_ERR_INVALID", INVALID), ("TVR_ERR_UNSUPPORTED", UNSUPPORTED), ("TVR_ERR_HIP", ERR_HIP)):
        assert f"{name} = {value}" in text.replace("  ", " "), name


def test_gradient_matches_differences_of_the_value(ngp_scene):
    """The fp64 reference's gradient against central differences of the fp64 reference's value, step 2^-10 / scale_max per side.  Only points whose two neighbours
    stay in the same cell at every level and keep the same ReLU pattern are compared: there raw is linear along the axis, so the difference quotient IS the derivative.
    The reference takes its fractions from fp32 positions and the fp32 fma (as the kernel does), so the step a level really sees is the difference of its fp32
    fractions, a few ulps of x at the finest level and not 2 * step * scale; the identity checked is therefore the one in those fractions,
        raw(p+) - raw(p-) = sum_l sum_c g_enc[2l+c] * (J[2l+c, k] / scale_l) * (f+[l,k] - f-[l,k]),
    which holds to fp64 rounding.  It ties the Jacobian (corner sums with one factor replaced by +-1) to the value's own trilinear blend, level by level."""
    levels, arrs = ngp_scene
    pos = K.sample_positions(4096, edges=False)
    scale = np.asarray(levels["scale"], np.float64)
    step = np.float32(2.0 ** -10 / scale.max())
    ref = K.density_gradient_ref(arrs, levels, pos, torch.float64)
    cells, pattern = K.cell_and_pattern(arrs, levels, pos)
    _, f0, _ = K.hash_geometry(levels, torch.as_tensor(pos))
    kept = 0
    for k in range(3):
        plus, minus = pos.copy(), pos.copy()
        plus[:, k] += step
        minus[:, k] -= step
        cp, pp = K.cell_and_pattern(arrs, levels, plus)
        cm, pm = K.cell_and_pattern(arrs, levels, minus)
        keep = (cp == cells).all((1, 2)) & (cm == cells).all((1, 2)) & (pp == pattern).all(1) & (pm == pattern).all(1)
        rp = K.density_gradient_ref(arrs, levels, plus, torch.float64)["raw"]
        rm = K.density_gradient_ref(arrs, levels, minus, torch.float64)["raw"]
        fp = K.hash_geometry(levels, torch.as_tensor(plus))[1].double().numpy()[:, :, k]
        fm = K.hash_geometry(levels, torch.as_tensor(minus))[1].double().numpy()[:, :, k]
        terms = ref["g_enc"] * ref["J"][:, :, k] * np.repeat((fp - fm) / scale[None, :], 2, axis=1)
        want, size = terms.sum(1), np.abs(terms).sum(1)
        err = np.abs((rp - rm) - want)
        bound = 1e-9 * size + 1e-12 * (np.abs(rp) + np.abs(rm))
        assert keep.mean() >= 0.5, f"axis {k}: only {keep.mean():.3f} of the points keep their cell and ReLU pattern"
        assert (err[keep] <= bound[keep]).all(), f"axis {k}: worst excess {float((err[keep] / bound[keep]).max()):.3e}"
        assert size[keep].min() > 0
        kept += int(keep.sum())
    assert kept >= 3 * 2048


@pytest.mark.parametrize("aabb_scale, n, gain", K.GRADIENT_CASES)
def test_relu_margin_cap_and_yardstick(ngp_scene, aabb_scale, n, gain):
    """The filter the GPU test applies keeps at least 99 % of its points on every scene, and the fp32 restatement's own scaled error (the yardstick the GPU bar is four
    times of) is small and not zero: printed for DESIGN.md 10.3.  grid_levels(16) ends at scale 2048 * 16 - 1 = 32767 (the library refuses scales above 65000), where
    the U(-1, 1) table's tangents stay just below the fp16 split's 65504; the third case multiplies the table by 4 so that they pass twice that bound."""
    levels, arrs = K.gradient_scene(ngp_scene, aabb_scale, gain)
    pos = K.sample_positions(n)
    ref = K.density_gradient_ref(arrs, levels, pos, torch.float64)
    keep = K.relu_margin_ok(ref)
    excluded = 1.0 - keep.mean()
    y = K.scaled_error(K.density_gradient_ref(arrs, levels, pos, torch.float32)["grad"], ref, keep)
    tangent = np.abs(ref["J"]).reshape(len(pos), -1).max(1)
    print(f"aabb_scale {aabb_scale} gain {gain}: {len(pos)} points, excluded {excluded:.4%}, fp32 yardstick worst scaled error {y:.3e}, "
          f"scale_max {float(max(levels['scale'])):.0f}, largest tangent {tangent.max():.0f}, points with a tangent > 65504: {(tangent > 65504).mean():.2%}")
    assert excluded <= K.MARGIN_CAP
    assert 0 < y < 1e-5
    assert np.isfinite(ref["grad"]).all() and (ref["S"][keep] > 0).all()
    if gain > 1:
        assert tangent.max() > 2 * 65504 and (tangent > 65504).mean() > 0.5  # the kernel's range argument is exercised


def test_sphere_scene_zero_set():
    """sphere_scene's fp64 field changes sign within sqrt(3) / scale of the sphere along 256 rays from the centre (a convex combination of a 1-Lipschitz function's
    values over a cell of diagonal sqrt(3) / scale is within that of the function)."""
    from oracle import ngp_oracle as N
    levels = N.grid_levels(4)
    R, k = 0.2, 40.0
    arrs = K.sphere_scene(levels, R, k)
    l, scale, res = K.sphere_level(levels)
    assert (l, res) == (3, 56) and abs(scale - 54.7) < 0.1
    rng = np.random.default_rng(5)
    d = rng.normal(size=(256, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    lo, hi = np.full(256, 0.05), np.full(256, 0.4)

    def raw_at(r):
        return K.density_gradient_ref(arrs, levels, (0.5 + r[:, None] * d).astype(np.float32), torch.float64)["raw"]
    assert (raw_at(lo) > 0).all() and (raw_at(hi) < 0).all()
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        inside = raw_at(mid) > 0
        lo, hi = np.where(inside, mid, lo), np.where(inside, hi, mid)
    root = 0.5 * (lo + hi)
    assert np.abs(root - R).max() <= math.sqrt(3.0) / scale, float(np.abs(root - R).max())
    # raw = k * interpolant: the value at the centre is k * (about R)
    assert abs(raw_at(np.zeros(256))[0] - k * R) <= k * math.sqrt(3.0) / scale


# ---------------------------------------------------------------------------------------------------------------- the built library
def _lib():
    from jittor_myc_nerfs_amd import _lib as L
    return L


def _cfg(aabb_scale=4):
    from jittor_myc_nerfs_amd import ngp
    offsets, scale, _ = ngp.grid_levels(aabb_scale)
    return ngp._grid_cfg(offsets, scale)


def _f3(*v):
    return (C.c_float * 3)(*v)


def _i3(*v):
    return (C.c_int32 * 3)(*v)


def test_exports_resolve():
    L = _lib()
    lib = L.lib()
    for name, n_args in (("tvr_ngp_density_gradient", 10), ("tvr_ngp_density_grid", 12)):
        assert hasattr(lib, name), name
        res, args = L.SYMBOLS[name]
        assert res is C.c_int and len(args) == n_args, name
    header = open(os.path.join(ROOT, "include", "tvr_ngp.h")).read()
    for name, n_args in (("tvr_ngp_density_gradient", 10), ("tvr_ngp_density_grid", 12)):
        decl = header[header.index(f"int {name}("):]
        assert decl[:decl.index(");")].count(",") + 1 == n_args, name


def test_density_gradient_argument_checks():
    lib = _lib().lib()
    cfg = _cfg()
    g = lib.tvr_ngp_density_gradient
    assert g(None, P, P, P, 3, 4, None, P, P, None) == INVALID and b"cfg" in lib.tvr_last_error()
    assert g(C.byref(cfg), None, P, P, 3, 4, None, P, P, None) == INVALID
    assert g(C.byref(cfg), P, None, P, 3, 4, None, P, P, None) == INVALID
    assert g(C.byref(cfg), P, P, None, 3, 4, None, P, P, None) == INVALID
    assert g(C.byref(cfg), P, P, P, 3, 4, None, P, None, None) == INVALID                       # grad_out is required, raw_out is not
    assert g(C.byref(cfg), P, P, P, 2, 4, None, P, P, None) == INVALID and b"pos_stride" in lib.tvr_last_error()
    assert g(C.byref(cfg), P, P, P, 3, -4, None, P, P, None) == INVALID
    assert g(C.byref(cfg), P, P + 4, P, 3, 4, None, P, P, None) == INVALID                      # misaligned weight image
    assert g(C.byref(cfg), P, P, P, 3, 0, None, None, None, None) == OK                         # nothing to do: no launch
    bad = _cfg()
    bad.scale[3] = 0.0
    assert g(C.byref(bad), P, P, P, 3, 4, None, P, P, None) == INVALID
    bad = _cfg()
    bad.offsets[9] = bad.offsets[8] + 1000                                                      # a hashed level whose table is no power of two
    assert g(C.byref(bad), P, P, P, 3, 4, None, P, P, None) in (INVALID, UNSUPPORTED)


def test_density_grid_argument_checks():
    lib = _lib().lib()
    cfg = _cfg()
    g = lib.tvr_ngp_density_grid
    lo, hi, org, sp, dims = _f3(-1.5, -1.5, -1.5), _f3(2.5, 2.5, 2.5), _f3(0, 0, 0), _f3(0.1, 0.1, 0.1), _i3(8, 8, 8)

    def call(cfg_=cfg, grid=P, net=P, bits=P, lo_=lo, hi_=hi, dims_=dims, org_=org, sp_=sp, out=P):
        return g(None if cfg_ is None else C.byref(cfg_), grid, net, bits, lo_, hi_, dims_, org_, sp_, -1e4, out, None)
    assert call(cfg_=None) == INVALID
    assert call(grid=None) == INVALID
    assert call(net=None) == INVALID
    assert call(net=P + 4) == INVALID
    assert call(out=None) == INVALID
    assert call(dims_=None) == INVALID and call(org_=None) == INVALID and call(sp_=None) == INVALID
    for d in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8), (8, 8, -2 ** 31)):
        assert call(dims_=_i3(*d)) == INVALID and b"dims" in lib.tvr_last_error(), d
    for d in ((2 ** 31 - 1, 2, 1), (1 << 16, 1 << 15, 2), (1291, 1291, 1291)):                  # beyond 2^31 points
        assert call(dims_=_i3(*d)) == UNSUPPORTED and b"2^31" in lib.tvr_last_error(), d
    assert call(sp_=_f3(0.1, float("nan"), 0.1)) == INVALID and call(org_=_f3(float("inf"), 0, 0)) == INVALID
    assert call(lo_=None) == INVALID and call(hi_=None) == INVALID                              # a bitfield needs the box
    assert call(lo_=_f3(2.5, -1.5, -1.5)) == INVALID                                            # hi <= lo
    # (every case above is refused before the launch: the fabricated pointers are never handed to a kernel)
