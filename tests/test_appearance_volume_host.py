"""CPU: the baked appearance volume's C-ABI surface (include/tvr.h, BAKED APPEARANCE VOLUME) — exports, the size query, the refusals of tvr_scene_set_appearance_volume,
attach / detach on a scene whose parameters are not packed yet (nothing is launched), the host's switch — and the identity the volume rests on, in fp64 on the tiny golden
scene, through the numpy restatement of the record layout that the GPU tests reuse (tests/appearance_volume_common.py)."""
import ctypes as C

import numpy as np
import pytest

import appearance_volume_common as AV
from conftest import TINY
from test_density_volume_host import _aligned, _desc, _scene


def test_exports_present_and_version_unchanged():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    assert lib.tvr_version() == 141
    for name in ("tvr_appearance_volume_bytes", "tvr_scene_set_appearance_volume"):
        assert name in L.SYMBOLS and getattr(lib, name) is not None


@pytest.mark.parametrize("grid", [(300, 300, 300), (5, 7, 9), (2, 2, 2), (64, 3, 4096)])
def test_appearance_volume_bytes(grid):
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    want = 128 * (grid[0] + 1) * (grid[1] + 1) * (grid[2] + 1)
    assert lib.tvr_appearance_volume_bytes(C.byref(_desc(L, grid))) == want == 32 * lib.tvr_density_volume_bytes(C.byref(_desc(L, grid)))
    if grid == (300, 300, 300):
        assert want == 3_490_675_328 < 1 << 32           # the 3.49 GB of the bench scene: below the 32-bit offsets' limit


def test_appearance_volume_bytes_of_a_bad_descriptor_is_zero():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    assert lib.tvr_appearance_volume_bytes(C.byref(_desc(L, (1, 300, 300)))) == 0 and b"grid[0]" in lib.tvr_last_error()
    assert lib.tvr_appearance_volume_bytes(C.byref(_desc(L, (300, 300, 4097)))) == 0 and b"grid[2]" in lib.tvr_last_error()
    assert lib.tvr_appearance_volume_bytes(C.byref(_desc(L, n_app=(49, 48, 48)))) == 0 and b"appearance_n_comp" in lib.tvr_last_error()
    assert lib.tvr_appearance_volume_bytes(None) == 0
    # descriptors whose scenes take no volume: REFTensoRF, more than two encoding frequencies
    d = _desc(L, (5, 7, 9))
    d.variant = 1
    assert lib.tvr_appearance_volume_bytes(C.byref(d)) == 0 and b"REFTensoRF" in lib.tvr_last_error()
    d = _desc(L, (5, 7, 9))
    d.view_pe = d.fea_pe = 6
    assert lib.tvr_appearance_volume_bytes(C.byref(d)) == 0 and b"frequencies" in lib.tvr_last_error()


def test_set_appearance_volume_refusals_and_detach():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    d = _desc(L, (5, 7, 9))
    need = lib.tvr_appearance_volume_bytes(C.byref(d))
    assert need == 128 * 6 * 8 * 10
    keep, buf = _aligned(need)
    assert lib.tvr_scene_set_appearance_volume(None, C.c_void_p(buf), need, None) == -1 and b"scene is NULL" in lib.tvr_last_error()           # TVR_ERR_INVALID
    h, keep_scene = _scene(L, d)
    try:
        for n in (need - 1, 0):                            # too small
            assert lib.tvr_scene_set_appearance_volume(h, C.c_void_p(buf), n, None) == -3                                                    # TVR_ERR_SCRATCH
            assert b"tvr_scene_set_appearance_volume" in lib.tvr_last_error() and str(need).encode() in lib.tvr_last_error()
        for off in (4, 16, 128):                           # misaligned
            assert lib.tvr_scene_set_appearance_volume(h, C.c_void_p(buf + off), need + 256, None) == -3 and b"aligned" in lib.tvr_last_error()
        # a good buffer on a scene whose parameters are not packed yet: attached, nothing launched (the first render bakes); larger than needed is fine
        assert lib.tvr_scene_set_appearance_volume(h, C.c_void_p(buf), need, None) == 0
        assert lib.tvr_scene_set_appearance_volume(h, C.c_void_p(buf), need + 1000, None) == 0
        # a refused call leaves the attached volume alone; detaching twice is fine; the density volume's calls are independent of it
        assert lib.tvr_scene_set_appearance_volume(h, C.c_void_p(buf), need - 1, None) == -3
        assert lib.tvr_scene_set_density_volume(h, None, 0, None) == 0
        assert lib.tvr_scene_set_appearance_volume(h, None, 0, None) == 0
        assert lib.tvr_scene_set_appearance_volume(h, None, 0, None) == 0
        assert lib.tvr_scene_touch(h) == 0
    finally:
        lib.tvr_scene_destroy(h)
    del keep, keep_scene


def test_set_appearance_volume_refuses_cp_ref_six_frequencies_and_4_gib():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    need = 128 * 6 * 8 * 10
    keep, buf = _aligned(need)
    cases = []
    cases.append((_desc(L, (5, 7, 9), n_sigma=(96, 0, 0), n_app=(288, 0, 0)), True, b"CP"))
    d = _desc(L, (5, 7, 9))
    d.variant = 1
    cases.append((d, False, b"REFTensoRF"))
    d = _desc(L, (5, 7, 9))
    d.view_pe = d.fea_pe = 6
    cases.append((d, False, b"frequencies"))
    for d, cp, word in cases:
        h, keep_scene = _scene(L, d, cp=cp)
        try:
            assert lib.tvr_scene_set_appearance_volume(h, C.c_void_p(buf), need, None) == -4 and word in lib.tvr_last_error(), word     # TVR_ERR_UNSUPPORTED
            assert lib.tvr_scene_set_appearance_volume(h, None, 0, None) == 0                                                         # detaching nothing is not an error
        finally:
            lib.tvr_scene_destroy(h)
        del keep_scene
    # 323^3 vertices x 128 B = 4.31e9 B >= 4 GiB: the size query reports it, the attach refuses whatever the buffer claims to hold
    d = _desc(L, (322, 322, 322))
    big = lib.tvr_appearance_volume_bytes(C.byref(d))
    assert big == 128 * 323 ** 3 >= 1 << 32
    h, keep_scene = _scene(L, d)
    try:
        assert lib.tvr_scene_set_appearance_volume(h, C.c_void_p(buf), big, None) == -4 and b"4 GiB" in lib.tvr_last_error()
    finally:
        lib.tvr_scene_destroy(h)
    # the largest cube below the limit is accepted (nothing is dereferenced before the parameters are packed)
    d = _desc(L, (321, 321, 321))
    ok = lib.tvr_appearance_volume_bytes(C.byref(d))
    assert ok == 128 * 322 ** 3 < 1 << 32
    h, keep_scene = _scene(L, d)
    try:
        assert lib.tvr_scene_set_appearance_volume(h, C.c_void_p(buf), ok, None) == 0
    finally:
        lib.tvr_scene_destroy(h)
    del keep


def test_host_switch_defaults():
    from jittor_myc_nerfs_amd import NerfPlusPlus, REFTensoRF, TensorCP, TensorVMSplit
    assert TensorVMSplit.appearance_volume is True
    assert NerfPlusPlus.appearance_volume is False             # opt-in, as its density volume
    assert REFTensoRF._variant == 1 and TensorCP._cp           # never eligible, whatever the switch says (TensorVMSplit._appearance_volume_eligible)


def test_record_order_is_the_render_kernels_lane_order():
    """Segment g (slots 8 g .. 8 g + 7) = rows 4 g .. 4 g + 3 of row block 0, then of row block 1: what lane group g holds behind the basis product."""
    for g in range(4):
        assert [AV.slot_row(8 * g + j) for j in range(8)] == [4 * g, 4 * g + 1, 4 * g + 2, 4 * g + 3, 16 + 4 * g, 17 + 4 * g, 18 + 4 * g, 19 + 4 * g]
    assert sorted(AV.slot_row(s) for s in range(32)) == list(range(32))
    assert sorted(s for s in range(32) if AV.slot_row(s) >= 27) == [23, 28, 29, 30, 31]         # zero in the volume: view direction, unused, constant


def test_the_identity_in_fp64_on_the_tiny_scene(tiny_dump, tiny_arrays):
    """Inside a cell plane(u, v) * line(w) is trilinear and basis_mat is linear without a bias: the trilinear interpolation of the corner features IS the factored
    feature.  fp64 corner values, fp64 interpolation, against the fp64 factored features at the golden dump's appearance positions — through records() / rows_of(),
    so a wrong channel order or axis order of the layout cannot pass.  Bound: both sides are sums of 144 products of magnitude M = sum_k |B_rk| |h_k| evaluated in
    different orders, 2 x 144 x 2^-53 x M each at worst, plus the seven lerps' roundings — 1e-12 M covers it thirtyfold."""
    grid = TINY["gridSize"]
    xyz = tiny_dump["app_xyz_norm"]
    F = AV.corner_features(tiny_arrays)
    assert F.shape == (grid[2], grid[1], grid[0], 27)
    vol = AV.records(F)
    assert vol.shape == (grid[2] + 1, grid[1] + 1, grid[0] + 1, 32)
    assert not vol[grid[2]].any() and not vol[:, grid[1]].any() and not vol[:, :, grid[0]].any() and not vol[..., [23, 28, 29, 30, 31]].any()
    got = AV.rows_of(AV.trilinear(vol, xyz, grid))
    want = AV.factored_features(tiny_arrays, xyz, grid)
    absarrs = {k: np.abs(v) for k, v in tiny_arrays.items()}
    M = AV.factored_features(absarrs, xyz, grid)
    err = np.abs(got - want)
    print(f"    {xyz.shape[0]} positions: max |F| {np.abs(want).max():.3f}, max |volume - factored| {err.max():.3g}, max over M {float((err / M).max()):.3g}")
    assert (err <= 1e-12 * M).all()
    # ... and both are the golden dump's features to its own fp32 precision (the project's bar)
    ref = tiny_dump["app_feature"]
    assert (np.abs(want - ref) <= 1e-4 * np.maximum(1.0, np.abs(ref))).all()
    # an axis swap or a channel permutation of the layout is far outside the bound: the check has teeth
    swapped = AV.rows_of(AV.trilinear(vol, xyz[:, [1, 0, 2]] * np.float32(0.5), grid))
    assert np.abs(swapped - want).max() > 1e-3


def test_basis_as_packed_is_basis_mat_to_22_bits(tiny_arrays):
    """The bake reads basis_mat as the kernel's operands hold it (fp16 hi + lo, truncated): within 2^-21 relative of the fp32 value, or 2^-24 absolute where the lo part
    is an fp16 subnormal."""
    b = tiny_arrays["basis_mat"].astype(np.float64)
    q = AV.basis_as_packed(tiny_arrays["basis_mat"])
    assert (np.abs(q - b) <= np.maximum(np.abs(b) * 2.0 ** -21, 2.0 ** -24)).all() and (np.abs(q) <= np.abs(b)).all()
