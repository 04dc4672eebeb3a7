"""CPU: the baked density volume's C-ABI surface (include/tvr.h, BAKED DENSITY VOLUME) — the size query, the refusals of tvr_scene_set_density_volume, attach / detach on a
scene whose parameters are not packed yet (nothing is launched), the exports — and the host's switch."""
import ctypes as C

import numpy as np
import pytest


def _desc(L, grid=(300, 300, 300), n_sigma=(16, 16, 16), n_app=(48, 48, 48)):
    d = L.SceneDesc()
    d.grid[:] = list(grid)
    d.aabb[:] = [-1.5] * 3 + [1.5] * 3
    d.inv_aabb_size[:] = [2.0 / 3.0] * 3
    d.density_n_comp[:] = list(n_sigma)
    d.app_n_comp[:] = list(n_app)
    d.app_dim, d.featureC, d.view_pe, d.fea_pe, d.step_size, d.variant = 27, 128, 2, 2, 0.005, 0
    return d


def _aligned(nbytes, align=256):
    """(keep-alive array, address): host memory standing in for a device buffer — the calls under test only look at the address and the size."""
    a = np.zeros(nbytes + align, np.uint8)
    addr = (a.ctypes.data + align - 1) // align * align
    return a, addr


def _scene(L, d, cp=False):
    lib = L.lib()
    n = (lib.tvr_cp_scene_packed_bytes if cp else lib.tvr_scene_packed_bytes)(C.byref(d))
    assert n > 0, lib.tvr_last_error()
    keep, addr = _aligned(256)                        # never dereferenced on the host: tvr_scene_create stores pointers into it
    h = C.c_void_p()
    rc = (lib.tvr_cp_scene_create if cp else lib.tvr_scene_create)(C.byref(d), C.c_void_p(addr), n, C.byref(h))
    assert rc == 0, lib.tvr_last_error()
    return h, keep


def test_exports_present_and_version_unchanged():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    assert lib.tvr_version() == 141
    for name in ("tvr_density_volume_bytes", "tvr_scene_set_density_volume"):
        assert name in L.SYMBOLS and getattr(lib, name) is not None


@pytest.mark.parametrize("grid", [(300, 300, 300), (5, 7, 9), (2, 2, 2), (64, 3, 4096)])
def test_density_volume_bytes(grid):
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    want = 4 * (grid[0] + 1) * (grid[1] + 1) * (grid[2] + 1)
    assert lib.tvr_density_volume_bytes(C.byref(_desc(L, grid))) == want
    if grid == (300, 300, 300):
        assert want == 109_083_604                    # the 109 MB of the bench scene


def test_density_volume_bytes_of_a_bad_descriptor_is_zero():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    assert lib.tvr_density_volume_bytes(C.byref(_desc(L, (1, 300, 300)))) == 0 and b"grid[0]" in lib.tvr_last_error()
    assert lib.tvr_density_volume_bytes(C.byref(_desc(L, (300, 300, 4097)))) == 0 and b"grid[2]" in lib.tvr_last_error()
    assert lib.tvr_density_volume_bytes(C.byref(_desc(L, n_sigma=(17, 16, 16)))) == 0 and b"density_n_comp" in lib.tvr_last_error()
    assert lib.tvr_density_volume_bytes(None) == 0


def test_set_density_volume_refusals_and_detach():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    d = _desc(L, (5, 7, 9))
    need = lib.tvr_density_volume_bytes(C.byref(d))
    assert need == 4 * 6 * 8 * 10
    keep, buf = _aligned(need)
    # NULL scene
    assert lib.tvr_scene_set_density_volume(None, C.c_void_p(buf), need, None) == -1 and b"scene is NULL" in lib.tvr_last_error()           # TVR_ERR_INVALID
    h, keep_scene = _scene(L, d)
    try:
        # too small (by one byte, and zero)
        for n in (need - 1, 0):
            assert lib.tvr_scene_set_density_volume(h, C.c_void_p(buf), n, None) == -3                                                    # TVR_ERR_SCRATCH
            assert b"tvr_scene_set_density_volume" in lib.tvr_last_error() and str(need).encode() in lib.tvr_last_error()
        # misaligned
        for off in (4, 16, 128):
            assert lib.tvr_scene_set_density_volume(h, C.c_void_p(buf + off), need + 256, None) == -3 and b"aligned" in lib.tvr_last_error()
        # a good buffer on a scene whose parameters are not packed yet: attached, nothing launched (the first render bakes); larger than needed is fine
        assert lib.tvr_scene_set_density_volume(h, C.c_void_p(buf), need, None) == 0
        assert lib.tvr_scene_set_density_volume(h, C.c_void_p(buf), need + 1000, None) == 0
        # a refused call leaves the attached volume alone and detaching twice is fine
        assert lib.tvr_scene_set_density_volume(h, C.c_void_p(buf), need - 1, None) == -3
        assert lib.tvr_scene_set_density_volume(h, None, 0, None) == 0
        assert lib.tvr_scene_set_density_volume(h, None, 0, None) == 0
        assert lib.tvr_scene_touch(h) == 0                 # marks the (detached) volume stale too: host only
    finally:
        lib.tvr_scene_destroy(h)
    del keep, keep_scene


def test_set_density_volume_refuses_a_cp_scene():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    d = _desc(L, (5, 7, 9), n_sigma=(96, 0, 0), n_app=(288, 0, 0))
    h, keep_scene = _scene(L, d, cp=True)
    try:
        keep, buf = _aligned(4 * 6 * 8 * 10)
        assert lib.tvr_scene_set_density_volume(h, C.c_void_p(buf), 4 * 6 * 8 * 10, None) == -4 and b"CP" in lib.tvr_last_error()           # TVR_ERR_UNSUPPORTED
        assert lib.tvr_scene_set_density_volume(h, None, 0, None) == 0                                                                  # detaching nothing is not an error
    finally:
        lib.tvr_scene_destroy(h)
    del keep_scene


def test_host_switch_defaults():
    from jittor_myc_nerfs_amd import NerfPlusPlus, REFTensoRF, TensorCP, TensorVMSplit
    assert TensorVMSplit.density_volume is True and REFTensoRF.density_volume is True
    assert NerfPlusPlus.density_volume is False                # explicit-depth march: factored
    assert TensorCP._cp and TensorVMSplit.DENSITY_VOLUME_MEMORY_SHARE == 4
