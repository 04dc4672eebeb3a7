"""CPU: what of TensorCP's training path can be checked without a GPU — the float64 reference of tests/cp_train_common.py (gradcheck; the power of the 5e-4 bar
against four deliberate defects on the inputs the GPU tests use), the new C-ABI entry points' declarations, exports and refusals, and the opt-in switches' defaults."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import cp_common as CC
import cp_train_common as T
import march_backward_common as MB
from conftest import ROOT

NEW_CALLS = ("tvr_cp_grad_scratch_bytes", "tvr_cp_march_forward", "tvr_cp_march_backward", "tvr_cp_app_backward")


@pytest.mark.parametrize("r", [(1, 1), (5, 50)])
def test_reference_passes_gradcheck(r):
    """the reference's autograd on a handful of rays: march (density lines) and features (appearance lines, basis_mat)"""
    full = T.cp_case(r)
    idx = np.nonzero(full.ref()["app"].any(1).numpy())[0]                                      # rays with appearance samples
    pick = idx[np.linspace(0, len(idx) - 1, 5).astype(int)]
    small = T.CpCase(full.arrs, full.hyper, full.rays[pick], full.S, full.eps_T, seed=3)
    assert small.n >= 3 and int(small.ref()["app"].sum()) > 0

    def march_loss(*lines):
        m = T.march64(small, list(lines))
        return (m["app"] * MB.g_of(m["xyz"]) * m["w"]).sum() + (small.a * m["acc"]).sum()

    assert torch.autograd.gradcheck(march_loss, T.leaves_of(small.arrs, T.DENSITY_NAMES), eps=1e-6, atol=1e-7, rtol=1e-5)
    xyz = torch.tensor(T.app_points("random", 6, seed=r[0])).double()
    G = torch.tensor(np.random.default_rng(5).standard_normal((6, 27)))
    assert torch.autograd.gradcheck(lambda *p: (G * T.features64(list(p[:3]), p[3], xyz)).sum(), T.leaves_of(small.arrs, T.APP_NAMES), eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("r", [(16, 48), (5, 50)])
def test_the_bar_sees_each_mutation_of_the_reference(r):
    case = T.cp_case(r)
    s = case.assert_not_vacuous()
    print(f"    {r}: {s}")
    assert sum(s["ends_in"]) >= 100 and s["miss"] >= 40, s
    good = case.ref()["grads"]
    for mut in ("lines_0_2_swapped", "uw_swapped", "T_not_carried"):
        bad = case.ref(mut)["grads"]
        errs = [MB.rel_err(b, g) for b, g in zip(bad, good)]
        print(f"    {mut}: {['%.3g' % e for e in errs]}")
        assert max(errs) > T.BAR_GRAD, (mut, errs)
    # the features: L = sum G * F at the case's own appearance samples
    xyz = case.ref()["xyz"][case.ref()["app"]][:2000].float().numpy()
    G = np.random.default_rng(9).standard_normal((xyz.shape[0], 27))
    good, bad = T.app_reference(case.arrs, xyz, G), T.app_reference(case.arrs, xyz, G, "basis_transposed")
    assert torch.equal(good["features"], bad["features"])                                  # a defect of the backward alone
    errs = [MB.rel_err(b, g) for b, g in zip(bad["grads"][:3], good["grads"][:3])]
    print(f"    basis_transposed: {['%.3g' % e for e in errs]}")
    assert min(errs) > T.BAR_GRAD, errs
    assert MB.rel_err(bad["grads"][3], good["grads"][3]) == 0.0                            # (dB does not pass through dh)


def test_every_rank_keeps_the_border_rule_below_its_cap():
    want = {(96, 288): 18, (16, 48): 16, (5, 50): 7, (1, 1): 5}
    for r in T.RANKS:
        s = T.cp_case(r).assert_not_vacuous()
        assert s["before"] == 768 and s["dropped"] == want[r], (r, s)
    assert T.cp_case((16, 48)).S == 210


def test_new_entry_points_are_declared_exported_and_in_the_makefile():
    from jittor_myc_nerfs_amd import _lib as L
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tvr.h")).read(), flags=re.S)
    l = C.CDLL(L.LIB_PATH)
    for n in NEW_CALLS:
        assert re.search(r"\b" + n + r"\s*\(", src), f"include/tvr.h does not declare {n}"
        assert hasattr(l, n) and n in L.SYMBOLS, n
    assert "tvr_cp_grads" in src and [f[0] for f in L.CpGrads._fields_] == ["density_line", "app_line", "basis_mat"]
    assert C.sizeof(L.CpGrads) == 7 * C.sizeof(C.c_void_p)
    assert "tvr_cp_train.hip" in open(os.path.join(ROOT, "jittor-myc-nerfs_amd", "csrc", "Makefile")).read()


def _aligned(nbytes, align=256):
    a = np.zeros(nbytes + align, np.uint8)
    return a, (a.ctypes.data + align - 1) // align * align


def _scene(L, cp):
    d = L.SceneDesc()
    d.grid[:] = [16, 20, 24]
    d.aabb[:] = [-1.5] * 3 + [1.5] * 3
    d.density_n_comp[:] = [16, 16, 16]
    d.app_n_comp[:] = [48, 48, 48]
    d.app_dim, d.featureC, d.view_pe, d.fea_pe, d.step_size, d.variant = 27, 128, 2, 2, 0.005, 0
    lib = L.lib()
    n = (lib.tvr_cp_scene_packed_bytes if cp else lib.tvr_scene_packed_bytes)(C.byref(d))
    assert n > 0, lib.tvr_last_error()
    keep, addr = _aligned(256)                        # never dereferenced on the host: the create call stores pointers into it
    h = C.c_void_p()
    assert (lib.tvr_cp_scene_create if cp else lib.tvr_scene_create)(C.byref(d), C.c_void_p(addr), n, C.byref(h)) == 0, lib.tvr_last_error()
    return h, keep


def _calls(L, sc, p, big, g):
    lib = L.lib()
    return {"tvr_cp_march_forward": lambda: lib.tvr_cp_march_forward(sc, p, 16, 8, None, 0.0, p, p, big, None),
            "tvr_cp_march_backward": lambda: lib.tvr_cp_march_backward(sc, p, 16, 8, None, 0.0, p, big, p, p, p, big, C.byref(g), None),
            "tvr_cp_app_backward": lambda: lib.tvr_cp_app_backward(sc, p, 16, p, big, p, big, C.byref(g), None)}


def test_new_entry_points_refuse_null_and_vm_scenes_without_a_gpu():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    p, big, g = C.c_void_p(4096), 1 << 40, L.CpGrads()
    # NULL scene
    assert lib.tvr_cp_grad_scratch_bytes(None) == 0
    for name, call in _calls(L, None, p, big, g).items():
        assert call() == -1 and b"NULL" in lib.tvr_last_error(), (name, lib.tvr_last_error())          # TVR_ERR_INVALID
    # a TensorVMSplit scene: TVR_ERR_UNSUPPORTED, before anything else is looked at
    h, keep = _scene(L, cp=False)
    try:
        assert lib.tvr_cp_grad_scratch_bytes(h) == 0 and b"not a CP scene" in lib.tvr_last_error()
        for name, call in _calls(L, h, p, big, g).items():
            assert call() == -4 and b"not a CP scene" in lib.tvr_last_error(), (name, lib.tvr_last_error())
    finally:
        lib.tvr_scene_destroy(h)
    # a CP scene whose parameters were never packed: the size query answers, the calls are refused (nothing is launched), and the old refusals stand beside them
    h, keep2 = _scene(L, cp=True)
    try:
        n = lib.tvr_cp_grad_scratch_bytes(h)
        assert 4 * ((17 + 21 + 25) * (16 + 48) + 27 * 48) <= n < 32768 and n % 256 == 0, n          # three lines of L + 1 texels per factor, basis_mat
        for name, call in _calls(L, h, p, big, g).items():
            assert call() == -1 and b"tvr_scene_update" in lib.tvr_last_error(), (name, lib.tvr_last_error())
        assert lib.tvr_grad_scratch_bytes(h) == 0 and b"CP" in lib.tvr_last_error()
        assert lib.tvr_march_forward(h, p, 16, 8, None, 0.0, p, p, big, None) == -4 and b"CP" in lib.tvr_last_error()
    finally:
        lib.tvr_scene_destroy(h)
    del keep, keep2


def test_cp_training_is_opt_in():
    from jittor_myc_nerfs_amd import TensorCP, reconstruct, _lib as L
    assert TensorCP.cp_training is False
    args = reconstruct.config_parser([])
    assert args.cp_training == 0 and reconstruct.config_parser(["--cp_training", "1"]).cp_training == 1
    from jittor_myc_nerfs_amd import synthetic
    hyp = dict(synthetic.HYPER, near_far=(2.0, 6.0), step_ratio=0.5)
    m = CC.make_cp_model(CC.cp_arrays(5, 50), hyp, device="cpu")
    rays = torch.tensor([[0.0, 0.0, -4.0, 0.0, 0.0, 1.0]])
    assert m.cp_training is False
    with pytest.raises(NotImplementedError, match="CP training is not built.*cp_training"):
        m.render_rays_autograd(rays)
    m.cp_training = True                                # opted in, but on the CPU: no fallback, as every other CP call
    with pytest.raises(L.TvrError):
        m.render_rays_autograd(rays)
    assert not m._fused_step_ok()
    # reconstruct: the attribute absent or 0 refuses before any data is touched; Ortho_weight has no meaning for TensorCP
    for extra in ({}, {"cp_training": 0}):
        a = types.SimpleNamespace(model_name="TensorCP", dataset_name="blender", datadir="/nonexistent/never/opened", ndc_ray=0, **extra)
        with pytest.raises(NotImplementedError, match="CP training is not built"):
            reconstruct.reconstruction(a, device="cpu")
    a = types.SimpleNamespace(model_name="TensorCP", dataset_name="blender", datadir="/nonexistent/never/opened", ndc_ray=0, cp_training=1, Ortho_weight=0.1)
    with pytest.raises(ValueError, match="Ortho_weight"):
        reconstruct.reconstruction(a, device="cpu")
