"""GPU (-m gpu): TensorCP's training path — tvr_cp_march_forward / _backward, tvr_cp_app_backward (csrc/tvr_cp_train.hip), the autograd Functions around them and the
opt-in switch `cp_training` — against the float64 reference of tests/cp_train_common.py (checked on the CPU by tests/test_cp_train_host.py).

Bars: BAR_GRAD = 5e-4 of a tensor's largest gradient entry and BAR_FWD = 2e-4 absolute, the project's own.  Where the fp32 torch restatement alone spends more than a
quarter of a bar, cp_common.allowance(ref32, ref64, relative=True) takes the bar's place; both numbers are printed."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import cp_common as CC
import cp_train_common as T
import march_backward_common as MB
from conftest import TINY, make_model

pytestmark = pytest.mark.gpu

CPA_ENTRIES = 256          # consecutive entries per workgroup of cp_app_backward_kernel (csrc/tvr_cp_train.hip): sizes 255 / 257 / 1000 straddle it


def _fresh(arrs, hyp, training=True):
    m = CC.make_cp_model(arrs, hyp)                      # a model of this test's own (test_gpu_cp.py's is cached and shared)
    m.cp_training = training
    return m


def _tol(what, ref32, ref64, bar, relative):
    """the bar, or the allowance where the fp32 restatement alone spends more than a quarter of it.  relative: in units of max |ref64| (gradients)"""
    scale = max(float(ref64.abs().max()), 1e-300) if relative else 1.0
    e32 = float((ref32.double() - ref64).abs().max()) / scale
    tol = bar
    if e32 > bar / 4:
        tol = CC.allowance(ref32, ref64, relative=True) / scale
    print(f"    {what}: fp32 restatement {e32:.3g}, bar {bar:.3g}, tolerance used {tol:.3g}")
    return tol


def _check(what, got, ref32, ref64, bar, relative):
    tol = _tol(what, ref32, ref64, bar, relative)
    got = got.detach().double().cpu()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    scale = max(float(ref64.abs().max()), 1e-300) if relative else 1.0
    err = float((got - ref64).abs().max()) / scale
    print(f"    {what}: |kernel - fp64| = {err:.3g}")
    assert torch.isfinite(got).all() and err <= tol, (what, err, tol)
    return err


def _march(m, case):
    """the march Function on a case's rays and the march's loss; -> (w, acc, xyz, ray_id, depth, density-line gradients)"""
    from jittor_myc_nerfs_amd.autograd_ops import _CpMarchFn
    rays = torch.tensor(case.rays, device="cuda")
    jitter = None if case.jitter is None else torch.tensor(case.jitter, device="cuda")
    for p in m.density_line:
        p.grad = None
    w, acc, xyz, ray_id, depth = _CpMarchFn.apply(m, rays, jitter, case.S, case.eps_T, *m.density_line)
    g = MB.g_of(xyz.double()).float()                     # the loss's factor at the queue's own positions: no entry <-> sample mapping is needed
    loss = (g * w).sum() + (case.a.float().cuda() * acc).sum()
    loss.backward()
    return w.detach(), acc.detach(), xyz, ray_id, depth, [p.grad.clone() for p in m.density_line]


def _compare_march(m, case, label):
    s = case.assert_not_vacuous()
    print(f"  {label}: {s}")
    ref, r32 = case.ref(), T.march_reference32(case)
    w, acc, xyz, ray_id, depth, grads = _march(m, case)
    app = ref["app"]
    assert w.shape[0] == int(app.sum()), (w.shape[0], int(app.sum()))                          # the border rule has removed the rays whose count may differ
    assert torch.equal(ray_id.cpu(), torch.nonzero(app)[:, 0])                                 # ray order, a ray's entries in sample order
    _check("w", w, r32["w"][app], ref["w"][app], T.BAR_FWD, False)
    _check("acc", acc, r32["acc"], ref["acc"], T.BAR_FWD, False)
    errs = []
    for i in range(3):
        g, g64 = grads[i], ref["grads"][i]
        assert tuple(g.shape) == tuple(m.density_line[i].shape) == tuple(g64.shape)            # reference-shaped: no pad texel, no pad channel
        errs.append(_check(f"d density_line.{i}", g, r32["grads"][i], g64, T.BAR_GRAD, True))
        # nothing leaked from (or into) the padding: the sums agree as the entries do
        assert abs(float(g.double().sum().cpu()) - float(g64.sum())) <= 4 * T.BAR_GRAD * float(g64.abs().max()) * np.sqrt(g64.numel()), i
    return errs


# ---- 1. march forward / backward against the float64 reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [False, True], ids=["nojitter", "jitter"])
@pytest.mark.parametrize("r", T.RANKS, ids=[f"{a}-{b}" for a, b in T.RANKS])
def test_march_forward_and_backward_match_float64(r, jitter):
    case = T.cp_case(r, jitter=jitter)
    assert case.S == 210 and sum(case.stats()["ends_in"]) >= 50 and case.stats()["miss"] >= 40
    _compare_march(_fresh(case.arrs, case.hyper), case, f"ranks {r}, jitter {jitter}")


def test_march_backward_relu():
    case = T.cp_case((16, 48), act="relu")
    _compare_march(_fresh(case.arrs, case.hyper), case, "relu")


def test_march_backward_with_an_alpha_mask_from_updateAlphaMask():
    base = T.cp_case((16, 48))
    m = _fresh(base.arrs, base.hyper)
    with torch.no_grad():
        m.updateAlphaMask(tuple(TINY["gridSize"]))
    arrs = dict(base.arrs, alpha_volume=m.alphaMask.alpha_volume.view(*m.alphaMask.alpha_volume.shape[-3:]).cpu().numpy(), alpha_aabb=m.alphaMask.aabb.numpy())
    case = T.masked_case(arrs)
    assert case.stats()["masked"] > 1000, case.stats()                                         # valid != in-box
    _compare_march(_fresh(arrs, case.hyper), case, "alpha mask")


# ---- 2. forward bits ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [False, True], ids=["nojitter", "jitter"])
def test_cp_march_forward_leaves_the_render_path_s_bits(jitter):
    from jittor_myc_nerfs_amd import _lib as L
    from jittor_myc_nerfs_amd.autograd_ops import _CpMarchFn
    case = T.cp_case((96, 288), jitter=jitter)
    m = _fresh(case.arrs, case.hyper)
    rays = torch.tensor(case.rays, device="cuda")
    jit = None if case.jitter is None else torch.tensor(case.jitter, device="cuda")
    n, S = rays.shape[0], case.S
    with torch.no_grad():
        w, acc, xyz, ray_id, depth = _CpMarchFn.apply(m, rays, jit, S, case.eps_T, *m.density_line)
        _, depth_r, d = m.render_rays(rays, white_bg=True, N_samples=S, jitter=jit, eps_T=case.eps_T, dense=True)
        _, depth_n = m.render_rays(rays, white_bg=True, N_samples=S, jitter=jit, eps_T=case.eps_T)
    # the non-dense render's queue, still in its scratch: the plain layout is a prefix of the CP render's; its order is the march kernel's, a ray's entries contiguous
    lay = L.ScratchLayout()
    L.check(L.lib().tvr_scratch_describe(n, S, C.byref(lay)), "tvr_scratch_describe")
    sb = m._scratch
    M = int(sb[lay.counter:lay.counter + 4].view(torch.int32).item())
    assert M == w.shape[0] > 1000
    q = sb[lay.q_pos:lay.q_pos + M * 16].view(torch.float32).view(M, 4)
    qr = sb[lay.q_ray:lay.q_ray + M * 4].view(torch.int32).long()
    order = torch.sort(qr, stable=True)[1]
    assert torch.equal(qr[order], ray_id)
    assert torch.equal(q[order, :3], xyz) and torch.equal(q[order, 3], w)
    assert torch.equal(sb[lay.acc:lay.acc + n * 4].view(torch.float32), acc)
    assert torch.equal(depth_n, depth) and torch.equal(depth_r, depth)
    # and the dense outputs of the same march: the weights above the threshold are the queue's, row by row
    dw = d["weight"]
    assert torch.equal(dw[dw > float(m.rayMarch_weight_thres)], w) and torch.equal(d["acc"].view(-1), acc)


# ---- 3. tvr_cp_app_backward alone ----------------------------------------------------------------------------------------------------------------------
def _app_backward(m, xyz, G, poison=True):
    from jittor_myc_nerfs_amd import _lib as L
    from jittor_myc_nerfs_amd.autograd_ops import _stream_ptr
    sc = m._ensure_scene(settle=False)
    grads = [torch.full_like(p, float("nan")) for p in list(m.app_line) + [m.basis_mat.weight]]   # the call OVERWRITES what it owns
    out = L.CpGrads()
    for i in range(3):
        out.app_line[i] = grads[i].data_ptr()
    out.basis_mat = grads[3].data_ptr()
    gs = m._get_cp_grad_scratch()
    if poison:
        gs.view(torch.float32).fill_(float("nan"))       # and zeroes its images itself
    n = xyz.shape[0]
    rc = L.lib().tvr_cp_app_backward(sc, xyz.data_ptr() if n else None, n, G.data_ptr() if n else None, G.numel() * 4, gs.data_ptr(), gs.numel(), C.byref(out),
                                     _stream_ptr(m.device))
    assert rc == 0, L.lib().tvr_last_error()
    torch.cuda.synchronize()
    return grads


@pytest.mark.parametrize("kind", ["random", "one_cell", "upper_boundary", "outside"])
@pytest.mark.parametrize("r", [(96, 288), (5, 50)], ids=["288", "50"])
def test_app_backward_against_float64(r, kind):
    arrs = CC.cp_arrays(*r)
    m = _fresh(arrs, T.hyper())
    for n in (1, CPA_ENTRIES - 1, CPA_ENTRIES + 1, 1000):       # one entry; a workgroup's run one short; a second workgroup of ONE entry (the run straddles); four workgroups
        xyz = T.app_points(kind, n, seed=n)
        G = np.random.default_rng(n).standard_normal((n, 27)).astype(np.float32)
        ref = T.app_reference(arrs, xyz, G)
        got = _app_backward(m, torch.tensor(xyz, device="cuda"), torch.tensor(G, device="cuda"))
        feats = m.compute_appfeature(torch.tensor(xyz, device="cuda"))
        assert tuple(feats.shape) == (n, 27)
        for name, g, g64 in zip(T.APP_NAMES, got, ref["grads"]):
            assert tuple(g.shape) == tuple(g64.shape), name
            if kind == "outside":                       # zeros padding: every product holds a factor with both tap weights zero
                assert float(g64.abs().max()) == 0.0 and float(g.abs().max()) == 0.0, (name, n)
                continue
            err = MB.rel_err(g, g64)
            print(f"    {kind} n={n} {name}: {err:.3g}")
            assert torch.isfinite(g).all() and err <= T.BAR_GRAD, (kind, n, name, err)
            assert abs(float(g.double().sum().cpu()) - float(g64.sum())) <= 4 * T.BAR_GRAD * float(g64.abs().max()) * np.sqrt(g64.numel()), (name, n)


# ---- 4. empty work -------------------------------------------------------------------------------------------------------------------------------------
def test_rays_that_all_miss_the_box():
    case = T.cp_case((16, 48))
    m = _fresh(case.arrs, case.hyper)
    rays = torch.tensor(case.rays[:64], device="cuda").clone()
    rays[:, 3:6] = -rays[:, 3:6]                         # looking away from the scene
    rgb, depth = m.render_rays_autograd(rays, white_bg=True, N_samples=case.S)
    assert torch.equal(rgb, torch.ones_like(rgb))
    (rgb.sum() + (rgb ** 2).sum()).backward()
    for name, p in m.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) == 0.0, name
    assert all(p.grad is not None for p in m.density_line)


def test_a_scene_below_the_threshold_learns_through_acc():
    base = CC.cp_arrays(16, 48)
    arrs = dict(base, **{f"density_line.{i}": base[f"density_line.{i}"] * 0.2 for i in range(3)})
    hyp = T.hyper()
    case = T.CpCase(arrs, hyp, T.frames(), T.n_samples(hyp), 1e-4, seed=5)
    assert case.n_dropped == 0 and int(case.ref()["app"].sum()) == 0 and float(case.ref()["acc"].max()) > 0
    m = _fresh(arrs, hyp)
    w, acc, xyz, ray_id, depth, grads = _march(m, case)
    assert w.shape[0] == 0                                # M == 0
    r32 = T.march_reference32(case)
    _check("acc", acc, r32["acc"], case.ref()["acc"], T.BAR_FWD, False)
    for i in range(3):
        _check(f"d density_line.{i}", grads[i], r32["grads"][i], case.ref()["grads"][i], T.BAR_GRAD, True)
    # the whole chain on an empty queue: finite everywhere, nothing for the appearance side
    for p in m.parameters():
        p.grad = None
    rgb, _ = m.render_rays_autograd(torch.tensor(case.rays, device="cuda"), white_bg=True, N_samples=case.S)
    ((rgb - 0.5) ** 2).mean().backward()
    for name, p in m.named_parameters():
        assert p.grad is None or torch.isfinite(p.grad).all(), name
    assert float(torch.stack([p.grad.abs().max() for p in m.density_line]).max()) > 0


def test_app_backward_of_no_entries():
    m = _fresh(CC.cp_arrays(5, 50), T.hyper())
    got = _app_backward(m, torch.zeros((0, 3), device="cuda"), torch.zeros((0, 27), device="cuda"))
    assert all(float(g.abs().max()) == 0.0 for g in got)


# ---- 5. the whole step -----------------------------------------------------------------------------------------------------------------------------------
def _step(m, case, target):
    for p in m.parameters():
        p.grad = None
    rgb, _ = m.render_rays_autograd(torch.tensor(case.rays, device="cuda"), white_bg=True, N_samples=case.S)
    loss = ((rgb - target) ** 2).mean()
    loss.backward()
    mlp = m.renderModule.mlp
    ps = dict(zip(T.DENSITY_NAMES + T.APP_NAMES + T.NET_NAMES,
                  list(m.density_line) + list(m.app_line) + [m.basis_mat.weight, mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias, mlp[4].weight, mlp[4].bias]))
    return rgb.detach(), {k: p.grad.clone() for k, p in ps.items()}


@pytest.mark.parametrize("r", [(16, 48), (96, 288)], ids=["16-48", "96-288"])
def test_whole_step_matches_autograd_through_the_float64_restatement(r):
    case = T.cp_case(r)
    case.assert_not_vacuous()
    target = np.random.default_rng(r[0]).random((case.n, 3)).astype(np.float32)
    r64, r32 = T.step_reference(case, target), T.step_reference(case, target, dtype=torch.float32)
    assert r64["n_app"] > 10000
    m = _fresh(case.arrs, case.hyper)
    assert m.eps_T is None and float(m.rayMarch_weight_thres) == case.eps_T
    tgt = torch.tensor(target, device="cuda")
    rgb, g1 = _step(m, case, tgt)
    _check("rgb_map", rgb, r32["rgb_map"], r64["rgb_map"], T.BAR_FWD, False)
    for k in T.DENSITY_NAMES + T.APP_NAMES + T.NET_NAMES:
        _check("d " + k, g1[k], r32["grads"][k], r64["grads"][k], T.BAR_GRAD, True)
    # two runs agree to rounding: the line and basis sums are float atomics (include/tvr.h, CP TRAINING).  A texel's sum takes at most two terms per ray (768 rays) in
    # an order that changes from run to run; reordering N fp32 additions moves a sum by at most N 2^-24 of the terms' absolute sum: 1e-4 of the largest entry bounds it
    _, g2 = _step(m, case, tgt)
    for k in g1:
        d = MB.rel_err(g2[k], g1[k])
        print(f"    run-to-run {k}: {d:.3g}")
        assert d <= 1e-4, (k, d)
    assert m.training_fault_flag().item() == 0.0 and m.check_training_faults() is None     # a model that never ran a fused step answers "no fault"


# ---- 6. it learns ----------------------------------------------------------------------------------------------------------------------------------------
def _teacher_views(n_views, wh):
    from jittor_myc_nerfs_amd import rays as R, synthetic
    hyp = dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=0.5)
    teacher = _fresh(CC.cp_arrays(16, 48, gridSize=[32, 32, 32]), hyp, training=False)
    rays = torch.cat([R.frame_rays(M, wh, wh, synthetic.SCENE_A["camera_angle_x"]) for M in R.sphere_poses(n_views, 4.0)]).cuda()
    with torch.no_grad():
        rgb, _ = teacher(rays, is_train=False, white_bg=True, N_samples=96)
    return rays, rgb


def test_adam_on_a_random_start_lowers_the_loss():
    from jittor_myc_nerfs_amd import TensorCP
    torch.manual_seed(0)
    rays, rgb = _teacher_views(4, 16)
    assert float(((rgb - 1.0) ** 2).mean()) > 1e-3                                            # the views show something
    m = TensorCP(TINY["aabb"], [24, 24, 24], "cuda", density_n_comp=[16], appearance_n_comp=[48], app_dim=27, near_far=TINY["near_far"], shadingMode="MLP_Fea",
                 view_pe=2, fea_pe=2, featureC=128, step_ratio=0.5)
    m.cp_training = True
    opt = torch.optim.Adam(m.get_optparam_groups(0.02, 0.001), betas=(0.9, 0.99))
    losses = []
    for it in range(48):
        opt.zero_grad()
        out, _ = m.render_rays_autograd(rays, white_bg=True, N_samples=64)
        loss = ((out - rgb) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"    loss {losses[0]:.5f} -> {losses[-1]:.5f} (min {min(losses):.5f})")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_reconstruct_trains_a_cp_model_when_asked_to(tmp_path):
    """reconstruct.reconstruction with cp_training = 1 on a synthetic dataset: one alpha-mask update with shrink, one upsampling, a checkpoint that reloads and renders"""
    from jittor_myc_nerfs_amd import TensorCP, load_checkpoint
    from jittor_myc_nerfs_amd.reconstruct import config_parser, reconstruction
    torch.manual_seed(0)
    wh = 16
    rays, rgb = _teacher_views(9, wh)
    train, val = types.SimpleNamespace(), types.SimpleNamespace()
    train.all_rays, train.all_rgbs = rays[:8 * wh * wh], rgb[:8 * wh * wh]
    val.all_rays, val.all_rgbs = rays[8 * wh * wh:].view(1, wh, wh, 6), rgb[8 * wh * wh:].view(1, wh, wh, 3)
    for d in (train, val):
        d.scene_bbox, d.white_bg, d.near_far = torch.tensor(TINY["aabb"], dtype=torch.float32).reshape(2, 3), True, list(TINY["near_far"])
    cmd = ["--dataset_name", "blender", "--expname", "cp", "--basedir", str(tmp_path), "--n_iters", "150", "--batch_size", "1024", "--N_voxel_init", str(16 ** 3),
           "--N_voxel_final", str(24 ** 3), "--N_vis", "0", "--vis_every", "100000", "--progress_refresh_rate", "50", "--model_name", "TensorCP", "--shadingMode", "MLP_Fea",
           "--view_pe", "2", "--fea_pe", "2", "--n_lamb_sigma", "16", "--n_lamb_sh", "48", "--upsamp_list", "110", "--update_AlphaMask_list", "100", "--white_bkgd",
           "--L1_weight_inital", "8e-5", "--L1_weight_rest", "4e-5", "--TV_weight_density", "0.1", "--TV_weight_app", "0.01"]
    with pytest.raises(NotImplementedError, match="CP training is not built"):
        reconstruction(config_parser(cmd), train_dataset=train, val_dataset=val)
    args = config_parser(cmd + ["--cp_training", "1"])
    lines = []
    m, folder, _ = reconstruction(args, log=lines.append, train_dataset=train, val_dataset=val)
    print("\n".join(lines[-2:]))
    assert type(m) is TensorCP and m.cp_training and m.alphaMask is not None and max(m.gridSize.tolist()) > 16
    test_rays, gt = val.all_rays.view(-1, 6), val.all_rgbs.view(-1, 3)
    with torch.no_grad():
        a, _ = m(test_rays, is_train=False, white_bg=True, N_samples=-1)
    psnr = float(-10 * torch.log10(torch.mean((a - gt) ** 2)))
    print(f"    held-out PSNR after 150 iterations: {psnr:.2f} dB (recorded in DESIGN.md 4.9; no bar)")
    assert np.isfinite(psnr)
    ckpt = load_checkpoint(f"{folder}/cp.th")
    m2 = TensorCP(**dict(ckpt["kwargs"], device="cuda"))
    m2.load(ckpt)
    assert m2.cp_training is False                       # the switch is the caller's, not the checkpoint's
    with torch.no_grad():
        b, _ = m2(test_rays, is_train=False, white_bg=True, N_samples=-1)
    assert torch.equal(a, b)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_default_refuses_and_the_new_calls_refuse_a_vm_scene(hyper_tiny):
    from jittor_myc_nerfs_amd import _lib as L, synthetic
    lib = L.lib()
    arrs = CC.cp_arrays(5, 50)
    m = _fresh(arrs, T.hyper(), training=False)
    rays = torch.tensor(T.frames()[:32], device="cuda")
    with pytest.raises(NotImplementedError, match="CP training is not built"):
        m.render_rays_autograd(rays)
    with pytest.raises(NotImplementedError, match="CP training is not built"):
        m(rays, is_train=True)
    m.cp_training = True
    rgb, _ = m(rays, is_train=True, white_bg=True, N_samples=64)
    assert rgb.requires_grad and tuple(rgb.shape) == (32, 3)
    vm = make_model(synthetic.make_scene_arrays(TINY["gridSize"], TINY["aabb"]), hyper_tiny)
    sc = vm._ensure_scene()
    p, big, g = C.c_void_p(4096), 1 << 40, L.CpGrads()       # never dereferenced: the scene check comes first
    assert lib.tvr_cp_grad_scratch_bytes(sc) == 0
    assert lib.tvr_cp_march_forward(sc, p, 16, 8, None, 0.0, p, p, big, None) == -4 and b"not a CP scene" in lib.tvr_last_error()
    assert lib.tvr_cp_march_backward(sc, p, 16, 8, None, 0.0, p, big, p, p, p, big, C.byref(g), None) == -4 and b"not a CP scene" in lib.tvr_last_error()
    assert lib.tvr_cp_app_backward(sc, p, 16, p, big, p, big, C.byref(g), None) == -4 and b"not a CP scene" in lib.tvr_last_error()
    torch.cuda.synchronize()                                 # nothing was launched, nothing faulted
