"""GPU (-m gpu): the training step.  Gradients of the HIP march / VM-gather backward kernels (plus the library-GEMM
MLP) against torch autograd through the op-for-op oracle; then a short optimisation run with the reference's loss terms."""
import numpy as np
import pytest
import torch

from conftest import TINY, make_model

pytestmark = pytest.mark.gpu


def _oracle_with_grads(arrs, hyper):
    from oracle import tensorf_oracle as TO
    sc = TO.scene_from_arrays(arrs, **hyper)
    leaves = {}
    for name in ("density_plane", "density_line", "app_plane", "app_line"):
        for i, t in enumerate(getattr(sc, name)):
            t.requires_grad_(True)
            leaves[f"{name}.{i}"] = t
    sc.basis_mat.requires_grad_(True)
    leaves["basis_mat"] = sc.basis_mat
    for k, t in sc.mlp.items():
        t.requires_grad_(True)
        leaves[k] = t
    return sc, leaves


@pytest.mark.parametrize("static", [True, False])
@pytest.mark.parametrize("white_bg,use_jitter", [(True, False), (False, True)])
def test_gradients_match_oracle_autograd(tiny_dump, tiny_arrays, hyper_tiny, white_bg, use_jitter, static):
    """static = True: the step as tvr_train_forward / tvr_train_backward (device-side counts, no host read); False: the eager chain of autograd Functions.
    This is the ONE-CHUNK, NO-EXIT case: 48 samples (march_backward_kernel's chunk loop runs once, nothing is carried), eps_T = 0 (no early exit), grid 16x20x24
    (the LDS form of both scatter kernels).  More than one chunk, early exit, skipped chunks and the grids beyond the LDS limits: tests/test_gpu_march_backward.py."""
    from oracle import tensorf_oracle as TO
    rays_np = tiny_dump["rays"]
    S = TINY["N_samples"]
    jit_np = np.random.default_rng(11).random(rays_np.shape[0]).astype(np.float32) if use_jitter else None
    cw = torch.tensor(np.random.default_rng(12).standard_normal((rays_np.shape[0], 3)).astype(np.float32))
    # oracle: autograd through the restated op sequence (eps_T = 0 semantics)
    sc, leaves = _oracle_with_grads(tiny_arrays, hyper_tiny)
    rgb_o, _ = TO.execute(sc, torch.tensor(rays_np), white_bg=white_bg, N_samples=S, jitter=jit_np)
    (rgb_o * cw).sum().backward()
    # HIP path
    m = make_model(tiny_arrays, hyper_tiny)
    m.eps_T = 0.0
    m.static_training = static
    rays = torch.tensor(rays_np, device="cuda")
    jitter = None if jit_np is None else torch.tensor(jit_np, device="cuda")
    rgb, depth = m.render_rays_autograd(rays, white_bg=white_bg, N_samples=S, jitter=jitter)
    assert (getattr(m, "_train_buf", None) is not None) == static
    assert np.abs(rgb.detach().cpu().numpy() - rgb_o.detach().numpy()).max() < 2e-4
    (rgb * cw.cuda()).sum().backward()
    mlp = m.renderModule.mlp
    got = {"basis_mat": m.basis_mat.weight.grad, "W1": mlp[0].weight.grad, "b1": mlp[0].bias.grad, "W2": mlp[2].weight.grad,
           "b2": mlp[2].bias.grad, "W3": mlp[4].weight.grad, "b3": mlp[4].bias.grad}
    for i in range(3):
        got[f"density_plane.{i}"], got[f"density_line.{i}"] = m.density_plane[i].grad, m.density_line[i].grad
        got[f"app_plane.{i}"], got[f"app_line.{i}"] = m.app_plane[i].grad, m.app_line[i].grad
    for k, ref in leaves.items():
        g, r = got[k].cpu().numpy(), ref.grad.numpy()
        scale = max(np.abs(r).max(), 1e-6)
        err = np.abs(g - r).max() / scale
        # fp32 atomics + a threshold-flip sample (weight ~1e-4) bound the agreement; 5e-4 of the largest entry is far below any
        # real defect (a wrong tap, sign or index shows up as O(1)); measured worst case 1.5e-5
        print(f"grad {k:18s} rel-max-err {err:.2e}  (max |g| {scale:.2e})")
        assert err < 5e-4, f"{k}: max |grad diff| / max |grad| = {err:.2e}"
        assert np.abs(r).max() > 0, f"{k}: oracle gradient is identically zero — test would be vacuous"


def test_training_loop_reduces_loss(tiny_arrays, hyper_tiny, tiny_dump):
    """train.py:219-271 in miniature: Adam on the param groups, MSE + the reference's regularisers, lr decay; the HIP forward
    and backward drive the loss down on a synthetic target rendered from a different scene."""
    from jittor_myc_nerfs_amd import OctreeRender_trilinear_fast, TVLoss, synthetic
    target_arrs = synthetic.make_scene_arrays(TINY["gridSize"], TINY["aabb"], seed=99)
    teacher = make_model(target_arrs, hyper_tiny)
    rays = torch.tensor(np.concatenate([tiny_dump["rays"]] * 4), device="cuda")
    rays[:, :3] += 0.01 * torch.randn_like(rays[:, :3])
    with torch.no_grad():
        gt, _ = teacher(rays, is_train=False, white_bg=True, N_samples=TINY["N_samples"])
    m = make_model(tiny_arrays, hyper_tiny)
    opt = torch.optim.Adam(m.get_optparam_groups(0.02, 0.001), betas=(0.9, 0.99))
    tv = TVLoss()
    losses = []
    for it in range(30):
        opt.zero_grad()
        rgb_map, _, depth_map, _, _ = OctreeRender_trilinear_fast(rays, m, chunk=4096, N_samples=TINY["N_samples"], white_bg=True, is_train=True)
        loss = torch.mean((rgb_map - gt) ** 2)
        total = loss + 1e-4 * m.vector_comp_diffs() + 1e-5 * m.density_L1() + 0.1 * m.TV_loss_density(tv) + 0.01 * m.TV_loss_app(tv)
        total.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < 0.5 * losses[0], f"loss did not drop: {losses[0]:.4e} -> {losses[-1]:.4e}"
    assert all(np.isfinite(losses))


@pytest.mark.parametrize("M,Ka,Kb", [(356_123, 128, 150), (50_001, 128, 128), (9_999, 3, 128), (70_000, 27, 144), (4_097, 1, 144), (100, 5, 7), (0, 4, 4)])
def test_gemm_tn_matches_fp64(M, Ka, Kb):
    """tvr_gemm_tn (the weight-gradient reduction dW = dY^T X) against a float64 product: fp32-class accuracy, ragged edges, empty input."""
    import ctypes as C
    from jittor_myc_nerfs_amd import _lib as L
    g = torch.Generator(device="cuda").manual_seed(M + Ka)
    A = torch.randn((M, Ka), device="cuda", generator=g)
    B = torch.randn((M, Kb), device="cuda", generator=g)
    out = torch.full((Ka, Kb), float("nan"), device="cuda")
    sc = torch.empty(max(L.lib().tvr_gemm_tn_scratch_bytes(Ka, Kb, M), 1), dtype=torch.uint8, device="cuda")
    L.check(L.lib().tvr_gemm_tn(A.data_ptr(), Ka, Ka, B.data_ptr(), Kb, Kb, M, out.data_ptr(), sc.data_ptr(), sc.numel(), None), "tvr_gemm_tn")
    ref = (A.double().t() @ B.double())
    err = float((out.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    lib = float(((A.t() @ B).double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    print(f"gemm_tn {M}x{Ka}x{Kb}: rel err {err:.2e} (library fp32 GEMM {lib:.2e})")
    assert err < 2e-6
    assert L.lib().tvr_gemm_tn(A.data_ptr(), Ka, Ka, B.data_ptr(), Kb, Kb, -1, out.data_ptr(), sc.data_ptr(), sc.numel(), None) < 0
    assert L.lib().tvr_gemm_tn(A.data_ptr(), Ka, 161, B.data_ptr(), Kb, 161, 10, out.data_ptr(), sc.data_ptr(), sc.numel(), None) < 0      # 6 x 6 tiles: refused
    if M > 0:
        assert L.lib().tvr_gemm_tn(A.data_ptr(), Ka, Ka, B.data_ptr(), Kb, Kb, M, out.data_ptr(), sc.data_ptr(), 16, None) == -3          # scratch too small


@pytest.mark.parametrize("M,Ka,Kb,lda,ldb,offa,offb", [(60_001, 128, 123, 128, 283, 0, 160), (33_333, 96, 160, 200, 283, 7, 0), (20_011, 640, 1, 640, 1, 0, 0),
                                                        (5_003, 150, 128, 150, 128, 0, 0), (16, 150, 128, 150, 128, 0, 0), (31, 30, 2, 30, 2, 0, 0),
                                                        (40_007, 64, 128, 72, 128, 0, 0), (40_007, 8, 128, 72, 128, 64, 0), (9_001, 64, 16, 72, 16, 0, 0),
                                                        (9_001, 4, 64, 8, 64, 0, 0), (21, 128, 36, 128, 36, 0, 0)])
def test_gemm_tn_strided_blocks_and_column_sums(M, Ka, Kb, lda, ldb, offa, offb):
    """The shapes autograd_ops._gemm_tn / _colsum / _BgNetFn hand over: column blocks of wider matrices (row stride > row length, unaligned starts: the dword
    staging path; multiples of 4 and aligned: the strided 16-B staging path), a 20 x 1 tile column sum (the direct-load kernel), and short / odd row counts
    through the 16-B staging paths' ragged ends."""
    from jittor_myc_nerfs_amd import _lib as L
    g = torch.Generator(device="cuda").manual_seed(M + Ka + lda)
    A = torch.randn((M, lda), device="cuda", generator=g)
    B = torch.randn((M, ldb), device="cuda", generator=g)
    out = torch.full((Ka, Kb), float("nan"), device="cuda")
    sc = torch.empty(max(L.lib().tvr_gemm_tn_scratch_bytes(Ka, Kb, M), 1), dtype=torch.uint8, device="cuda")
    L.check(L.lib().tvr_gemm_tn(A.data_ptr() + 4 * offa, lda, Ka, B.data_ptr() + 4 * offb, ldb, Kb, M, out.data_ptr(), sc.data_ptr(), sc.numel(), None), "tvr_gemm_tn")
    ref = A[:, offa:offa + Ka].double().t() @ B[:, offb:offb + Kb].double()
    err = float((out.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    assert err < 2e-6, err
    out2 = torch.empty_like(out)
    L.check(L.lib().tvr_gemm_tn(A.data_ptr() + 4 * offa, lda, Ka, B.data_ptr() + 4 * offb, ldb, Kb, M, out2.data_ptr(), sc.data_ptr(), sc.numel(), None), "tvr_gemm_tn")
    assert torch.equal(out, out2)
    # the same product with the column sums of A riding along as a virtual ones column of B (weight + bias gradient from one pass over dY)
    if ((Ka + 31) // 32) * ((Kb + 1 + 31) // 32) <= 20 and Ka + Kb <= 320:
        out3, cs = torch.full((Ka, Kb), float("nan"), device="cuda"), torch.full((Ka,), float("nan"), device="cuda")
        sc3 = torch.empty(max(L.lib().tvr_gemm_tn_scratch_bytes(Ka, Kb + 1, M), 1), dtype=torch.uint8, device="cuda")
        L.check(L.lib().tvr_gemm_tn_bias(A.data_ptr() + 4 * offa, lda, Ka, B.data_ptr() + 4 * offb, ldb, Kb, M, out3.data_ptr(), cs.data_ptr(), sc3.data_ptr(), sc3.numel(),
                                         None), "tvr_gemm_tn_bias")
        assert torch.equal(out3, out), "the ones column changed the product"
        ref_cs = A[:, offa:offa + Ka].double().sum(0)
        assert float((cs.double() - ref_cs).abs().max()) / max(1.0, float(ref_cs.abs().max())) < 2e-6


def test_fused_adam_updates_reach_the_packed_scene(tiny_arrays, hyper_tiny, tiny_dump):
    """torch.optim.Adam(fused=True) writes the parameters without bumping their version counters; the packed device scene must follow
    anyway (the training forward re-packs, and a backward invalidates the pack for whatever renders next)."""
    from jittor_myc_nerfs_amd import TensorVMSplit
    rays = torch.tensor(tiny_dump["rays"], device="cuda")
    m = make_model(tiny_arrays, hyper_tiny)
    opt = torch.optim.Adam(m.get_optparam_groups(0.02, 0.001), betas=(0.9, 0.99), fused=True)
    gt = torch.rand((rays.shape[0], 3), device="cuda")
    for _ in range(3):
        opt.zero_grad()
        rgb, _ = m(rays, is_train=True, white_bg=True, N_samples=TINY["N_samples"])
        torch.mean((rgb - gt) ** 2).backward()
        opt.step()
    with torch.no_grad():
        after, _ = m(rays, is_train=False, white_bg=True, N_samples=TINY["N_samples"])          # evaluation right after the last step
    fresh = TensorVMSplit(**dict(m.get_kwargs(), device="cuda"))
    fresh.load({"state_dict": m.state_dict()})
    with torch.no_grad():
        want, _ = fresh(rays, is_train=False, white_bg=True, N_samples=TINY["N_samples"])
    assert torch.equal(after, want)


def test_fused_pe_concat_and_tv_loss_match_torch():
    """tvr_pe_concat / tvr_tv_loss against the torch formulations they replace in the training step (values and gradients)."""
    from jittor_myc_nerfs_amd import TVLoss
    from jittor_myc_nerfs_amd.autograd_ops import _mlp_input, _pe
    g = torch.Generator(device="cuda").manual_seed(5)
    for with_dot in (False, True):
        f = (torch.randn((5003, 27), device="cuda", generator=g) * 3).requires_grad_(True)
        v = torch.randn((5003, 3), device="cuda", generator=g).requires_grad_(True)
        d = torch.randn((5003, 1), device="cuda", generator=g).requires_grad_(True) if with_dot else None
        X = _mlp_input(f, v, 2, 2, d)
        ref = torch.cat(([d] if with_dot else []) + [f, v, _pe(f, 2), _pe(v, 2)], dim=-1)
        assert X.shape == ref.shape == (5003, 151 if with_dot else 150) and float((X - ref).abs().max()) < 1e-6
        cw = torch.randn(X.shape, device="cuda", generator=g)
        got = torch.autograd.grad((X * cw).sum(), [f, v] + ([d] if with_dot else []))
        want = torch.autograd.grad((ref * cw).sum(), [f, v] + ([d] if with_dot else []))
        for a, b in zip(got, want):
            assert a.shape == b.shape and float((a - b).abs().max()) < 2e-5
    tv = TVLoss(0.7)
    for shape in ((1, 16, 33, 47), (1, 48, 5, 1), (1, 3, 2, 9), (1, 16, 33, 48), (1, 5, 7, 4), (1, 48, 300, 300)):        # W % 4 == 0: the float4 form
        x = torch.randn(shape, device="cuda", generator=g).requires_grad_(True)
        val = tv(x)
        xr = x.detach().cpu().double().requires_grad_(True)
        ref = tv(xr)                                                   # the reference's torch formulation (CPU, float64)
        assert abs(float(val) - float(ref)) < 1e-5 * max(1.0, abs(float(ref)))
        (gx,) = torch.autograd.grad(val * 3.0, x)
        (gr,) = torch.autograd.grad(ref * 3.0, xr)
        assert float((gx.cpu().double() - gr).abs().max()) < 1e-6


@pytest.mark.gpu
def test_fused_regularisers_match_the_torch_formulations(tiny_arrays, hyper_tiny):
    """tvr_l1_mean / tvr_line_ortho (density_L1, vector_comp_diffs; tensoRF.py:178-194) against the torch expressions they replace: values, the gradients of
    every factor under a non-trivial upstream weight, bit-reproducible sums, and the model methods taking the fused path."""
    from jittor_myc_nerfs_amd.losses import _L1MeanFn, _LineOrthoFn
    from conftest import make_model
    g = torch.Generator(device="cuda").manual_seed(3)
    planes = [torch.randn((1, 16, h, w), device="cuda", generator=g) * 0.1 for h, w in ((300, 300), (37, 53), (129, 64))]
    lines = [torch.randn((1, 16, n, 1), device="cuda", generator=g) * 0.1 for n in (300, 53, 129)]
    planes[0].view(-1)[:5] = 0.0                                       # exact zeros: sign(0) = 0 as torch.abs' gradient has it
    xs = [t.clone().requires_grad_(True) for pair in zip(planes, lines) for t in pair]
    ref = [t.detach().clone().requires_grad_(True) for t in xs]
    v = _L1MeanFn.apply(*xs)
    (8e-5 * v).backward()
    vr = sum(torch.mean(torch.abs(t)) for t in ref)
    (8e-5 * vr).backward()
    assert abs(float(v) - float(vr)) <= 2e-6 * abs(float(vr))
    for a, b in zip(xs, ref):
        assert torch.equal(a.grad, b.grad)                             # +-(8e-5 / n) or 0: the same single rounding in both
    assert float(_L1MeanFn.apply(*xs)) == float(v)                     # fixed order

    def vector_diffs(vs):                                              # the torch form kept in field.vectorDiffs
        total = 0
        for x in vs:
            n_comp, n_size = x.shape[1:-1]
            m = x.view(n_comp, n_size)
            dotp = m @ m.t()
            nd = dotp.view(-1)[1:].view(n_comp - 1, n_comp + 1)[..., :-1]
            total = total + torch.mean(torch.abs(nd))
        return total
    vs = [torch.randn((1, c, n, 1), device="cuda", generator=g).requires_grad_(True) for c, n in ((16, 300), (16, 53), (48, 300), (48, 129), (5, 7), (2, 301),
                                                                                                      (48, 321), (16, 1000))]   # nc * ns > 15 360 floats: ortho_kernel's global-memory path
    rs = [t.detach().double().requires_grad_(True) for t in vs]
    v = _LineOrthoFn.apply(*vs)
    (1e-4 * v).backward()
    vr = vector_diffs(rs)
    (1e-4 * vr).backward()
    assert abs(float(v) - float(vr)) <= 1e-5 * abs(float(vr))
    for a, b in zip(vs, rs):
        err = float((a.grad.double() - b.grad).abs().max()) / float(b.grad.abs().max())
        # (a Gram entry within rounding of zero may flip its sign between fp32 and fp64: measure against the largest entry)
        assert err < 1e-4, err
    assert float(_LineOrthoFn.apply(*vs)) == float(v)

    # the model's methods take the fused path on the device and agree with the torch loop they keep for other devices
    m = make_model(tiny_arrays, hyper_tiny)
    l1 = m.density_L1()
    od = m.vector_comp_diffs()
    assert type(l1.grad_fn).__name__.startswith("_L1MeanFn") and type(od.grad_fn).__name__.startswith("_LineOrthoFn")
    l1_ref = sum(torch.mean(torch.abs(m.density_plane[i])) + torch.mean(torch.abs(m.density_line[i])) for i in range(3))
    od_ref = m.vectorDiffs(m.density_line) + m.vectorDiffs(m.app_line)
    assert abs(float(l1) - float(l1_ref)) <= 2e-6 * abs(float(l1_ref)) and abs(float(od) - float(od_ref)) <= 1e-5 * abs(float(od_ref))


def test_fixed_order_reductions_are_bit_reproducible():
    """tvr_gemm_tn and tvr_tv_loss sum in a fixed order: repeated calls return identical bits (the scatter kernels use fp32 atomics and do not)."""
    from jittor_myc_nerfs_amd import TVLoss, _lib as L
    g = torch.Generator(device="cuda").manual_seed(9)
    A, B = torch.randn((200_003, 128), device="cuda", generator=g), torch.randn((200_003, 150), device="cuda", generator=g)
    outs = []
    for _ in range(3):
        junk = torch.full((8 << 20,), 0x7F, dtype=torch.uint8, device="cuda")        # perturb what the allocator hands out next
        out = torch.empty((128, 150), device="cuda")
        sc = torch.empty(L.lib().tvr_gemm_tn_scratch_bytes(128, 150, A.shape[0]), dtype=torch.uint8, device="cuda")
        L.check(L.lib().tvr_gemm_tn(A.data_ptr(), 128, 128, B.data_ptr(), 150, 150, A.shape[0], out.data_ptr(), sc.data_ptr(), sc.numel(), None), "gemm")
        outs.append(out.clone())
        del junk
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    x = torch.randn((1, 48, 301, 301), device="cuda", generator=g).requires_grad_(True)
    tv = TVLoss()
    vals, grads = [], []
    for _ in range(3):
        v = tv(x)
        (gx,) = torch.autograd.grad(v, x)
        vals.append(v.detach().clone()); grads.append(gx.clone())
    assert torch.equal(vals[0], vals[1]) and torch.equal(vals[0], vals[2]) and torch.equal(grads[0], grads[2])


def test_wide_weight_and_bias_gradients_through_gemm_tn():
    """_gemm_tn cuts products wider than 20 output tiles into column blocks; _colsum is gy^T 1 (the background network's M = 2.1e6 rows)."""
    from jittor_myc_nerfs_amd.autograd_ops import _LinearFn, _colsum, _gemm_tn
    g = torch.Generator(device="cuda").manual_seed(0)
    M = 1_050_001
    gy = torch.randn(M, 256, device="cuda", generator=g)
    x = torch.randn(M, 164, device="cuda", generator=g)
    want = (gy.double().t() @ x.double())
    got = _gemm_tn(gy, x)
    assert (got.double() - want).abs().max().item() < 2e-6 * M ** 0.5 * 4
    assert torch.equal(got, _gemm_tn(gy, x))                           # fixed summation order
    cs = _colsum(gy)
    assert (cs.double() - gy.double().sum(0)).abs().max().item() < 2e-6 * M ** 0.5 * 4
    # through the autograd function at this size (bias path switches to _colsum at M >= 1e6)
    w = torch.randn(64, 164, device="cuda", generator=g, requires_grad=True)
    b = torch.zeros(64, device="cuda", requires_grad=True)
    xin = x.clone().requires_grad_(True)
    y = _LinearFn.apply(xin, w, b)
    gyy = torch.randn(M, 64, device="cuda", generator=g)
    y.backward(gyy)
    assert (w.grad.double() - gyy.double().t() @ x.double()).abs().max().item() < 1e-2
    assert (b.grad.double() - gyy.double().sum(0)).abs().max().item() < 1e-2
    assert (xin.grad - gyy @ w.detach()).abs().max().item() < 1e-3


@pytest.mark.parametrize("model_name", ["TensorVMSplit", "REFTensoRF"])
def test_first_training_step_from_fresh_init_at_shipped_resolution(model_name):
    """configs/Scar.txt at iteration 0: N_voxel_init = 128^3, 0.1*randn factors, density_shift = -10 -> every weight is ~3e-5, below
    rayMarch_weight_thres = 1e-4, so the appearance queue is EMPTY (the reference's `if app_mask.any()`, tensorBase.py:515) and density
    learns through the white-background acc_map term alone.  One full step (forward, backward, fused Adam) must run and move density."""
    import jittor_myc_nerfs_amd as P
    from jittor_myc_nerfs_amd import rays as R, synthetic
    torch.manual_seed(20211202)
    aabb = [[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]]
    m = getattr(P, model_name)(aabb, [128, 128, 128], "cuda", density_n_comp=[16] * 3, appearance_n_comp=[48] * 3, app_dim=27, near_far=[2.0, 6.0],
                               shadingMode="MLP_Fea", alphaMask_thres=1e-4, density_shift=-10, distance_scale=25, pos_pe=6, view_pe=2, fea_pe=2,
                               featureC=128, step_ratio=0.5, fea2denseAct="softplus")
    rays = R.frame_rays(R.sphere_poses(8, 4.0)[1], 64, 64, synthetic.SCENE_A["camera_angle_x"]).to("cuda")
    gt = torch.rand((rays.shape[0], 3), device="cuda") * 0.5
    opt = torch.optim.Adam(m.get_optparam_groups(0.02, 0.001), betas=(0.9, 0.99), fused=True)
    before = [p.detach().clone() for p in m.density_plane]
    st = torch.zeros(8, dtype=torch.int64, device="cuda")
    with torch.no_grad():
        m.render_rays(rays, white_bg=True, N_samples=443, stats=st)
    assert int(st[2]) == 0 and int(st[0]) > 0, "a fresh 128^3 scene marches samples but queues no appearance sample"
    for _ in range(2):
        opt.zero_grad()
        rgb, _ = m(rays, is_train=True, white_bg=True, N_samples=443)              # train.py:225-226 (nSamples = 443 at 128^3)
        loss = torch.mean((rgb - gt) ** 2)
        loss.backward()
        for p in list(m.density_plane) + list(m.density_line):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all())
        assert float(sum(p.grad.abs().sum() for p in m.density_plane)) > 0, "no density gradient through acc_map"
        for p in list(m.app_plane) + [m.basis_mat.weight]:
            assert p.grad is None or float(p.grad.abs().sum()) == 0.0              # nothing was shaded
        opt.step()
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, m.density_plane))
    assert np.isfinite(float(loss))


@pytest.mark.parametrize("M", [10_007, 37])
def test_fused_mlp_training_kernels_match_float64_autograd(tiny_arrays, hyper_tiny, M):
    """tvr_mlp_train_forward / _backward (+ the tvr_gemm_tn reductions) against torch autograd of the same network in float64: rgb, the gradient
    w.r.t. h and all seven parameter gradients; and the forward equals the inference kernel bit for bit (tvr_app_feature -> tvr_mlp_render)."""
    from jittor_myc_nerfs_amd.autograd_ops import _MlpTrainFn
    m = make_model(tiny_arrays, hyper_tiny)
    g = torch.Generator(device="cuda").manual_seed(M)
    h = (torch.randn((M, 144), device="cuda", generator=g) * 0.7).requires_grad_(True)
    vd = torch.nn.functional.normalize(torch.randn((M, 3), device="cuda", generator=g), dim=-1)
    cw = torch.randn((M, 3), device="cuda", generator=g) * 3e-5          # the size of a real loss gradient (MSE mean over a 4096-ray batch)
    mlp = m.renderModule.mlp
    params = [m.basis_mat.weight, mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias, mlp[4].weight, mlp[4].bias]
    m._ensure_scene(force=True)
    rgb = _MlpTrainFn.apply(m, h, vd, *params)
    got = torch.autograd.grad((rgb * cw).sum(), [h] + params)
    # float64 reference
    hd = h.detach().double().requires_grad_(True)
    pd = [p.detach().double().requires_grad_(True) for p in params]
    def pe64(x):                                                        # tensorBase.py:9-15 in float64
        pts = (x[..., None] * torch.tensor([1.0, 2.0], dtype=torch.float64, device=x.device)).reshape(x.shape[0], -1)
        return torch.cat([torch.sin(pts), torch.cos(pts)], dim=-1)
    f = hd @ pd[0].t()
    X = torch.cat([f, vd.double(), pe64(f), pe64(vd.double())], dim=-1)  # :77-82
    ref = torch.sigmoid(torch.relu(torch.relu(X @ pd[1].t() + pd[2]) @ pd[3].t() + pd[4]) @ pd[5].t() + pd[6])
    assert float((rgb.detach().double() - ref.detach()).abs().max()) < 2e-5
    want = torch.autograd.grad((ref * cw.double()).sum(), [hd] + pd)
    names = ["dh", "basis_mat", "W1", "b1", "W2", "b2", "W3", "b3"]
    for n, a, b in zip(names, got, want):
        scale = max(float(b.abs().max()), 1e-30)
        err = float((a.double() - b).abs().max()) / scale
        print(f"M={M} {n:9s} rel-max-err {err:.2e} (max |g| {scale:.2e})")
        assert a.shape == b.shape and err < 2e-4, f"{n}: {err:.2e}"
    # bit-identical to the inference kernels
    with torch.no_grad():                                                # tvr_mlp_render on the features the training forward saved... recomputed by a library product
        rgb_inf = m.renderModule(None, vd, (h.detach() @ m.basis_mat.weight.t()))
    assert float((rgb_inf - rgb.detach()).abs().max()) < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,n_valid,K,w_off", [(40_003, 128, 128, 128, 0), (9_001, 80, 65, 128, 0), (9_001, 16, 3, 64, 0), (20_011, 128, 128, 128, 36), (33, 32, 32, 32, 0),
                                                  (5_000, 64, 64, 96, 0)])
def test_linear_dx_matches_float64(M, N, n_valid, K, w_off):
    """tvr_linear_dx — dX = (dY W) * (mask > 0), the input gradient of `relu(Linear(x))` over a tall batch — in its fp32-input form and in the fp16-split form at a
    power-of-two scale, against float64; strided operands, a column block of a wider weight, rows of W beyond n_valid taken as zero; and the saturation flag."""
    from jittor_myc_nerfs_amd.autograd_ops import _linear_dx
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    ldw = K + w_off + 4
    dY = torch.randn((M, N), device="cuda", generator=g) * 1e-4
    dY[:, n_valid:] = 0.0
    W = torch.randn((n_valid, ldw), device="cuda", generator=g)
    mask = torch.randn((M, K), device="cuda", generator=g)
    ref = (dY[:, :n_valid].double() @ W[:, w_off:w_off + K].double()) * (mask > 0)
    for scaled in (False, True):
        out = torch.full((M, K), float("nan"), device="cuda")
        scale = torch.tensor([2.0 ** 18], device="cuda") if scaled else None
        sat = torch.zeros(1, dtype=torch.int32, device="cuda")
        _linear_dx(dY, N, N, W, ldw, n_valid, K, mask, K, out, K, M, w_off=w_off, scale=scale, sat=sat if scaled else None)
        err = float((out.double() - ref).abs().max()) / float(ref.abs().max())
        assert err < 2e-6, (scaled, err)
        assert int(sat.item()) == 0
    # no mask; and a scale that drives dY out of fp16's range must raise the flag instead of returning garbage silently
    out = torch.empty((M, K), device="cuda")
    _linear_dx(dY, N, N, W, ldw, n_valid, K, None, 0, out, K, M, w_off=w_off)
    ref2 = dY[:, :n_valid].double() @ W[:, w_off:w_off + K].double()
    assert float((out.double() - ref2).abs().max()) / float(ref2.abs().max()) < 2e-6
    sat = torch.zeros(1, dtype=torch.int32, device="cuda")
    _linear_dx(dY, N, N, W, ldw, n_valid, K, None, 0, out, K, M, w_off=w_off, scale=torch.tensor([2.0 ** 40], device="cuda"), sat=sat)
    assert int(sat.item()) == 1


@pytest.mark.gpu
def test_gemm_tn_scaled_matches_the_fp32_form():
    """tvr_gemm_tn_scaled (fp16-split products of A * scale, divided by the scale again) against float64 and the fp32-input form, with the column sums riding along."""
    from jittor_myc_nerfs_amd.autograd_ops import _gemm_tn_bias_call, _gemm_tn_scaled_call
    g = torch.Generator(device="cuda").manual_seed(9)
    for M, Ka, Kb, lda in ((60_001, 128, 128, 128), (20_011, 80, 128, 80), (9_001, 64, 16, 80), (5_003, 16, 64, 16), (9_001, 128, 36, 128)):
        A = torch.randn((M, lda), device="cuda", generator=g) * 3e-5
        B = torch.randn((M, Kb), device="cuda", generator=g) * 2.0
        scale = torch.tensor([2.0 ** 16], device="cuda")
        C1, cs1 = _gemm_tn_scaled_call(A, lda, Ka, B, Kb, Kb, M, scale)
        C0, cs0 = _gemm_tn_bias_call(A, lda, Ka, B, Kb, Kb, M)
        ref = A[:, :Ka].double().t() @ B.double()
        rcs = A[:, :Ka].double().sum(0)
        for C, cs in ((C1, cs1), (C0, cs0)):
            assert float((C.double() - ref).abs().max()) / float(ref.abs().max()) < 3e-6
            assert float((cs.double() - rcs).abs().max()) / float(rcs.abs().max()) < 3e-6
        C2, none = _gemm_tn_scaled_call(A, lda, Ka, B, Kb, Kb, M, scale, bias=False)
        assert none is None and torch.equal(C2, C1)                    # fixed order: the ones column does not change the product


@pytest.mark.gpu
def test_colsum_and_empty_inputs_of_the_new_entry_points():
    """tvr_colsum against float64 (strided, offset columns, one row, fixed order); and the zero-size cases of the round-3 entry points return cleanly."""
    from jittor_myc_nerfs_amd import _lib as L
    from jittor_myc_nerfs_amd.autograd_ops import _colsum_call, _linear_dx
    g = torch.Generator(device="cuda").manual_seed(2)
    for M, lda, K, off in ((100_003, 80, 72, 0), (9_001, 128, 128, 0), (5_000, 80, 1, 64), (1, 16, 3, 0)):
        A = torch.randn((M, lda), device="cuda", generator=g)
        cs = _colsum_call(A, lda, K, M, a_off=off)
        ref = A[:, off:off + K].double().sum(0)
        assert float((cs.double() - ref).abs().max()) < 2e-6 * max(1.0, float(ref.abs().max()))
        assert torch.equal(cs, _colsum_call(A, lda, K, M, a_off=off))
    lib = L.lib()
    out = torch.zeros((4, 32), device="cuda")
    _linear_dx(out, 32, 32, out, 32, 4, 32, None, 0, out, 32, 0)                       # M = 0: nothing launched
    z = torch.zeros(8, device="cuda")
    assert lib.tvr_colsum(None, 4, 4, 0, z.data_ptr(), z.data_ptr(), 32, None) == -3                                         # scratch too small: refused
    sc = torch.empty(lib.tvr_colsum_scratch_bytes(), dtype=torch.uint8, device="cuda")
    assert lib.tvr_colsum(None, 4, 4, 0, z.data_ptr(), sc.data_ptr(), sc.numel(), None) == 0 and float(z[:4].abs().max()) == 0.0   # M = 0: zeros
