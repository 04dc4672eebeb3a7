"""GPU (-m gpu): tvr_render_normals (csrc/tvr_normals.hip) and TensorBase.render_normals — the normal map of a ray batch.

The oracle is the tests' own fp64 restatement (tests/normal_map_common.py); everything is on the TINY grid (16 x 20 x 24) at S = 48.  Per ray the bar is

    |N - N64|_inf <= max(4 max|N32 - N64|, 1e-5) + 1e-4 f_i   (+ eps_T with early termination)

computed from the fp64 and fp32 restatements alone (normal_map_common.bar): the floor 1e-5 is the project's bar on acc for the same march (tests/test_gpu_cp.py) —
|n_e| <= 1, so a weight error enters N no larger than it enters acc; f_i counts the samples of ray i whose `weight > thres` mask differs between
render_rays(dense=True) and the fp64 restatement, each of which carries at most thres = 1e-4 (at most 2 in a whole batch, the cap of tests/test_gpu_cp.py); the
transmittance left when a ray stops at eps_T bounds the summed weight of everything skipped.  acc and depth are the march's own and are held bit-equal to
render_rays(dense=True)'s.  On the CPU the restatements give max|N32 - N64| = 2e-7 .. 6e-7, smallest |g| over contributing samples >= 1.3, no mask difference,
38 .. 56 of the 64 rays with entries — except the rank-(1, 1) CP scene, where 20 rays have entries (the guard below asks 15 there, as tests/test_gpu_cp.py lowers
its own count for that rank)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cp_common as CC
import gradient_common as GC
import normal_map_common as NC
from conftest import TINY, make_model

pytestmark = pytest.mark.gpu

S = NC.S


def _check(m, rays, e64, e32, label, jitter=None, modes=(0.0, None)):
    """render_normals against the fp64 restatement in exact mode and with the default eps_T; acc / depth against render_rays(dense=True) bit for bit"""
    jit = None if jitter is None else torch.tensor(jitter, device="cuda")
    for eps in modes:
        eps_val = 0.0 if eps == 0.0 else float(m.rayMarch_weight_thres)
        N, acc, depth = m.render_normals(rays, N_samples=S, jitter=jit, eps_T=eps)
        _, depth_r, d = m.render_rays(rays, white_bg=True, N_samples=S, jitter=jit, eps_T=eps, dense=True)
        torch.cuda.synchronize()
        assert N.shape == (rays.shape[0], 3) and acc.shape == (rays.shape[0],) and depth.shape == (rays.shape[0],)
        assert bool(torch.isfinite(N).all())
        flips = (d["weight"].cpu() > NC.THRES) != e64["app"]
        f = flips.sum(1)
        assert int(f.sum()) <= NC.MAX_FLIPS, f"app-mask Hamming distance {int(f.sum())}"
        tol = NC.bar(e32["N"], e64["N"], f, eps_val)
        err = (N.cpu().double() - e64["N"]).abs().max(-1).values
        print(f"    {label} / eps_T = {eps_val:g}: max |N64| = {float(e64['N'].norm(dim=-1).max()):.4g}, fp32 restatement error = "
              f"{float((e32['N'].double() - e64['N']).abs().max()):.3g}, kernel error = {float(err.max()):.3g}, allowance = {float(tol.min()):.3g} "
              f"(+ 1e-4 per flipped sample: {int(f.sum())} in the batch), smallest |g| = {e64['gmin']:.3g}")
        assert bool((err <= tol).all()), (label, eps, float((err - tol).max()))
        assert torch.equal(acc, d["acc"]) and torch.equal(depth, depth_r)                     # the same march
        assert bool((N.norm(dim=-1) <= acc + 1e-6).all())
    return N, acc, depth


@pytest.mark.parametrize("name", NC.SCENES)
def test_normal_map_against_fp64_restatement(name):
    e64, e32 = NC.tiny_case(name)
    cnt = e64["app"].sum(1)
    assert int((cnt > 0).sum()) >= (15 if name == "cp1" else 30), int((cnt > 0).sum())        # the scene has surfaces: nothing below is vacuous
    assert float(e64["N"].norm(dim=-1).max()) > 0.9                                             # (|N| is the vector's length, as in |N_i| <= acc_i)
    m = NC.make_model(name)
    if name == "ref":
        assert type(m).__name__ == "REFTensoRF"
    rays = torch.tensor(NC.golden_rays(), device="cuda")
    _check(m, rays, e64, e32, name)


@pytest.mark.parametrize("name", ["vm", "cp5"])
@pytest.mark.parametrize("am,jit", [(False, False), (True, False), (True, True), (False, True)])
def test_normal_map_edge_fixture(tiny_edge, name, am, jit):
    base, kind = NC.scene_arrays(name)
    arrs = dict(base)
    if am:
        arrs["alpha_volume"], arrs["alpha_aabb"] = tiny_edge["alpha_volume"], tiny_edge["alpha_aabb"]
    m = CC.make_cp_model(arrs, NC.hyper()) if kind == "cp" else make_model(arrs, NC.hyper())
    jitter = tiny_edge["jitter"] if jit else None
    e64, e32 = (NC.normal_map_restatement(arrs, NC.hyper(), tiny_edge["rays"], S, kind, jitter=jitter, dtype=dt) for dt in (torch.float64, torch.float32))
    assert int(e64["app"].sum()) > 50
    rays = torch.tensor(tiny_edge["rays"], device="cuda")
    assert rays.shape[0] == 23
    N, acc, depth = _check(m, rays, e64, e32, f"{name} am={int(am)} jit={int(jit)}", jitter=jitter)
    assert bool((N[3] == 0).all()) and float(acc[3]) == 0.0 and float(depth[3]) == float(tiny_edge["rays"][3, 5])   # the ray that misses the box


@pytest.mark.parametrize("name", ["vm", "cp5"])
def test_normal_map_is_independent_of_batch_chunk_and_repetition(name):
    m = NC.make_model(name)
    rays = torch.tensor(NC.golden_rays(), device="cuda")
    ref = m.render_normals(rays, N_samples=S, eps_T=0.0)
    assert int((ref[0].abs().sum(-1) > 0).sum()) >= 30
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))
    assert same(m.render_normals(rays, N_samples=S, eps_T=0.0), ref)                            # a second identical call
    assert same(m.render_normals(rays, N_samples=S, eps_T=0.0, chunk=16), ref)                  # chunks of 16 (and 7: a ragged last one)
    assert same(m.render_normals(rays, N_samples=S, eps_T=0.0, chunk=7), ref)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(3)).cuda()
    out = m.render_normals(rays[perm].contiguous(), N_samples=S, eps_T=0.0)
    inv = torch.argsort(perm)
    assert same([o[inv] for o in out], ref)                                                     # a shuffled batch, un-shuffled
    for n in (1, 63, 64):
        assert same(m.render_normals(rays[:n].contiguous(), N_samples=S, eps_T=0.0), [r[:n] for r in ref]), n
    assert same(m.render_normals(rays[40:41].contiguous(), N_samples=S, eps_T=0.0), [r[40:41] for r in ref])
    cell = GC.cell(TINY["gridSize"]).tolist()
    assert same(m.render_normals(rays, N_samples=S, eps_T=0.0, half_width=cell), ref)           # the default half width is one cell
    other = m.render_normals(rays, N_samples=S, eps_T=0.0, half_width=[0.5 * c for c in cell])
    assert not torch.equal(other[0], ref[0]) and torch.equal(other[1], ref[1])
    with pytest.raises(ValueError):
        m.render_normals(rays, N_samples=S, half_width=[0.1, 0.1])
    e = m.render_normals(rays[:0], N_samples=S)
    assert e[0].shape == (0, 3) and e[1].shape == (0,) and e[2].shape == (0,)


def test_normal_map_of_a_gaussian_blob():
    e64, e32 = NC.tiny_case("blob")
    assert int((e64["app"].sum(1) > 0).sum()) >= 30 and float(e64["N"].norm(dim=-1).max()) > 0.9
    m = NC.make_model("blob")
    rays = torch.tensor(NC.golden_rays(), device="cuda")
    N, acc, _ = _check(m, rays, e64, e32, "blob")
    assert bool(torch.isfinite(N).all()) and bool((N.norm(dim=-1) <= acc + 1e-6).all())


def test_normal_map_argument_checks_come_before_any_launch(tiny_arrays, tiny_npp_arrays):
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    rays = torch.tensor(NC.golden_rays(), device="cuda")
    n = rays.shape[0]
    for m in (make_model(tiny_arrays, NC.hyper()), CC.make_cp_model(CC.cp_arrays(5, 50), NC.hyper())):
        sc = m._ensure_scene()
        nbytes = lib.tvr_render_normals_scratch_bytes(sc, n, S)
        assert nbytes < lib.tvr_render_scratch_bytes(sc, n, S)                                  # neither q_out nor the CP staging regions
        scratch = L.dev_bytes(nbytes, "cuda")
        normal = torch.full((n, 3), -7.0, device="cuda")
        acc = torch.full((n,), -7.0, device="cuda")
        depth = torch.full((n,), -7.0, device="cuda")
        good = (C.c_float * 3)(0.1, 0.1, 0.1)

        def call(hw, count=n, S_=S, eps=0.0, rp=rays.data_ptr(), np_=normal.data_ptr(), nb=None, ab=None, db=None, sp=scratch.data_ptr(), sb=nbytes, scene=sc):
            return lib.tvr_render_normals(scene, rp, count, S_, None, eps, hw, np_, L.nbytes(normal) if nb is None else nb, acc.data_ptr(),
                                          L.nbytes(acc) if ab is None else ab, depth.data_ptr(), L.nbytes(depth) if db is None else db, sp, sb, None)

        for bad in (0.0, -0.1, float("nan"), float("inf")):
            for k in range(3):
                hw = (C.c_float * 3)(0.1, 0.1, 0.1)
                hw[k] = bad
                assert call(C.byref(hw)) == -1 and b"half_width" in lib.tvr_last_error(), (bad, k)
        assert call(None) == -1 and b"half_width" in lib.tvr_last_error()
        assert call(C.byref(good), scene=None) == -1
        assert call(C.byref(good), count=-1) == -1
        assert call(C.byref(good), rp=None) == -1 and call(C.byref(good), np_=None) == -1
        assert call(C.byref(good), S_=0) == -1 and call(C.byref(good), S_=4097) == -1
        assert call(C.byref(good), eps=-1.0) == -1 and call(C.byref(good), eps=1.0) == -1
        assert call(C.byref(good), nb=n * 12 - 4) == -3 and b"normal_out" in lib.tvr_last_error()
        assert call(C.byref(good), ab=n * 4 - 4) == -3 and b"acc_out" in lib.tvr_last_error()
        assert call(C.byref(good), db=n * 4 - 4) == -3 and b"depth_out" in lib.tvr_last_error()
        assert call(C.byref(good), sb=nbytes - 256) == -3 and b"scratch" in lib.tvr_last_error()
        assert call(C.byref(good), sp=None) == -3
        assert call(C.byref(good), sp=scratch.data_ptr() + 16, sb=nbytes - 16) == -3            # undersized, and misaligned
        torch.cuda.synchronize()
        assert bool((normal == -7.0).all()) and bool((acc == -7.0).all()) and bool((depth == -7.0).all())      # nothing was launched
        assert call(C.byref(good), count=0) == 0
        assert lib.tvr_render_normals(sc, None, 0, S, None, 0.0, C.byref(good), None, 0, None, 0, None, 0, None, 0, None) == 0
        torch.cuda.synchronize()
        assert bool((normal == -7.0).all()) and bool((acc == -7.0).all()) and bool((depth == -7.0).all())
        assert call(C.byref(good)) == 0                                                         # and the same call with everything right runs
        torch.cuda.synchronize()
        assert not bool((normal == -7.0).any()) and not bool((acc == -7.0).any()) and not bool((depth == -7.0).any())
        got = m.render_normals(rays, N_samples=S, eps_T=0.0, half_width=0.1)
        assert torch.equal(got[0], normal) and torch.equal(got[1], acc) and torch.equal(got[2], depth)
        # acc_out / depth_out NULL: the same normals
        n2 = torch.full((n, 3), -7.0, device="cuda")
        assert lib.tvr_render_normals(sc, rays.data_ptr(), n, S, None, 0.0, C.byref(good), n2.data_ptr(), L.nbytes(n2), None, 0, None, 0, scratch.data_ptr(), nbytes,
                                      None) == 0
        torch.cuda.synchronize()
        assert torch.equal(n2, normal)
        with pytest.raises(L.TvrError):
            m.render_normals(rays, N_samples=S, half_width=0.0)
    npp = make_model(tiny_npp_arrays, NC.hyper())
    assert type(npp).__name__ == "NerfPlusPlus"
    with pytest.raises(NotImplementedError, match="NerfPlusPlus"):
        npp.render_normals(rays, N_samples=S)
