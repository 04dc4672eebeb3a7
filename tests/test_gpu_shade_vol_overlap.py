"""GPU (-m gpu): the volume shade kernel at the queue lengths where its waves take a second and a third tile (twelve waves per workgroup, three per
SIMD, against the factored kernel's eight).  The approach is test_gpu_appearance_volume.py::test_partial_and_empty_tiles': rays picked by their own appearance-sample
counts so that the queue holds exactly 32 T and 32 T + 1 entries; every call equals the rays' rows of ONE big call bit for bit, is finite, and lies within RGB_TIGHT
of the factored kernel's picture.  A launch is 256 workgroups: 2 048 waves of the factored kernel, 3 072 of the volume kernel, so that
  T = 2 047 / 2 048 (+ 1 entry)   the last wave of an 8-wave grid has no tile / every wave one (and one wave one entry of a second)
  T = 3 071 / 3 072 (+ 1 entry)   the same for the 12-wave grid
  T = 6 144, 9 216 (+ 1 entry)    a third (fourth) tile at 8 waves, a second and third at 12, and one entry of the next round."""
import numpy as np
import pytest
import torch

from conftest import TINY, make_model
from test_gpu_appearance_volume import _many_rays, _subset_with_sum
from test_gpu_parity import RGB_TIGHT, _np

pytestmark = pytest.mark.gpu

TILE = 32
QUEUE = 300_000                                  # entries the big call's queue must hold: 32 x 9 216 + 1 and a margin for the subset sum
TILES = (2047, 2048, 3071, 3072, 6144, 9216)


@pytest.fixture(scope="module")
def big(tiny_dump, tiny_arrays, hyper_tiny):
    """The tiny scene with the volume attached, the dump's rays copied (perturbed) until they shade QUEUE samples, and the one big call every case is compared with."""
    m = make_model(tiny_arrays, hyper_tiny)
    f = make_model(tiny_arrays, hyper_tiny)
    f.appearance_volume = False
    m.render_piece_rays = f.render_piece_rays = 0
    S = TINY["N_samples"]
    kw = dict(white_bg=True, N_samples=S, eps_T=0.0, dense=True)
    probe = torch.tensor(_many_rays(tiny_dump, 8), device="cuda")
    per_copy = int((m.render_rays(probe, **kw)[2]["weight"] > m.rayMarch_weight_thres).sum()) / 8.0
    copies = int(np.ceil(1.15 * QUEUE / per_copy))
    rays = torch.tensor(_many_rays(tiny_dump, copies), device="cuda")
    rgb, depth, d = m.render_rays(rays, **kw)
    assert m._fvol is not None
    counts = _np((d["weight"] > m.rayMarch_weight_thres).sum(1)).astype(np.int64)
    assert int(counts.sum()) >= QUEUE, (copies, int(counts.sum()))
    torch.cuda.synchronize()
    return dict(m=m, f=f, S=S, rays=rays, rgb=rgb.clone(), depth=depth.clone(), srgb=d["rgb"].clone(), counts=counts, cum=np.concatenate([[0], np.cumsum(counts)]))


def _rays_shading(big, total):
    """Indices of rays that shade exactly `total` samples: a prefix of the list, then a subset sum over the next few hundred rays for the remainder."""
    counts, cum = big["counts"], big["cum"]
    p = int(np.searchsorted(cum, total - 4 * TINY["N_samples"], side="right")) - 1      # the prefix stops a few rays' worth short of the total
    p = max(p, 0)
    rest = _subset_with_sum(counts[p:p + 400].tolist(), total - int(cum[p]))
    assert rest is not None, f"no subset of rays {p} .. {p + 400} shades the remaining {total - int(cum[p])} samples"
    return list(range(p)) + [p + i for i in rest]


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("T", TILES)
def test_second_and_third_tiles(big, T, extra):
    m, f, S, rays = big["m"], big["f"], big["S"], big["rays"]
    n = TILE * T + extra
    idx = _rays_shading(big, n)
    sub = rays[idx].contiguous()
    assert int(big["counts"][idx].sum()) == n
    r, dp, dd = m.render_rays(sub, white_bg=True, N_samples=S, eps_T=0.0, dense=True)
    assert m._fvol is not None
    assert int((dd["weight"] > m.rayMarch_weight_thres).sum()) == n
    assert torch.equal(r, big["rgb"][idx]) and torch.equal(dp, big["depth"][idx]) and torch.equal(dd["rgb"], big["srgb"][idx]), (T, extra)
    # one of the calls once more in pieces (a call with `dense` is never cut; a ray shades at most S samples, so there are more than six pieces' worth of rays):
    # two shade kernels at once on the library's two streams
    pieces = (T, extra) == (6144, 1)
    if pieces:
        assert len(idx) >= 6 * 512
        m.render_piece_rays = 512
        try:
            rp, dpp = m.render_rays(sub, white_bg=True, N_samples=S, eps_T=0.0)
        finally:
            m.render_piece_rays = 0
        assert torch.equal(rp, r) and torch.equal(dpp, dp)
    rf, _ = f.render_rays(sub, white_bg=True, N_samples=S, eps_T=0.0)
    assert f._fvol is None
    err = float((r - rf).abs().max())
    print(f"    T={T} + {extra}: {len(idx)} rays, {n} entries{', in pieces' if pieces else ''}; against the factored kernel {err:.3g}")
    assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(dd["rgb"]).all()) and err < RGB_TIGHT, (T, extra)
