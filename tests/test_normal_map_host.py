"""CPU: the host side of the normal-map feature — the two C symbols (declared, exported, in the ctypes table, refusing bad arguments without a GPU), the refusals of
TensorBase.render_normals off the device, evaluation.normal_map_to_rgb8 on hand-computed values, evaluation(..., normal_maps=True) with a stub model, and the
reconstruct option.  The kernel itself: tests/test_gpu_normal_map.py."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import cp_common as CC
from conftest import TINY, make_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tvr_render_normals_scratch_bytes", "tvr_render_normals")


def _hyper():
    from jittor_myc_nerfs_amd import synthetic
    return dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=TINY["step_ratio"])


def test_symbols_are_declared_exported_and_in_the_ctypes_table():
    from jittor_myc_nerfs_amd import _lib as L
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tvr.h")).read(), flags=re.S)
    raw = C.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", src), f"include/tvr.h does not declare {n}"
        assert hasattr(raw, n), f"libtvr.so does not export {n}"
        assert n in L.SYMBOLS
    assert L.SYMBOLS["tvr_render_normals_scratch_bytes"][0] is C.c_size_t and len(L.SYMBOLS["tvr_render_normals"][1]) == 16
    assert L.lib().tvr_version() == 141                                      # additive exports


def test_c_calls_refuse_bad_arguments_without_a_gpu():
    from jittor_myc_nerfs_amd import _lib as L
    lib = L.lib()
    size = lib.tvr_render_normals_scratch_bytes
    assert size(None, 0, 48) == 256 and size(None, -1, 48) == 256 and size(None, 64, 0) == 256
    n, S = 4096, 512
    # header + four per-ray arrays + 20 B per sample of capacity (q_pos 16, q_ray 4), each region rounded up to 256 B: nothing else
    assert n * S * 20 + 4 * n * 4 + 256 <= size(None, n, S) <= n * S * 20 + 4 * n * 4 + 256 + 7 * 256
    assert size(None, n, S) < lib.tvr_render_scratch_bytes(None, n, S)       # no q_out, no q_j
    assert size(None, 63, 48) <= size(None, 64, 48) < size(None, 64, 49)
    good = (C.c_float * 3)(0.1, 0.1, 0.1)
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    # a NULL scene is refused before anything else is looked at, whatever the other arguments are
    for args in ((None, p, 4, 48, None, 0.0, C.byref(good), p, 48, None, 0, None, 0, p, 256, None),
                 (None, None, 0, 48, None, 0.0, C.byref(good), None, 0, None, 0, None, 0, None, 0, None),
                 (None, p, -1, 0, None, -1.0, None, None, 0, None, 0, None, 0, None, 0, None)):
        assert lib.tvr_render_normals(*args) == -1
        assert b"tvr_render_normals" in lib.tvr_last_error() and b"scene" in lib.tvr_last_error()
    assert all(v == 0.0 for v in buf)


def test_render_normals_has_no_cpu_fallback(tiny_arrays, tiny_npp_arrays):
    from jittor_myc_nerfs_amd import _lib as L
    rays = torch.tensor([[0.0, 0.0, -4.0, 0.0, 0.0, 1.0]])
    for m in (make_model(tiny_arrays, _hyper(), device="cpu"), CC.make_cp_model(CC.cp_arrays(5, 50), _hyper(), device="cpu")):
        with pytest.raises(L.TvrError):
            m.render_normals(rays)
    npp = make_model(tiny_npp_arrays, _hyper(), device="cpu")
    assert type(npp).__name__ == "NerfPlusPlus"
    with pytest.raises(NotImplementedError, match="NerfPlusPlus"):
        npp.render_normals(rays)


def test_normal_map_to_rgb8_on_hand_computed_values():
    import jittor_myc_nerfs_amd as pkg
    from jittor_myc_nerfs_amd.evaluation import normal_map_to_rgb8
    assert pkg.normal_map_to_rgb8 is normal_map_to_rgb8
    N = torch.tensor([[0.0, 0.0, 0.0],          # acc = 0: the background
                      [0.0, 0.0, 1.0],          # facing +z, opaque: (128, 128, 255)  (127.5 rounds to even)
                      [-1.0, 0.0, 0.0],         # facing -x, opaque: (0, 128, 128)
                      [0.0, 0.5, 0.0],          # half opaque, facing +y: 0.5 * (0, .5, 0) + 0.25 + 0.5 bg
                      [0.6, -0.6, 0.2],         # opaque, oblique: 0.5 * (.6, -.6, .2) + 0.5 = (.8, .2, .6)
                      [2.0, -2.0, 0.0]])        # out of range: clamped
    acc = torch.tensor([0.0, 1.0, 1.0, 0.5, 1.0, 1.0])
    white = normal_map_to_rgb8(N, acc, white_bg=True)
    black = normal_map_to_rgb8(N, acc, white_bg=False)
    assert white.dtype == torch.uint8 and white.shape == (6, 3)
    assert white.tolist() == [[255, 255, 255], [128, 128, 255], [0, 128, 128], [191, 255, 191], [204, 51, 153], [255, 0, 128]]
    #   row 3, white: (0.25 + 0.5, 0.25 + 0.25 + 0.5, 0.75) = (0.75, 1.0, 0.75) -> 191.25, 255, 191.25;  black: (0.25, 0.5, 0.25) -> 63.75, 127.5 (-> 128), 63.75
    assert black.tolist() == [[0, 0, 0], [128, 128, 255], [0, 128, 128], [64, 128, 64], [204, 51, 153], [255, 0, 128]]
    assert torch.equal(normal_map_to_rgb8(N, acc), white)                     # white is the default
    img = normal_map_to_rgb8(N.view(2, 3, 3), acc.view(2, 3))                 # any leading shape
    assert img.shape == (2, 3, 3) and torch.equal(img.view(6, 3), white)
    before = (N.clone(), acc.clone())
    normal_map_to_rgb8(N, acc)
    assert torch.equal(N, before[0]) and torch.equal(acc, before[1])          # pure


class _StubModel:
    """what evaluation() needs of a model when the renderer is a stub too: render_normals with fixed tensors"""

    def __init__(self, normal, acc):
        self.normal, self.acc, self.calls = normal, acc, []

    def render_normals(self, rays, N_samples=-1, **kw):
        self.calls.append((tuple(rays.shape), N_samples))
        return self.normal, self.acc, torch.zeros_like(self.acc)


def _stub_setup(H=3, W=4):
    g = torch.Generator().manual_seed(11)
    normal = torch.rand((H * W, 3), generator=g) * 2 - 1
    acc = torch.rand((H * W,), generator=g)
    normal = normal / normal.norm(dim=-1, keepdim=True) * acc[:, None]
    ds = types.SimpleNamespace(all_rays=torch.zeros((1, H * W, 6)), all_rgbs=[], img_wh=(W, H), near_far=[2.0, 6.0], focal=5.0)
    rgb = torch.rand((H * W, 3), generator=g)

    def renderer(rays, tensorf, chunk=1024, N_samples=-1, ndc_ray=False, white_bg=True, device="cpu"):
        return rgb, None, torch.full((rays.shape[0],), 3.0), None, None

    return _StubModel(normal, acc), ds, renderer, normal, acc


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize("white_bg", [True, False])
def test_evaluation_writes_the_encoded_normal_map(tmp_path, white_bg):
    from PIL import Image
    from jittor_myc_nerfs_amd.evaluation import evaluation, evaluation_path, normal_map_to_rgb8
    H, W = 3, 4
    m, ds, renderer, normal, acc = _stub_setup(H, W)
    plain, with_n = str(tmp_path / "plain"), str(tmp_path / "normals")
    evaluation(ds, m, None, renderer, plain, N_vis=-1, N_samples=7, white_bg=white_bg, device="cpu")
    assert m.calls == []                                                      # the default: render_normals is never called, no new file
    evaluation(ds, m, None, renderer, with_n, N_vis=-1, N_samples=7, white_bg=white_bg, device="cpu", normal_maps=True)
    assert m.calls == [((H * W, 6), 7)]
    assert _files(with_n) == sorted(_files(plain) + ["normal/000.png"])
    for f in _files(plain):                                                   # with the flag, every other file holds the same bytes
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(with_n, f), "rb").read(), f
    got = np.asarray(Image.open(os.path.join(with_n, "normal", "000.png")))
    want = normal_map_to_rgb8(normal, acc, white_bg).reshape(H, W, 3).numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    # without savePath nothing is rendered or written
    evaluation(ds, m, None, renderer, None, N_vis=-1, N_samples=7, white_bg=white_bg, device="cpu", normal_maps=True)
    assert len(m.calls) == 1
    # evaluation_path: the same file beside its images
    out = str(tmp_path / "path")
    frames = evaluation_path(ds, m, [np.eye(4, dtype=np.float32)], renderer, out, N_samples=7, white_bg=white_bg, device="cpu", normal_maps=True)
    assert len(frames) == 1 and len(m.calls) == 2
    assert np.array_equal(np.asarray(Image.open(os.path.join(out, "normal", "000.png"))), want)
    out2 = str(tmp_path / "path_plain")
    evaluation_path(ds, m, [np.eye(4, dtype=np.float32)], renderer, out2, N_samples=7, white_bg=white_bg, device="cpu")
    assert len(m.calls) == 2 and not os.path.exists(os.path.join(out2, "normal"))


def test_reconstruct_accepts_render_normals_and_refuses_nerfplusplus():
    from jittor_myc_nerfs_amd import reconstruct
    assert reconstruct.config_parser([]).render_normals == 0
    args = reconstruct.config_parser(["--render_normals", "1", "--render_only", "1", "--render_test", "1"])
    assert args.render_normals == 1
    assert reconstruct._normal_maps_wanted(args) is True
    assert reconstruct._normal_maps_wanted(reconstruct.config_parser(["--model_name", "NerfPlusPlus"])) is False
    npp = reconstruct.config_parser(["--render_normals", "1", "--model_name", "NerfPlusPlus"])
    with pytest.raises(NotImplementedError, match="NerfPlusPlus"):
        reconstruct._normal_maps_wanted(npp)
    npp.dataset_name, npp.datadir = "blender", "/nonexistent/never/opened"
    with pytest.raises(NotImplementedError, match="NerfPlusPlus"):          # refused before any data is touched
        reconstruct.reconstruction(npp, device="cpu")
