"""Every refusal of the training entry points of csrc/tvr_train_api.hip (and of tvr_march_forward(_z), which shares their march-argument check), byte for byte.

tests/golden/train_api_errors.json holds rows (entry point, case, status, message).  They were recorded from the library built from the commit BEFORE the training
entry points moved out of tvr_api.hip and their argument checks were folded into shared helpers, never from the code under test:
    TVR_LIB_PATH=<that libtvr.so> python tests/test_train_api_errors_host.py record host          (no GPU)
    TVR_LIB_PATH=<that libtvr.so> python tests/test_train_api_errors_host.py record gpu [path]    (on an MI355X, in a run of its own)
The tests replay every case against the built library and assert that the status and the bytes of tvr_last_error() are the recorded ones.

Two parts.
  No GPU: every case that is refused without an updated scene.  The entry points that take no scene, and of those that take one the checks in front of "scene is NULL
  or tvr_scene_update has not run": the byte checks of the outputs, the CP / not-CP refusals (on scenes made by tvr_scene_create / tvr_cp_scene_create over a
  fabricated, aligned packed pointer: neither call launches anything) and that refusal itself.  Pointers are fabricated integers and are never dereferenced.
  `gpu`: the checks behind it, on the smallest scenes the library accepts (grid 2 x 2 x 2, 16 / 48 components: TensorVMSplit, REFTensoRF, a CP scene and a
  TensorVMSplit scene with 24 appearance components), each updated once, with n_rays = 4, n_samples = 8, m = app_cap = 4.  Every pointer is a real, zeroed device
  allocation of the size the good call needs (a misaligned pointer: the same allocation plus 16 bytes; a short size: one byte less) and the rays miss the scene's box, so
  a case that reached a launch — the recorded library tests the gradient output pointers of tvr_march_backward / tvr_app_h_backward behind its kernels, and
  tvr_train_backward runs its steps 1 - 3 before it looks at them — runs on valid memory with nothing to march.  The call whose arguments are all good is never made.
No case may return TVR_ERR_HIP.

Per entry point (the layout of tests/test_mesh_api_errors_host.py): `ladder` starts with every argument of its groups bad at once, which pins the check that comes
first, and repairs one group per step in the order the checks read them; `extra` holds the other ways an argument can be wrong, each on otherwise good arguments."""
import ctypes as C
import functools
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TABLE = os.path.join(HERE, "golden", "train_api_errors.json")
OK, ERR_HIP = 0, -2

PTR, MISALIGNED, ODD = 1 << 20, (1 << 20) + 16, (1 << 20) + 4      # 256-byte aligned; 16- but not 256-byte aligned; not 16-byte aligned
BIG = 1 << 40                                                      # a byte count no check finds short
N_RAYS, S, M = 4, 8, 4                                             # rays, samples per ray, entries (= app_cap)
ROWS_ABOVE = (1 << 32) // 576 + 1                                  # the first m with m * 576 >= 2^32
GPU = "gpu:"                                                       # prefix of the cases of the gpu part in the table

MOVED = ["tvr_grad_scratch_bytes", "tvr_march_backward", "tvr_march_backward_z", "tvr_app_h_forward", "tvr_app_h_backward", "tvr_mlp_train_image_bytes",
         "tvr_mlp_train_forward", "tvr_mlp_train_forward_ref", "tvr_mlp_train_backward", "tvr_mlp_train_backward_ref", "tvr_cp_grad_scratch_bytes",
         "tvr_cp_march_forward", "tvr_cp_march_backward", "tvr_cp_app_backward", "tvr_train_work_bytes", "tvr_train_work_describe", "tvr_train_forward",
         "tvr_train_backward", "tvr_pe_concat", "tvr_pe_concat_backward", "tvr_tv_loss", "tvr_l1_mean_scratch_bytes", "tvr_l1_mean", "tvr_l1_mean_backward",
         "tvr_line_ortho", "tvr_line_ortho_backward", "tvr_linear_dx", "tvr_colsum_scratch_bytes", "tvr_colsum", "tvr_gemm_tn_scratch_bytes", "tvr_gemm_tn",
         "tvr_gemm_tn_scaled", "tvr_gemm_tn_bias"]
NEVER_REFUSE = ["tvr_mlp_train_image_bytes", "tvr_colsum_scratch_bytes", "tvr_l1_mean_scratch_bytes"]     # no argument, or 0 without a message
SHARE_A_CHECK = ["tvr_march_forward", "tvr_march_forward_z"]       # stayed in tvr_api.hip; their march arguments go through the one copy of the check


def _lib():
    from jittor_myc_nerfs_amd import _lib as L
    return L


class Entry:
    """One entry point: `params` = [(name, good value, bad value)] in the order of the C signature; `ladder` = groups of parameter names in the order the checks read
    them (a parameter outside every group keeps its good value); `extra` = {case: {name: value}} on otherwise good arguments."""

    def __init__(self, params, ladder, extra):
        self.names = [p[0] for p in params]
        self.good = {p[0]: p[1] for p in params}
        self.bad = {p[0]: p[2] for p in params}
        self.ladder, self.extra = ladder, extra
        self.rungs = {n for group in ladder for n in group}
        for n in self.rungs:
            assert n in self.good and self.bad[n] is not self.good[n], n
        for kw in extra.values():
            assert set(kw) <= set(self.good), kw

    def cases(self):
        for k in range(len(self.ladder)):
            repaired = {n for group in self.ladder[:k] for n in group}
            yield f"ladder_{k:02d}", [self.bad[n] if n in self.rungs - repaired else self.good[n] for n in self.names]
        for case, kw in self.extra.items():
            yield case, [kw.get(n, self.good[n]) for n in self.names]


def ptr(name, good=PTR):
    return (name, good, None)


def same(name, v=None):                                            # an argument no check reads, or one that stays good
    return (name, v, v)


def size(name, good=BIG, bad=0):
    return (name, good, bad)


def _array(ctype, values):
    return (ctype * len(values))(*values)


def scene_desc(variant=0, app=48, cp=False):
    d = _lib().SceneDesc()
    d.aabb[:] = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
    d.grid[:] = [2, 2, 2]
    d.density_n_comp[:] = [16] * 3
    d.app_n_comp[:] = [app] * 3
    d.app_dim, d.featureC, d.view_pe, d.fea_pe = 27, 128, 2, 2
    d.near_, d.far_, d.step_size = 2.0, 6.0, 0.5
    d.inv_aabb_size[:] = [1.0, 1.0, 1.0]
    d.density_shift, d.distance_scale, d.weight_thres, d.fea2dense_act, d.variant = -10.0, 25.0, 1e-4, 0, variant
    return d


def make_scene(d, packed, cp=False):
    """tvr_scene_create / tvr_cp_scene_create over `packed` (None: a fabricated pointer — the scene is never updated).  -> (handle, packed bytes)"""
    lib = _lib().lib()
    nbytes = (lib.tvr_cp_scene_packed_bytes if cp else lib.tvr_scene_packed_bytes)(C.byref(d))
    assert nbytes > 0
    h = C.c_void_p()
    rc = (lib.tvr_cp_scene_create if cp else lib.tvr_scene_create)(C.byref(d), PTR if packed is None else packed(nbytes), nbytes, C.byref(h))
    assert rc == OK and h.value, lib.tvr_last_error()
    return h


# ---- the part without a GPU -----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_entries():
    """-> ({entry point: Entry}, {size query: {case: arguments}})"""
    L = _lib()
    lib = L.lib()
    vm, cp = make_scene(scene_desc(), None), make_scene(scene_desc(cp=True), None, cp=True)       # never updated: whatever passes the checks in front ends at scene_ready
    stream = same("stream")
    scene = same("s", vm)
    not_ready = {"scene_null": {"s": None}, "not_updated": {}}
    no_cp = {"cp_scene": {"s": cp}, **not_ready}
    cp_only = {"scene_null": {"s": None}, "vm_scene": {"s": vm}, "not_updated": {"s": cp}}
    image_bytes = lib.tvr_mlp_train_image_bytes()
    assert image_bytes > 0
    vm_grads = L.VmGrads()
    cp_grads = L.CpGrads()
    for i in range(3):
        vm_grads.density_plane[i] = vm_grads.density_line[i] = vm_grads.app_plane[i] = vm_grads.app_line[i] = cp_grads.density_line[i] = cp_grads.app_line[i] = PTR
    cp_grads.basis_mat = PTR
    rows = lambda cols: 4 * M * cols - 1                           # one byte short of [M, cols] fp32

    E = {}
    march = [scene, ptr("rays"), same("n_rays", N_RAYS), same("S", S), same("jitter"), same("eps_T", 0.0)]
    E["tvr_march_forward"] = Entry(march + [ptr("depth_out"), ptr("scratch"), size("scratch_bytes"), stream], [], no_cp)
    E["tvr_march_forward_z"] = Entry(march[:4] + [ptr("z_vals"), same("eps_T", 0.0), ptr("depth_out"), same("t_last_tiny_out"), ptr("scratch"), size("scratch_bytes"), stream],
                                     [], {"z_vals_null": {"z_vals": None}, **no_cp})
    backward = [ptr("fwd_scratch"), size("fwd_bytes"), ptr("grad_w"), ptr("grad_acc")]
    grads = [ptr("grad_scratch"), size("grad_bytes"), same("out", C.byref(vm_grads)), stream]
    E["tvr_march_backward"] = Entry(march + backward + grads, [], no_cp)
    E["tvr_march_backward_z"] = Entry(march[:4] + [ptr("z_vals"), same("eps_T", 0.0)] + backward + [same("t_last_tiny"), same("grad_t_last_tiny")] + grads, [],
                                      {"z_vals_null": {"z_vals": None}, "t_last_tiny_alone": {"t_last_tiny": PTR}, "its_gradient_alone": {"grad_t_last_tiny": PTR}, **no_cp})
    E["tvr_app_h_forward"] = Entry([scene, ptr("xyz"), same("m", M), ptr("h_out"), size("h_bytes"), stream], [], {"h_one_short": {"h_bytes": rows(144)}, **no_cp})
    E["tvr_app_h_backward"] = Entry([scene, ptr("xyz"), same("m", M), ptr("dh"), size("dh_bytes")] + grads, [], {"dh_one_short": {"dh_bytes": rows(144)}, **no_cp})
    forward = [scene, ptr("h"), ptr("viewdirs"), same("m", M), ptr("rgb"), size("rgb_bytes"), ptr("feats32"), size("feats32_bytes"), ptr("h1"), size("h1_bytes"), ptr("h2"),
               size("h2_bytes")]
    forward_extra = {"rgb_one_short": {"rgb_bytes": rows(3)}, "feats32_one_short": {"feats32_bytes": rows(32)}, "h1_one_short": {"h1_bytes": rows(128)},
                     "h2_one_short": {"h2_bytes": rows(128)}, "rows_above": {"m": ROWS_ABOVE}, **no_cp}
    E["tvr_mlp_train_forward"] = Entry(forward + [stream], [["rgb_bytes", "feats32_bytes", "h1_bytes", "h2_bytes"]], forward_extra)
    E["tvr_mlp_train_forward_ref"] = Entry(forward + [ptr("g8"), size("g8_bytes"), ptr("rgb_s"), size("rgb_s_bytes"), stream],
                                           [["rgb_bytes", "feats32_bytes", "h1_bytes", "h2_bytes", "g8_bytes", "rgb_s_bytes"]],
                                           {"g8_one_short": {"g8_bytes": rows(8)}, "rgb_s_one_short": {"rgb_s_bytes": rows(3)}, **forward_extra})
    outs = ["d_out4", "dh2", "dh1", "dfeats32", "dh"]
    out_args = lambda names: [a for n in names for a in (ptr(n), size(n + "_bytes"))]
    tail = [ptr("sat_flag_dev"), ptr("image"), ("image_bytes", image_bytes, 0), stream]
    backward_extra = {"image_one_short": {"image_bytes": image_bytes - 1}, "image_misaligned": {"image": MISALIGNED}, "rows_above": {"m": ROWS_ABOVE},
                      "feats32_odd": {"feats32": ODD}, "dh_odd": {"dh": ODD}, "d_out4_one_short": {"d_out4_bytes": rows(4)}, "dh_one_short": {"dh_bytes": rows(144)},
                      "dh1_one_short": {"dh1_bytes": rows(128)}}
    weights = [ptr(n) for n in ("W1", "W2", "W3", "basis")]
    saved = [ptr(n) for n in ("feats32", "h1", "h2")]
    E["tvr_mlp_train_backward"] = Entry(
        weights + [ptr("grad_rgb"), ptr("rgb")] + saved + [("m", M, -1), ptr("gscale_dev")] + out_args(outs) + tail,
        [["m"]] + [[n + "_bytes"] for n in outs] + [["W1", "W2", "W3", "basis", "grad_rgb", "rgb", "feats32", "h1", "h2", "gscale_dev", "image"] + outs], backward_extra)
    heads, heads_one_null = _array(C.c_void_p, [PTR] * 4), _array(C.c_void_p, [PTR, PTR, None, PTR])
    outs_ref = ["d_out4", "dh2", "dh1", "dfeats32", "dg8", "dh"]
    E["tvr_mlp_train_backward_ref"] = Entry(
        weights + [("heads_W", C.byref(heads), None), ptr("grad_rgb"), same("grad_in0"), ptr("rgb_s")] + saved + [ptr("g8"), ptr("viewdirs"), ("m", M, -1), ptr("gscale_dev")]
        + out_args(outs_ref) + tail,
        [["m"]] + [[n + "_bytes"] for n in outs_ref]
        + [["W1", "W2", "W3", "basis", "heads_W", "grad_rgb", "rgb_s", "feats32", "h1", "h2", "g8", "viewdirs", "gscale_dev", "image"] + outs_ref],
        {"one_head_null": {"heads_W": C.byref(heads_one_null)}, "g8_odd": {"g8": ODD}, "dg8_odd": {"dg8": ODD}, "dg8_one_short": {"dg8_bytes": rows(8)},
         "viewdirs_null": {"viewdirs": None}, **backward_extra})
    cp_scene = same("s", cp)
    E["tvr_cp_march_forward"] = Entry([cp_scene] + march[1:] + [ptr("depth_out"), ptr("scratch"), size("scratch_bytes"), stream], [], cp_only)
    E["tvr_cp_march_backward"] = Entry([cp_scene] + march[1:] + backward + [ptr("grad_scratch"), size("grad_bytes"), same("out", C.byref(cp_grads)), stream], [], cp_only)
    E["tvr_cp_app_backward"] = Entry([cp_scene, ptr("xyz"), same("m", M), ptr("grad_features"), size("grad_features_bytes"), ptr("grad_scratch"), size("grad_bytes"),
                                      same("out", C.byref(cp_grads)), stream], [], cp_only)
    layout = L.TrainWorkLayout()
    E["tvr_train_work_describe"] = Entry([scene, ("n_rays", N_RAYS, 0), ("n_samples", S, 0), ("app_cap", M, 0), ("out", C.byref(layout), None)], [["out", "n_rays", "n_samples", "app_cap"]],
                                         {"cp_scene": {"s": cp}, "scene_null": {"s": None}, "out_null": {"out": None}, "app_cap_zero": {"app_cap": 0}})
    step = [scene, ptr("rays"), same("n_rays", N_RAYS), same("S", S), same("jitter"), same("eps_T", 0.0), same("white_bg", 1), ptr("fwd_scratch"), size("fwd_bytes"), ptr("work"),
            size("work_bytes"), same("app_cap", M)]
    E["tvr_train_forward"] = Entry(step + [ptr("rgb_map"), ptr("depth"), same("pen_ray"), stream], [], no_cp)
    E["tvr_train_backward"] = Entry(step + [same("wt"), ptr("grad_rgb_map"), same("grad_pen_ray"), same("grad_scale_target", 1024.0), ptr("grad_scratch"), size("grad_bytes"),
                                            same("vm_out"), same("mo"), ptr("sat_flag_dev"), stream], [], no_cp)
    E["tvr_pe_concat"] = Entry([ptr("features"), ptr("viewdirs"), same("dot_product"), ("m", M, -1), ptr("X"), size("X_bytes"), stream],
                               [["m"], ["X_bytes"], ["features", "viewdirs", "X"]],
                               {"X_one_short": {"X_bytes": rows(150)}, "X_with_dot_one_short": {"dot_product": PTR, "X_bytes": rows(151)}})
    E["tvr_pe_concat_backward"] = Entry([ptr("features"), ptr("viewdirs"), ptr("grad_X"), ("m", M, -1), same("with_dot", 0), ptr("grad_features"), size("grad_features_bytes"),
                                         same("grad_viewdirs", PTR), same("grad_dot"), stream],
                                        [["m"], ["grad_features_bytes"], ["features", "viewdirs", "grad_X", "grad_features"]], {"grad_features_one_short": {"grad_features_bytes": rows(27)}})
    E["tvr_tv_loss"] = Entry([ptr("x"), ("C", 16, 0), ("H", 3, 0), ("W", 3, 0), same("weight", 1.0), ptr("value"), ptr("grad"), ptr("scratch"), ("scratch_bytes", 2048, 0), stream],
                             [["x", "value", "grad", "C", "H", "W"], ["scratch", "scratch_bytes"]],
                             {"width_zero": {"W": 0}, "scratch_null": {"scratch": None}, "scratch_one_short": {"scratch_bytes": 2047}})
    xs, xs_one_null = _array(C.c_void_p, [PTR, PTR]), _array(C.c_void_p, [PTR, None])
    counts, counts_one_zero = _array(C.c_int64, [100, 200]), _array(C.c_int64, [100, 0])
    l1_scratch = lib.tvr_l1_mean_scratch_bytes(counts, 2)
    assert l1_scratch > 0
    E["tvr_l1_mean"] = Entry([("xs", xs, None), ("counts", counts, None), ("n", 2, 0), ptr("value"), ptr("scratch"), ("scratch_bytes", l1_scratch, 0), stream],
                             [["n"], ["xs", "counts"], ["value"], ["scratch", "scratch_bytes"]],
                             {"n_above": {"n": 9}, "tensor_null": {"xs": xs_one_null}, "count_zero": {"counts": counts_one_zero}, "scratch_null": {"scratch": None},
                              "scratch_one_short": {"scratch_bytes": l1_scratch - 1}})
    E["tvr_l1_mean_backward"] = Entry([("xs", xs, None), ("grads", xs, None), ("counts", counts, None), ("n", 2, 0), ptr("grad_value"), stream],
                                      [["n"], ["xs", "counts", "grads"], ["grad_value"]], {"grads_null": {"grads": None}, "gradient_null": {"grads": xs_one_null}})
    n_comp, n_size = _array(C.c_int32, [16, 48]), _array(C.c_int32, [3, 3])
    ortho_extra = {"n_above": {"n": 9}, "one_component": {"n_comp": _array(C.c_int32, [16, 1])}, "components_above": {"n_comp": _array(C.c_int32, [49, 48])},
                   "size_zero": {"n_size": _array(C.c_int32, [3, 0])}, "factor_null": {"vs": xs_one_null}, "n_size_null": {"n_size": None}}
    E["tvr_line_ortho"] = Entry([("vs", xs, None), ("n_comp", n_comp, None), ("n_size", n_size, None), ("n", 2, 0), ptr("value"), ptr("scratch"), ("scratch_bytes", 256, 0), stream],
                                [["n_comp", "n_size"], ["n"], ["vs"], ["value"], ["scratch", "scratch_bytes"]],
                                {"scratch_null": {"scratch": None}, "scratch_one_short": {"scratch_bytes": 255}, **ortho_extra})
    E["tvr_line_ortho_backward"] = Entry([("vs", xs, None), ("grads", xs, None), ("n_comp", n_comp, None), ("n_size", n_size, None), ("n", 2, 0), ptr("grad_value"), stream],
                                         [["n_comp", "n_size"], ["n"], ["vs", "grads"], ["grad_value"]], {"gradient_null": {"grads": xs_one_null}, **ortho_extra})
    E["tvr_linear_dx"] = Entry(
        [ptr("dY"), same("ldy", 128), same("N", 128), ptr("W"), same("ldw", 128), same("n_valid", 128), same("K", 128), same("mask"), same("ldm", 0), same("mask_bits"), ptr("dX"),
         same("ldx", 128), size("dX_bytes"), same("M", M), same("scale_dev"), same("sat_flag_dev", PTR), stream], [],
        {"mask_and_bits": {"mask": PTR, "ldm": 128, "mask_bits": PTR}, "bits_odd": {"mask_bits": ODD}, "scaled_N": {"scale_dev": PTR, "N": 8, "n_valid": 8}, "M_negative": {"M": -1},
         "N_no_multiple": {"N": 12, "n_valid": 12}, "N_above": {"N": 136}, "n_valid_zero": {"n_valid": 0}, "n_valid_above": {"N": 64, "n_valid": 65}, "K_other": {"K": 48},
         "ldy_short": {"ldy": 64}, "ldw_short": {"ldw": 64}, "ldx_no_multiple": {"ldx": 130}, "ldm_short": {"mask": PTR, "ldm": 64}, "dY_null": {"dY": None}, "dX_odd": {"dX": ODD},
         "mask_odd": {"mask": ODD, "ldm": 128}, "dX_one_short": {"dX_bytes": 4 * ((M - 1) * 128 + 128) - 1}})
    colsum_scratch = lib.tvr_colsum_scratch_bytes()
    E["tvr_colsum"] = Entry([ptr("A"), ("lda", 32, 0), ("K", 32, 0), ("M", M, -1), ptr("out"), ptr("scratch"), ("scratch_bytes", colsum_scratch, 0), stream],
                            [["M", "K", "lda"], ["out", "A"], ["scratch", "scratch_bytes"]],
                            {"K_above": {"K": 129, "lda": 129}, "lda_short": {"lda": 31}, "scratch_null": {"scratch": None}, "scratch_one_short": {"scratch_bytes": colsum_scratch - 1}})
    gemm = [ptr("A"), ("lda", 32, 0), ("Ka", 32, 0), ptr("B"), ("ldb", 32, 0), ("Kb", 32, 0), ("M", M, -1), ptr("C")]
    gemm_scratch, gemm_scratch_ones = lib.tvr_gemm_tn_scratch_bytes(32, 32, M), lib.tvr_gemm_tn_scratch_bytes(32, 33, M)
    assert min(gemm_scratch, gemm_scratch_ones) > 0
    wide = {"Ka": 64, "lda": 64, "Kb": 288, "ldb": 288}            # 2 x 9 (or 10) tiles, 352 staged columns
    gemm_extra = {"tiles_above": {"Ka": 160, "lda": 160, "Kb": 160, "ldb": 160}, "lda_short": {"lda": 31}, "ldb_short": {"ldb": 31}, "scratch_null": {"scratch": None}}
    E["tvr_gemm_tn"] = Entry(gemm + [ptr("scratch"), ("scratch_bytes", gemm_scratch, 0), stream], [["Ka", "Kb", "M"], ["A", "B", "C"], ["lda", "ldb"], ["scratch", "scratch_bytes"]],
                             {"scratch_one_short": {"scratch_bytes": gemm_scratch - 1}, "empty_without_C": {"M": 0, "C": None, "A": None, "B": None}, **gemm_extra})
    E["tvr_gemm_tn_scaled"] = Entry(
        gemm + [same("colsum_A"), ptr("scale_dev"), ptr("scratch"), ("scratch_bytes", gemm_scratch_ones, 0), stream],
        [["Ka", "Kb", "M"], ["A", "B", "C", "scale_dev"], ["lda", "ldb"], ["scratch", "scratch_bytes"]],
        {"scratch_one_short": {"scratch_bytes": gemm_scratch - 1}, "scratch_with_sums_one_short": {"colsum_A": PTR, "scratch_bytes": gemm_scratch_ones - 1},
         "Ka_above": {"Ka": 160, "lda": 160}, "columns_above": wide, "tiles_above_with_sums": {"colsum_A": PTR, "Kb": 640, "ldb": 640}, "scale_null": {"scale_dev": None},
         **gemm_extra})
    E["tvr_gemm_tn_bias"] = Entry(
        gemm + [ptr("colsum_A"), ptr("scratch"), ("scratch_bytes", gemm_scratch_ones, 0), stream],
        [["Ka", "Kb", "M"], ["A", "B", "C", "colsum_A"], ["lda", "ldb"], ["scratch", "scratch_bytes"]],
        {"scratch_one_short": {"scratch_bytes": gemm_scratch_ones - 1}, "columns_above": wide, "tiles_above_with_sums": {"Kb": 640, "ldb": 640}, "colsum_null": {"colsum_A": None},
         **gemm_extra})
    Q = {
        "tvr_grad_scratch_bytes": {"cp_scene": (cp,)},
        "tvr_cp_grad_scratch_bytes": {"scene_null": (None,), "vm_scene": (vm,)},
        "tvr_train_work_bytes": {"cp_scene": (cp, N_RAYS, S, M)},
        "tvr_gemm_tn_scratch_bytes": {"Ka_zero": (0, 32, M), "M_negative": (32, 32, -1), "tiles_above": (160, 160, M)},
    }
    return E, Q


# ---- the gpu part ---------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gpu_entries():
    """-> {entry point: [Entry per scene it is tried on]}.  Every pointer is a zeroed device allocation that the returned closure keeps alive."""
    import torch
    L = _lib()
    lib = L.lib()
    dev = torch.device("cuda:0")
    keep = []

    def alloc(nbytes):                                             # 256 spare bytes: `+ 16` stays inside, and so would a kernel that started there
        t = torch.zeros(int(nbytes) + 256, dtype=torch.uint8, device=dev)
        assert t.data_ptr() % 256 == 0
        keep.append(t)
        return t.data_ptr()

    def floats(*shape):
        n = 4
        for x in shape:
            n *= x
        return alloc(n)

    def updated(d, cp=False):
        h = make_scene(d, alloc, cp=cp)
        sp = L.SceneParams()
        r_d, r_a = d.density_n_comp[0], d.app_n_comp[0]
        for i in range(3):
            sp.density_line[i], sp.app_line[i] = floats(r_d, 2), floats(r_a, 2)
            if not cp:
                sp.density_plane[i], sp.app_plane[i] = floats(r_d, 2, 2), floats(r_a, 2, 2)
        sp.basis_mat = floats(27, r_a if cp else 3 * r_a)
        sp.W1, sp.b1, sp.W2, sp.b2, sp.W3, sp.b3 = floats(128, 151), floats(128), floats(128, 128), floats(128), floats(3, 128), floats(3)
        for i, rows_ in enumerate((3, 3, 1, 1)):
            if d.variant == 1:
                sp.ref_W[i], sp.ref_b[i] = floats(rows_, 144), floats(rows_)
        assert lib.tvr_scene_update(h, C.byref(sp), None) == OK, lib.tvr_last_error()
        return h

    vm, ref, narrow, cp = updated(scene_desc()), updated(scene_desc(variant=1)), updated(scene_desc(app=24)), updated(scene_desc(cp=True), cp=True)
    layout = L.ScratchLayout()
    assert lib.tvr_scratch_describe(N_RAYS, S, C.byref(layout)) == OK
    fwd_bytes = layout.total
    rays_host = torch.tensor([[10.0, 10.0, 10.0, 1.0, 0.0, 0.0]] * N_RAYS, dtype=torch.float32)      # they miss the box [-1, 1]^3: nothing to march
    rays_dev = rays_host.to(dev)
    keep.append(rays_dev)
    rays = rays_dev.data_ptr()
    stream = same("stream")
    one_short = lambda name, n: {name + "_one_short": {name + "_bytes": n - 1}}
    misaligned = lambda name, p: {name + "_misaligned": {name: p + 16}}
    march_extra = {"S_above": {"S": 4097}, "product_above": {"n_rays": 1 << 20, "S": 4096}, "eps_T_above": {"eps_T": 1.0}, "eps_T_nan": {"eps_T": float("nan")}}

    def grads_of(scene, is_cp=False, **null):
        g = (L.CpGrads if is_cp else L.VmGrads)()
        for name, _ in g._fields_:
            if name == "basis_mat":
                g.basis_mat = floats(27, 48)
            else:
                for i in range(3):
                    getattr(g, name)[i] = floats(48, 3, 3)
        for name, i in null.items():
            if name == "basis_mat":
                g.basis_mat = None
            else:
                getattr(g, name)[i] = None
        keep.append(g)
        return C.byref(g)

    E = {}

    def add(name, entry):
        E.setdefault(name, []).append(entry)

    def march_args(scene):
        return [same("s", scene), ("rays", rays, None), ("n_rays", N_RAYS, 0), ("S", S, 0), same("jitter"), ("eps_T", 0.0, -1.0)]

    scratch = alloc(fwd_bytes)
    scratch_args = [("scratch", scratch, None), ("scratch_bytes", fwd_bytes, fwd_bytes - 1), stream]
    forward_ladder = [["rays", "depth_out", "n_rays"], ["S"], ["eps_T"], ["scratch"], ["scratch_bytes"]]
    forward_extra = {**march_extra, **misaligned("scratch", scratch)}
    depth = ("depth_out", floats(N_RAYS), None)
    add("tvr_march_forward", Entry(march_args(vm) + [depth] + scratch_args, forward_ladder, forward_extra))
    add("tvr_march_forward_z", Entry(march_args(vm)[:4] + [same("z_vals", floats(N_RAYS, S)), ("eps_T", 0.0, -1.0), depth, same("t_last_tiny_out")] + scratch_args,
                                     forward_ladder, forward_extra))
    add("tvr_cp_march_forward", Entry(march_args(cp) + [depth] + scratch_args, forward_ladder, forward_extra))

    grad_bytes, cp_grad_bytes = lib.tvr_grad_scratch_bytes(vm), lib.tvr_cp_grad_scratch_bytes(cp)
    assert min(grad_bytes, cp_grad_bytes) > 0
    fwd = [("fwd_scratch", scratch, None), ("fwd_bytes", fwd_bytes, fwd_bytes - 1), ("grad_w", floats(N_RAYS, S), None), ("grad_acc", floats(N_RAYS), None)]
    grad_scratch, cp_grad_scratch = alloc(grad_bytes), alloc(cp_grad_bytes)
    grad_args = [("grad_scratch", grad_scratch, None), ("grad_bytes", grad_bytes, grad_bytes - 1)]
    add("tvr_march_backward", Entry(
        march_args(vm) + fwd + grad_args + [("out", grads_of(vm), None), stream],
        [["rays", "fwd_scratch", "grad_w", "grad_acc", "grad_scratch", "out", "n_rays"], ["fwd_bytes"], ["grad_bytes"]],
        {**misaligned("grad_scratch", grad_scratch), "density_plane_null": {"out": grads_of(vm, density_plane=1)}, "density_line_null": {"out": grads_of(vm, density_line=2)}}))
    add("tvr_march_backward_z", Entry(          # the checks are march_backward_impl's; with z_vals and the t_last_tiny pair given, the wrapper hands every argument on
        march_args(vm)[:4] + [same("z_vals", floats(N_RAYS, S)), same("eps_T", 0.0)] + fwd + [same("t_last_tiny", floats(N_RAYS)), same("grad_t_last_tiny", floats(N_RAYS))]
        + grad_args + [("out", grads_of(vm), None), stream],
        [["rays", "fwd_scratch", "grad_w", "grad_acc", "grad_scratch", "out", "n_rays"], ["fwd_bytes"], ["grad_bytes"]], misaligned("grad_scratch", grad_scratch)))
    add("tvr_cp_march_backward", Entry(
        march_args(cp) + fwd + [("grad_scratch", cp_grad_scratch, None), ("grad_bytes", cp_grad_bytes, cp_grad_bytes - 1), ("out", grads_of(cp, True), None), stream],
        [["rays", "fwd_scratch", "grad_w", "grad_acc", "grad_scratch", "out", "n_rays"], ["S"], ["eps_T"], ["fwd_bytes"], ["grad_bytes"]],
        {**march_extra, **misaligned("fwd_scratch", scratch), **misaligned("grad_scratch", cp_grad_scratch), "density_line_null": {"out": grads_of(cp, True, density_line=1)}}))

    xyz, h144 = floats(M, 4), floats(M, 144)
    add("tvr_app_h_forward", Entry([same("s", vm), ("xyz", xyz, None), same("m", M), ("h_out", h144, None), same("h_bytes", 4 * M * 144), stream], [["xyz", "h_out"]],
                                   {"m_negative": {"m": -1}}))
    add("tvr_app_h_backward", Entry(
        [same("s", vm), ("xyz", xyz, None), same("m", M), ("dh", h144, None), same("dh_bytes", 4 * M * 144)] + grad_args + [("out", grads_of(vm), None), stream],
        [["grad_scratch", "out", "xyz", "dh"], ["grad_bytes"]],
        {**misaligned("grad_scratch", grad_scratch), "m_negative": {"m": -1}, "app_plane_null": {"out": grads_of(vm, app_plane=0)}, "app_line_null": {"out": grads_of(vm, app_line=2)}}))
    gf_bytes = 4 * M * 27
    add("tvr_cp_app_backward", Entry(
        [same("s", cp), ("xyz", xyz, None), same("m", M), ("grad_features", floats(M, 27), None), ("grad_features_bytes", gf_bytes, gf_bytes - 1),
         ("grad_scratch", cp_grad_scratch, None), ("grad_bytes", cp_grad_bytes, cp_grad_bytes - 1), ("out", grads_of(cp, True), None), stream],
        [["grad_scratch", "out", "xyz", "grad_features"], ["grad_features_bytes"], ["grad_bytes"]],
        {**misaligned("grad_scratch", cp_grad_scratch), "m_negative": {"m": -1}, "m_above": {"m": 1 << 32, "grad_features_bytes": BIG},
         "app_line_null": {"out": grads_of(cp, True, app_line=1)}, "basis_mat_null": {"out": grads_of(cp, True, basis_mat=0)}}))

    def mlp_forward(scene, with_ref):
        sized = lambda name, cols: [(name, floats(M, cols), None), same(name + "_bytes", 4 * M * cols)]
        h = floats(M, 144)
        args = [same("s", scene), ("h", h, None), ("viewdirs", floats(M, 3), None), same("m", M)] + sized("rgb", 3) + sized("feats32", 32) + sized("h1", 128) + sized("h2", 128)
        names = ["h", "viewdirs", "rgb", "feats32", "h1", "h2"]
        if with_ref:
            args += sized("g8", 8) + sized("rgb_s", 3)
            names += ["g8", "rgb_s"]
        return args + [stream], names, h

    args, names, h = mlp_forward(vm, False)
    add("tvr_mlp_train_forward", Entry(args, [names], {"m_negative": {"m": -1}, "h_odd": {"h": h + 4}}))
    add("tvr_mlp_train_forward", Entry(mlp_forward(ref, False)[0], [], {"reftensorf_scene": {}}))
    add("tvr_mlp_train_forward", Entry(mlp_forward(narrow, False)[0], [], {"narrow_scene": {}}))
    args, names, h = mlp_forward(ref, True)
    add("tvr_mlp_train_forward_ref", Entry(args, [names], {"m_negative": {"m": -1}, "h_odd": {"h": h + 4}, "g8_null": {"g8": None}}))
    add("tvr_mlp_train_forward_ref", Entry(mlp_forward(vm, True)[0], [], {"vm_scene": {}}))

    def step(scene):
        work_bytes = lib.tvr_train_work_bytes(scene, N_RAYS, S, M)
        assert work_bytes > 0
        work = alloc(work_bytes)
        args = [same("s", scene), ("rays", rays, None), ("n_rays", N_RAYS, 0), ("S", S, 0), same("jitter"), same("eps_T", 0.0), same("white_bg", 1), ("fwd_scratch", scratch, None),
                ("fwd_bytes", fwd_bytes, fwd_bytes - 1), ("work", work, None), ("work_bytes", work_bytes, work_bytes - 1), ("app_cap", M, 0)]
        ladder = [["rays", "n_rays", "S", "app_cap"], ["fwd_scratch"], ["fwd_bytes"], ["work"], ["work_bytes"]]
        extra = {"S_above": {"S": 4097}, "product_above": {"n_rays": 1 << 20, "S": 4096}, "app_cap_above": {"app_cap": ROWS_ABOVE}, **misaligned("fwd_scratch", scratch),
                 **misaligned("work", work)}
        return args, ladder, extra

    for scene, is_ref in ((vm, False), (ref, True)):
        args, ladder, extra = step(scene)
        outs = [("rgb_map", floats(N_RAYS, 3), None), ("depth", floats(N_RAYS), None), same("pen_ray", floats(N_RAYS) if is_ref else None), stream]
        if is_ref:
            add("tvr_train_forward", Entry(args + outs, [], {"pen_ray_null": {"pen_ray": None}}))
        else:
            add("tvr_train_forward", Entry(args + outs, ladder + [["rgb_map", "depth"]], {**extra, "eps_T_negative": {"eps_T": -1.0}, "eps_T_above": {"eps_T": 1.0}}))

        def weights(**null):
            wt, mo = L.TrainWeights(), L.TrainMlpGrads()
            for struct in (wt, mo):
                for name, ctype in struct._fields_:
                    if ctype is C.c_void_p:
                        setattr(struct, name, floats(128, 152))
                    else:
                        for i in range(4):
                            getattr(struct, name)[i] = floats(3, 144)
            for name, (struct, i) in null.items():
                struct = wt if struct == "wt" else mo
                if i is None:
                    setattr(struct, name, None)
                else:
                    getattr(struct, name)[i] = None
            keep.extend([wt, mo])
            return C.byref(wt), C.byref(mo)

        wt, mo = weights()
        tail = [("wt", wt, None), ("grad_rgb_map", floats(N_RAYS, 3), None), same("grad_pen_ray", floats(N_RAYS) if is_ref else None), ("grad_scale_target", 1024.0, 0.0)] + grad_args \
            + [("vm_out", grads_of(scene), None), ("mo", mo, None), same("sat_flag_dev", alloc(256)), stream]
        if is_ref:
            add("tvr_train_backward", Entry(args + tail, [], {"head_weight_null": {"wt": weights(heads_W=("wt", 2))[0]}, "head_bias_gradient_null": {"mo": weights(heads_b=("mo", 3))[1]}}))
        else:
            add("tvr_train_backward", Entry(
                args + tail, ladder + [["wt", "grad_rgb_map", "vm_out", "mo", "grad_scale_target"]],
                {**extra, "W1_null": {"wt": weights(W1=("wt", None))[0]}, "scale_target_nan": {"grad_scale_target": float("nan")}, "b2_gradient_null": {"mo": weights(b2=("mo", None))[1]},
                 "grad_scratch_one_short": {"grad_bytes": grad_bytes - 1}, **misaligned("grad_scratch", grad_scratch), "app_plane_null": {"vm_out": grads_of(scene, app_plane=2)},
                 "density_line_null": {"vm_out": grads_of(scene, density_line=0)}, "both_null": {"vm_out": grads_of(scene, app_line=1, density_plane=0)}}))
    E["__keep__"] = keep
    return E


def entry_points():
    return sorted(MOVED + SHARE_A_CHECK)


def replay(name, part):
    """-> [(case, status, message)] of one entry point against the loaded library.  A case that is not refused stops the replay of its entry point."""
    lib = _lib().lib()
    fn = getattr(lib, name)
    if part == "host":
        E, Q = host_entries()
        cases = list(E[name].cases()) if name in E else [(case, list(args)) for case, args in Q.get(name, {}).items()]
        query = name in Q
    else:
        cases = [(f"{GPU}{k}:{case}", args) for k, entry in enumerate(gpu_entries().get(name, [])) for case, args in entry.cases()]
        query = False
    out = []
    for case, args in cases:
        status = fn(*args)
        message = lib.tvr_last_error()
        out.append((case, status, message.decode("utf-8")))
        if query:
            assert status == 0 and message, f"{name} / {case}: a refused size query returns 0 and sets the message, got {status} / {message!r}"
        else:
            assert status != ERR_HIP, f"{name} / {case} reached a launch that failed: {message!r}"
            assert status < 0, f"{name} / {case} was not refused"
    if part == "gpu":
        import torch
        torch.cuda.synchronize()                                   # whatever a refused call did launch (see the head of this file) has run on valid memory
    return out


def record(part, path=TABLE):
    """Run by hand, once per part, with TVR_LIB_PATH naming the library of the commit before the change under test; never at test time.  The other part's rows are kept."""
    is_gpu = lambda case: case.startswith(GPU)
    kept = [r for r in (json.load(open(TABLE, encoding="utf-8")) if os.path.exists(TABLE) else []) if is_gpu(r[1]) != (part == "gpu")]
    rows = [[name, case, status, message] for name in entry_points() for case, status, message in replay(name, part)]
    rows = sorted(kept + rows, key=lambda r: (r[0], is_gpu(r[1])))
    with open(path, "w", encoding="utf-8") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, ensure_ascii=False) for r in rows) + "\n]\n")
    print(f"{len(rows) - len(kept)} rows ({part}) of {len(entry_points())} entry points from {_lib().LIB_PATH}, {len(kept)} kept -> {path}")


@functools.lru_cache(maxsize=None)
def table():
    by_entry = {}
    for name, case, status, message in json.load(open(TABLE, encoding="utf-8")):
        by_entry.setdefault((name, "gpu" if case.startswith(GPU) else "host"), []).append((case, status, message))
    return by_entry


def _compare(name, part):
    got, want = replay(name, part), table().get((name, part), [])
    assert [c for c, _, _ in got] == [c for c, _, _ in want]
    for (case, status, message), (_, want_status, want_message) in zip(got, want):
        assert (status, message.encode()) == (want_status, want_message.encode()), (name, case)


def test_the_table_covers_every_moved_entry_point():
    E, Q = host_entries()
    assert len(MOVED) == 33 and set(MOVED) <= set(_lib().SYMBOLS)
    assert sorted(list(E) + list(Q) + NEVER_REFUSE) == entry_points()
    assert sorted({name for name, _ in table()}) == sorted(set(entry_points()) - set(NEVER_REFUSE))
    for (name, part), rows in table().items():
        if name in Q:
            assert all(status == 0 and message for _, status, message in rows), name
        else:
            assert all(status in (-1, -3, -4) for _, status, _ in rows), name      # TVR_ERR_INVALID / _SCRATCH / _UNSUPPORTED: never TVR_ERR_HIP, never TVR_OK
    scene_taking = [n for n in E if E[n].names[0] == "s"]
    assert len(scene_taking) == 14 and sorted(n for n, part in table() if part == "gpu") == sorted(set(scene_taking) - {"tvr_train_work_describe"})


@pytest.mark.parametrize("name", sorted(set(MOVED + SHARE_A_CHECK) - set(NEVER_REFUSE)))
def test_refusals_are_the_recorded_bytes(name):
    _compare(name, "host")


@pytest.mark.gpu
def test_refusals_behind_an_updated_scene_are_the_recorded_bytes():
    """One test for the 13 entry points: the four scenes and the buffers are made once."""
    names = sorted(n for n, part in table() if part == "gpu")
    assert names
    for name in names:
        _compare(name, "gpu")


if __name__ == "__main__":
    if len(sys.argv) in (3, 4) and sys.argv[1] == "record" and sys.argv[2] in ("host", "gpu"):
        record(sys.argv[2], *sys.argv[3:])
    else:
        sys.exit("usage: TVR_LIB_PATH=<libtvr.so of the commit before the change> python tests/test_train_api_errors_host.py record host|gpu [path]")
