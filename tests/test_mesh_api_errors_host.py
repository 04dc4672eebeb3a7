"""No GPU: every refusal of the tvr_mesh_* entry points of csrc/tvr_mesh_api.hip, byte for byte.

tests/golden/mesh_api_errors.json holds rows (entry point, case, status, message).  They were recorded from the library built from the commit BEFORE the mesh
entry points moved out of tvr_api.hip and their argument checks were folded into shared helpers (`TVR_LIB_PATH=<that libtvr.so> python
tests/test_mesh_api_errors_host.py record`), never from the code under test.  The test replays every case against the built library and asserts that the
status and the bytes of tvr_last_error() are the recorded ones.

Every case is refused by an argument check that precedes the first launch: pointers are fabricated integers (256-byte aligned where a check wants that) and are never
dereferenced; what the host does read (dims, lattices, cameras, cell sizes) are real host arrays.  No case may return TVR_ERR_HIP: that would mean it reached a launch.

Per entry point: `ladder` starts with every argument bad at once (NULL pointers, counts -1, sizes 0), which pins the check that comes first, and then repairs one
group of arguments per step, in the order the checks read them, up to the last check before the launch; `extra` holds the other ways an argument can be wrong
(too large, misaligned, one byte short), each on otherwise good arguments.  The size queries are covered as "returns 0 and sets the message"."""
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
TABLE = os.path.join(HERE, "golden", "mesh_api_errors.json")
OK, ERR_HIP = 0, -2

PTR, MISALIGNED, ODD = 1 << 20, (1 << 20) + 16, (1 << 20) + 4      # 256-byte aligned; 8- but not 256-byte aligned; not 8-byte aligned
BIG = 1 << 40                                                      # a byte count no check finds short
TOP = 2 ** 31 - 1
MAX_F = 1 << 30                                                    # TVR_MESH_BVH_MAX_TRIANGLES
V, F, H = 1000, 3000, 6000                                         # vertices, triangles, half-edges of the mesh the good arguments describe
NAN, INF = float("nan"), float("inf")


def _lib():
    from jittor_myc_nerfs_amd import _lib as L
    return L


def _floats(*v):
    return (C.c_float * len(v))(*v)


def _dims(*v):
    return (C.c_int32 * 3)(*v)


def _camera(**kw):
    f = dict(c2w=(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0), H=48, W=64, fx=50.0, fy=50.0, cx=32.0, cy=24.0, near_=0.1, cull=0, large_bbox=0)
    f.update(kw)
    cam = _lib().MeshCamera()
    cam.c2w = (C.c_float * 12)(*f.pop("c2w"))
    for k, v in f.items():
        setattr(cam, k, v)
    return cam


def _lattice(dims=(10, 10, 10), origin=(0.0, 0.0, 0.0), spacing=(0.1, 0.1, 0.1)):
    lat = _lib().MeshLattice()
    lat.origin, lat.spacing, lat.dims = _floats(*origin), _floats(*spacing), _dims(*dims)
    return lat


class Entry:
    """One entry point: `params` = [(name, good value, bad value)] in the order of the C signature; `ladder` = groups of parameter names in the order the checks read
    them; `extra` = {case: {name: value}} on otherwise good arguments.  The arguments that are all good are never passed: they would reach the launch."""

    def __init__(self, params, ladder, extra):
        self.names = [p[0] for p in params]
        self.good = {p[0]: p[1] for p in params}
        self.bad = {p[0]: p[2] for p in params}
        self.ladder, self.extra = ladder, extra
        for group in ladder:
            for n in group:
                assert n in self.good and self.bad[n] != self.good[n], n
        for kw in extra.values():
            assert kw and set(kw) <= set(self.good), kw

    def cases(self):
        for k in range(len(self.ladder)):
            repaired = {n for group in self.ladder[:k] for n in group}
            yield f"ladder_{k:02d}", [self.good[n] if n in repaired else self.bad[n] for n in self.names]
        for case, kw in self.extra.items():
            yield case, [kw.get(n, self.good[n]) for n in self.names]


def _ref(x):
    return None if x is None else C.byref(x)


@functools.lru_cache(maxsize=None)
def entries():
    """-> ({entry point: Entry}, {size query: {case: arguments}}).  Sizes that a check compares exactly come from the library's own queries."""
    L = _lib()
    lib = L.lib()
    dims = _dims(8, 8, 8)                                          # 512 points
    mc_scratch = lib.tvr_mesh_scratch_bytes(dims)
    unit, origin = _floats(1.0, 1.0, 1.0), _floats(0.0, 0.0, 0.0)
    cam, lat = _camera(), _lattice()
    bvh_bytes, bvh_scratch = lib.tvr_mesh_bvh_bytes(F), lib.tvr_mesh_bvh_scratch_bytes(F)
    pn_bytes, pn_scratch = lib.tvr_mesh_pseudonormals_bytes(V, F), lib.tvr_mesh_pseudonormals_scratch_bytes(F)
    wn_bytes, wn_scratch = lib.tvr_mesh_winding_bytes(F), lib.tvr_mesh_winding_scratch_bytes(F)
    assert min(mc_scratch, bvh_bytes, bvh_scratch, pn_bytes, pn_scratch, wn_bytes, wn_scratch) > 0

    def ptr(name):
        return (name, PTR, None)

    def size(name, bad=0):
        return (name, BIG, bad)

    same = lambda name, v: (name, v, v)                            # an argument no check reads
    nv, nt, stream, counts = ("n_vertices", V, -1), ("n_triangles", F, -1), same("stream", None), same("counts_dev", PTR)
    mesh = [ptr("verts"), nv, ptr("faces"), nt]                    # the (verts, n_vertices, faces, n_triangles) head of the hierarchy's calls
    mesh_ladder = [["n_triangles"], ["n_vertices"], ["faces", "verts"], ["fault_flag_dev"]]
    mesh_extra = {"triangles_above": {"n_triangles": MAX_F + 1}, "vertices_above": {"n_vertices": TOP + 1}}
    blob = [ptr("bvh"), ("bvh_bytes", bvh_bytes, bvh_bytes - 1)]
    blob_ladder = [["bvh"], ["bvh_bytes"]]
    blob_extra = {"bvh_misaligned": {"bvh": MISALIGNED}}
    counts_above = {"vertices_above": {"n_vertices": TOP + 1}, "triangles_above": {"n_triangles": TOP + 1}}
    scratch_misaligned = {"scratch_misaligned": {"scratch": MISALIGNED}}
    lattice_extra = {
        "points_and_lattice": {"lattice": _ref(lat)},
        "lattice_dims_negative": {"points": None, "lattice": _ref(_lattice(dims=(10, -1, 10)))},
        "lattice_origin_nan": {"points": None, "lattice": _ref(_lattice(origin=(0.0, NAN, 0.0)))},
        "lattice_spacing_inf": {"points": None, "lattice": _ref(_lattice(spacing=(0.1, 0.1, INF)))},
        "lattice_above": {"points": None, "lattice": _ref(_lattice(dims=(2000, 2000, 2000)))},
        "points_above": {"n_points": TOP + 1},
        "table_misaligned": {"table": MISALIGNED},
    }
    E = {}
    E["tvr_mesh_count"] = Entry(
        [ptr("volume"), ("dims", dims, None), same("level", 0.5), ptr("scratch"), ("scratch_bytes", mc_scratch, 0), ptr("counts_dev"), stream],
        [["dims"], ["volume", "counts_dev"], ["scratch"], ["scratch_bytes"]],
        {"dims_below": {"dims": _dims(8, 1, 8)}, "dims_above": {"dims": _dims(900, 900, 900)}, "scratch_one_short": {"scratch_bytes": mc_scratch - 1}, **scratch_misaligned})
    E["tvr_mesh_emit"] = Entry(
        [ptr("volume"), ("dims", dims, None), same("level", 0.5), ("origin", origin, None), ("spacing", unit, None), ptr("scratch"), ("scratch_bytes", mc_scratch, 0),
         ptr("verts"), ("verts_bytes", 1200, 0), ("n_vertices", 100, -1), ptr("faces"), ("faces_bytes", 2400, 0), ("n_triangles", 200, -1), same("flip", 0),
         ptr("fault_flag_dev"), stream],
        [["dims"], ["volume", "origin", "spacing", "fault_flag_dev"], ["scratch"], ["scratch_bytes"], ["n_vertices", "n_triangles"], ["verts", "faces"], ["verts_bytes"],
         ["faces_bytes"]],
        {"dims_below": {"dims": _dims(1, 8, 8)}, "dims_above": {"dims": _dims(900, 900, 900)}, "vertices_above": {"n_vertices": 3 * 512 + 1},
         "triangles_above": {"n_triangles": 5 * 512 + 1}, "verts_one_short": {"verts_bytes": 1199}, "faces_one_short": {"faces_bytes": 2399}, **scratch_misaligned})
    E["tvr_mesh_components"] = Entry(
        [ptr("faces"), nt, nv, ptr("vertex_label"), size("vertex_label_bytes"), ptr("component_faces"), size("component_faces_bytes"), ptr("n_components_dev"),
         ptr("scratch"), ("scratch_bytes", 256, 0), ptr("fault_flag_dev"), stream],
        [["n_triangles", "n_vertices"], ["n_components_dev", "fault_flag_dev"], ["faces", "vertex_label", "component_faces"],
         ["vertex_label_bytes", "component_faces_bytes"], ["scratch"], ["scratch_bytes"]],
        {"component_faces_one_short": {"component_faces_bytes": 4 * V - 1}, "scratch_one_short": {"scratch_bytes": 255}, **counts_above, **scratch_misaligned})
    filter_scratch = lib.tvr_mesh_filter_scratch_bytes(V, F)
    E["tvr_mesh_filter_count"] = Entry(
        [ptr("faces"), nt, nv, ptr("vertex_label"), ptr("keep_root"), ptr("scratch"), ("scratch_bytes", filter_scratch, 0), ptr("counts_dev"), ptr("fault_flag_dev"), stream],
        [["n_triangles", "n_vertices"], ["counts_dev", "fault_flag_dev"], ["faces", "vertex_label", "keep_root"], ["scratch"], ["scratch_bytes"]],
        {"scratch_one_short": {"scratch_bytes": filter_scratch - 1}, **counts_above, **scratch_misaligned})
    E["tvr_mesh_filter_emit"] = Entry(
        [same("verts", PTR), ptr("faces"), nt, nv, ptr("scratch"), ("scratch_bytes", filter_scratch, 0), ptr("verts_out"), size("verts_out_bytes"),
         ("n_vertices_out", 500, -1), ptr("faces_out"), size("faces_out_bytes"), ("n_triangles_out", 1500, -1), ptr("kept_vertex"), size("kept_vertex_bytes"),
         ptr("fault_flag_dev"), stream],
        [["n_triangles", "n_vertices"], ["fault_flag_dev"], ["faces"], ["scratch"], ["scratch_bytes"], ["n_vertices_out", "n_triangles_out"],
         ["verts_out", "faces_out", "kept_vertex"], ["verts_out_bytes"], ["faces_out_bytes"], ["kept_vertex_bytes"]],
        {"vertices_out_above": {"n_vertices_out": V + 1}, "triangles_out_above": {"n_triangles_out": F + 1}, "verts_out_one_short": {"verts_out_bytes": 12 * 500 - 1},
         "faces_out_one_short": {"faces_out_bytes": 12 * 1500 - 1}, "kept_vertex_one_short": {"kept_vertex_bytes": 4 * 500 - 1},
         "no_verts_then_faces_out_short": {"verts": None, "verts_out": None, "verts_out_bytes": 0, "faces_out_bytes": 0}, **counts_above, **scratch_misaligned})
    simplify_scratch = lib.tvr_mesh_simplify_scratch_bytes(V, F)
    simplify_head = [ptr("verts"), nv, ptr("faces"), nt, ("origin", origin, None), ("cell", unit, None), ("inv_cell", unit, None), ptr("scratch"),
                     ("scratch_bytes", simplify_scratch, 0)]
    simplify_ladder = [["n_vertices", "n_triangles"], ["origin", "cell", "inv_cell", "fault_flag_dev"], ["verts", "faces"], ["scratch"], ["scratch_bytes"]]
    simplify_extra = {"cell_zero": {"cell": _floats(1.0, 0.0, 1.0)}, "cell_nan": {"cell": _floats(NAN, 1.0, 1.0)}, "inv_cell_inf": {"inv_cell": _floats(1.0, 1.0, INF)},
                      "inv_cell_negative": {"inv_cell": _floats(-1.0, 1.0, 1.0)}, "scratch_one_short": {"scratch_bytes": simplify_scratch - 1}, **counts_above,
                      **scratch_misaligned}
    E["tvr_mesh_simplify_count"] = Entry(simplify_head + [ptr("counts_dev"), ptr("fault_flag_dev"), stream], simplify_ladder + [["counts_dev"]], simplify_extra)
    E["tvr_mesh_simplify_emit"] = Entry(
        simplify_head + [ptr("verts_out"), size("verts_out_bytes"), ("n_vertices_out", 500, -1), ptr("faces_out"), size("faces_out_bytes"), ("n_triangles_out", 1500, -1),
                         ptr("vertex_map"), size("vertex_map_bytes"), ptr("fault_flag_dev"), stream],
        simplify_ladder + [["n_vertices_out", "n_triangles_out"], ["verts_out", "faces_out", "vertex_map"], ["verts_out_bytes"], ["faces_out_bytes"], ["vertex_map_bytes"]],
        {"vertices_out_above": {"n_vertices_out": V + 1}, "triangles_out_above": {"n_triangles_out": F + 1}, "verts_out_one_short": {"verts_out_bytes": 12 * 500 - 1},
         "faces_out_one_short": {"faces_out_bytes": 12 * 1500 - 1}, "vertex_map_one_short": {"vertex_map_bytes": 4 * V - 1}, **simplify_extra})
    adj_scratch = lib.tvr_mesh_adjacency_scratch_bytes(V, F)
    adj_head = [ptr("faces"), nt, nv, ptr("scratch"), ("scratch_bytes", adj_scratch, 0)]
    adj_ladder = [["n_triangles", "n_vertices"], ["fault_flag_dev"], ["faces"], ["scratch"], ["scratch_bytes"]]
    adj_extra = {"vertices_above": {"n_vertices": TOP + 1}, "triangles_above": {"n_triangles": TOP // 6 + 1}, "scratch_one_short": {"scratch_bytes": adj_scratch - 1},
                 **scratch_misaligned}
    E["tvr_mesh_adjacency_count"] = Entry(adj_head + [ptr("counts_dev"), ptr("fault_flag_dev"), stream], adj_ladder + [["counts_dev"]], adj_extra)
    E["tvr_mesh_adjacency_emit"] = Entry(
        adj_head + [ptr("offsets"), size("offsets_bytes"), ptr("neighbours"), size("neighbours_bytes"), ptr("edge_faces"), size("edge_faces_bytes"),
                    ("n_half_edges", H, -1), ptr("fault_flag_dev"), stream],
        adj_ladder + [["n_half_edges"], ["offsets", "neighbours", "edge_faces"], ["offsets_bytes"], ["neighbours_bytes"], ["edge_faces_bytes"]],
        {"half_edges_above": {"n_half_edges": 6 * F + 1}, "offsets_one_short": {"offsets_bytes": 4 * (V + 1) - 1}, "neighbours_one_short": {"neighbours_bytes": 4 * H - 1},
         "edge_faces_one_short": {"edge_faces_bytes": 4 * H - 1}, **adj_extra})
    smooth_scratch = lib.tvr_mesh_smooth_scratch_bytes(V, H)
    E["tvr_mesh_smooth"] = Entry(
        [ptr("verts"), nv, ptr("offsets"), ptr("neighbours"), ptr("edge_faces"), ("n_half_edges", H, -1), ("iterations", 3, -1), ("lambda", 0.5, NAN), ("mu", -0.53, INF),
         same("pin_boundary", 1), ptr("scratch"), ("scratch_bytes", smooth_scratch, 0), ptr("verts_out"), ("verts_out_bytes", 12 * V, 0), ptr("fault_flag_dev"), stream],
        [["n_vertices", "n_half_edges"], ["iterations"], ["lambda", "mu"], ["fault_flag_dev", "offsets"], ["verts", "verts_out", "neighbours"], ["edge_faces"],
         ["verts_out_bytes"], ["scratch"], ["scratch_bytes"]],
        {"vertices_above": {"n_vertices": TOP + 1}, "half_edges_above": {"n_half_edges": TOP + 1}, "iterations_above": {"iterations": 1001},
         "verts_out_one_more": {"verts_out_bytes": 12 * V + 1}, "scratch_one_short": {"scratch_bytes": smooth_scratch - 1}, **scratch_misaligned})
    raster_scratch = lib.tvr_mesh_raster_scratch_bytes(F, 48, 64)
    n_pixels = 48 * 64
    E["tvr_mesh_raster"] = Entry(
        [ptr("verts"), nv, ptr("faces"), nt, ("cam", _ref(cam), None), ptr("attr"), ("n_attr", 2, -1), ptr("depth"), size("depth_bytes"), ptr("tri"), size("tri_bytes"),
         ptr("bary"), size("bary_bytes"), ptr("attr_out"), size("attr_out_bytes"), ptr("scratch"), ("scratch_bytes", raster_scratch, 0), ptr("counts_dev"),
         ptr("fault_flag_dev"), stream],
        [["cam"], ["depth", "tri", "bary", "scratch", "counts_dev", "fault_flag_dev"], ["n_vertices"], ["n_attr"], ["attr", "attr_out"], ["n_triangles"], ["faces", "verts"],
         ["depth_bytes"], ["tri_bytes"], ["bary_bytes"], ["attr_out_bytes"], ["scratch_bytes"]],
        {"c2w_nan": {"cam": _ref(_camera(c2w=(1, 0, 0, 0, 0, NAN, 0, 0, 0, 0, 1, 0)))}, "fx_zero": {"cam": _ref(_camera(fx=0.0))}, "fy_inf": {"cam": _ref(_camera(fy=INF))},
         "cx_inf": {"cam": _ref(_camera(cx=INF))}, "near_negative": {"cam": _ref(_camera(near_=-1.0))}, "cull_two": {"cam": _ref(_camera(cull=2))},
         "large_bbox_negative": {"cam": _ref(_camera(large_bbox=-1))}, "n_attr_above": {"n_attr": 9}, "height_zero": {"cam": _ref(_camera(H=0))},
         "width_above": {"cam": _ref(_camera(W=(1 << 24) + 1))}, "pixels_above": {"cam": _ref(_camera(H=65536, W=65536))}, "triangles_above": {"n_triangles": TOP + 1},
         "vertices_above": {"n_vertices": TOP + 1}, "depth_one_short": {"depth_bytes": 4 * n_pixels - 1}, "tri_one_short": {"tri_bytes": 4 * n_pixels - 1},
         "bary_one_short": {"bary_bytes": 12 * n_pixels - 1}, "attr_out_one_short": {"attr_out_bytes": 8 * n_pixels - 1},
         "scratch_one_short": {"scratch_bytes": raster_scratch - 1}, **scratch_misaligned})
    atlas_h, atlas_w = 94 * 8, 16 * 8                              # 3000 triangles -> 1500 squares, 16 per row, patch side 8
    E["tvr_mesh_atlas_points"] = Entry(
        [ptr("verts"), nv, ptr("faces"), nt, ("P", 8, 0), ("C", 16, 0), ("texel0", 0, -1), ("n", 1000, -1), ptr("pos_out"), size("pos_bytes"), ptr("tri_out"),
         size("tri_bytes"), ptr("fault_flag_dev"), stream],
        [["fault_flag_dev"], ["n_vertices"], ["n_triangles"], ["P"], ["C"], ["faces", "verts"], ["texel0", "n"], ["pos_out", "tri_out"], ["pos_bytes"], ["tri_bytes"]],
        {"P_above": {"P": 65}, "triangles_above": {"n_triangles": TOP + 1}, "atlas_above": {"n_triangles": TOP, "P": 64, "C": 1}, "vertices_above": {"n_vertices": TOP + 1},
         "range_leaves_atlas": {"texel0": atlas_h * atlas_w - 999}, "pos_one_short": {"pos_bytes": 11999}, "tri_one_short": {"tri_bytes": 3999}})
    E["tvr_mesh_texture_sample"] = Entry(
        [ptr("tri"), ptr("bary"), ("n_pix", 1000, -1), ptr("atlas"), ("fmt", 0, 2), ("Ha", atlas_h, 0), ("Wa", atlas_w, 0), ("P", 8, 0), ("C", 16, 0), nt, ptr("out"),
         size("out_bytes"), stream],
        [["n_pix"], ["fmt"], ["n_triangles"], ["P"], ["C"], ["Ha", "Wa"], ["atlas"], ["tri", "bary", "out"], ["out_bytes"]],
        {"pixels_above": {"n_pix": TOP + 1}, "triangles_above": {"n_triangles": TOP + 1}, "height_off_by_one": {"Ha": atlas_h + 8}, "out_one_short": {"out_bytes": 11999}})
    E["tvr_mesh_bvh_describe"] = Entry([nt, ("out", _ref(L.MeshBvhLayout()), None)], [["out"], ["n_triangles"]], {"triangles_above": {"n_triangles": MAX_F + 1}})
    bvh_scratch_args = [ptr("scratch"), ("scratch_bytes", bvh_scratch, bvh_scratch - 1)]
    E["tvr_mesh_bvh_keys"] = Entry(
        mesh + [ptr("keys_out"), ("keys_bytes", 8 * F, 8 * F - 1)] + bvh_scratch_args + [ptr("fault_flag_dev"), stream],
        mesh_ladder + [["keys_out"], ["keys_bytes"], ["scratch"], ["scratch_bytes"]],
        {"keys_out_odd": {"keys_out": ODD}, **mesh_extra, **scratch_misaligned})
    E["tvr_mesh_bvh_build"] = Entry(
        mesh + [ptr("sorted_keys")] + blob + bvh_scratch_args + [same("counts_dev", PTR), ptr("fault_flag_dev"), stream],
        mesh_ladder + [["sorted_keys"]] + blob_ladder + [["scratch"], ["scratch_bytes"]],
        {"sorted_keys_odd": {"sorted_keys": ODD}, **mesh_extra, **blob_extra, **scratch_misaligned})
    E["tvr_mesh_bvh_cast"] = Entry(
        mesh + blob + [ptr("origins"), ptr("dirs"), ("n_rays", 100, -1), ("t_min", 0.0, NAN), ("t_max", INF, NAN), ("mode", 0, 2), ("cull", 0, 2), ptr("t"),
                       ("t_bytes", 400, 399), ptr("tri"), ("tri_bytes", 400, 399), ptr("bary"), ("bary_bytes", 1200, 1199), ptr("hit"), ("hit_bytes", 100, 99), counts,
                       ptr("fault_flag_dev"), stream],
        mesh_ladder + [["n_rays"], ["mode"], ["cull"], ["t_min", "t_max"]] + blob_ladder + [["origins", "dirs"], ["t", "tri", "bary"], ["t_bytes"], ["tri_bytes"],
                                                                                          ["bary_bytes"]],
        {"rays_above": {"n_rays": TOP + 1}, "t_max_nan": {"t_max": NAN}, "any_hit_without_hit": {"mode": 1, "hit": None, "t": None, "tri": None, "bary": None},
         "any_hit_one_short": {"mode": 1, "hit_bytes": 99}, **mesh_extra, **blob_extra})
    E["tvr_mesh_bvh_occlusion"] = Entry(
        mesh + blob + [ptr("points"), ptr("normals"), ("n_points", 100, -1), ptr("dirs"), ("n_dirs", 16, -1), ("bias", 1e-3, NAN), ("t_max", INF, NAN), ptr("out"),
                       ("out_bytes", 400, 399), counts, ptr("fault_flag_dev"), stream],
        mesh_ladder + [["n_points", "n_dirs"], ["bias"], ["t_max"]] + blob_ladder + [["points", "normals", "out"], ["dirs"], ["out_bytes"]],
        {"points_above": {"n_points": TOP + 1}, "dirs_above": {"n_dirs": 65537}, "dirs_negative": {"n_dirs": -1}, "bias_inf": {"bias": INF}, **mesh_extra, **blob_extra})
    E["tvr_mesh_bvh_nearest"] = Entry(
        mesh + blob + [ptr("points"), ("n_points", 100, -1), ("max_dist", INF, -1.0), ptr("dist"), ("dist_bytes", 400, 399), ptr("tri"), ("tri_bytes", 400, 399),
                       ptr("bary"), ("bary_bytes", 1200, 1199), counts, ptr("fault_flag_dev"), stream],
        mesh_ladder + [["n_points"], ["max_dist"]] + blob_ladder + [["points", "dist", "tri", "bary"], ["dist_bytes"], ["tri_bytes"], ["bary_bytes"]],
        {"points_above": {"n_points": TOP + 1}, "max_dist_nan": {"max_dist": NAN}, **mesh_extra, **blob_extra})
    E["tvr_mesh_pseudonormals_describe"] = Entry([nv, nt, ("out", _ref(L.MeshPseudonormalsLayout()), None)], [["out"], ["n_triangles"], ["n_vertices"]], mesh_extra)
    E["tvr_mesh_pseudonormals_keys"] = Entry(
        [ptr("faces"), nv, nt, ptr("corner_keys_out"), ptr("edge_keys_out"), ("keys_bytes", 24 * F, 24 * F - 1), ptr("fault_flag_dev"), stream],
        [["n_triangles"], ["n_vertices"], ["fault_flag_dev"], ["faces", "corner_keys_out", "edge_keys_out"], ["keys_bytes"]],
        {"corner_keys_odd": {"corner_keys_out": ODD}, "edge_keys_odd": {"edge_keys_out": ODD}, **mesh_extra})
    E["tvr_mesh_pseudonormals_build"] = Entry(
        mesh + [ptr("sorted_corner_keys"), ptr("sorted_edge_keys"), ptr("edge_order"), ptr("table"), ("table_bytes", pn_bytes, pn_bytes - 1), ptr("scratch"),
                ("scratch_bytes", pn_scratch, pn_scratch - 1), same("counts_dev", PTR), ptr("fault_flag_dev"), stream],
        mesh_ladder + [["sorted_corner_keys", "sorted_edge_keys", "edge_order"], ["table"], ["table_bytes"], ["scratch"], ["scratch_bytes"]],
        {"corner_keys_odd": {"sorted_corner_keys": ODD}, "edge_order_odd": {"edge_order": ODD}, "table_misaligned": {"table": MISALIGNED}, **mesh_extra, **scratch_misaligned})
    E["tvr_mesh_bvh_signed"] = Entry(
        mesh + blob + [ptr("table"), ("table_bytes", pn_bytes, pn_bytes - 1), ptr("points"), ("n_points", 100, -1), same("lattice", None), ("max_dist", INF, -1.0),
                       ptr("sdist"), ("sdist_bytes", 400, 399), same("tri", PTR), ("tri_bytes", 400, 399), same("bary", PTR), ("bary_bytes", 1200, 1199),
                       same("feature", PTR), ("feature_bytes", 100, 99), counts, ptr("fault_flag_dev"), stream],
        mesh_ladder + [["n_points"], ["max_dist"]] + blob_ladder + [["table"], ["table_bytes"], ["points", "sdist"], ["sdist_bytes"], ["tri_bytes"], ["bary_bytes"],
                                                                    ["feature_bytes"]],
        {"table_of_another_mesh": {"table_bytes": pn_bytes + 256}, "lattice_without_sdist": {"points": None, "lattice": _ref(lat), "sdist": None},
         "lattice_sdist_one_short": {"points": None, "lattice": _ref(lat), "sdist_bytes": 3999}, "max_dist_nan": {"max_dist": NAN}, **lattice_extra, **mesh_extra,
         **blob_extra})
    E["tvr_mesh_winding_describe"] = Entry([nt, ("out", _ref(L.MeshWindingLayout()), None)], [["out"], ["n_triangles"]], {"triangles_above": {"n_triangles": MAX_F + 1}})
    E["tvr_mesh_winding_build"] = Entry(
        mesh + blob + [ptr("table"), ("table_bytes", wn_bytes, wn_bytes - 1), ptr("scratch"), ("scratch_bytes", wn_scratch, wn_scratch - 1), ptr("fault_flag_dev"), stream],
        mesh_ladder + blob_ladder + [["table"], ["table_bytes"], ["scratch"], ["scratch_bytes"]],
        {"table_misaligned": {"table": MISALIGNED}, **mesh_extra, **blob_extra, **scratch_misaligned})
    E["tvr_mesh_winding_query"] = Entry(
        mesh + blob + [ptr("table"), ("table_bytes", wn_bytes, wn_bytes - 1), ptr("points"), ("n_points", 100, -1), same("lattice", None), ("beta", 2.0, 0.5), ptr("w"),
                       ("w_bytes", 400, 399), counts, ptr("fault_flag_dev"), stream],
        mesh_ladder + [["beta"], ["n_points"]] + blob_ladder + [["table"], ["table_bytes"], ["points", "w"], ["w_bytes"]],
        {"table_of_another_mesh": {"table_bytes": wn_bytes + 256}, "lattice_without_w": {"points": None, "lattice": _ref(lat), "w": None},
         "lattice_w_one_short": {"points": None, "lattice": _ref(lat), "w_bytes": 3999}, "beta_nan": {"beta": NAN}, **lattice_extra, **mesh_extra, **blob_extra})
    query = [("mode", 1, 2), ptr("verts_q"), ("n_vertices_q", 500, -1), ptr("faces_q"), ("n_triangles_q", 800, -1)]
    query_ladder = mesh_ladder + [["mode"], ["n_triangles_q", "n_vertices_q"], ["faces_q", "verts_q"]] + blob_ladder
    query_extra = {"query_triangles_above": {"n_triangles_q": MAX_F + 1}, "query_vertices_above": {"n_vertices_q": TOP + 1}, "query_vertices_negative": {"n_vertices_q": -1},
                   **mesh_extra, **blob_extra}
    E["tvr_mesh_crossings_count"] = Entry(
        mesh + blob + query + [ptr("count_out"), ("count_bytes", 4 * 800, 4 * 800 - 1), ptr("total_dev"), counts, ptr("fault_flag_dev"), stream],
        query_ladder + [["total_dev"], ["count_out"], ["count_bytes"]],
        {"self_without_count_out": {"mode": 0, "count_out": None}, "self_one_short": {"mode": 0, "count_bytes": 4 * F - 1}, **query_extra})
    E["tvr_mesh_crossings_emit"] = Entry(
        mesh + blob + query + [ptr("offsets"), ("offsets_bytes", 8 * 801, 8 * 801 - 1), ("n_pairs", 50, -1), ptr("pairs"), ("pairs_bytes", 400, 399), ptr("n_pierce"),
                               ("n_pierce_bytes", 200, 199), same("points", PTR), ("points_bytes", 1200, 1199), ptr("fault_flag_dev"), stream],
        query_ladder + [["n_pairs"], ["offsets"], ["offsets_bytes"], ["pairs", "n_pierce"], ["pairs_bytes"], ["n_pierce_bytes"], ["points_bytes"]],
        {"pairs_above": {"n_pairs": TOP + 1}, "offsets_odd": {"offsets": ODD}, "self_offsets_one_short": {"mode": 0, "offsets_bytes": 8 * (F + 1) - 1}, **query_extra})

    two_counts = {"vertices_negative": (-1, 5), "second_negative": (5, -1), "vertices_above": (TOP + 1, 5), "second_above": (5, TOP + 1)}
    triangles = {"negative": (-1,), "above": (MAX_F + 1,)}
    Q = {
        "tvr_mesh_scratch_bytes": {"dims_null": (None,), "dims_below": (_dims(8, 8, 1),), "dims_above": (_dims(900, 900, 900),)},
        "tvr_mesh_components_scratch_bytes": two_counts,
        "tvr_mesh_filter_scratch_bytes": two_counts,
        "tvr_mesh_simplify_scratch_bytes": two_counts,
        "tvr_mesh_adjacency_scratch_bytes": {**two_counts, "second_above": (5, TOP // 6 + 1)},
        "tvr_mesh_smooth_scratch_bytes": two_counts,
        "tvr_mesh_raster_scratch_bytes": {"triangles_negative": (-1, 4, 4), "height_zero": (5, 0, 4), "width_above": (5, 4, (1 << 24) + 1), "pixels_above": (5, 65536, 65536),
                                          "triangles_above": (TOP + 1, 4, 4)},
        "tvr_mesh_bvh_bytes": triangles,
        "tvr_mesh_bvh_scratch_bytes": triangles,
        "tvr_mesh_pseudonormals_bytes": {"triangles_negative": (5, -1), "triangles_above": (5, MAX_F + 1), "vertices_negative": (-1, 5), "vertices_above": (TOP + 1, 5)},
        "tvr_mesh_pseudonormals_scratch_bytes": triangles,
        "tvr_mesh_winding_bytes": triangles,
        "tvr_mesh_winding_scratch_bytes": triangles,
    }
    return E, Q


def moved_entry_points():
    """The tvr_mesh_* names of _lib.SYMBOLS but tvr_mesh_project, which reads a scene and stayed in tvr_api.hip."""
    return sorted(n for n in _lib().SYMBOLS if n.startswith("tvr_mesh_") and n != "tvr_mesh_project")


def replay(name):
    """-> [(case, status, message)] of one entry point against the loaded library.  A case that is not refused stops the replay of its entry point: the cases after it
    are not tried."""
    lib = _lib().lib()
    E, Q = entries()
    fn = getattr(lib, name)
    cases = list(E[name].cases()) if name in E else list(Q[name].items())
    out = []
    for case, args in cases:
        status = fn(*args)
        message = lib.tvr_last_error()
        out.append((case, status, message.decode("ascii")))
        if name in E:
            assert status != ERR_HIP, f"{name} / {case} reached a launch: {message!r}"
            assert status < 0, f"{name} / {case} was not refused"
        else:
            assert status == 0 and message, f"{name} / {case}: a refused size query returns 0 and sets the message, got {status} / {message!r}"
    return out


def record(path=TABLE):
    """Run by hand, once, with TVR_LIB_PATH naming the library of the commit before the change under test; never at test time."""
    rows = [[name, case, status, message] for name in moved_entry_points() for case, status, message in replay(name)]
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} rows of {len(moved_entry_points())} entry points from {_lib().LIB_PATH} -> {path}")


@functools.lru_cache(maxsize=None)
def table():
    by_entry = {}
    for name, case, status, message in json.load(open(TABLE)):
        by_entry.setdefault(name, []).append((case, status, message))
    return by_entry


def test_the_table_covers_every_moved_entry_point():
    E, Q = entries()
    names = moved_entry_points()
    assert len(names) == 41 and sorted(list(E) + list(Q)) == names == sorted(table())
    for name in E:
        rows = table()[name]
        assert rows[0][0] == "ladder_00" and len(rows) >= 2
        assert all(status in (-1, -3, -4) for _, status, _ in rows), name         # TVR_ERR_INVALID / _SCRATCH / _UNSUPPORTED: never TVR_ERR_HIP, never TVR_OK
    for name in Q:
        assert all(status == 0 and message for _, status, message in table()[name]), name


@pytest.mark.parametrize("name", moved_entry_points())
def test_refusals_are_the_recorded_bytes(name):
    got, want = replay(name), table()[name]
    assert [c for c, _, _ in got] == [c for c, _, _ in want]
    for (case, status, message), (_, want_status, want_message) in zip(got, want):
        assert (status, message.encode()) == (want_status, want_message.encode()), (name, case)


if __name__ == "__main__":
    if sys.argv[1:] == ["record"]:
        record()
    else:
        sys.exit("usage: TVR_LIB_PATH=<libtvr.so of the commit before the change> python tests/test_mesh_api_errors_host.py record")
