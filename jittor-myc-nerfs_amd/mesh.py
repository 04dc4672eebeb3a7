"""Iso-surface extraction and the PLY file behind `--export_mesh 1` (reference tensorf-myc/utils.py:146-207 `convert_sdf_samples_to_ply`, which calls
skimage.measure.marching_cubes and plyfile on the CPU).  Here the extraction is the HIP marching cubes of csrc/tvr_mesh.hip (include/tvr.h tvr_mesh_*,
DESIGN.md §4.10) and the PLY reader / writer is numpy.  There is no CPU fallback for the extraction: a CPU tensor raises TvrError like every other product path.

Orientation: triangle normals (right-hand rule) point from `>= level` to `< level`, i.e. out of the dense region.  The reference reverses the vertex order
skimage returns (utils.py:171); whether that equals this orientation cannot be checked without skimage, hence `flip`."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .autograd_ops import _stream_ptr

MESH_TILE = 1024            # include/tvr.h TVR_MESH_TILE: points per scan tile
MESH_SCAN_CHUNK = 256       # include/tvr.h TVR_MESH_SCAN_CHUNK: tile sums per step of the one workgroup that scans them


def _volume_on_device(volume) -> torch.Tensor:
    if not torch.is_tensor(volume) or volume.device.type != "cuda":
        where = volume.device if torch.is_tensor(volume) else type(volume).__name__
        raise L.TvrError(f"marching_cubes runs on an MI355X (HIP) device only; the volume is on {where}. There is no CPU fallback.")
    if volume.dim() != 3:
        raise L.TvrError(f"marching_cubes takes a volume [nx, ny, nz]; got shape {tuple(volume.shape)}")
    return volume.detach().to(torch.float32).contiguous()


def _dims(volume):
    return (C.c_int32 * 3)(*[int(s) for s in volume.shape])


def mesh_count(volume: torch.Tensor, level: float):
    """First step (tvr_mesh_count): (volume as passed to the library, filled scratch buffer, n_vertices, n_triangles).  Reads the two totals from the device once."""
    vol = _volume_on_device(volume)
    lib, dims = L.lib(), _dims(vol)
    nbytes = lib.tvr_mesh_scratch_bytes(dims)
    if nbytes == 0:
        raise L.TvrError("marching_cubes: " + lib.tvr_last_error().decode(errors="replace"))
    scratch = L.dev_bytes(nbytes, vol.device, what="mesh scratch")
    counts = L.dev_empty((2,), torch.int64, vol.device, what="mesh counts")
    L.check(lib.tvr_mesh_count(vol.data_ptr(), dims, float(level), scratch.data_ptr(), L.nbytes(scratch), counts.data_ptr(), _stream_ptr(vol.device)), "tvr_mesh_count")
    n_vertices, n_triangles = (int(x) for x in counts.cpu().tolist())
    return vol, scratch, n_vertices, n_triangles


def mesh_emit(vol: torch.Tensor, level: float, scratch: torch.Tensor, n_vertices: int, n_triangles: int, spacing=(1, 1, 1), origin=(0, 0, 0), flip: bool = False):
    """Second step (tvr_mesh_emit) into buffers of exactly the declared counts: (verts [V,3] float32, faces [F,3] int32, fault flag [1] int32 on the device).
    Counts that are not the ones mesh_count found raise the flag and leave the buffers unwritten."""
    lib, dims = L.lib(), _dims(vol)
    verts = L.dev_empty((int(n_vertices), 3), torch.float32, vol.device, what="mesh verts")
    faces = L.dev_empty((int(n_triangles), 3), torch.int32, vol.device, what="mesh faces")
    flag = L.dev_bytes(4, vol.device, zero=True, what="mesh fault flag").view(torch.int32)
    org, sp = (C.c_float * 3)(*[float(x) for x in origin]), (C.c_float * 3)(*[float(x) for x in spacing])
    L.check(lib.tvr_mesh_emit(vol.data_ptr(), dims, float(level), org, sp, scratch.data_ptr(), L.nbytes(scratch), verts.data_ptr() if n_vertices else None,
                              L.nbytes(verts), int(n_vertices), faces.data_ptr() if n_triangles else None, L.nbytes(faces), int(n_triangles), 1 if flip else 0,
                              flag.data_ptr(), _stream_ptr(vol.device)), "tvr_mesh_emit")
    return verts, faces, flag


def marching_cubes(volume: torch.Tensor, level: float, spacing=(1, 1, 1), origin=(0, 0, 0), flip: bool = False):
    """Iso-surface `volume == level` of a dense fp32 device volume [nx, ny, nz] -> (verts [V,3] float32, faces [F,3] int32), both on the volume's device.

    A grid point is inside iff value >= level.  One vertex per grid edge whose ends straddle the level, at `origin + (index + t) * spacing` with
    t = (level - a) / (b - a) along the edge; vertices are ordered by (owner grid point, axis), triangles by cell — the result is indexed, welded and the same
    bit for bit on every run.  Normals point from inside to outside; `flip=True` reverses every triangle.  An empty surface gives empty tensors."""
    vol, scratch, n_vertices, n_triangles = mesh_count(volume, level)
    verts, faces, flag = mesh_emit(vol, level, scratch, n_vertices, n_triangles, spacing, origin, flip)
    if int(flag.item()) != 0:
        raise L.TvrError("tvr_mesh_emit raised its fault flag: the counted totals and the declared capacities disagree (include/tvr.h)")
    return verts, faces


# ---- connected components and the component filter (csrc/tvr_mesh_cc.hip, include/tvr.h tvr_mesh_components / tvr_mesh_filter_*) -------------------------------------------
def _faces_on_device(faces, what: str) -> torch.Tensor:
    if not torch.is_tensor(faces) or faces.device.type != "cuda":
        where = faces.device if torch.is_tensor(faces) else type(faces).__name__
        raise L.TvrError(f"{what} runs on an MI355X (HIP) device only; the faces are on {where}. There is no CPU fallback.")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise L.TvrError(f"{what} takes faces [F, 3]; got shape {tuple(faces.shape)}")
    return faces.detach().to(torch.int32).contiguous()


def _ptr(t: torch.Tensor):
    return t.data_ptr() if t.numel() else None


def _policy(min_faces, keep_largest):
    min_faces, keep_largest = int(min_faces), int(keep_largest)
    if min_faces < 0 or keep_largest < 0:
        raise ValueError(f"min_faces = {min_faces} / keep_largest = {keep_largest}: negative values mean nothing (0 switches an option off)")
    return min_faces, keep_largest


def mesh_components(faces: torch.Tensor, n_vertices: int, stats: dict = None):
    """Connected components of an indexed triangle mesh on the device -> (vertex_label [V] int32, component_faces [V] int32, n_components).

    Two vertices are connected iff a chain of triangles links them; a vertex no triangle uses is a component of its own.  vertex_label[v] is the SMALLEST vertex
    index of v's component; component_faces holds, at each label, the number of triangles whose first vertex carries it (0 elsewhere).  All three are functions of the
    mesh alone: the same on every run.  A face index outside 0 .. V-1 raises TvrError.  `stats` (a dict) receives max_walk_steps / walk_step_bound."""
    f = _faces_on_device(faces, "mesh_components")
    V, F = int(n_vertices), int(f.shape[0])
    lib, dev = L.lib(), f.device
    nbytes = lib.tvr_mesh_components_scratch_bytes(V, F)
    if nbytes == 0:
        raise L.TvrError("mesh_components: " + lib.tvr_last_error().decode(errors="replace"))
    scratch = L.dev_bytes(nbytes, dev, what="mesh components scratch")
    label = L.dev_empty((V,), torch.int32, dev, what="mesh vertex labels")
    sizes = L.dev_empty((V,), torch.int32, dev, what="mesh component sizes")
    n_comp = L.dev_empty((1,), torch.int64, dev, what="mesh component count")
    flag = L.dev_bytes(4, dev, zero=True, what="mesh components fault flag").view(torch.int32)
    L.check(lib.tvr_mesh_components(_ptr(f), F, V, _ptr(label), L.nbytes(label), _ptr(sizes), L.nbytes(sizes), n_comp.data_ptr(), scratch.data_ptr(), L.nbytes(scratch),
                                    flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_components")
    if int(flag.item()) != 0:
        raise L.TvrError(f"tvr_mesh_components raised its fault flag: a face index lies outside 0 .. {V - 1} (or a walk gave up; include/tvr.h)")
    if stats is not None:
        stats["max_walk_steps"] = int(scratch[4:8].view(torch.int32).item())
        stats["walk_step_bound"] = min(2 * V + 64, 2 ** 32 - 1)
    return label, sizes, int(n_comp.item())


def component_keep_mask(vertex_label: torch.Tensor, component_faces: torch.Tensor, min_faces: int = 0, keep_largest: int = 0) -> torch.Tensor:
    """The size policy as keep_root [V] uint8 (1 at the labels of the components to keep, read at labels only), on the tensors' device — CPU tensors work too.

    In this order: min_faces = m keeps the components with at least m triangles; keep_largest = K then keeps, among those, the K with the most triangles, ties going to
    the SMALLER label.  0 switches an option off; with either option on, components without triangles (unused vertices) are never kept; with both off every component is."""
    min_faces, keep_largest = _policy(min_faces, keep_largest)
    V = int(vertex_label.shape[0])
    sizes = component_faces.to(torch.int64)
    keep = vertex_label.to(torch.int64) == torch.arange(V, dtype=torch.int64, device=vertex_label.device)
    if min_faces or keep_largest:
        keep &= sizes >= max(min_faces, 1)
    if keep_largest:
        roots = keep.nonzero().view(-1)                              # ascending labels
        if roots.numel() > keep_largest:
            key = (sizes.max() - sizes[roots]) * max(V, 1) + roots   # (size descending, label ascending) in one int64: both factors are below 2^31
            keep = torch.zeros_like(keep)
            keep[roots[torch.argsort(key)[:keep_largest]]] = True
    return keep.to(torch.uint8)


def filter_count(faces: torch.Tensor, n_vertices: int, vertex_label: torch.Tensor, keep_root: torch.Tensor):
    """First step (tvr_mesh_filter_count): (filled scratch buffer, surviving vertices, surviving triangles, fault flag [1] int32 on the device)."""
    lib, dev = L.lib(), faces.device
    V, F = int(n_vertices), int(faces.shape[0])
    nbytes = lib.tvr_mesh_filter_scratch_bytes(V, F)
    if nbytes == 0:
        raise L.TvrError("filter_components: " + lib.tvr_last_error().decode(errors="replace"))
    scratch = L.dev_bytes(nbytes, dev, what="mesh filter scratch")
    counts = L.dev_empty((2,), torch.int64, dev, what="mesh filter counts")
    flag = L.dev_bytes(4, dev, zero=True, what="mesh filter fault flag").view(torch.int32)
    L.check(lib.tvr_mesh_filter_count(_ptr(faces), F, V, _ptr(vertex_label), _ptr(keep_root), scratch.data_ptr(), L.nbytes(scratch), counts.data_ptr(), flag.data_ptr(),
                                      _stream_ptr(dev)), "tvr_mesh_filter_count")
    n_v, n_f = (int(x) for x in counts.cpu().tolist())
    return scratch, n_v, n_f, flag


def filter_emit(verts, faces: torch.Tensor, n_vertices: int, scratch: torch.Tensor, n_vertices_out: int, n_triangles_out: int, flag: torch.Tensor):
    """Second step (tvr_mesh_filter_emit) into buffers of exactly the declared counts: (verts_out [V',3] or None when verts is None, faces_out [F',3], kept_vertex [V'])."""
    lib, dev = L.lib(), faces.device
    verts_out = None if verts is None else L.dev_empty((int(n_vertices_out), 3), torch.float32, dev, what="filtered verts")
    faces_out = L.dev_empty((int(n_triangles_out), 3), torch.int32, dev, what="filtered faces")
    kept = L.dev_empty((int(n_vertices_out),), torch.int32, dev, what="kept vertices")
    L.check(lib.tvr_mesh_filter_emit(None if verts is None else _ptr(verts), _ptr(faces), int(faces.shape[0]), int(n_vertices), scratch.data_ptr(), L.nbytes(scratch),
                                     None if verts_out is None else _ptr(verts_out), 0 if verts_out is None else L.nbytes(verts_out), int(n_vertices_out), _ptr(faces_out),
                                     L.nbytes(faces_out), int(n_triangles_out), _ptr(kept), L.nbytes(kept), flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_filter_emit")
    return verts_out, faces_out, kept


def filter_components(verts: torch.Tensor, faces: torch.Tensor, min_faces: int = 0, keep_largest: int = 0, stats: dict = None):
    """Drop whole connected components of an indexed mesh by size -> (verts [V',3] float32, faces [F',3] int32, kept_vertex [V'] int32), on the device.

    The policy is component_keep_mask's (min_faces first, then keep_largest, ties to the smaller label).  Surviving vertices and faces keep their order; the
    coordinates are the input's bit for bit, the faces are re-indexed and nothing else; kept_vertex[i] is the old index of new vertex i (use it to carry per-vertex
    attributes over).  With both options 0 the inputs are returned as they are with kept_vertex = None and the library is not called.  No CPU fallback.
    `stats` (a dict) receives components / components_kept / triangles_dropped."""
    min_faces, keep_largest = _policy(min_faces, keep_largest)
    if not (min_faces or keep_largest):
        return verts, faces, None
    f = _faces_on_device(faces, "filter_components")
    if not torch.is_tensor(verts) or verts.device != f.device or verts.dim() != 2 or verts.shape[1] != 3:
        raise L.TvrError(f"filter_components takes verts [V, 3] on the faces' device ({f.device})")
    v = verts.detach().to(torch.float32).contiguous()
    V = int(v.shape[0])
    label, sizes, n_components = mesh_components(f, V)
    keep_root = component_keep_mask(label, sizes, min_faces, keep_largest)
    scratch, n_v, n_f, flag = filter_count(f, V, label, keep_root)
    if int(flag.item()) != 0:
        raise L.TvrError("tvr_mesh_filter_count raised its fault flag: a face index or a label lies outside the mesh (include/tvr.h)")
    verts_out, faces_out, kept = filter_emit(v, f, V, scratch, n_v, n_f, flag)
    if int(flag.item()) != 0:
        raise L.TvrError("tvr_mesh_filter_emit raised its fault flag: the counted totals and the declared capacities disagree (include/tvr.h)")
    if stats is not None:
        stats.update(components=n_components, components_kept=int(keep_root.sum().item()), triangles_dropped=int(f.shape[0]) - n_f)
    return verts_out, faces_out, kept


# ---- vertex-clustering simplification (csrc/tvr_mesh_simplify.hip, include/tvr.h tvr_mesh_simplify_*) -------------------------------------------------------------------
def _lattice(cell, origin):
    """(origin, cell, inv_cell) as three fp32 triples; inv_cell = float32(1) / float32(cell), the value include/tvr.h's definition is stated with."""
    c = np.asarray(cell, dtype=np.float64).reshape(-1)
    if c.size == 1:
        c = np.repeat(c, 3)
    if c.size != 3 or not (np.isfinite(c).all() and (c > 0).all()):
        raise ValueError(f"cell = {cell!r}: one positive finite edge length, or three")
    o = np.asarray(origin, dtype=np.float32).reshape(-1)
    if o.size != 3:
        raise ValueError(f"origin = {origin!r}: three coordinates")
    with np.errstate(all="ignore"):
        c = c.astype(np.float32)
        inv = np.float32(1) / c
    if not (np.isfinite(inv).all() and (inv > 0).all() and (c > 0).all()):
        raise ValueError(f"cell = {cell!r}: the edge length or its inverse is not a positive finite fp32 number")
    return o, c, inv


def _c3(a):
    return (C.c_float * 3)(*[float(x) for x in a])


def simplify_count(verts: torch.Tensor, faces: torch.Tensor, origin, cell, inv_cell):
    """First step (tvr_mesh_simplify_count): (filled scratch buffer, vertices out, triangles out, fault flag [1] int32 on the device)."""
    lib, dev = L.lib(), faces.device
    V, F = int(verts.shape[0]), int(faces.shape[0])
    nbytes = lib.tvr_mesh_simplify_scratch_bytes(V, F)
    if nbytes == 0:
        raise L.TvrError("simplify_clustering: " + lib.tvr_last_error().decode(errors="replace"))
    scratch = L.dev_bytes(nbytes, dev, what="mesh simplify scratch")
    counts = L.dev_empty((2,), torch.int64, dev, what="mesh simplify counts")
    flag = L.dev_bytes(4, dev, zero=True, what="mesh simplify fault flag").view(torch.int32)
    L.check(lib.tvr_mesh_simplify_count(_ptr(verts), V, _ptr(faces), F, _c3(origin), _c3(cell), _c3(inv_cell), scratch.data_ptr(), L.nbytes(scratch), counts.data_ptr(),
                                        flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_simplify_count")
    n_v, n_f = (int(x) for x in counts.cpu().tolist())
    return scratch, n_v, n_f, flag


def simplify_emit(verts: torch.Tensor, faces: torch.Tensor, origin, cell, inv_cell, scratch: torch.Tensor, n_vertices_out: int, n_triangles_out: int, flag: torch.Tensor):
    """Second step (tvr_mesh_simplify_emit) into buffers of exactly the declared counts: (verts_out [V',3], faces_out [F',3], vertex_map [V] old -> new)."""
    lib, dev = L.lib(), faces.device
    V, F = int(verts.shape[0]), int(faces.shape[0])
    verts_out = L.dev_empty((int(n_vertices_out), 3), torch.float32, dev, what="simplified verts")
    faces_out = L.dev_empty((int(n_triangles_out), 3), torch.int32, dev, what="simplified faces")
    vmap = L.dev_empty((V,), torch.int32, dev, what="simplify vertex map")
    L.check(lib.tvr_mesh_simplify_emit(_ptr(verts), V, _ptr(faces), F, _c3(origin), _c3(cell), _c3(inv_cell), scratch.data_ptr(), L.nbytes(scratch), _ptr(verts_out),
                                       L.nbytes(verts_out), int(n_vertices_out), _ptr(faces_out), L.nbytes(faces_out), int(n_triangles_out), _ptr(vmap), L.nbytes(vmap),
                                       flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_simplify_emit")
    return verts_out, faces_out, vmap


def simplify_table_capacities(n_vertices: int, n_triangles: int):
    """(cell table slots, triangle table slots): the power of two >= max(256, 2 x elements) include/tvr.h states."""
    def cap(n):
        c = 256
        while c < 2 * int(n):
            c *= 2
        return c
    return cap(n_vertices), cap(n_triangles)


def simplify_clustering(verts: torch.Tensor, faces: torch.Tensor, cell, origin=(0, 0, 0), stats: dict = None):
    """Vertex-clustering simplification on the device -> (verts [V',3] float32, faces [F',3] int32, vertex_map [V] int32 old -> new).

    Vertices fall into the cells of a lattice (edge `cell`, a float or three, world units; corner `origin`; a coordinate on a boundary belongs to the upper cell); each
    cell's vertices merge into their mean (an exact integer mean of the in-cell fractions quantised to 2^-20 of a cell), numbered by their smallest old index; faces are
    re-indexed, the ones with two equal corners go, and of the faces equal up to rotation the one with the smallest old index stays, in its own corner order.  A reversed
    face is another face.  Every cell keeps its vertex whether a face still uses it or not.  The result is a function of the arguments alone: the same bit for bit on
    every run (include/tvr.h tvr_mesh_simplify_* has the arithmetic).  ValueError for a cell that is not positive and finite; TvrError when the library raises its fault
    flag: a vertex outside the lattice (below `origin`, beyond 2^21 cells, NaN) or a face index outside the vertices.  No CPU fallback.
    `stats` (a dict) receives vertices_in / vertices_out / triangles_in / triangles_out / max_probe (longest probe sequence of either hash table, in slots) /
    table_capacity (slots of the larger table; also cell_table_capacity / triangle_table_capacity)."""
    o, c, inv = _lattice(cell, origin)
    f = _faces_on_device(faces, "simplify_clustering")
    if not torch.is_tensor(verts) or verts.device != f.device or verts.dim() != 2 or verts.shape[1] != 3:
        raise L.TvrError(f"simplify_clustering takes verts [V, 3] on the faces' device ({f.device})")
    v = verts.detach().to(torch.float32).contiguous()
    V, F = int(v.shape[0]), int(f.shape[0])
    scratch, n_v, n_f, flag = simplify_count(v, f, o, c, inv)
    if int(flag.item()) != 0:
        raise L.TvrError("tvr_mesh_simplify_count raised its fault flag: a vertex lies outside the lattice (below origin, beyond 2^21 cells, or not a number) or a face "
                         f"index lies outside 0 .. {V - 1} (include/tvr.h)")
    verts_out, faces_out, vmap = simplify_emit(v, f, o, c, inv, scratch, n_v, n_f, flag)
    if int(flag.item()) != 0:
        raise L.TvrError("tvr_mesh_simplify_emit raised its fault flag: the counted totals and the declared capacities disagree (include/tvr.h)")
    if stats is not None:
        cap_v, cap_t = simplify_table_capacities(V, F)
        stats.update(vertices_in=V, vertices_out=n_v, triangles_in=F, triangles_out=n_f, max_probe=int(scratch[4:8].view(torch.int32).item()),
                     table_capacity=max(cap_v, cap_t), cell_table_capacity=cap_v, triangle_table_capacity=cap_t)
    return verts_out, faces_out, vmap


# ---- vertex adjacency and Taubin smoothing (csrc/tvr_mesh_smooth.hip, include/tvr.h tvr_mesh_adjacency_* / tvr_mesh_smooth) --------------------------------------------------
ADJ_SHORT_ROW = 64          # include/tvr.h TVR_MESH_ADJ_SHORT_ROW: raw rows up to this length are sorted by one thread, longer ones by one workgroup
SMOOTH_MAX_ITERATIONS = 1000        # include/tvr.h TVR_MESH_SMOOTH_MAX_ITERATIONS
SMOOTH_LAMBDA, SMOOTH_MU = 0.5, -0.53       # Taubin's pair as export_mesh(smooth=) uses it: the pass band ends at 1/lambda + 1/mu ~ 0.113


def adjacency_count(faces: torch.Tensor, n_vertices: int):
    """First step (tvr_mesh_adjacency_count): (filled scratch buffer, (half_edges, boundary_edges, nonmanifold_edges, max_degree), fault flag [1] int32 on the device)."""
    lib, dev = L.lib(), faces.device
    V, F = int(n_vertices), int(faces.shape[0])
    nbytes = lib.tvr_mesh_adjacency_scratch_bytes(V, F)
    if nbytes == 0:
        raise L.TvrError("mesh_adjacency: " + lib.tvr_last_error().decode(errors="replace"))
    scratch = L.dev_bytes(nbytes, dev, what="mesh adjacency scratch")
    counts = L.dev_empty((4,), torch.int64, dev, what="mesh adjacency counts")
    flag = L.dev_bytes(4, dev, zero=True, what="mesh adjacency fault flag").view(torch.int32)
    L.check(lib.tvr_mesh_adjacency_count(_ptr(faces), F, V, scratch.data_ptr(), L.nbytes(scratch), counts.data_ptr(), flag.data_ptr(), _stream_ptr(dev)),
            "tvr_mesh_adjacency_count")
    return scratch, tuple(int(x) for x in counts.cpu().tolist()), flag


def adjacency_emit(faces: torch.Tensor, n_vertices: int, scratch: torch.Tensor, n_half_edges: int, flag: torch.Tensor):
    """Second step (tvr_mesh_adjacency_emit) into buffers of exactly the declared size: (offsets [V+1], neighbours [H], edge_faces [H]), int32."""
    lib, dev = L.lib(), faces.device
    V, F, H = int(n_vertices), int(faces.shape[0]), int(n_half_edges)
    offsets = L.dev_empty((V + 1,), torch.int32, dev, what="adjacency offsets")
    nbrs = L.dev_empty((H,), torch.int32, dev, what="adjacency neighbours")
    edge_faces = L.dev_empty((H,), torch.int32, dev, what="adjacency edge_faces")
    L.check(lib.tvr_mesh_adjacency_emit(_ptr(faces), F, V, scratch.data_ptr(), L.nbytes(scratch), offsets.data_ptr(), L.nbytes(offsets), _ptr(nbrs), L.nbytes(nbrs),
                                        _ptr(edge_faces), L.nbytes(edge_faces), H, flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_adjacency_emit")
    return offsets, nbrs, edge_faces


def mesh_adjacency(faces: torch.Tensor, n_vertices: int, stats: dict = None):
    """Vertex adjacency of an indexed triangle mesh on the device -> (offsets [V+1], neighbours [H], edge_faces [H]), all int32.

    A face (a, b, c) has the sides {a,b}, {b,c}, {c,a}; a side with two equal ends is ignored.  Row v = neighbours[offsets[v]:offsets[v+1]] holds the DISTINCT vertices
    that share a side with v, ascending (empty for a vertex no side uses); edge_faces, parallel to it, is the number of sides on that edge over all faces (a face listed
    twice counts twice, orientation is ignored): 1 = boundary edge, 2 = closed manifold edge, more = non-manifold.  Every undirected edge appears in both ends' rows.
    The result is a function of the arguments alone.  A face index outside 0 .. V-1 raises TvrError.  No CPU fallback.
    `stats` (a dict) receives half_edges / boundary_edges (undirected edges with one side) / nonmanifold_edges (more than two) / max_degree: a mesh is closed iff
    boundary_edges == 0."""
    f = _faces_on_device(faces, "mesh_adjacency")
    V = int(n_vertices)
    if V < 0:
        raise ValueError(f"n_vertices = {n_vertices}: negative")
    scratch, (H, boundary, nonmanifold, max_degree), flag = adjacency_count(f, V)
    if int(flag.item()) != 0:
        raise L.TvrError(f"tvr_mesh_adjacency_count raised its fault flag: a face index lies outside 0 .. {V - 1} (include/tvr.h)")
    out = adjacency_emit(f, V, scratch, H, flag)
    if int(flag.item()) != 0:
        raise L.TvrError("tvr_mesh_adjacency_emit raised its fault flag: the counted half-edges and the declared capacity disagree (include/tvr.h)")
    if stats is not None:
        stats.update(half_edges=H, boundary_edges=boundary, nonmanifold_edges=nonmanifold, max_degree=max_degree)
    return out


def _smooth_arguments(iterations, lam, mu):
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 0 <= int(iterations) <= SMOOTH_MAX_ITERATIONS:
        raise ValueError(f"iterations = {iterations!r}: an integer in 0 .. {SMOOTH_MAX_ITERATIONS}")
    lam, mu = float(lam), float(mu)
    if not 0 < lam <= 1:
        raise ValueError(f"lam = {lam}: the shrinking step's weight, 0 < lam <= 1")
    if not -1 <= mu <= 1:
        raise ValueError(f"mu = {mu}: the inflating step's weight, -1 <= mu <= 1 (Taubin: mu < -lam; mu = lam is plain Laplacian smoothing)")
    return int(iterations), lam, mu


def smooth_taubin(verts: torch.Tensor, faces: torch.Tensor, iterations: int, lam: float = SMOOTH_LAMBDA, mu: float = SMOOTH_MU, pin_boundary: bool = True,
                  adjacency=None, stats: dict = None) -> torch.Tensor:
    """Taubin lambda|mu smoothing on the device -> verts' [V,3] float32; the faces are unchanged.

    One iteration is two half steps, weight lam then weight mu; in a half step every vertex with neighbours moves by weight x (mean of its neighbours - itself), all
    vertices reading the previous half step's positions.  The mean sums the neighbours in mesh_adjacency's ascending order in fp32, one rounded operation at a time, and
    no atomics are involved: the result is the same bit for bit on every run (include/tvr.h tvr_mesh_smooth has the arithmetic).  pin_boundary keeps every vertex on an
    edge with a single face side where it is.  iterations = 0 returns a copy.  Non-finite coordinates spread, they are not an error.
    adjacency: the (offsets, neighbours, edge_faces) of mesh_adjacency(faces, V) when the caller has them already.
    ValueError unless iterations is an integer in 0 .. 1000, 0 < lam <= 1 and -1 <= mu <= 1; TvrError for CPU tensors (no CPU fallback) and when the library raises its
    fault flag (an adjacency that does not belong to V vertices).  `stats` (a dict) receives mesh_adjacency's counts (when it is computed here) and smooth_iterations."""
    iterations, lam, mu = _smooth_arguments(iterations, lam, mu)
    f = _faces_on_device(faces, "smooth_taubin")
    if not torch.is_tensor(verts) or verts.device != f.device or verts.dim() != 2 or verts.shape[1] != 3:
        raise L.TvrError(f"smooth_taubin takes verts [V, 3] on the faces' device ({f.device})")
    v = verts.detach().to(torch.float32).contiguous()
    V = int(v.shape[0])
    if adjacency is None:
        adjacency = mesh_adjacency(f, V, stats=stats)
    offsets, nbrs, edge_faces = (a.detach().to(device=f.device, dtype=torch.int32).contiguous() for a in adjacency)
    if offsets.numel() != V + 1 or nbrs.numel() != edge_faces.numel():
        raise L.TvrError(f"smooth_taubin: adjacency of {offsets.numel() - 1} vertices / {nbrs.numel()} and {edge_faces.numel()} half-edges for {V} vertices")
    H = int(nbrs.numel())
    lib, dev = L.lib(), f.device
    nbytes = lib.tvr_mesh_smooth_scratch_bytes(V, H)
    if nbytes == 0:
        raise L.TvrError("smooth_taubin: " + lib.tvr_last_error().decode(errors="replace"))
    scratch = L.dev_bytes(nbytes, dev, what="mesh smooth scratch")
    out = L.dev_empty((V, 3), torch.float32, dev, what="smoothed verts")
    flag = L.dev_bytes(4, dev, zero=True, what="mesh smooth fault flag").view(torch.int32)
    L.check(lib.tvr_mesh_smooth(_ptr(v), V, offsets.data_ptr(), _ptr(nbrs), _ptr(edge_faces), H, iterations, lam, mu, 1 if pin_boundary else 0, scratch.data_ptr(),
                                L.nbytes(scratch), _ptr(out), L.nbytes(out), flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_smooth")
    if int(flag.item()) != 0:
        raise L.TvrError(f"tvr_mesh_smooth raised its fault flag: offsets do not run from 0 to {H} without decreasing, or a neighbour lies outside 0 .. {V - 1} "
                         "(include/tvr.h)")
    if stats is not None:
        stats["smooth_iterations"] = iterations
    return out


# ---- PLY: the subset plyfile writes for the reference (utils.py:192-207) -----------------------------------------------------------------------------------
_VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


_NORMAL_FIELDS = [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
_COLOR_FIELDS = [("red", "u1"), ("green", "u1"), ("blue", "u1")]


def _vertex_dtype(normals: bool, colors: bool) -> np.dtype:
    return np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + (_NORMAL_FIELDS if normals else []) + (_COLOR_FIELDS if colors else []))


def ply_header(n_vertices: int, n_faces: int, normals: bool = False, colors: bool = False) -> bytes:
    extra = ("property float nx\nproperty float ny\nproperty float nz\n" if normals else "") + \
            ("property uchar red\nproperty uchar green\nproperty uchar blue\n" if colors else "")
    return (f"ply\nformat binary_little_endian 1.0\nelement vertex {int(n_vertices)}\nproperty float x\nproperty float y\nproperty float z\n{extra}"
            f"element face {int(n_faces)}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")


def _host(a, dtype):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a).reshape(-1, 3), dtype=dtype)


def write_ply(path, verts, faces, normals=None, colors=None) -> None:
    """Binary little-endian PLY with the two elements the reference writes through plyfile: `vertex` (float x, y, z) and `face`
    (property list uchar int vertex_indices, three indices per face).  verts [V,3], faces [F,3]: tensors (any device) or arrays.
    normals [V,3] float / colors [V,3] uint8 (optional, not in the reference's files) append `float nx ny nz` / `uchar red green blue` to the vertex element."""
    v, f = _host(verts, "<f4"), _host(faces, "<i4")
    rows = np.empty(len(f), dtype=_FACE_DTYPE)
    rows["n"] = 3
    rows["v"] = f
    if normals is None and colors is None:
        body = v.tobytes()
    else:
        vr = np.empty(len(v), dtype=_vertex_dtype(normals is not None, colors is not None))
        vr["x"], vr["y"], vr["z"] = v[:, 0], v[:, 1], v[:, 2]
        for given, fields, dt, what in ((normals, _NORMAL_FIELDS, "<f4", "normals"), (colors, _COLOR_FIELDS, "u1", "colors")):
            if given is None:
                continue
            a = given.detach().cpu().numpy() if torch.is_tensor(given) else np.asarray(given)
            if what == "colors" and a.dtype != np.uint8:
                raise ValueError(f"colors must be uint8 (0..255), got {a.dtype}")
            a = _host(a, dt)
            if len(a) != len(v):
                raise ValueError(f"{what} holds {len(a)} rows for {len(v)} vertices")
            for j, (name, _) in enumerate(fields):
                vr[name] = a[:, j]
        body = vr.tobytes()
    with open(path, "wb") as out:
        out.write(ply_header(len(v), len(f), normals is not None, colors is not None))
        out.write(body)
        out.write(rows.tobytes())


def read_ply(path):
    """Reads back what write_ply writes: (verts [V,3] float32, faces [F,3] int32) as numpy arrays.  Anything outside that subset is a ValueError."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = data[:end].decode("ascii").split("\n")
    body = data[end + len(b"end_header\n"):]
    counts = {}
    for line in lines:
        tok = line.split()
        if tok[:1] == ["element"]:
            counts[tok[1]] = int(tok[2])
    if set(counts) != {"vertex", "face"} or data[:end + len(b"end_header\n")] != ply_header(counts["vertex"], counts["face"]):
        raise ValueError(f"{path}: only binary little-endian PLY with float x y z vertices and uchar/int triangle lists is read")
    nv, nf = counts["vertex"], counts["face"]
    if len(body) != nv * _VERTEX_DTYPE.itemsize + nf * _FACE_DTYPE.itemsize:
        raise ValueError(f"{path}: body of {len(body)} B does not hold {nv} vertices and {nf} triangles")
    v = np.frombuffer(body, dtype="<f4", count=nv * 3).reshape(nv, 3).astype(np.float32)
    rows = np.frombuffer(body, dtype=_FACE_DTYPE, count=nf, offset=nv * _VERTEX_DTYPE.itemsize)
    if nf and not (rows["n"] == 3).all():
        raise ValueError(f"{path}: a face is not a triangle")
    return v, rows["v"].astype(np.int32).reshape(nf, 3)


def read_ply_attributes(path):
    """Reads back every file write_ply can write: (verts [V,3] float32, faces [F,3] int32, attributes) with attributes a dict that holds "normals" [V,3] float32 and /
    or "colors" [V,3] uint8 when the file has them.  Any other property set, format or body size is a ValueError."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    head = data[:end + len(b"end_header\n")]
    body = data[len(head):]
    counts = {}
    try:
        for line in head.decode("ascii").split("\n"):
            tok = line.split()
            if tok[:1] == ["element"]:
                counts[tok[1]] = int(tok[2])
    except (UnicodeDecodeError, IndexError, ValueError):
        raise ValueError(f"{path}: malformed PLY header") from None
    if set(counts) != {"vertex", "face"}:
        raise ValueError(f"{path}: a vertex and a face element are read, the file declares {sorted(counts)}")
    nv, nf = counts["vertex"], counts["face"]
    if nv < 0 or nf < 0:
        raise ValueError(f"{path}: negative element count")
    for has_n, has_c in ((False, False), (True, False), (False, True), (True, True)):
        if head == ply_header(nv, nf, has_n, has_c):
            break
    else:
        raise ValueError(f"{path}: only binary little-endian PLY with float x y z [nx ny nz] [uchar red green blue] vertices and uchar/int triangle lists is read")
    vdt = _vertex_dtype(has_n, has_c)
    if len(body) != nv * vdt.itemsize + nf * _FACE_DTYPE.itemsize:
        raise ValueError(f"{path}: body of {len(body)} B does not hold {nv} vertices and {nf} triangles")
    vr = np.frombuffer(body, dtype=vdt, count=nv)
    rows = np.frombuffer(body, dtype=_FACE_DTYPE, count=nf, offset=nv * vdt.itemsize)
    if nf and not (rows["n"] == 3).all():
        raise ValueError(f"{path}: a face is not a triangle")
    attrs = {}
    if has_n:
        attrs["normals"] = np.stack((vr["nx"], vr["ny"], vr["nz"]), -1).astype(np.float32).reshape(nv, 3)
    if has_c:
        attrs["colors"] = np.stack((vr["red"], vr["green"], vr["blue"]), -1).astype(np.uint8).reshape(nv, 3)
    verts = np.stack((vr["x"], vr["y"], vr["z"]), -1).astype(np.float32).reshape(nv, 3)
    return verts, rows["v"].astype(np.int32).reshape(nf, 3), attrs


# ---- z-buffer rasteriser (csrc/tvr_mesh_raster.hip, include/tvr.h tvr_mesh_raster) ------------------------------------------------------------------------------------------
RASTER_LARGE_BBOX = 64      # include/tvr.h TVR_MESH_RASTER_LARGE_BBOX: a screen box above this many pixels is drawn by a workgroup, not by one lane
RASTER_MAX_ATTR = 8         # include/tvr.h TVR_MESH_RASTER_MAX_ATTR


def mesh_camera(c2w, H: int, W: int, focal, center=None, near: float = 0.0, cull: bool = False, large_bbox: int = 0) -> "L.MeshCamera":
    """The tvr_mesh_camera of a pose: c2w is the 3x4 (or 4x4) matrix rays.get_rays takes, focal a number or (fx, fy), center (cx, cy) or None = (W/2, H/2)."""
    m = np.asarray(c2w.detach().cpu().numpy() if torch.is_tensor(c2w) else c2w, dtype=np.float32)
    if m.shape not in ((3, 4), (4, 4)):
        raise ValueError(f"c2w has shape {m.shape}: a 3x4 or 4x4 camera-to-world matrix is taken")
    if torch.is_tensor(focal):
        focal = focal.detach().cpu().tolist()
    fx, fy = (focal, focal) if np.ndim(focal) == 0 else tuple(focal)
    cx, cy = (W / 2, H / 2) if center is None else tuple(center)
    cam = L.MeshCamera()
    cam.c2w[:] = [float(x) for x in m[:3, :4].reshape(-1)]
    cam.H, cam.W, cam.fx, cam.fy, cam.cx, cam.cy = int(H), int(W), float(fx), float(fy), float(cx), float(cy)
    cam.near_, cam.cull, cam.large_bbox = float(near), 1 if cull else 0, int(large_bbox)
    return cam


def render_mesh(verts: torch.Tensor, faces: torch.Tensor, c2w, H: int, W: int, focal, center=None, near: float = 0.0, cull: bool = False, attributes=None,
                large_bbox: int = 0, stats: dict = None):
    """Depth-buffer picture of an indexed triangle mesh from one camera, on the device -> (depth [H,W] float32, tri [H,W] int32, bary [H,W,3] float32,
    attr [H,W,A] float32 or None).

    The camera is rays.py's: c2w is what rays.get_rays takes (after BLENDER2OPENCV), pixel (j, i) looks along get_ray_directions(H, W, focal, center)[j, i], so it is
    the ray of row j * W + i of frame_rays.  depth is the Euclidean distance from the camera to the nearest triangle the pixel's ray passes through (+inf where there is
    none), tri that triangle's index (-1), bary its barycentric weights at the hit, attr the per-vertex `attributes` [V, A] (A <= 8) interpolated with them (zeros).
    One sample per pixel centre; a ray through an edge two triangles share belongs to exactly one of them; ties in depth go to the smaller index; cull drops triangles
    whose outward side (right-hand rule) faces away.  The result is a function of the arguments alone: the same bit for bit on every run and for every large_bbox (the
    box size, in pixels, above which a triangle is drawn by a workgroup instead of one lane; 0 = 64).  include/tvr.h tvr_mesh_raster has the arithmetic.
    A face index outside the vertices raises TvrError.  No CPU fallback.  `stats` (a dict) receives pixels_hit / triangles_skipped (zero area or non-finite) /
    triangles_without_pixel / triangles_large."""
    f = _faces_on_device(faces, "render_mesh")
    if not torch.is_tensor(verts) or verts.device != f.device or verts.dim() != 2 or verts.shape[1] != 3:
        raise L.TvrError(f"render_mesh takes verts [V, 3] on the faces' device ({f.device})")
    v = verts.detach().to(torch.float32).contiguous()
    V, F, dev = int(v.shape[0]), int(f.shape[0]), f.device
    cam = mesh_camera(c2w, H, W, focal, center, near, cull, large_bbox)
    a, A = None, 0
    if attributes is not None:
        if not torch.is_tensor(attributes) or attributes.device != dev or attributes.dim() != 2 or attributes.shape[0] != V:
            raise L.TvrError(f"render_mesh takes attributes [V, A] on the faces' device ({dev}), one row per vertex")
        a = attributes.detach().to(torch.float32).contiguous()
        A = int(a.shape[1])
        if A and V == 0:
            a = torch.zeros((1, A), dtype=torch.float32, device=dev)        # no vertex, no row to read: the library still wants a pointer beside n_attr > 0
    lib = L.lib()
    nbytes = lib.tvr_mesh_raster_scratch_bytes(F, cam.H, cam.W)
    if nbytes == 0:
        raise L.TvrError("render_mesh: " + lib.tvr_last_error().decode(errors="replace"))
    scratch = L.dev_bytes(nbytes, dev, what="mesh raster scratch")
    depth = L.dev_empty((cam.H, cam.W), torch.float32, dev, what="mesh raster depth")
    tri = L.dev_empty((cam.H, cam.W), torch.int32, dev, what="mesh raster tri")
    bary = L.dev_empty((cam.H, cam.W, 3), torch.float32, dev, what="mesh raster bary")
    out = L.dev_empty((cam.H, cam.W, A), torch.float32, dev, what="mesh raster attr") if A else None
    counts = L.dev_empty((4,), torch.int32, dev, what="mesh raster counts")
    flag = L.dev_bytes(4, dev, zero=True, what="mesh raster fault flag").view(torch.int32)
    L.check(lib.tvr_mesh_raster(_ptr(v), V, _ptr(f), F, C.byref(cam), _ptr(a) if A else None, A, depth.data_ptr(), L.nbytes(depth), tri.data_ptr(), L.nbytes(tri),
                                bary.data_ptr(), L.nbytes(bary), out.data_ptr() if A else None, L.nbytes(out) if A else 0, scratch.data_ptr(), L.nbytes(scratch),
                                counts.data_ptr(), flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_raster")
    if int(flag.item()) != 0:
        raise L.TvrError(f"tvr_mesh_raster raised its fault flag: a face index lies outside 0 .. {V - 1} (include/tvr.h)")
    if stats is not None:
        hit, skipped, nopix, large = (int(x) for x in counts.cpu().tolist())
        stats.update(pixels_hit=hit, triangles_skipped=skipped, triangles_without_pixel=nopix, triangles_large=large)
    return depth, tri, bary, out


def render_mesh_frame(verts, faces, transform_matrix, H: int, W: int, camera_angle_x: float, **kwargs):
    """render_mesh from one frame of a transforms_*.json, as rays.frame_rays reads it: pose = transform_matrix @ BLENDER2OPENCV, focal = focal_from_angle."""
    from . import rays as R
    pose = np.asarray(transform_matrix, dtype=np.float64) @ R.BLENDER2OPENCV
    return render_mesh(verts, faces, pose.astype(np.float32), H, W, R.focal_from_angle(float(camera_angle_x), W), **kwargs)


def face_normals(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """Unit face normals [F,3] (right-hand rule; zeros for a face without area), on the tensors' device.  Host-side helper of the flat-shaded view."""
    v, f = verts.to(torch.float32), faces.to(torch.int64)
    n = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=-1)
    return n / n.norm(dim=-1, keepdim=True).clamp_min(1e-30)


def mesh_view_to_rgb8(tri: torch.Tensor, attr, mode: str = "normal", white_bg: bool = True, face_normal=None) -> torch.Tensor:
    """uint8 [H,W,3] picture of a render_mesh result.  tri [H,W] (>= 0 where hit), attr [H,W,3] the interpolated attributes or None.

    mode "normal": attr are interpolated vertex normals; they are renormalised and coloured as evaluation.normal_map_to_rgb8 colours a unit normal (0.5 n + 0.5), with
    the hit mask in the place of acc.  mode "color": attr are vertex colours in 0 .. 255 (the PLY's uint8 values) and are shown as they are.  attr None: a flat-shaded
    view from `face_normal` [F,3] (face_normals(verts, faces)), coloured like "normal" — what a bare reference-style PLY can show.  Pixels without a hit show the
    background (white or black).  Pure; either device."""
    hit = tri >= 0
    bg = 1.0 if white_bg else 0.0
    if attr is None:
        if face_normal is None:
            raise ValueError("mesh_view_to_rgb8 without attributes takes face_normal [F, 3] (mesh.face_normals) for the flat-shaded view")
        fn = face_normal.to(torch.float32).reshape(-1, 3)
        if fn.shape[0] == 0:                                          # a mesh without faces: nothing is hit, the picture is the background
            fn = torch.zeros((1, 3), dtype=torch.float32, device=fn.device)
        n = fn[tri.clamp_min(0).to(torch.int64)]
        mode = "normal"
    else:
        if attr.shape[-1] != 3:
            raise ValueError(f"mesh_view_to_rgb8 takes three attribute channels, got {attr.shape[-1]}")
        n = attr.to(torch.float32)
    if mode == "normal":
        n = n / n.norm(dim=-1, keepdim=True).clamp_min(1e-30)
        x = 0.5 * n + 0.5
    elif mode == "color":
        x = n / 255.0
    else:
        raise ValueError(f"mode = {mode!r}: 'normal' or 'color'")
    m = hit.unsqueeze(-1)
    x = torch.where(m, x, torch.full_like(x, bg))
    return torch.round(255.0 * x.clamp(0.0, 1.0)).to(torch.uint8)


# ---- per-triangle texture atlas (csrc/tvr_mesh_texture.hip, include/tvr.h tvr_mesh_atlas_points / tvr_mesh_texture_sample) -------------------------------
ATLAS_MIN_P, ATLAS_MAX_P = 5, 64        # include/tvr.h TVR_MESH_ATLAS_MIN_P / TVR_MESH_ATLAS_MAX_P: the patch side in texels


def atlas_shape(F: int, P: int, C: int = None):
    """(Ha, Wa, C) of the atlas of F triangles at patch side P with C squares per row (default: ceil(sqrt(S)), S = ceil(F / 2) squares, so the atlas is about
    square): Wa = C * P, Ha = max(ceil(S / C), 1) * P.  P outside 5 .. 64, C < 1 or F < 0 is a ValueError."""
    import math
    F, P = int(F), int(P)
    if F < 0:
        raise ValueError(f"F = {F}: a triangle count")
    if not ATLAS_MIN_P <= P <= ATLAS_MAX_P:
        raise ValueError(f"P = {P}: the patch side in texels, {ATLAS_MIN_P} .. {ATLAS_MAX_P}")
    S = (F + 1) // 2
    C = (math.isqrt(S - 1) + 1 if S > 0 else 1) if C is None else int(C)
    if C < 1:
        raise ValueError(f"C = {C}: an atlas row holds at least one square")
    return max(-(-S // C), 1) * P, C * P, C


def atlas_points(verts: torch.Tensor, faces: torch.Tensor, P: int, C: int, texel0: int, n: int):
    """Where the texels texel0 .. texel0 + n - 1 of the atlas (linear index Y * Wa + X) lie on the mesh, on the device -> (points [n,3] float32, tri [n] int32): the
    owning triangle and the point b0 v0 + b1 v1 + b2 v2 of the texel's local coordinates (include/tvr.h tvr_mesh_atlas_points); -1 and a zero point for a texel no
    triangle owns.  A face index outside the vertices raises TvrError.  No CPU fallback."""
    f = _faces_on_device(faces, "atlas_points")
    if not torch.is_tensor(verts) or verts.device != f.device or verts.dim() != 2 or verts.shape[1] != 3:
        raise L.TvrError(f"atlas_points takes verts [V, 3] on the faces' device ({f.device})")
    v = verts.detach().to(torch.float32).contiguous()
    V, F, dev, n = int(v.shape[0]), int(f.shape[0]), f.device, int(n)
    pos = L.dev_empty((max(n, 0), 3), torch.float32, dev, what="atlas points")
    tri = L.dev_empty((max(n, 0),), torch.int32, dev, what="atlas owners")
    flag = L.dev_bytes(4, dev, zero=True, what="atlas fault flag").view(torch.int32)
    L.check(L.lib().tvr_mesh_atlas_points(_ptr(v), V, _ptr(f), F, int(P), int(C), int(texel0), n, _ptr(pos), L.nbytes(pos), _ptr(tri), L.nbytes(tri), flag.data_ptr(),
                                          _stream_ptr(dev)), "tvr_mesh_atlas_points")
    if int(flag.item()) != 0:
        raise L.TvrError(f"tvr_mesh_atlas_points raised its fault flag: a face index lies outside 0 .. {V - 1} (include/tvr.h)")
    return pos, tri


def atlas_uv(F: int, P: int, C: int = None) -> np.ndarray:
    """[F,3,2] float64 texture coordinates of every triangle corner in the atlas of atlas_shape(F, P, C): corner k of triangle t sits at the atlas texel (X, Y) of its
    local corner (0,0), (L,0), (0,L), L = P - 4; u = (X + .5) / Wa, v = 1 - (Y + .5) / Ha (image row 0 = Y = 0, the OBJ convention's top)."""
    Ha, Wa, C = atlas_shape(F, P, C)
    P, Lp = int(P), int(P) - 4
    t = np.arange(int(F), dtype=np.int64)
    s, h = t >> 1, t & 1
    X0, Y0 = (s % C) * P, (s // C) * P
    lx, ly = np.array([0, Lp, 0], dtype=np.int64), np.array([0, 0, Lp], dtype=np.int64)
    a = np.where(h[:, None] == 0, lx[None], P - 1 - lx[None])
    b = np.where(h[:, None] == 0, ly[None], P - 1 - ly[None])
    X, Y = (X0[:, None] + a).astype(np.float64), (Y0[:, None] + b).astype(np.float64)
    return np.stack(((X + 0.5) / Wa, 1.0 - (Y + 0.5) / Ha), -1)


def atlas_layout_from_uv(uv: np.ndarray, Ha: int, Wa: int):
    """(P, C) of an atlas written by write_obj, from its per-corner uv [F,3,2] and the picture's size: triangle 0's corners 0 and 1 lie L = P - 4 texels apart.
    ValueError when the coordinates are not atlas_uv's for that layout (a file this package did not write)."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 3, 2)
    F = uv.shape[0]
    if F == 0:
        if Ha != Wa or not ATLAS_MIN_P <= Ha <= ATLAS_MAX_P:
            raise ValueError(f"an atlas of {Ha} x {Wa} texels is not the one patch of a mesh without triangles")
        return int(Ha), 1
    P = int(round((uv[0, 1, 0] - uv[0, 0, 0]) * Wa)) + 4
    if not ATLAS_MIN_P <= P <= ATLAS_MAX_P or Wa % P:
        raise ValueError(f"texture coordinates that put a patch side of {P} texels into an atlas {Wa} wide: not an atlas of this package")
    C = Wa // P
    if atlas_shape(F, P, C)[:2] != (int(Ha), int(Wa)) or not np.allclose(uv, atlas_uv(F, P, C), rtol=0, atol=1e-7):
        raise ValueError(f"the texture coordinates are not those of the per-triangle atlas of {F} triangles at P = {P}, C = {C} ({Ha} x {Wa} texels)")
    return P, C


def sample_texture(tri: torch.Tensor, bary: torch.Tensor, atlas: torch.Tensor, P: int, C: int, F: int) -> torch.Tensor:
    """The atlas' colour at every hit of a render_mesh result, on the device -> [..., 3] float32 in the atlas' own units (0 .. 255 for uint8), zeros where tri < 0.
    tri [...] int32, bary [..., 3] float32, atlas [Ha, Wa, 3] uint8 or float32 of atlas_shape(F, P, C): bilinear between the four texels around (b1 * L, b2 * L) in the
    triangle's own patch (include/tvr.h tvr_mesh_texture_sample).  No CPU fallback."""
    if not (torch.is_tensor(tri) and torch.is_tensor(bary) and torch.is_tensor(atlas)) or tri.device.type != "cuda" or bary.device != tri.device or \
            atlas.device != tri.device:
        raise L.TvrError("sample_texture runs on an MI355X (HIP) device only: tri, bary and atlas are tensors on one such device. There is no CPU fallback.")
    if bary.shape != tuple(tri.shape) + (3,):
        raise L.TvrError(f"sample_texture takes tri [...] and bary [..., 3]; got {tuple(tri.shape)} and {tuple(bary.shape)}")
    if atlas.dim() != 3 or atlas.shape[2] != 3 or atlas.dtype not in (torch.uint8, torch.float32):
        raise L.TvrError(f"sample_texture takes an atlas [Ha, Wa, 3] of uint8 or float32; got {tuple(atlas.shape)} {atlas.dtype}")
    t, b, a = tri.detach().to(torch.int32).contiguous(), bary.detach().to(torch.float32).contiguous(), atlas.detach().contiguous()
    n, dev = int(t.numel()), t.device
    out = L.dev_empty(tuple(tri.shape) + (3,), torch.float32, dev, what="texture samples")
    L.check(L.lib().tvr_mesh_texture_sample(_ptr(t), _ptr(b), n, a.data_ptr(), 0 if a.dtype == torch.uint8 else 1, int(a.shape[0]), int(a.shape[1]), int(P), int(C),
                                            int(F), _ptr(out), L.nbytes(out), _stream_ptr(dev)), "tvr_mesh_texture_sample")
    return out


def write_texture_png(path, atlas) -> None:
    """The atlas [Ha, Wa, 3] uint8 (tensor on any device, or array) as a PNG, row 0 = atlas row Y = 0."""
    from PIL import Image
    a = atlas.detach().cpu().numpy() if torch.is_tensor(atlas) else np.asarray(atlas)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"a texture is uint8 [Ha, Wa, 3]; got {a.dtype} {a.shape}")
    Image.fromarray(np.ascontiguousarray(a)).save(path)


def read_texture_png(path) -> np.ndarray:
    """The picture write_texture_png wrote, uint8 [Ha, Wa, 3]."""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)              # (a copy: the array PIL exposes is read-only)


def write_obj(path, verts, faces, uv, texture_png, normals=None) -> None:
    """Wavefront OBJ of a textured mesh: `path` (x.obj) and x.mtl beside it.  verts [V,3], faces [F,3], uv [F,3,2] (atlas_uv: one `vt` per triangle corner),
    texture_png the picture's path (its base name goes into the .mtl's map_Kd: the three files travel together), normals [V,3] optional.  The .obj carries mtllib,
    usemtl, v, vt, [vn] and f a/ta[/na] (1-based); v with 9 significant digits (fp32 round-trips), vt with 10 decimals."""
    import os
    path = str(path)
    if not path.endswith(".obj"):
        raise ValueError(f"{path!r}: write_obj writes x.obj and x.mtl")
    v, f = _host(verts, np.float32), _host(faces, np.int64)
    t = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    if len(t) != 3 * len(f):
        raise ValueError(f"uv holds {len(t)} corners for {len(f)} triangles")
    nr = None if normals is None else _host(normals, np.float32)
    if nr is not None and len(nr) != len(v):
        raise ValueError(f"normals holds {len(nr)} rows for {len(v)} vertices")
    mtl = path[:-4] + ".mtl"
    with open(mtl, "w") as out:
        out.write(f"newmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {os.path.basename(str(texture_png))}\n")
    lines = [f"mtllib {os.path.basename(mtl)}", "usemtl atlas"]
    lines += ["v %.9g %.9g %.9g" % tuple(r) for r in v.tolist()]
    lines += ["vt %.10f %.10f" % tuple(r) for r in t.tolist()]
    if nr is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(r) for r in nr.tolist()]
    c = 3 * np.arange(len(f), dtype=np.int64)[:, None] + np.arange(1, 4, dtype=np.int64)[None]
    if nr is None:
        lines += ["f %d/%d %d/%d %d/%d" % (a[0], b[0], a[1], b[1], a[2], b[2]) for a, b in zip((f + 1).tolist(), c.tolist())]
    else:
        lines += ["f %d/%d/%d %d/%d/%d %d/%d/%d" % (a[0], b[0], a[0], a[1], b[1], a[1], a[2], b[2], a[2]) for a, b in zip((f + 1).tolist(), c.tolist())]
    with open(path, "w") as out:
        out.write("\n".join(lines) + "\n")


def read_obj(path):
    """Reads back what write_obj writes, and no more: (verts [V,3] float32, faces [F,3] int32, uv [F,3,2] float64, texture path) — the picture named by the .mtl's
    map_Kd, beside the .obj.  `vn` lines are skipped (a textured view needs none).  Anything else is a ValueError."""
    import os
    path = str(path)
    v, vt, fv, ft, mtllib = [], [], [], [], None
    with open(path) as src:
        for ln, line in enumerate(src, 1):
            tok = line.split()
            if not tok or tok[0] in ("vn", "usemtl"):
                continue
            try:
                if tok[0] == "v" and len(tok) == 4:
                    v.append([float(x) for x in tok[1:]])
                elif tok[0] == "vt" and len(tok) == 3:
                    vt.append([float(x) for x in tok[1:]])
                elif tok[0] == "f" and len(tok) == 4:
                    parts = [x.split("/") for x in tok[1:]]
                    fv.append([int(p[0]) - 1 for p in parts])
                    ft.append([int(p[1]) - 1 for p in parts])
                elif tok[0] == "mtllib" and len(tok) == 2:
                    mtllib = tok[1]
                else:
                    raise ValueError
            except (ValueError, IndexError):
                raise ValueError(f"{path}:{ln}: only what write_obj writes is read (mtllib, usemtl, v, vt, vn, f a/ta[/na] of triangles)") from None
    if mtllib is None:
        raise ValueError(f"{path}: no mtllib line: not a textured OBJ of write_obj")
    verts, uvs = np.asarray(v, dtype=np.float32).reshape(-1, 3), np.asarray(vt, dtype=np.float64).reshape(-1, 2)
    faces, fts = np.asarray(fv, dtype=np.int64).reshape(-1, 3), np.asarray(ft, dtype=np.int64).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= len(verts) or fts.min() < 0 or fts.max() >= len(uvs)):
        raise ValueError(f"{path}: a face names a vertex or a texture coordinate the file does not hold")
    texture = None
    with open(os.path.join(os.path.dirname(path), mtllib)) as src:
        for line in src:
            tok = line.split()
            if tok[:1] == ["map_Kd"] and len(tok) == 2:
                texture = os.path.join(os.path.dirname(path), tok[1])
    if texture is None:
        raise ValueError(f"{path}: {mtllib} names no map_Kd picture")
    return verts, faces.astype(np.int32), uvs[fts.reshape(-1)].reshape(-1, 3, 2), texture


# ---- ray queries: a linear BVH, closest / any hit, ambient occlusion (csrc/tvr_mesh_bvh.hip, include/tvr.h tvr_mesh_bvh_*) ---------------------------------
BVH_MAX_TRIANGLES = 1 << 30     # include/tvr.h TVR_MESH_BVH_MAX_TRIANGLES
BVH_MAX_DIRS = 65536            # include/tvr.h TVR_MESH_BVH_MAX_DIRS
BVH_CAST_CHUNK = 1 << 24        # rays per tvr_mesh_bvh_cast call of cast_rays (results do not depend on it)


class MeshBVH:
    """What build_bvh returns: the blob (uint8, on the device) and the mesh it was built over — verts [V,3] float32 and faces [F,3] int32 as the library reads them
    (the casts read both again, so they must not change while the hierarchy is in use).  height / triangles_skipped are the build's counts."""

    def __init__(self, blob, verts, faces, height, triangles_skipped):
        self.blob, self.verts, self.faces, self.height, self.triangles_skipped = blob, verts, faces, int(height), int(triangles_skipped)
        self.pseudonormals = None       # the MeshPseudonormals of this mesh once build_pseudonormals was asked for it (signed_distance needs it)
        self.winding = None             # the MeshWinding of this hierarchy once build_winding was asked for it (winding_number needs it)

    @property
    def n_triangles(self) -> int:
        return int(self.faces.shape[0])

    @property
    def n_vertices(self) -> int:
        return int(self.verts.shape[0])

    @property
    def device(self):
        return self.blob.device

    def layout(self) -> dict:
        """tvr_mesh_bvh_describe of this blob: byte offsets, strides and node counts (what a test reads the tree with)."""
        return bvh_layout(self.n_triangles)


def bvh_layout(n_triangles: int) -> dict:
    """tvr_mesh_bvh_describe(F) as a dict (header / boxes / children / leaf_order / total offsets, box / child / leaf strides, n_nodes, n_internal).  Host only."""
    lay = L.MeshBvhLayout()
    L.check(L.lib().tvr_mesh_bvh_describe(int(n_triangles), C.byref(lay)), "tvr_mesh_bvh_describe")
    return {n: int(getattr(lay, n)) for n, _ in L.MeshBvhLayout._fields_}


def _mesh_on_device(verts, faces, what: str):
    f = _faces_on_device(faces, what)
    if not torch.is_tensor(verts) or verts.device != f.device or verts.dim() != 2 or verts.shape[1] != 3:
        raise L.TvrError(f"{what} takes verts [V, 3] on the faces' device ({f.device})")
    return verts.detach().to(torch.float32).contiguous(), f


def build_bvh(verts: torch.Tensor, faces: torch.Tensor, stats: dict = None) -> MeshBVH:
    """A bounding-volume hierarchy over the triangles of an indexed mesh, on the device: what cast_rays and ambient_occlusion walk.

    One 64-bit key per triangle (Morton code of the centroid, triangle index) from tvr_mesh_bvh_keys, sorted with torch.sort on the device (plumbing: the keys are
    unique, every correct sort gives the same order), then tvr_mesh_bvh_build: Karras' topology from the sorted keys, exact boxes, a refit in kernel-separated passes.
    The blob is a function of (verts, faces) alone — the same bytes on every run.  A triangle with a non-finite vertex is kept out of every box and is never hit.
    A face index outside the vertices raises TvrError.  No CPU fallback.  `stats` (a dict) receives triangles_skipped / height / internal_nodes / blob_bytes."""
    v, f = _mesh_on_device(verts, faces, "build_bvh")
    V, F, dev, lib = int(v.shape[0]), int(f.shape[0]), f.device, L.lib()
    nblob, nscratch = lib.tvr_mesh_bvh_bytes(F), lib.tvr_mesh_bvh_scratch_bytes(F)
    if nblob == 0 or nscratch == 0:
        raise L.TvrError("build_bvh: " + lib.tvr_last_error().decode(errors="replace"))
    blob = L.dev_bytes(nblob, dev, what="mesh bvh blob")
    scratch = L.dev_bytes(nscratch, dev, what="mesh bvh scratch")
    keys = L.dev_empty((F,), torch.int64, dev, what="mesh bvh keys")
    counts = L.dev_empty((4,), torch.int32, dev, what="mesh bvh build counts")
    flag = L.dev_bytes(4, dev, zero=True, what="mesh bvh fault flag").view(torch.int32)
    L.check(lib.tvr_mesh_bvh_keys(_ptr(v), V, _ptr(f), F, _ptr(keys), L.nbytes(keys), scratch.data_ptr(), L.nbytes(scratch), flag.data_ptr(), _stream_ptr(dev)),
            "tvr_mesh_bvh_keys")
    ordered = torch.sort(keys)[0].contiguous()               # keys stay below 2^62: the signed order is the unsigned one
    L.check(lib.tvr_mesh_bvh_build(_ptr(v), V, _ptr(f), F, _ptr(ordered), blob.data_ptr(), L.nbytes(blob), scratch.data_ptr(), L.nbytes(scratch), counts.data_ptr(),
                                   flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_bvh_build")
    if int(flag.item()) != 0:
        raise L.TvrError(f"tvr_mesh_bvh_build raised its fault flag: a face index lies outside 0 .. {V - 1}, or the keys were not sorted (include/tvr.h)")
    skipped, height, internal, _ = (int(x) for x in counts.cpu().tolist())
    if stats is not None:
        stats.update(triangles_skipped=skipped, height=height, internal_nodes=internal, blob_bytes=int(nblob))
    return MeshBVH(blob, v, f, height, skipped)


def _bvh_arg(bvh, what: str) -> MeshBVH:
    if not isinstance(bvh, MeshBVH):
        raise L.TvrError(f"{what} takes the MeshBVH that build_bvh returns; got {type(bvh).__name__}")
    return bvh


def _rays_on_device(x, dev, what: str, name: str) -> torch.Tensor:
    if not torch.is_tensor(x) or x.device.type != "cuda":
        where = x.device if torch.is_tensor(x) else type(x).__name__
        raise L.TvrError(f"{what} runs on an MI355X (HIP) device only; {name} is on {where}. There is no CPU fallback.")
    if x.device != dev:
        raise L.TvrError(f"{what}: {name} is on {x.device}, the hierarchy on {dev}")
    return x.detach().to(torch.float32)


def cast_rays(bvh: MeshBVH, rays_or_origins, dirs=None, t_min: float = 0.0, t_max: float = float("inf"), any_hit: bool = False, cull: bool = False, stats: dict = None):
    """What rays hit on a mesh -> (t [N] float32, tri [N] int32, bary [N,3] float32), or with any_hit=True -> hit [N] uint8.

    rays_or_origins is [N,6] rows (origin, direction) as rays.py makes them, or origins [N,3] beside dirs [N,3].  A direction need not be unit length; t is parametric
    (the hit point is o + t d) and a hit needs t_min < t <= t_max.  Closest hit: the smallest t, ties to the smaller triangle index; +inf / -1 / zeros on a miss; bary
    are the hit's barycentric weights.  Any hit: 1 iff some triangle is hit (it returns at the first one found).  cull drops triangles whose outward side (right-hand
    rule) faces away from the ray.  A (ray, triangle) pair is judged by the rasteriser's expressions (include/tvr.h): a ray across an edge two triangles share belongs
    to exactly one of them; nothing is promised for a ray exactly through a vertex.  A ray with a non-finite component or a zero direction never hits.  Results do not
    depend on the order or batching of the rays.  No CPU fallback.  `stats` (a dict) receives rays_hit / rays_refused / node_tests / triangle_tests."""
    b = _bvh_arg(bvh, "cast_rays")
    dev = b.device
    r = _rays_on_device(rays_or_origins, dev, "cast_rays", "rays_or_origins")
    if dirs is None:
        if r.dim() != 2 or r.shape[1] != 6:
            raise L.TvrError(f"cast_rays takes rays [N, 6], or origins [N, 3] and dirs [N, 3]; got {tuple(r.shape)} and no dirs")
        o, d = r[:, :3].contiguous(), r[:, 3:].contiguous()
    else:
        d = _rays_on_device(dirs, dev, "cast_rays", "dirs")
        if r.dim() != 2 or r.shape[1] != 3 or d.shape != r.shape:
            raise L.TvrError(f"cast_rays takes rays [N, 6], or origins [N, 3] and dirs [N, 3]; got {tuple(r.shape)} and {tuple(d.shape)}")
        o, d = r.contiguous(), d.contiguous()
    N, lib = int(o.shape[0]), L.lib()
    hit = L.dev_empty((N,), torch.uint8, dev, what="mesh bvh hit") if any_hit else None
    t = None if any_hit else L.dev_empty((N,), torch.float32, dev, what="mesh bvh t")
    tri = None if any_hit else L.dev_empty((N,), torch.int32, dev, what="mesh bvh tri")
    bary = None if any_hit else L.dev_empty((N, 3), torch.float32, dev, what="mesh bvh bary")
    counts = L.dev_empty((4,), torch.int64, dev, what="mesh bvh cast counts")
    total = torch.zeros(4, dtype=torch.int64, device=dev)
    flag = L.dev_bytes(4, dev, zero=True, what="mesh bvh fault flag").view(torch.int32)
    for i0 in range(0, max(N, 1), BVH_CAST_CHUNK):
        n = min(BVH_CAST_CHUNK, N - i0)
        oc, dc = o[i0:i0 + n], d[i0:i0 + n]
        outs = []                                                    # (pointer, bytes) of this chunk's rows of t, tri, bary, hit; (NULL, 0) for the other mode's
        for x in (t, tri, bary, hit):
            rows = None if x is None else x[i0:i0 + n]
            outs += [None, 0] if rows is None else [_ptr(rows), L.nbytes(rows)]
        L.check(lib.tvr_mesh_bvh_cast(_ptr(b.verts), b.n_vertices, _ptr(b.faces), b.n_triangles, b.blob.data_ptr(), L.nbytes(b.blob), _ptr(oc), _ptr(dc), n, float(t_min),
                                      float(t_max), 1 if any_hit else 0, 1 if cull else 0, *outs, counts.data_ptr(), flag.data_ptr(), _stream_ptr(dev)),
                "tvr_mesh_bvh_cast")
        total += counts
    if int(flag.item()) != 0:
        raise L.TvrError("tvr_mesh_bvh_cast raised its fault flag: the blob does not belong to this mesh, or a face index lies outside the vertices (include/tvr.h)")
    if stats is not None:
        h, r_, nt, tt = (int(x) for x in total.cpu().tolist())
        stats.update(rays_hit=h, rays_refused=r_, node_tests=nt, triangle_tests=tt)
    return hit if any_hit else (t, tri, bary)


def fibonacci_sphere(K: int) -> torch.Tensor:
    """The default direction table of ambient_occlusion: K unit vectors spread over the sphere, float32 [K,3] on the host, computed in float64:
    z_k = 1 - (2k + 1) / K, azimuth 2 pi frac(k * 0.6180339887498949), (x, y) = sqrt(1 - z^2) (cos, sin)."""
    K = int(K)
    if K < 1 or K > BVH_MAX_DIRS:
        raise ValueError(f"fibonacci_sphere takes 1 .. {BVH_MAX_DIRS} directions; got {K}")
    k = np.arange(K, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / K
    phi = 2.0 * np.pi * np.modf(k * 0.6180339887498949)[0]
    s = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    return torch.from_numpy(np.stack((s * np.cos(phi), s * np.sin(phi), z), -1).astype(np.float32))


def ambient_occlusion(bvh: MeshBVH, normals, n_dirs: int = 64, bias: float = 1e-3, t_max: float = float("inf"), points=None, dirs=None, stats: dict = None) -> torch.Tensor:
    """Cosine-weighted openness in [0, 1] of points on a mesh -> [M] float32 on the device: 1 = nothing in sight, 0 = every direction blocked.

    points [M,3] (default: the mesh's vertices) with normals [M,3]; dirs [K,3] a direction table (default: fibonacci_sphere(n_dirs)).  Per point and table entry the
    direction is flipped into the normal's hemisphere, weighted by its cosine w = d . n, and an any-hit ray runs from p + bias n over (0, t_max];
    the result is sum(w * visible) / sum(w), summed in table order (include/tvr.h tvr_mesh_bvh_occlusion), 1 where the normal is zero or non-finite.  bias is in the
    mesh's units (the default suits a mesh of unit size).  Two runs give the same bits.  No CPU fallback.  `stats` as for cast_rays, per ray."""
    b = _bvh_arg(bvh, "ambient_occlusion")
    dev = b.device
    n = _rays_on_device(normals, dev, "ambient_occlusion", "normals").contiguous()
    p = b.verts if points is None else _rays_on_device(points, dev, "ambient_occlusion", "points").contiguous()
    if p.dim() != 2 or p.shape[1] != 3 or n.shape != p.shape:
        raise L.TvrError(f"ambient_occlusion takes points [M, 3] and normals [M, 3]; got {tuple(p.shape)} and {tuple(n.shape)}")
    table = fibonacci_sphere(n_dirs) if dirs is None else dirs
    if not torch.is_tensor(table) or table.dim() != 2 or table.shape[1] != 3:
        raise L.TvrError("ambient_occlusion takes dirs [K, 3]")
    table = table.detach().to(device=dev, dtype=torch.float32).contiguous()
    M, K = int(p.shape[0]), int(table.shape[0])
    out = L.dev_empty((M,), torch.float32, dev, what="mesh bvh occlusion")
    counts = L.dev_empty((4,), torch.int64, dev, what="mesh bvh occlusion counts")
    flag = L.dev_bytes(4, dev, zero=True, what="mesh bvh fault flag").view(torch.int32)
    L.check(L.lib().tvr_mesh_bvh_occlusion(_ptr(b.verts), b.n_vertices, _ptr(b.faces), b.n_triangles, b.blob.data_ptr(), L.nbytes(b.blob), _ptr(p), _ptr(n), M, _ptr(table),
                                           K, float(bias), float(t_max), _ptr(out), L.nbytes(out), counts.data_ptr(), flag.data_ptr(), _stream_ptr(dev)),
            "tvr_mesh_bvh_occlusion")
    if int(flag.item()) != 0:
        raise L.TvrError("tvr_mesh_bvh_occlusion raised its fault flag: the blob does not belong to this mesh, or a face index lies outside the vertices (include/tvr.h)")
    if stats is not None:
        h, r_, nt, tt = (int(x) for x in counts.cpu().tolist())
        stats.update(rays_hit=h, rays_refused=r_, node_tests=nt, triangle_tests=tt)
    return out


# ---- closest points and the distance between two meshes (csrc/tvr_mesh_bvh.hip bv_nearest_kernel, include/tvr.h tvr_mesh_bvh_nearest) -----------------------
BVH_NEAREST_CHUNK = 1 << 24     # points per tvr_mesh_bvh_nearest call of closest_points (results do not depend on it)


def closest_points(bvh: MeshBVH, points, max_dist: float = float("inf"), stats: dict = None):
    """The closest point of a mesh to every point -> (dist [N] float32, tri [N] int32, bary [N,3] float32) on the device.

    points [N,3] on the hierarchy's device.  dist is the distance to the nearest point of the surface, tri the triangle it lies on (ties in distance go to the smaller
    index) and bary its weights there: the closest point is sum_k bary_k * v_k of that triangle.  A point farther than max_dist from every triangle, a point with a
    non-finite component and every point of an empty mesh get +inf / -1 / zeros.  A point that is a vertex of the mesh gets exactly 0.0 and the smallest triangle index
    of the vertex's fan.  The distance is unsigned.  The pair arithmetic is defined in include/tvr.h (Ericson's regions in the frame translated to the point);
    results do not depend on the order or batching of the points and two runs give the same bits.  No CPU fallback.  `stats` (a dict) receives points_answered /
    points_refused / node_tests / triangle_tests."""
    b = _bvh_arg(bvh, "closest_points")
    dev = b.device
    p = _rays_on_device(points, dev, "closest_points", "points")
    if p.dim() != 2 or p.shape[1] != 3:
        raise L.TvrError(f"closest_points takes points [N, 3]; got {tuple(p.shape)}")
    max_dist = float(max_dist)
    if not max_dist >= 0.0:
        raise L.TvrError(f"closest_points: max_dist = {max_dist} must be >= 0 (+inf = no limit)")
    p = p.contiguous()
    N, lib = int(p.shape[0]), L.lib()
    dist = L.dev_empty((N,), torch.float32, dev, what="mesh bvh nearest dist")
    tri = L.dev_empty((N,), torch.int32, dev, what="mesh bvh nearest tri")
    bary = L.dev_empty((N, 3), torch.float32, dev, what="mesh bvh nearest bary")
    counts = L.dev_empty((4,), torch.int64, dev, what="mesh bvh nearest counts")
    total = torch.zeros(4, dtype=torch.int64, device=dev)
    flag = L.dev_bytes(4, dev, zero=True, what="mesh bvh fault flag").view(torch.int32)
    for i0 in range(0, max(N, 1), BVH_NEAREST_CHUNK):
        n = min(BVH_NEAREST_CHUNK, N - i0)
        pc, dc, tc, bc = p[i0:i0 + n], dist[i0:i0 + n], tri[i0:i0 + n], bary[i0:i0 + n]
        L.check(lib.tvr_mesh_bvh_nearest(_ptr(b.verts), b.n_vertices, _ptr(b.faces), b.n_triangles, b.blob.data_ptr(), L.nbytes(b.blob), _ptr(pc), n, max_dist, _ptr(dc),
                                         L.nbytes(dc), _ptr(tc), L.nbytes(tc), _ptr(bc), L.nbytes(bc), counts.data_ptr(), flag.data_ptr(), _stream_ptr(dev)),
                "tvr_mesh_bvh_nearest")
        total += counts
    if int(flag.item()) != 0:
        raise L.TvrError("tvr_mesh_bvh_nearest raised its fault flag: the blob does not belong to this mesh, or a face index lies outside the vertices (include/tvr.h)")
    if stats is not None:
        a, r_, nt, tt = (int(x) for x in total.cpu().tolist())
        stats.update(points_answered=a, points_refused=r_, node_tests=nt, triangle_tests=tt)
    return dist, tri, bary


def subdivision_weights(subdiv: int) -> np.ndarray:
    """The barycentric weights [n^2, 3] (float64) of the centroids of the n^2 sub-triangles of a triangle's regular n-fold subdivision: first the n (n + 1) / 2 upright
    ones, rows j = 0 .. n-1 and i = 0 .. n-1-j within a row, at (v, w) = ((3 i + 1) / (3 n), (3 j + 1) / (3 n)); then the n (n - 1) / 2 inverted ones in the same order
    at ((3 i + 2) / (3 n), (3 j + 2) / (3 n)).  Column 0 is 1 - v - w."""
    n = int(subdiv)
    if n < 1 or n > 64:
        raise ValueError(f"subdiv = {subdiv!r}: the subdivisions per edge, an integer in 1 .. 64")
    up = [((3 * i + 1) / (3.0 * n), (3 * j + 1) / (3.0 * n)) for j in range(n) for i in range(n - j)]
    down = [((3 * i + 2) / (3.0 * n), (3 * j + 2) / (3.0 * n)) for j in range(n - 1) for i in range(n - 1 - j)]
    vw = np.asarray(up + down, np.float64).reshape(-1, 2)
    return np.concatenate([1.0 - vw.sum(1, keepdims=True), vw], 1)


def surface_samples(verts: torch.Tensor, faces: torch.Tensor, subdiv: int = 2):
    """Points spread over a mesh with the area each stands for -> (points [F n^2 + V, 3] float32, weights [F n^2 + V] float32), on the mesh's device (torch plumbing).

    Per triangle, in face order, the centroids of the n^2 sub-triangles of its regular n-fold subdivision (n = subdiv, subdivision_weights' order), each weighted
    area / n^2; then the V vertices with weight 0 — they count for a maximum only.  A zero-area triangle, and one with a non-finite vertex, has weight 0.  The output
    is a function of its arguments alone."""
    if not torch.is_tensor(verts) or not torch.is_tensor(faces) or verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("surface_samples takes verts [V, 3] and faces [F, 3] tensors")
    if faces.device != verts.device:
        raise ValueError(f"surface_samples: the faces are on {faces.device}, the vertices on {verts.device}")
    bw = torch.from_numpy(subdivision_weights(subdiv).astype(np.float32)).to(verts.device)           # [n^2, 3]
    v = verts.detach().to(torch.float32)
    corners = v[faces.detach().long()]                                                               # [F, 3, 3]
    pts = (bw[None, :, 0, None] * corners[:, None, 0] + bw[None, :, 1, None] * corners[:, None, 1]) + bw[None, :, 2, None] * corners[:, None, 2]
    area = 0.5 * torch.linalg.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0], dim=-1).norm(dim=-1)
    area = torch.where(torch.isfinite(area), area, torch.zeros_like(area)) / float(bw.shape[0])
    weights = torch.cat([area[:, None].expand(-1, bw.shape[0]).reshape(-1), torch.zeros(v.shape[0], dtype=torch.float32, device=v.device)])
    return torch.cat([pts.reshape(-1, 3), v]).contiguous(), weights.contiguous()


def weighted_quantile(dist: torch.Tensor, weights: torch.Tensor, q) -> torch.Tensor:
    """The smallest distance whose cumulative weight, after a sort by distance, reaches q x the total weight -> one value per entry of q (float64, on dist's device;
    NaN when the total weight is 0).  Samples of weight 0 never decide a quantile."""
    d, order = torch.sort(dist.to(torch.float64))
    cum = torch.cumsum(weights.to(torch.float64)[order], 0)
    if d.numel() == 0:
        return torch.full((len(q),), float("nan"), dtype=torch.float64, device=dist.device)
    target = torch.as_tensor(list(q), dtype=torch.float64, device=dist.device) * cum[-1]
    idx = torch.searchsorted(cum, target).clamp(max=d.numel() - 1)                                  # the first index whose cumulative weight is >= the target
    return torch.where(cum[-1] > 0, d[idx], torch.full_like(target, float("nan")))


DISTANCE_STATISTICS = ("max", "mean", "rms", "median", "p95", "samples", "refused")


def distance_statistics(dist: torch.Tensor, weights: torch.Tensor, unit: float = 1.0) -> torch.Tensor:
    """DISTANCE_STATISTICS of one direction of mesh_distance -> [7] float64 on dist's device, no host read: dist / unit over the samples that were answered (finite
    dist); mean and rms weighted by `weights`, median and p95 by weighted_quantile; samples = all, refused = those without an answer."""
    ok = torch.isfinite(dist)                                        # (masked, not gathered: a boolean gather would read the count back)
    d = torch.where(ok, dist.to(torch.float64) / float(unit), torch.zeros((), dtype=torch.float64, device=dist.device))
    w = torch.where(ok, weights.to(torch.float64), torch.zeros((), dtype=torch.float64, device=dist.device))
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dist.device)
    total = w.sum()
    mx = torch.where(ok.any(), torch.where(ok, d, -torch.ones_like(d)).max(), nan) if d.numel() else nan
    mean = torch.where(total > 0, (w * d).sum() / total, nan)
    rms = torch.where(total > 0, torch.sqrt((w * d * d).sum() / total), nan)
    qs = weighted_quantile(d, w, (0.5, 0.95))
    n = torch.tensor([float(dist.numel())], dtype=torch.float64, device=dist.device)
    return torch.cat([torch.stack([mx, mean, rms, qs[0], qs[1]]), n, n - ok.sum().to(torch.float64)])


def mesh_distance(verts_a, faces_a, verts_b, faces_b, subdiv: int = 2, symmetric: bool = True, unit: float = 1.0, bvh_a: MeshBVH = None, bvh_b: MeshBVH = None,
                  stats: dict = None) -> dict:
    """How far two meshes are apart -> {"a_to_b": {max, mean, rms, median, p95, samples, refused}, and with symmetric also "b_to_a", "hausdorff", "chamfer"}.

    a_to_b: the distances, divided by `unit`, from surface_samples(A, subdiv) to the surface of B (closest_points on B's hierarchy).  mean and rms are weighted by
    area; median and p95 are the smallest distance whose cumulative area, after a sort by distance, reaches 0.5 and 0.95 of the total; max is over the samples and the
    vertices; samples counts the queries, refused those that got no answer (non-finite coordinates, or an empty B) and are left out of the figures.  hausdorff is the
    larger of the two max, chamfer the mean of the two mean.  Distances are unsigned and one-sided figures are not symmetric: a hole in B does not show in a_to_b.
    bvh_a / bvh_b: hierarchies built over exactly these meshes (build_bvh), built here when absent (bvh_a is only needed with symmetric).  The statistics are computed
    on the device and read once.  No CPU fallback.  `stats` (a dict) receives closest_points' counters summed over the directions.
    signed_mesh_distance adds the direction of the difference."""
    return _mesh_distance(verts_a, faces_a, verts_b, faces_b, subdiv, symmetric, unit, bvh_a, bvh_b, stats, False)


def signed_mesh_distance(verts_a, faces_a, verts_b, faces_b, subdiv: int = 2, symmetric: bool = True, unit: float = 1.0, bvh_a: MeshBVH = None, bvh_b: MeshBVH = None,
                         stats: dict = None) -> dict:
    """mesh_distance, and in which direction the meshes differ -> mesh_distance's dict (the same figures: the queries are signed_distance's, and |sdist| is
    closest_points' dist bit for bit) in which every direction also carries SIGNED_STATISTICS — signed_mean, the area-weighted mean of the signed distance / unit
    (positive: A lies outside B), and inside_fraction, the area-weighted share of A's samples inside B.  A direction whose target is not closed (build_pseudonormals)
    carries None for both and "signed_reason" says why; the unsigned figures are reported all the same.  `stats` (a dict) receives signed_distance's counters summed
    over the directions and "closedness": per direction the target's counters.  No CPU fallback."""
    return _mesh_distance(verts_a, faces_a, verts_b, faces_b, subdiv, symmetric, unit, bvh_a, bvh_b, stats, True)


def _mesh_distance(verts_a, faces_a, verts_b, faces_b, subdiv, symmetric, unit, bvh_a, bvh_b, stats, signed) -> dict:
    unit = float(unit)
    if not unit > 0.0 or not np.isfinite(unit):
        raise ValueError(f"mesh_distance: unit = {unit} must be positive and finite")
    va, fa = _mesh_on_device(verts_a, faces_a, "mesh_distance")
    vb, fb = _mesh_on_device(verts_b, faces_b, "mesh_distance")
    if va.device != vb.device:
        raise L.TvrError(f"mesh_distance: mesh A is on {va.device}, mesh B on {vb.device}")
    sides = [("a_to_b", va, fa, _bvh_arg(bvh_b, "mesh_distance") if bvh_b is not None else build_bvh(vb, fb))]
    if symmetric:
        sides.append(("b_to_a", vb, fb, _bvh_arg(bvh_a, "mesh_distance") if bvh_a is not None else build_bvh(va, fa)))
    rows, counters, closedness = [], {}, {}
    for name, v, f, target in sides:
        pts, w = surface_samples(v, f, subdiv)
        st = {}
        if signed:
            closedness[name] = {}
            build_pseudonormals(target, stats=closedness[name])
            sd = signed_distance(target, pts, strict=False, stats=st)[0]
            rows.append(torch.cat([distance_statistics(sd.abs(), w, unit), signed_statistics(sd, w, unit)]))
        else:
            rows.append(distance_statistics(closest_points(target, pts, stats=st)[0], w, unit))
        for k, x in st.items():
            counters[k] = counters.get(k, 0) + x
    host = torch.stack(rows).cpu().tolist()                          # the one host read of the figures
    out = {}
    for (name, _, _, _), row in zip(sides, host):
        out[name] = {k: (int(x) if k in ("samples", "refused") else float(x)) for k, x in zip(DISTANCE_STATISTICS, row)}
        if signed:
            closed = closedness[name]["closed"]
            out[name].update({k: (float(x) if closed else None) for k, x in zip(SIGNED_STATISTICS, row[len(DISTANCE_STATISTICS):])})
            if not closed:
                out[name]["signed_reason"] = "the target mesh is not closed: " + _closedness_text(closedness[name])
    if signed:
        counters["closedness"] = closedness
    if symmetric:
        out["hausdorff"] = max(out["a_to_b"]["max"], out["b_to_a"]["max"])
        out["chamfer"] = 0.5 * (out["a_to_b"]["mean"] + out["b_to_a"]["mean"])
    if stats is not None:
        stats.update(counters)
    return out


# ---- signed distance: pseudo-normals and an inside test (csrc/tvr_mesh_pseudo.hip, csrc/tvr_mesh_bvh.hip bv_signed_kernel; include/tvr.h tvr_mesh_pseudonormals_* /
# tvr_mesh_bvh_signed) ------------------------------------------------------------------------------------------------------------------------------------------
BVH_SIGNED_CHUNK = 1 << 24      # points per tvr_mesh_bvh_signed call of signed_distance (results do not depend on it)
CLOSEDNESS_COUNTERS = ("degenerate_faces", "open_edges", "nonmanifold_edges", "inconsistent_edges")
SIGNED_STATISTICS = ("signed_mean", "inside_fraction")
FEATURES = ("vertex A", "vertex B", "edge AB", "vertex C", "edge AC", "edge BC", "face")      # what signed_distance's `feature` 0 .. 6 names


class MeshPseudonormals:
    """What build_pseudonormals keeps on a MeshBVH: the table (uint8 blob on the device: face_n, edge_n, vert_n; pseudonormals_layout) and the mesh's closedness counters."""

    def __init__(self, blob, counters: dict):
        self.blob, self.counters = blob, dict(counters)

    @property
    def closed(self) -> bool:
        return all(self.counters[k] == 0 for k in CLOSEDNESS_COUNTERS)


def pseudonormals_layout(n_vertices: int, n_triangles: int) -> dict:
    """tvr_mesh_pseudonormals_describe(V, F) as a dict (header / face_n / edge_n / vert_n / total offsets, face / edge / vert strides).  Host only."""
    lay = L.MeshPseudonormalsLayout()
    L.check(L.lib().tvr_mesh_pseudonormals_describe(int(n_vertices), int(n_triangles), C.byref(lay)), "tvr_mesh_pseudonormals_describe")
    return {n: int(getattr(lay, n)) for n, _ in L.MeshPseudonormalsLayout._fields_}


def _closedness_text(counters: dict) -> str:
    return ", ".join(f"{k} = {counters[k]}" for k in CLOSEDNESS_COUNTERS)


def build_pseudonormals(bvh: MeshBVH, stats: dict = None) -> MeshPseudonormals:
    """The pseudo-normal table of a hierarchy's mesh, built once and kept as bvh.pseudonormals: per face its unit normal, per edge the sum of the normals of the faces
    on it, per vertex the angle-weighted sum over its fan (Baerentzen & Aanaes) — the normals whose product with (point - closest point) has the sign of outside /
    inside on a closed mesh, at edges and vertices too, where a face normal fails.

    Two arrays of 64-bit keys from tvr_mesh_pseudonormals_keys (corner by vertex, half-edge by undirected edge) are sorted with torch.sort on the device (plumbing;
    the second stably), then tvr_mesh_pseudonormals_build checks them and forms every sum in ascending face order in one thread: no float atomics, the same bytes on
    every run.  `stats` (a dict) receives degenerate_faces / open_edges / nonmanifold_edges / inconsistent_edges, closed (all four are 0) and table_bytes.  No CPU
    fallback."""
    b = _bvh_arg(bvh, "build_pseudonormals")
    if b.pseudonormals is None:
        V, F, dev, lib = b.n_vertices, b.n_triangles, b.device, L.lib()
        nblob, nscratch = lib.tvr_mesh_pseudonormals_bytes(V, F), lib.tvr_mesh_pseudonormals_scratch_bytes(F)
        if nblob == 0 or nscratch == 0:
            raise L.TvrError("build_pseudonormals: " + lib.tvr_last_error().decode(errors="replace"))
        blob = L.dev_bytes(nblob, dev, what="mesh pseudonormals blob")
        scratch = L.dev_bytes(nscratch, dev, what="mesh pseudonormals scratch")
        ck = L.dev_empty((3 * F,), torch.int64, dev, what="mesh pseudonormals corner keys")
        ek = L.dev_empty((3 * F,), torch.int64, dev, what="mesh pseudonormals edge keys")
        counts = L.dev_empty((4,), torch.int32, dev, what="mesh pseudonormals counts")
        flag = L.dev_bytes(4, dev, zero=True, what="mesh pseudonormals fault flag").view(torch.int32)
        L.check(lib.tvr_mesh_pseudonormals_keys(_ptr(b.faces), V, F, _ptr(ck), _ptr(ek), L.nbytes(ck), flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_pseudonormals_keys")
        cks = torch.sort(ck)[0].contiguous()                         # keys stay below 2^63: the signed order is the unsigned one
        eks, order = torch.sort(ek, stable=True)
        eks, order = eks.contiguous(), order.contiguous()
        L.check(lib.tvr_mesh_pseudonormals_build(_ptr(b.verts), V, _ptr(b.faces), F, _ptr(cks), _ptr(eks), _ptr(order), blob.data_ptr(), L.nbytes(blob), scratch.data_ptr(),
                                                 L.nbytes(scratch), counts.data_ptr(), flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_pseudonormals_build")
        if int(flag.item()) != 0:
            raise L.TvrError(f"tvr_mesh_pseudonormals_build raised its fault flag: a face index lies outside 0 .. {V - 1}, or the keys were not sorted (include/tvr.h)")
        b.pseudonormals = MeshPseudonormals(blob, dict(zip(CLOSEDNESS_COUNTERS, (int(x) for x in counts.cpu().tolist()))))
    if stats is not None:
        stats.update(b.pseudonormals.counters, closed=b.pseudonormals.closed, table_bytes=int(b.pseudonormals.blob.numel()))
    return b.pseudonormals


def _signed_table(b: MeshBVH, strict: bool, what: str) -> MeshPseudonormals:
    table = build_pseudonormals(b)
    if strict and not table.closed:
        raise L.TvrError(f"{what}: the mesh is not closed ({_closedness_text(table.counters)}), so inside and outside are not defined; strict=False answers anyway, "
                         f"without a promise about the signs")
    return table


def _signed_stats(stats, total):
    if stats is not None:
        a, r_, nt, tt, u = (int(x) for x in total.cpu().tolist())
        stats.update(points_answered=a, points_refused=r_, node_tests=nt, triangle_tests=tt, points_undecided=u)


_SIGNED_FAULT = ("tvr_mesh_bvh_signed raised its fault flag: the hierarchy or the pseudo-normal table does not belong to this mesh, or a face index lies outside the "
                 "vertices (include/tvr.h)")


def signed_distance(bvh: MeshBVH, points, max_dist: float = float("inf"), strict: bool = True, stats: dict = None):
    """The signed distance of every point to a closed mesh -> (sdist [N] float32, tri [N] int32, bary [N,3] float32, feature [N] int8) on the device.

    |sdist|, tri and bary are closest_points' answers, bit for bit; sdist is negative inside the mesh (the side the right-hand-rule normals point away from), +0.0 on
    it, +inf where closest_points gives +inf.  feature says what the closest point lies on: FEATURES[feature] of triangle tri, -1 without an answer.  The sign is that
    of N . (p - closest) with N the pseudo-normal of that feature (build_pseudonormals, built here when absent).  strict: a mesh that is not closed raises TvrError
    naming the counters; strict=False answers anyway and the signs are then not promised.  A point whose sign the normal cannot decide (N . (p - closest) == 0 off the
    surface, or a zero normal) is reported as +dist and counted.  Results do not depend on the order or batching of the points.  No CPU fallback.  `stats` (a dict)
    receives points_answered / points_refused / node_tests / triangle_tests / points_undecided."""
    b = _bvh_arg(bvh, "signed_distance")
    dev = b.device
    p = _rays_on_device(points, dev, "signed_distance", "points")
    if p.dim() != 2 or p.shape[1] != 3:
        raise L.TvrError(f"signed_distance takes points [N, 3]; got {tuple(p.shape)}")
    max_dist = float(max_dist)
    if not max_dist >= 0.0:
        raise L.TvrError(f"signed_distance: max_dist = {max_dist} must be >= 0 (+inf = no limit)")
    table = _signed_table(b, strict, "signed_distance")
    p = p.contiguous()
    N, lib = int(p.shape[0]), L.lib()
    sdist = L.dev_empty((N,), torch.float32, dev, what="mesh bvh signed sdist")
    tri = L.dev_empty((N,), torch.int32, dev, what="mesh bvh signed tri")
    bary = L.dev_empty((N, 3), torch.float32, dev, what="mesh bvh signed bary")
    feature = L.dev_empty((N,), torch.int8, dev, what="mesh bvh signed feature")
    counts = L.dev_empty((5,), torch.int64, dev, what="mesh bvh signed counts")
    total = torch.zeros(5, dtype=torch.int64, device=dev)
    flag = L.dev_bytes(4, dev, zero=True, what="mesh bvh fault flag").view(torch.int32)
    for i0 in range(0, max(N, 1), BVH_SIGNED_CHUNK):
        n = min(BVH_SIGNED_CHUNK, N - i0)
        pc, sc, tc, bc, fc = p[i0:i0 + n], sdist[i0:i0 + n], tri[i0:i0 + n], bary[i0:i0 + n], feature[i0:i0 + n]
        L.check(lib.tvr_mesh_bvh_signed(_ptr(b.verts), b.n_vertices, _ptr(b.faces), b.n_triangles, b.blob.data_ptr(), L.nbytes(b.blob), table.blob.data_ptr(),
                                        L.nbytes(table.blob), _ptr(pc), n, None, max_dist, _ptr(sc), L.nbytes(sc), _ptr(tc), L.nbytes(tc), _ptr(bc), L.nbytes(bc), _ptr(fc),
                                        L.nbytes(fc), counts.data_ptr(), flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_bvh_signed")
        total += counts
    if int(flag.item()) != 0:
        raise L.TvrError(_SIGNED_FAULT)
    _signed_stats(stats, total)
    return sdist, tri, bary, feature


def contains(bvh: MeshBVH, points, strict: bool = True) -> torch.Tensor:
    """Which points lie inside a closed mesh -> [N] bool on the device: signed_distance(bvh, points, strict=strict) < 0.  A point on the surface is not inside."""
    return signed_distance(bvh, points, strict=strict)[0] < 0


def signed_distance_grid(bvh: MeshBVH, dims, origin=(0, 0, 0), spacing=(1, 1, 1), max_dist: float = float("inf"), strict: bool = True, stats: dict = None) -> torch.Tensor:
    """The signed distance field of a closed mesh on a lattice -> volume [nx, ny, nz] float32 on the device, laid out as marching_cubes reads its volume.

    Grid point (i, j, k) sits at origin + (i, j, k) * spacing, formed in the kernel in fp32 (one product, one sum per axis): no point tensor is materialised, and the
    values are bit-equal to signed_distance on the same points.  marching_cubes(-volume, 0.0, spacing, origin) (a grid point is inside iff value >= level) extracts the
    mesh's surface again.  dims [3] with at most 2^31 - 1 grid points.  strict, max_dist, `stats` as for signed_distance.  No CPU fallback."""
    b = _bvh_arg(bvh, "signed_distance_grid")
    dev = b.device
    dims = [int(x) for x in dims]
    if len(dims) != 3 or min(dims) < 0 or dims[0] * dims[1] * dims[2] > 2 ** 31 - 1:
        raise L.TvrError(f"signed_distance_grid takes dims [3] of non-negative sizes with at most 2^31 - 1 grid points; got {dims}")
    max_dist = float(max_dist)
    if not max_dist >= 0.0:
        raise L.TvrError(f"signed_distance_grid: max_dist = {max_dist} must be >= 0 (+inf = no limit)")
    table = _signed_table(b, strict, "signed_distance_grid")
    lat = L.MeshLattice()
    lat.origin[:], lat.spacing[:], lat.dims[:] = [float(x) for x in origin], [float(x) for x in spacing], dims
    vol = L.dev_empty(tuple(dims), torch.float32, dev, what="mesh bvh signed volume")
    counts = L.dev_empty((5,), torch.int64, dev, what="mesh bvh signed counts")
    flag = L.dev_bytes(4, dev, zero=True, what="mesh bvh fault flag").view(torch.int32)
    L.check(L.lib().tvr_mesh_bvh_signed(_ptr(b.verts), b.n_vertices, _ptr(b.faces), b.n_triangles, b.blob.data_ptr(), L.nbytes(b.blob), table.blob.data_ptr(),
                                        L.nbytes(table.blob), None, 0, C.byref(lat), max_dist, _ptr(vol), L.nbytes(vol), None, 0, None, 0, None, 0, counts.data_ptr(),
                                        flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_bvh_signed")
    if int(flag.item()) != 0:
        raise L.TvrError(_SIGNED_FAULT)
    _signed_stats(stats, counts)
    return vol


def signed_statistics(sdist: torch.Tensor, weights: torch.Tensor, unit: float = 1.0) -> torch.Tensor:
    """SIGNED_STATISTICS of one direction of signed_mesh_distance -> [2] float64 on sdist's device, no host read: over the samples that were answered (finite
    sdist), weighted by `weights`, the mean of sdist / unit and the share of the weight whose sdist is negative; NaN when the total weight is 0."""
    ok = torch.isfinite(sdist)
    zero = torch.zeros((), dtype=torch.float64, device=sdist.device)
    d = torch.where(ok, sdist.to(torch.float64) / float(unit), zero)
    w = torch.where(ok, weights.to(torch.float64), zero)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=sdist.device)
    total = w.sum()
    return torch.stack([torch.where(total > 0, (w * d).sum() / total, nan), torch.where(total > 0, (w * (d < 0).to(torch.float64)).sum() / total, nan)])


# ---- winding numbers: inside / outside for any soup, and a watertight remesh (csrc/tvr_mesh_winding.hip; include/tvr.h tvr_mesh_winding_*) -------------------
BVH_WINDING_CHUNK = 1 << 24     # points per tvr_mesh_winding_query call of winding_number (results do not depend on it)
WINDING_COUNTS = ("points_answered", "points_refused", "node_visits", "dipole_terms", "triangle_terms")


class MeshWinding:
    """What build_winding keeps on a MeshBVH: the table of node moments (uint8 blob on the device; winding_layout)."""

    def __init__(self, blob):
        self.blob = blob


def winding_layout(n_triangles: int) -> dict:
    """tvr_mesh_winding_describe(F) as a dict (header / rows / total offsets, row_stride, n_rows).  Host only."""
    lay = L.MeshWindingLayout()
    L.check(L.lib().tvr_mesh_winding_describe(int(n_triangles), C.byref(lay)), "tvr_mesh_winding_describe")
    return {n: int(getattr(lay, n)) for n, _ in L.MeshWindingLayout._fields_}


def build_winding(bvh: MeshBVH, stats: dict = None) -> MeshWinding:
    """The table of node moments of a hierarchy, built once and kept as bvh.winding: per internal node the summed area vector of the triangles below it, their
    area-weighted centroid, the radius about it that holds the node's box, and the summed area — what lets winding_number replace a far subtree by one dipole.

    The sums are formed bottom-up, (left child) + (right child), in kernel-separated passes as the hierarchy's boxes are: no float atomics, the same bytes on every
    run.  `stats` (a dict) receives internal_nodes and table_bytes.  No CPU fallback."""
    b = _bvh_arg(bvh, "build_winding")
    if b.winding is None:
        V, F, dev, lib = b.n_vertices, b.n_triangles, b.device, L.lib()
        nblob, nscratch = lib.tvr_mesh_winding_bytes(F), lib.tvr_mesh_winding_scratch_bytes(F)
        if nblob == 0 or nscratch == 0:
            raise L.TvrError("build_winding: " + lib.tvr_last_error().decode(errors="replace"))
        blob = L.dev_bytes(nblob, dev, what="mesh winding table")
        scratch = L.dev_bytes(nscratch, dev, what="mesh winding scratch")
        flag = L.dev_bytes(4, dev, zero=True, what="mesh winding fault flag").view(torch.int32)
        L.check(lib.tvr_mesh_winding_build(_ptr(b.verts), V, _ptr(b.faces), F, b.blob.data_ptr(), L.nbytes(b.blob), blob.data_ptr(), L.nbytes(blob), scratch.data_ptr(),
                                           L.nbytes(scratch), flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_winding_build")
        if int(flag.item()) != 0:
            raise L.TvrError("tvr_mesh_winding_build raised its fault flag: the blob is not this mesh's hierarchy, or the passes did not reach the root (include/tvr.h)")
        b.winding = MeshWinding(blob)
    if stats is not None:
        stats.update(internal_nodes=max(b.n_triangles - 1, 0), table_bytes=int(b.winding.blob.numel()))
    return b.winding


def _winding_beta(beta, what: str) -> float:
    beta = float(beta)
    if not beta >= 1.0:
        raise L.TvrError(f"{what}: beta = {beta} must lie in 1 .. +inf (+inf = the exact sum)")
    return beta


def _winding_stats(stats, total):
    if stats is not None:
        stats.update(zip(WINDING_COUNTS, (int(x) for x in total.cpu().tolist())))


_WINDING_FAULT = ("tvr_mesh_winding_query raised its fault flag: the hierarchy or the winding table does not belong to this mesh, or a face index lies outside the "
                  "vertices (include/tvr.h)")


def winding_number(bvh: MeshBVH, points, beta: float = 2.0, stats: dict = None) -> torch.Tensor:
    """The generalized winding number of a mesh at every point -> w [N] float32 on the device: 1 inside a closed outward-oriented shell, 0 outside, k inside k
    overlapping shells, and a smooth value in between where the soup has holes — defined for ANY triangle soup (open, non-manifold, self-intersecting, unwelded),
    where signed_distance refuses or answers wrongly.

    One walk of the hierarchy per point: a subtree whose centroid is farther than beta x its radius is replaced by one dipole (build_winding's table, built here when
    absent), a leaf adds its triangle's exact solid angle.  beta in [1, inf]: larger is more accurate and slower, inf is the exact sum (DESIGN.md §4.20 has the
    measured error).  A point with a non-finite component gets NaN and is counted.  Results do not depend on the order or batching of the points.  No CPU fallback.
    `stats` (a dict) receives points_answered / points_refused / node_visits / dipole_terms / triangle_terms."""
    b = _bvh_arg(bvh, "winding_number")
    dev = b.device
    p = _rays_on_device(points, dev, "winding_number", "points")
    if p.dim() != 2 or p.shape[1] != 3:
        raise L.TvrError(f"winding_number takes points [N, 3]; got {tuple(p.shape)}")
    beta = _winding_beta(beta, "winding_number")
    table = build_winding(b)
    p = p.contiguous()
    N, lib = int(p.shape[0]), L.lib()
    w = L.dev_empty((N,), torch.float32, dev, what="mesh winding numbers")
    counts = L.dev_empty((5,), torch.int64, dev, what="mesh winding counts")
    total = torch.zeros(5, dtype=torch.int64, device=dev)
    flag = L.dev_bytes(4, dev, zero=True, what="mesh winding fault flag").view(torch.int32)
    for i0 in range(0, max(N, 1), BVH_WINDING_CHUNK):
        n = min(BVH_WINDING_CHUNK, N - i0)
        pc, wc = p[i0:i0 + n], w[i0:i0 + n]
        L.check(lib.tvr_mesh_winding_query(_ptr(b.verts), b.n_vertices, _ptr(b.faces), b.n_triangles, b.blob.data_ptr(), L.nbytes(b.blob), table.blob.data_ptr(),
                                           L.nbytes(table.blob), _ptr(pc), n, None, beta, _ptr(wc), L.nbytes(wc), counts.data_ptr() if stats is not None else None,
                                           flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_winding_query")
        if stats is not None:
            total += counts
    if int(flag.item()) != 0:
        raise L.TvrError(_WINDING_FAULT)
    _winding_stats(stats, total)
    return w


def winding_contains(bvh: MeshBVH, points, beta: float = 2.0) -> torch.Tensor:
    """Which points lie inside a mesh, whatever its defects -> [N] bool on the device: winding_number(bvh, points, beta) > 0.5.  A refused point is not inside."""
    return winding_number(bvh, points, beta) > 0.5


def winding_number_grid(bvh: MeshBVH, dims, origin=(0, 0, 0), spacing=(1, 1, 1), beta: float = 2.0, stats: dict = None) -> torch.Tensor:
    """The winding-number field of a mesh on a lattice -> volume [nx, ny, nz] float32 on the device, laid out as marching_cubes reads its volume.

    Grid point (i, j, k) sits at origin + (i, j, k) * spacing, formed in the kernel in fp32 (one product, one sum per axis): no point tensor is materialised, and the
    values are bit-equal to winding_number on the same points.  marching_cubes(volume, 0.5, spacing, origin) extracts one closed, outward-oriented surface.  dims [3]
    with at most 2^31 - 1 grid points.  beta, `stats` as for winding_number.  No CPU fallback."""
    b = _bvh_arg(bvh, "winding_number_grid")
    dev = b.device
    dims = [int(x) for x in dims]
    if len(dims) != 3 or min(dims) < 0 or dims[0] * dims[1] * dims[2] > 2 ** 31 - 1:
        raise L.TvrError(f"winding_number_grid takes dims [3] of non-negative sizes with at most 2^31 - 1 grid points; got {dims}")
    beta = _winding_beta(beta, "winding_number_grid")
    table = build_winding(b)
    lat = L.MeshLattice()
    lat.origin[:], lat.spacing[:], lat.dims[:] = [float(x) for x in origin], [float(x) for x in spacing], dims
    vol = L.dev_empty(tuple(dims), torch.float32, dev, what="mesh winding volume")
    counts = L.dev_empty((5,), torch.int64, dev, what="mesh winding counts")
    flag = L.dev_bytes(4, dev, zero=True, what="mesh winding fault flag").view(torch.int32)
    L.check(L.lib().tvr_mesh_winding_query(_ptr(b.verts), b.n_vertices, _ptr(b.faces), b.n_triangles, b.blob.data_ptr(), L.nbytes(b.blob), table.blob.data_ptr(),
                                           L.nbytes(table.blob), None, 0, C.byref(lat), beta, _ptr(vol), L.nbytes(vol), counts.data_ptr() if stats is not None else None,
                                           flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_winding_query")
    if int(flag.item()) != 0:
        raise L.TvrError(_WINDING_FAULT)
    _winding_stats(stats, counts)
    return vol


def signed_distance_winding(bvh: MeshBVH, points, max_dist: float = float("inf"), beta: float = 2.0, stats: dict = None):
    """The signed distance of every point to a mesh that need not be closed -> (sdist [N] float32, tri [N] int32, bary [N,3] float32) on the device.

    |sdist|, tri and bary are closest_points' answers, bit for bit; sdist is negative where winding_contains says inside, +0.0 on the surface, +inf where closest_points
    gives +inf.  Unlike signed_distance the sign does not come from the closest feature's normal, so it holds for overlapping shells, soups and meshes with holes.
    `stats` (a dict) receives closest_points' counts and node_visits / dipole_terms / triangle_terms of the winding walk.  No CPU fallback."""
    b = _bvh_arg(bvh, "signed_distance_winding")
    beta = _winding_beta(beta, "signed_distance_winding")
    near, wind = ({}, {}) if stats is not None else (None, None)
    dist, tri, bary = closest_points(b, points, max_dist, stats=near)
    inside = winding_number(b, points, beta, stats=wind) > 0.5
    if stats is not None:
        stats.update(near, node_visits=wind["node_visits"], dipole_terms=wind["dipole_terms"], triangle_terms=wind["triangle_terms"])
    return torch.where(inside & (dist > 0) & torch.isfinite(dist), -dist, dist), tri, bary       # (+inf beyond max_dist stays +inf)


def remesh_watertight(verts, faces, resolution: int = 256, voxel: float = None, pad: int = 2, beta: float = 2.0, level: float = 0.5, stats: dict = None):
    """Any triangle soup -> (verts [V,3] float32, faces [F,3] int32) of ONE closed, outward-oriented surface, on the device: the `level` set of the soup's winding
    number field, extracted by marching_cubes.  Overlapping components are unioned, internal walls disappear, small holes are bridged, unwelded corners are welded.

    The lattice is the bounding box of the soup's finite vertices, grown by `pad` cubic voxels on every side; `voxel` defaults to the longest box edge / `resolution`.
    Every vertex of the result lies within one voxel of the input surface wherever the field jumps across it.  `stats` (a dict) receives dims, voxel, origin, the
    closedness counters of the input and of the result (input / result: build_pseudonormals' counters and closed) and the result's component count.  No CPU fallback."""
    v, f = _mesh_on_device(verts, faces, "remesh_watertight")
    beta = _winding_beta(beta, "remesh_watertight")
    pad = int(pad)
    if pad < 1:
        raise L.TvrError(f"remesh_watertight: pad = {pad} must be at least 1 (the surface must not touch the lattice's border)")
    fin = v[torch.isfinite(v).all(1)]
    if f.shape[0] == 0 or fin.shape[0] == 0:
        raise L.TvrError("remesh_watertight: the mesh has no triangle or no finite vertex")
    lo, hi = fin.min(0)[0].double().cpu().numpy(), fin.max(0)[0].double().cpu().numpy()
    if voxel is None:
        if int(resolution) < 1:
            raise L.TvrError(f"remesh_watertight: resolution = {resolution} must be at least 1")
        voxel = float((hi - lo).max()) / int(resolution)
    voxel = float(voxel)
    if not (voxel > 0.0 and np.isfinite(voxel)):
        raise L.TvrError(f"remesh_watertight: voxel = {voxel} must be a finite number > 0 (a mesh without extent has no surface to extract)")
    origin = [float(x) for x in lo - pad * voxel]
    dims = [int(np.ceil(float(e) / voxel)) + 1 + 2 * pad for e in hi - lo]
    bvh = build_bvh(v, f)
    vol = winding_number_grid(bvh, dims, origin, (voxel,) * 3, beta)
    ov, of = marching_cubes(vol, float(level), (voxel,) * 3, origin)
    if stats is not None:
        cin, cout = {}, {}
        build_pseudonormals(bvh, stats=cin)
        build_pseudonormals(build_bvh(ov, of), stats=cout)
        keep = CLOSEDNESS_COUNTERS + ("closed",)
        stats.update(dims=dims, voxel=voxel, origin=origin, input={k: cin[k] for k in keep}, result={k: cout[k] for k in keep},
                     components=mesh_components(of, int(ov.shape[0]))[2] if int(ov.shape[0]) else 0)
    return ov, of


# ---- which triangles cut through which: the triangle-pair query (csrc/tvr_mesh_crossings.hip; include/tvr.h tvr_mesh_crossings_*) ---------------------------
CROSSINGS_COUNTS = ("pairs", "triangles_refused", "node_tests", "pair_tests")
_CROSSINGS_FAULT = ("tvr_mesh_crossings raised its fault flag: the hierarchy does not belong to this mesh, or a face index of the hierarchy's mesh lies outside the "
                    "vertices (include/tvr.h)")


def _crossings_mesh(b: MeshBVH, query):
    """the arguments both passes share (include/tvr.h tvr_mesh_crossings_*), and the number of query triangles; query: None (self) or (verts_q, faces_q) on the device"""
    if query is None:
        return (_ptr(b.verts), b.n_vertices, _ptr(b.faces), b.n_triangles, b.blob.data_ptr(), L.nbytes(b.blob), 0, None, 0, None, 0), b.n_triangles
    vq, fq = query
    return (_ptr(b.verts), b.n_vertices, _ptr(b.faces), b.n_triangles, b.blob.data_ptr(), L.nbytes(b.blob), 1, _ptr(vq), int(vq.shape[0]), _ptr(fq), int(fq.shape[0])), \
        int(fq.shape[0])


def crossings_count(bvh: MeshBVH, query=None, stats: dict = None):
    """First pass (tvr_mesh_crossings_count): (per_triangle [Nq] int32 — how many triangles each query triangle crosses —, n_pairs).  Reads the total from the device once."""
    dev, lib = bvh.device, L.lib()
    mesh, Nq = _crossings_mesh(bvh, query)
    per = L.dev_empty((Nq,), torch.int32, dev, what="mesh crossings counts per triangle")
    total = L.dev_empty((1,), torch.int64, dev, what="mesh crossings total")
    counts = L.dev_empty((4,), torch.int64, dev, what="mesh crossings counts")
    flag = L.dev_bytes(4, dev, zero=True, what="mesh crossings fault flag").view(torch.int32)
    L.check(lib.tvr_mesh_crossings_count(*mesh, _ptr(per), L.nbytes(per), total.data_ptr(), counts.data_ptr(), flag.data_ptr(), _stream_ptr(dev)), "tvr_mesh_crossings_count")
    if int(flag.item()) != 0:
        raise L.TvrError(_CROSSINGS_FAULT)
    if stats is not None:
        stats.update(zip(CROSSINGS_COUNTS, (int(x) for x in counts.cpu().tolist())))
    return per, int(total.item())


def crossings_emit(bvh: MeshBVH, per_triangle: torch.Tensor, n_pairs: int, query=None, points: bool = False):
    """Second pass (tvr_mesh_crossings_emit) into buffers of exactly the counted size: (pairs [P,2] int32, n_pierce [P] int32, points [P,2,3] float32 or None), the rows
    of one query triangle together and in walk order — not yet sorted.  Counts that are not the ones crossings_count found raise TvrError."""
    dev, lib, P = bvh.device, L.lib(), int(n_pairs)
    mesh, Nq = _crossings_mesh(bvh, query)
    offsets = torch.zeros(Nq + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(per_triangle, 0, dtype=torch.int64)
    pairs = L.dev_empty((P, 2), torch.int32, dev, what="mesh crossings pairs")
    n_pierce = L.dev_empty((P,), torch.int32, dev, what="mesh crossings n_pierce")
    pts = L.dev_empty((P, 2, 3), torch.float32, dev, what="mesh crossings points") if points else None
    flag = L.dev_bytes(4, dev, zero=True, what="mesh crossings fault flag").view(torch.int32)
    L.check(lib.tvr_mesh_crossings_emit(*mesh, offsets.data_ptr(), L.nbytes(offsets), P, _ptr(pairs), L.nbytes(pairs), _ptr(n_pierce), L.nbytes(n_pierce),
                                        None if pts is None else _ptr(pts), 0 if pts is None else L.nbytes(pts), flag.data_ptr(), _stream_ptr(dev)),
            "tvr_mesh_crossings_emit")
    if int(flag.item()) != 0:
        raise L.TvrError(_CROSSINGS_FAULT + "; or the two passes disagree")
    return pairs, n_pierce, pts


def _crossings(b: MeshBVH, query, points: bool, stats, what: str):
    """Both passes and the caller's job after them: the sort of the rows by (first, second)."""
    per, P = crossings_count(b, query, stats)
    if P > 2 ** 31 - 1:
        raise L.TvrError(f"{what}: {P} crossing pairs; at most 2^31 - 1 are written by one call")
    pairs, n_pierce, pts = crossings_emit(b, per, P, query, points)
    order = torch.sort((pairs[:, 0].to(torch.int64) << 32) | pairs[:, 1].to(torch.int64))[1]      # the keys are unique: every correct sort gives this order
    out = (pairs[order].contiguous(), n_pierce[order].contiguous())
    return out + (pts[order].contiguous(),) if points else out


def self_intersections(bvh: MeshBVH, points: bool = False, stats: dict = None):
    """Which triangles of a mesh cut through which -> (pairs [P,2] int32, n_pierce [P] int32[, points [P,2,3] float32]) on the device.

    pairs holds every i < j whose triangles cross, ascending by (i, j).  Two triangles cross iff a side of one pierces the other (six segment-triangle tests per pair,
    each the casts' own ray-triangle test over 0 < t <= 1); n_pierce says how many of the six do — 2 in general position — and points (with points=True) holds the first
    two piercing points, the ends of the pair's intersection segment.  A side is never tested against a triangle that has a corner at the POSITION of one of the side's
    ends, so neighbours do not report rounding noise, welded or not; pairs that share an edge and duplicate faces are therefore never reported.  NOT detected: coplanar
    overlap (a segment in a triangle's plane never pierces).  A triangle with a non-finite corner crosses nothing and is counted.  The same bytes on every run.  No CPU
    fallback.  `stats` (a dict) receives pairs / triangles_refused / node_tests / pair_tests."""
    return _crossings(_bvh_arg(bvh, "self_intersections"), None, points, stats, "self_intersections")


def mesh_intersections(bvh: MeshBVH, verts_q, faces_q, points: bool = False, stats: dict = None):
    """Which triangles of a second mesh cut through which triangles of a hierarchy's mesh -> (pairs [P,2] int32, n_pierce [P] int32[, points [P,2,3] float32]): the
    collision test between two meshes.

    pairs holds every (q, a), q a triangle of (verts_q, faces_q) and a a triangle of bvh's mesh, ascending by (q, a).  The pair test, n_pierce, points, the sharing rule
    (by position, so a query mesh that reuses the hierarchy's vertices behaves as one mesh would) and `stats` are self_intersections'.  A query triangle with a non-finite
    corner or an index outside verts_q crosses nothing and is counted.  Permuting faces_q permutes the rows and nothing else.  No CPU fallback."""
    b = _bvh_arg(bvh, "mesh_intersections")
    vq, fq = _mesh_on_device(verts_q, faces_q, "mesh_intersections")
    if fq.device != b.device:
        raise L.TvrError(f"mesh_intersections: the query mesh is on {fq.device}, the hierarchy on {b.device}")
    return _crossings(b, (vq, fq), points, stats, "mesh_intersections")


def crossing_faces(pairs, n_faces: int, column: int = None) -> torch.Tensor:
    """The triangles involved in crossings -> [n_faces] bool on pairs' device.  column = None: both columns (a self query); 0 / 1: that column alone (the query mesh's
    triangles / the hierarchy's, in a two-mesh query)."""
    mask = torch.zeros(int(n_faces), dtype=torch.bool, device=pairs.device)
    idx = pairs.reshape(-1) if column is None else pairs[:, int(column)]
    mask[idx.to(torch.int64)] = True
    return mask


def mesh_check(verts, faces, bvh: MeshBVH = None) -> dict:
    """Is a mesh usable for printing, simulation, boolean operations?  -> a dict of plain ints and floats: vertices, triangles; build_pseudonormals' counters
    degenerate_faces / open_edges / nonmanifold_edges / inconsistent_edges and closed (the topological half); components (mesh_components); and the geometric half from
    self_intersections: crossing_pairs, crossing_faces (triangles involved), crossing_length (the summed length |points[1] - points[0]| of the pairs' intersection
    segments, in the mesh's units, float64) and n_pierce_histogram {n_pierce: pairs}.  bvh: the mesh's hierarchy, when the caller has one.  No CPU fallback."""
    b = build_bvh(verts, faces) if bvh is None else _bvh_arg(bvh, "mesh_check")
    closed = {}
    build_pseudonormals(b, stats=closed)
    pairs, n_pierce, pts = self_intersections(b, points=True)
    seg = (pts[:, 1].double() - pts[:, 0].double())
    values, counts = torch.unique(n_pierce, return_counts=True)
    report = {"vertices": b.n_vertices, "triangles": b.n_triangles}
    report.update({k: int(closed[k]) for k in CLOSEDNESS_COUNTERS}, closed=bool(closed["closed"]))
    report.update(components=int(mesh_components(b.faces, b.n_vertices)[2]) if b.n_vertices else 0, crossing_pairs=int(pairs.shape[0]),
                  crossing_faces=int(crossing_faces(pairs, b.n_triangles).sum().item()), crossing_length=float(seg.pow(2).sum(1).sqrt().sum().item()),
                  n_pierce_histogram={int(v): int(c) for v, c in zip(values.cpu().tolist(), counts.cpu().tolist())})
    return report


def write_obj_segments(path, points) -> None:
    """Line segments as a Wavefront OBJ of `v` and `l` records only — what a viewer shows as curves: points [P,2,3] (self_intersections' piercing points), segment p
    joins vertices 2p+1 and 2p+2.  Coordinates are written with 9 significant digits, which round-trip float32."""
    p = _host(points, np.float32).reshape(-1, 2, 3)
    with open(path, "w") as f:
        for a in p.reshape(-1, 3):
            f.write(f"v {a[0]:.9g} {a[1]:.9g} {a[2]:.9g}\n")
        for i in range(len(p)):
            f.write(f"l {2 * i + 1} {2 * i + 2}\n")
