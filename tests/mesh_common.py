"""Shared by tests/test_mesh_host.py and tests/test_gpu_mesh.py: test volumes, numpy restatements of what csrc/tvr_mesh.hip specifies (vertex order and
positions, and — from the generator's table — the triangles), and the mesh checks.  The checks read the OUTPUT only (index ranges, directed edges, Euler
characteristic, signed volume): they do not restate the case table, so they catch a wrong table as well as a wrong kernel."""
import importlib.util
import os

import numpy as np

from conftest import ROOT


def load_generator():
    """scripts/gen_mc_table.py imported by file path."""
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "scripts", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- volumes ----------------------------------------------------------------------------------------------------------------------------------------------
def noise_volume(shape, seed=0):
    """uniform [0, 1) in the interior, a zero boundary layer: at level 0.5 the surface is closed."""
    vol = np.zeros(shape, np.float32)
    vol[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed).random(tuple(s - 2 for s in shape)).astype(np.float32)
    return vol


def _grid(shape):
    return np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")


def sphere_volume(shape=(16, 16, 16), centre=(7.3, 8.1, 6.8), radius=5.3):
    """radius - distance: inside (>= 0) the ball."""
    x, y, z = _grid(shape)
    return (radius - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)).astype(np.float32)


def torus_volume(shape=(16, 16, 16), centre=(7.4, 7.6, 7.5), R=4.6, r=1.9):
    x, y, z = _grid(shape)
    q = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2) - R
    return (r - np.sqrt(q ** 2 + (z - centre[2]) ** 2)).astype(np.float32)


def two_spheres_volume(shape=(16, 16, 16)):
    return np.maximum(sphere_volume(shape, (4.2, 4.4, 4.1), 2.7), sphere_volume(shape, (11.1, 10.8, 11.3), 2.9))


def slab_volume(shape=(12, 10, 9)):
    """inside where x + 0.3 y lies in a band: the surface leaves the volume through its y and z faces."""
    x, y, z = _grid(shape)
    return (2.2 - np.abs(x + 0.3 * y - 6.1)).astype(np.float32)


def integer_volume(shape=(14, 12, 10), seed=3):
    """integer values 0..3 inside a zero boundary layer; with level 2.0 the level is an attained value (t = 0 or 1 on many edges)."""
    vol = np.zeros(shape, np.float32)
    vol[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed).integers(0, 4, tuple(s - 2 for s in shape)).astype(np.float32)
    return vol


# ---- numpy restatement of the specification ----------------------------------------------------------------------------------------------------------------
def straddle_masks(vol, level):
    """[nx, ny, nz, 3] bool: does the edge leaving the point along +x / +y / +z exist and have one end >= level and one end below."""
    inside = vol >= np.float32(level)
    m = np.zeros(vol.shape + (3,), bool)
    m[:-1, :, :, 0] = inside[:-1] != inside[1:]
    m[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    m[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    return m


def reference_vertices(vol, level, spacing=(1, 1, 1), origin=(0, 0, 0)):
    """The crossing points in the specified order (owner point ascending, then axis x, y, z), separately rounded fp32:
    t = (level - a) / (b - a); voxel coordinate = index + t; world = origin + coord * spacing."""
    vol = np.asarray(vol, np.float32)
    level = np.float32(level)
    m = straddle_masks(vol, level)
    i, j, k, ax = np.nonzero(m)                      # C order = (point, axis) order
    a = vol[i, j, k]
    b = vol[i + (ax == 0), j + (ax == 1), k + (ax == 2)]
    with np.errstate(all="ignore"):
        t = (level - a) / (b - a)
    coord = np.stack((i, j, k), -1).astype(np.float32)
    coord[np.arange(len(ax)), ax] = coord[np.arange(len(ax)), ax] + t
    sp, org = np.asarray(spacing, np.float32), np.asarray(origin, np.float32)
    return org[None] + coord * sp[None]


def numpy_marching_cubes(vol, level, tri_table, tri_count, edge_lo):
    """(verts [V,3] voxel coordinates, faces [F,3]) from a case table, in the kernels' order: the table applied on the CPU (CPU checks of the TABLE on whole volumes)."""
    vol = np.asarray(vol, np.float32)
    nx, ny, nz = vol.shape
    m = straddle_masks(vol, level)
    vbase = (np.cumsum(m.reshape(-1)) - m.reshape(-1)).reshape(m.shape)          # index of the vertex on (point, axis), where there is one
    inside = vol >= np.float32(level)
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    faces = []
    ci, cj, ck = np.nonzero((case > 0) & (case < 255))              # C order = cell index order
    cs = case[ci, cj, ck]
    for n in range(len(cs)):
        for t in range(int(tri_count[cs[n]])):
            tri = []
            for e in tri_table[cs[n]][t]:
                lo = int(edge_lo[int(e)])
                tri.append(vbase[ci[n] + (lo & 1), cj[n] + ((lo >> 1) & 1), ck[n] + ((lo >> 2) & 1), int(e) >> 2])
            faces.append(tri)
    return reference_vertices(vol, level), np.asarray(faces, np.int64).reshape(-1, 3)


def all_cases_occur(vol, level):
    vol = np.asarray(vol, np.float32)
    nx, ny, nz = vol.shape
    inside = vol >= np.float32(level)
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    return np.bincount(case.reshape(-1), minlength=256)


# ---- checks on a mesh ---------------------------------------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))


def edge_usage(faces, n_verts):
    """(keys of the directed edges, count of each distinct directed edge, whether its reverse occurs, the distinct edges [n,2])"""
    e = directed_edges(faces)
    key = e[:, 0] * n_verts + e[:, 1]
    uniq, counts = np.unique(key, return_counts=True)
    rev = (uniq % n_verts) * n_verts + uniq // n_verts
    return uniq, counts, np.isin(rev, uniq), np.stack((uniq // n_verts, uniq % n_verts), -1)


def assert_closed_and_oriented(faces, n_verts):
    """every face index < V; every directed edge occurs exactly once and its reverse exactly once."""
    f = np.asarray(faces, np.int64)
    assert f.min(initial=0) >= 0 and f.max(initial=-1) < n_verts
    _, counts, has_rev, _ = edge_usage(f, n_verts)
    assert (counts == 1).all(), f"{int((counts != 1).sum())} directed edges occur more than once"
    assert has_rev.all(), f"{int((~has_rev).sum())} directed edges lack their reverse"


def euler_characteristic(n_verts, faces):
    e = np.sort(directed_edges(faces), axis=1)
    n_edges = len(np.unique(e[:, 0] * n_verts + e[:, 1]))
    return n_verts - n_edges + len(faces)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def cell_count_bounds(vol, level):
    """(cells with all eight corners inside, cells with any corner inside): the enclosed volume of a surface that separates inside from outside corners
    and stays within the cells it cuts lies between the two (unit spacing)."""
    hist = all_cases_occur(vol, level)
    return int(hist[255]), int(hist[1:].sum())


def ulp_distance(a, b):
    """|a - b| in units of the fp32 spacing at max(|a|, |b|) (elementwise)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
