"""Shared by tests/test_mesh_simplify_host.py and tests/test_gpu_mesh_simplify.py: the numpy oracle for vertex-clustering simplification, restated from the definition
in include/tvr.h (tvr_mesh_simplify_*) and NOT from the kernels: it sorts keys (np.unique) where the kernels hash them, and sums with np.add.at where they add
atomically.  Floating point: np.float32 array operations one at a time (numpy rounds each on its own), np.floor, integer sums, one float64 quotient.  Every comparison
with the oracle is exact: np.array_equal on indices and counts, the uint32 view for positions.  No tolerance appears anywhere."""
import numpy as np

CELL_LIMIT = 2 ** 21        # cells per axis
Q_SCALE = 1048576.0         # 2^20 steps inside a cell


class OutsideLattice(ValueError):
    """a vertex whose cell is not in 0 .. 2^21-1 on some axis (NaN and infinity included): the library raises its fault flag"""


def lattice(cell, origin=(0, 0, 0)):
    """(origin, cell, inv_cell) as float32 triples; inv_cell = float32(1) / float32(cell)"""
    c = np.asarray(cell, np.float64).reshape(-1)
    c = (np.repeat(c, 3) if c.size == 1 else c).astype(np.float32)
    return np.asarray(origin, np.float32).reshape(3), c, np.float32(1) / c


def cells_of(verts, origin, inv_cell):
    """(g [V,3] float32, c [V,3] float32 = floor(g)): g = (v - origin) * inv_cell, two separately rounded float32 operations"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d = v - origin[None]
        g = d * inv_cell[None]
        c = np.floor(g)
    assert d.dtype == np.float32 and g.dtype == np.float32 and c.dtype == np.float32
    if not ((c >= 0) & (c < CELL_LIMIT)).all():          # (a NaN fails both comparisons)
        raise OutsideLattice("a vertex lies outside the lattice")
    return g, c


def canonical_rotation(tri):
    """rows of [n,3] rotated so that the smallest entry leads (orientation kept); entries of a row are distinct"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    k = np.argmin(tri, axis=1)
    idx = (k[:, None] + np.arange(3)[None]) % 3
    return np.take_along_axis(tri, idx, axis=1)


def simplify_oracle(verts, faces, cell, origin=(0, 0, 0)):
    """(verts' [V',3] float32, faces' [F',3] int64, vertex_map [V] int64).  Raises OutsideLattice / IndexError where the library raises its flag."""
    o, cl, inv = lattice(cell, origin)
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    if f.size and (f.min() < 0 or f.max() >= V):
        raise IndexError("a face index lies outside the vertices")
    g, c = cells_of(v, o, inv)
    ci = c.astype(np.int64)
    key = ci[:, 0] | (ci[:, 1] << 21) | (ci[:, 2] << 42)
    # clusters in ascending order of their representative = the FIRST (smallest) vertex index with the key
    _, rep, inverse = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(rep, kind="stable")
    rank = np.empty(len(rep), np.int64)
    rank[order] = np.arange(len(rep))
    vmap = rank[inverse.reshape(-1)]
    rep = rep[order]
    n_out = len(rep)
    # positions: integer sums of the truncated in-cell fractions, one float64 quotient
    frac = g - c
    assert frac.dtype == np.float32
    q = (frac * np.float32(Q_SCALE)).astype(np.uint32).astype(np.int64)          # truncates; the product is exact
    assert (q < 2 ** 20).all()
    sums = np.zeros((n_out, 3), np.int64)
    np.add.at(sums, vmap, q)
    members = np.bincount(vmap, minlength=n_out).astype(np.float64)
    mean = (sums.astype(np.float64) / (members[:, None] * Q_SCALE)).astype(np.float32)
    corner = o[None] + c[rep] * cl[None]
    pos = corner + mean * cl[None]
    assert corner.dtype == np.float32 and pos.dtype == np.float32
    # triangles
    m = vmap[f] if len(f) else np.zeros((0, 3), np.int64)
    alive = np.nonzero((m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2]))[0]
    if len(alive):
        _, first = np.unique(canonical_rotation(m[alive]), axis=0, return_index=True)          # first occurrence = smallest old index
        alive = alive[np.sort(first)]
    return pos.reshape(-1, 3), m[alive].reshape(-1, 3), vmap


def brute_force(verts, faces, cell, origin=(0, 0, 0)):
    """The same definition by O(V^2) / O(F^2) comparisons in Python loops, for small meshes: (verts', faces', vertex_map)."""
    o, cl, inv = lattice(cell, origin)
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    g, c = cells_of(v, o, inv)
    V = len(v)
    rep = np.arange(V)
    for a in range(V):
        for b in range(a):
            if (c[a] == c[b]).all():
                rep[a] = b                      # the smallest earlier vertex of the same cell
                break
    reps = [a for a in range(V) if rep[a] == a]
    new = {r: i for i, r in enumerate(reps)}
    vmap = np.array([new[rep[a]] for a in range(V)], np.int64).reshape(-1)
    pos = np.zeros((len(reps), 3), np.float32)
    for i, r in enumerate(reps):
        mem = [a for a in range(V) if rep[a] == r]
        for k in range(3):
            total = 0
            for a in mem:
                total += int(np.float32(g[a, k] - c[a, k]) * np.float32(Q_SCALE))
            mean = np.float32(float(total) / (float(len(mem)) * Q_SCALE))
            pos[i, k] = np.float32(o[k] + np.float32(c[r, k] * cl[k])) + np.float32(mean * cl[k])
    kept = []
    for t in range(len(f)):
        x, y, z = (int(vmap[i]) for i in f[t])
        if x == y or y == z or x == z:
            continue
        rots = {(x, y, z), (y, z, x), (z, x, y)}
        if any(tuple(int(vmap[i]) for i in f[u]) in rots for u in kept):
            continue
        kept.append(t)
    out = np.array([[vmap[i] for i in f[t]] for t in kept], np.int64).reshape(-1, 3)
    return pos, out, vmap


def random_mesh(rng, n_vertices, n_faces, extent=4.0, snap=0.5):
    """random vertices in [0, extent)^3, about half of their coordinates snapped to multiples of `snap` (so that cell boundaries are hit), random faces with repeats"""
    v = (rng.random((n_vertices, 3)) * extent).astype(np.float32)
    on = rng.random((n_vertices, 3)) < 0.5
    v[on] = (np.floor(v[on] / snap) * snap).astype(np.float32)
    f = rng.integers(0, n_vertices, (n_faces, 3))
    if n_faces >= 4:
        f[n_faces // 2] = f[0]                         # a duplicate
        f[n_faces // 2 + 1] = f[1][[1, 2, 0]]          # a rotation
        f[n_faces - 1] = f[2][::-1]                    # a reversal
    return v, f.astype(np.int64)
