"""Shared by tests/test_mesh_smooth_host.py and tests/test_gpu_mesh_smooth.py: the numpy oracle for the vertex adjacency and for Taubin smoothing, restated from the
definitions in include/tvr.h (tvr_mesh_adjacency_* / tvr_mesh_smooth) and NOT from the kernels: the adjacency is np.unique with counts on the directed pairs (the kernels
fill raw rows through atomic cursors and sort each row), the smoothing is a loop over the neighbour slot k with one float32 array operation per step (numpy rounds each
on its own, as the kernels do with contraction off), and a Python-loop version of both serves small meshes.  Every comparison with the oracle is exact: np.array_equal on
integers, the uint32 view on positions.  No tolerance appears in any comparison with the oracle."""
import numpy as np


def adjacency_oracle(faces, n_vertices):
    """(offsets [V+1], neighbours [H], edge_faces [H], stats) as int64 arrays and a dict {half_edges, boundary_edges, nonmanifold_edges, max_degree}.
    IndexError where the library raises its flag (a face index outside 0 .. V-1)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = int(n_vertices)
    if f.size and (f.min() < 0 or f.max() >= V):
        raise IndexError("a face index lies outside the vertices")
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)                # the sides {a,b}, {b,c}, {c,a} of every face
    proper = a != b
    a, b = a[proper], b[proper]
    key = np.concatenate((a, b)) * max(V, 1) + np.concatenate((b, a))            # every side once from each end; sorting the key sorts by (row, neighbour)
    uniq, count = np.unique(key, return_counts=True)
    row, nbr = uniq // max(V, 1), uniq % max(V, 1)
    deg = np.bincount(row, minlength=V).astype(np.int64) if V else np.zeros(0, np.int64)
    offsets = np.zeros(V + 1, np.int64)
    offsets[1:] = np.cumsum(deg)
    once = row < nbr                                                 # every undirected edge at its smaller end
    stats = dict(half_edges=int(len(uniq)), boundary_edges=int((once & (count == 1)).sum()), nonmanifold_edges=int((once & (count > 2)).sum()),
                 max_degree=int(deg.max()) if V else 0)
    return offsets, nbr.astype(np.int64), count.astype(np.int64), stats


def adjacency_brute_force(faces, n_vertices):
    """The same definition with a dictionary per vertex, in Python loops."""
    V = int(n_vertices)
    rows = [dict() for _ in range(V)]
    for t in np.asarray(faces, np.int64).reshape(-1, 3):
        for q in range(3):
            u, w = int(t[q]), int(t[(q + 1) % 3])
            if u == w:
                continue
            rows[u][w] = rows[u].get(w, 0) + 1
            rows[w][u] = rows[w].get(u, 0) + 1
    offsets, nbrs, counts = [0], [], []
    for v in range(V):
        for u in sorted(rows[v]):
            nbrs.append(u)
            counts.append(rows[v][u])
        offsets.append(len(nbrs))
    edges = [(v, u, c) for v in range(V) for u, c in rows[v].items() if v < u]
    stats = dict(half_edges=len(nbrs), boundary_edges=sum(c == 1 for _, _, c in edges), nonmanifold_edges=sum(c > 2 for _, _, c in edges),
                 max_degree=max((len(r) for r in rows), default=0))
    return np.array(offsets, np.int64), np.array(nbrs, np.int64), np.array(counts, np.int64), stats


def pinned_vertices(offsets, edge_faces):
    """bool [V]: the vertices with an edge that has a single face side"""
    offsets, edge_faces = np.asarray(offsets, np.int64), np.asarray(edge_faces, np.int64)
    V = len(offsets) - 1
    rows = np.repeat(np.arange(V), np.diff(offsets))
    pinned = np.zeros(V, bool)
    pinned[rows[edge_faces == 1]] = True
    return pinned


def smooth_oracle(verts, offsets, neighbours, edge_faces, iterations, lam=0.5, mu=-0.53, pin_boundary=True):
    """verts' [V,3] float32 after `iterations` Taubin iterations over the given adjacency."""
    p = np.array(verts, np.float32).reshape(-1, 3)
    offsets, nbrs = np.asarray(offsets, np.int64), np.asarray(neighbours, np.int64)
    V = len(p)
    deg = np.diff(offsets)
    moves = deg > 0
    if pin_boundary:
        moves &= ~pinned_vertices(offsets, edge_faces)
    idx = np.nonzero(moves)[0]
    start, d = offsets[idx], deg[idx]
    n = d.astype(np.float32)[:, None]
    top = int(d.max()) if len(d) else 0
    order = np.argsort(-d, kind="stable")                            # longest rows first: the rows that still have a slot k are a prefix of `order`
    active = np.searchsorted(-d[order], -np.arange(top), side="left")            # active[k] = rows with more than k neighbours
    with np.errstate(all="ignore"):
        for _ in range(int(iterations)):
            for w in (np.float32(lam), np.float32(mu)):
                s = p[nbrs[start]]                                   # the sum starts from the first neighbour
                for k in range(1, top):
                    sel = order[:active[k]]
                    s[sel] = s[sel] + p[nbrs[start[sel] + k]]
                m = s / n
                diff = m - p[idx]
                t = w * diff
                q = p.copy()
                q[idx] = p[idx] + t
                assert s.dtype == m.dtype == diff.dtype == t.dtype == q.dtype == np.float32
                p = q
    return p


def smooth_brute_force(verts, offsets, neighbours, edge_faces, iterations, lam=0.5, mu=-0.53, pin_boundary=True):
    """The same definition, one float32 scalar operation at a time."""
    p = np.array(verts, np.float32).reshape(-1, 3)
    V = len(p)
    with np.errstate(all="ignore"):
        for _ in range(int(iterations)):
            for w in (np.float32(lam), np.float32(mu)):
                q = p.copy()
                for v in range(V):
                    lo, hi = int(offsets[v]), int(offsets[v + 1])
                    if hi == lo or (pin_boundary and any(int(c) == 1 for c in edge_faces[lo:hi])):
                        continue
                    for a in range(3):
                        s = p[int(neighbours[lo]), a]
                        for k in range(lo + 1, hi):
                            s = np.float32(s + p[int(neighbours[k]), a])
                        m = np.float32(s / np.float32(hi - lo))
                        q[v, a] = np.float32(p[v, a] + np.float32(w * np.float32(m - p[v, a])))
                p = q
    return p


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def signed_volume(verts, faces):
    v, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def mean_umbrella(verts, offsets, neighbours):
    """mean over the vertices with neighbours of |mean of the neighbours - vertex|, in float64: what smoothing is meant to bring down"""
    v, offsets, nbrs = np.asarray(verts, np.float64), np.asarray(offsets, np.int64), np.asarray(neighbours, np.int64)
    deg = np.diff(offsets)
    rows = np.repeat(np.arange(len(v)), deg)
    sums = np.zeros_like(v)
    np.add.at(sums, rows, v[nbrs])
    has = deg > 0
    return float(np.linalg.norm(sums[has] / deg[has, None] - v[has], axis=1).mean())


# ---- synthetic index buffers ---------------------------------------------------------------------------------------------------------------------------------
def with_equal_corners(rng, faces, n_vertices, n_extra):
    """`faces` followed by faces with two equal corners (one proper side, listed twice) and with three (no side)"""
    extra = rng.integers(0, n_vertices, (n_extra, 3))
    extra[:, 2] = extra[np.arange(n_extra), rng.integers(0, 2, n_extra)]
    extra[::3, 1] = extra[::3, 0]
    return np.concatenate((np.asarray(faces, np.int64), extra.astype(np.int64)))


def fan(hub_degree, lead=3, tail=5, closed=False):
    """(verts [V,3] float32, faces [F,3]): a hub joined to `hub_degree` rim vertices on a wavy circle; `lead` unused vertices before the hub and `tail` after the rim.
    An open fan has hub_degree - 1 faces (the hub's raw row: 2 hub_degree - 2 entries), a closed one hub_degree (2 hub_degree entries)."""
    n = int(hub_degree)
    hub = lead
    rim = hub + 1 + np.arange(n, dtype=np.int64)
    nxt = np.roll(rim, -1)
    f = np.stack((np.full(n, hub, np.int64), rim, nxt), -1)
    if not closed:
        f = f[:-1]
    ang = np.arange(n) * (2 * np.pi / n)
    v = np.zeros((lead + 1 + n + tail, 3), np.float32)
    v[rim] = np.stack((np.cos(ang) * (1 + 0.05 * np.sin(7 * ang)), np.sin(ang), 0.1 * np.cos(5 * ang)), -1).astype(np.float32)
    v[hub] = (0.01, -0.02, 0.5)
    v[:lead] = 3.0
    v[lead + 1 + n:] = -3.0
    return v, f
