"""Shared by tests/test_mesh_components_host.py and tests/test_gpu_mesh_components.py: the numpy oracle for connected components, the size policy and the filter,
restated from the definitions in include/tvr.h (NOT from the kernels: the oracle propagates minimum labels, the kernels hook roots), and the test meshes.
Every comparison with the oracle is np.array_equal: all quantities are integers or copied floats."""
import functools

import numpy as np

import mesh_common as MC

# (min_faces, keep_largest) pairs; the values cut through the ties of the fixtures (8-face and 32-face components tie on the noise and integer volumes)
POLICY_GRID = [(0, 1), (0, 2), (0, 3), (0, 5), (1, 0), (8, 0), (9, 0), (32, 0), (33, 0), (8, 4), (32, 2), (300, 1), (10 ** 9, 0), (0, 10 ** 6)]


def components_oracle(faces, n_vertices):
    """(vertex_label [V], component_faces [V], n_components): label = smallest vertex index of the component; size = triangles whose FIRST vertex carries the label.
    Union-find restated as its fixed point: every vertex takes the smallest label seen across its triangles, labels are chased (label[label]) until nothing changes."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    assert f.size == 0 or (f.min() >= 0 and f.max() < n_vertices)
    label = np.arange(n_vertices, dtype=np.int64)
    while True:
        low = label[f].min(axis=1) if len(f) else np.zeros(0, np.int64)
        new = label.copy()
        for k in range(3):
            np.minimum.at(new, f[:, k], low)          # a triangle connects its three vertices
            np.minimum.at(new, label[f[:, k]], low)   # ... and thereby the components they already belong to
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    sizes = np.bincount(label[f[:, 0]], minlength=n_vertices).astype(np.int64) if len(f) else np.zeros(n_vertices, np.int64)
    return label, sizes, int((label == np.arange(n_vertices)).sum())


def keep_oracle(label, sizes, min_faces=0, keep_largest=0):
    """keep_root [V] uint8: min_faces first, then the keep_largest biggest, ties to the smaller label; zero-face components go once either option is on."""
    roots = [int(r) for r in np.nonzero(label == np.arange(len(label)))[0]]
    if min_faces or keep_largest:
        roots = [r for r in roots if sizes[r] >= max(min_faces, 1)]
    if keep_largest:
        roots = sorted(roots, key=lambda r: (-int(sizes[r]), r))[:keep_largest]
    keep = np.zeros(len(label), np.uint8)
    keep[roots] = 1
    return keep


def filter_oracle(verts, faces, label, keep_root):
    """(verts', faces', kept_vertex): survivors in their order, faces re-indexed."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    kv = keep_root[label].astype(bool) if len(label) else np.zeros(0, bool)
    kf = kv[f[:, 0]] if len(f) else np.zeros(0, bool)
    new = np.cumsum(kv) - 1
    return (None if verts is None else np.asarray(verts)[kv]), new[f[kf]].reshape(-1, 3), np.nonzero(kv)[0]


@functools.lru_cache(maxsize=None)
def table():
    gen = MC.load_generator()
    tri, cnt = gen.build_table()
    return tri, cnt, [lo for lo, _ in gen.EDGE_CORNERS]


VOLUMES = {"two_spheres": (MC.two_spheres_volume, 0.0), "noise": (lambda: MC.noise_volume((24, 20, 18)), 0.5), "integer": (MC.integer_volume, 2.0),
           "sphere": (MC.sphere_volume, 0.0), "torus": (MC.torus_volume, 0.0), "slab": (MC.slab_volume, 0.0)}
CLOSED = ("two_spheres", "noise", "integer", "sphere", "torus")


@functools.lru_cache(maxsize=None)
def cpu_mesh(name):
    """(verts, faces) of a fixture volume from the case table applied in numpy — computed once, never written to."""
    make, level = VOLUMES[name]
    v, f = MC.numpy_marching_cubes(make(), level, *table())
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


# ---- synthetic index buffers ---------------------------------------------------------------------------------------------------------------------------------
def strip_faces(n_vertices):
    """triangle strip (i, i+1, i+2): one component, and the deepest chain a union-find can be handed"""
    i = np.arange(n_vertices - 2, dtype=np.int64)
    return np.stack((i, i + 1, i + 2), -1)


def disjoint_triangles(n, offset=0):
    return (np.arange(3 * n, dtype=np.int64) + offset).reshape(n, 3)
