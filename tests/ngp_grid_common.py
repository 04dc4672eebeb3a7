"""float32 numpy restatement of the occupancy-grid update (include/tvr_ngp.h, "the occupancy grid from the network"), written from the header's
definitions: a vectorised pcg32, the sample generator, mark-untrained, the splat (max over duplicates, fp64 exponent: the reference value of a
tolerance test) and the ema.  Shared by tests/test_ngp_grid_host.py and tests/test_gpu_ngp_grid.py, together with the inputs both use."""
import math

import numpy as np

G = 128
CELLS = G ** 3
N_CELLS_ALL = 5 * CELLS
F = np.float32
U32 = np.uint32
U64 = np.uint64
M32 = 0xFFFFFFFF
PCG_MULT = U64(0x5851F42D4C957F2D)
MIN_CONE_STEPSIZE = F(1.73205080757) / F(1024)
SQRT3 = F(1.73205080757)


# ---------------------------------------------------------------------------------------------------------------- pcg32, vectorised
def pcg_advance(state, inc, delta):
    """state advanced by delta[k] steps, for every k: uint64 arrays (uint64 products wrap)."""
    delta = np.array(delta, dtype=U64, ndmin=1)
    shape = delta.shape
    cur_mult, cur_plus = np.full(shape, PCG_MULT), np.full(shape, U64(inc))
    acc_mult, acc_plus = np.ones(shape, U64), np.zeros(shape, U64)
    with np.errstate(over="ignore"):
        while delta.any():
            odd = (delta & U64(1)).astype(bool)
            acc_mult = np.where(odd, acc_mult * cur_mult, acc_mult)
            acc_plus = np.where(odd, acc_plus * cur_mult + cur_plus, acc_plus)
            cur_plus = (cur_mult + U64(1)) * cur_plus
            cur_mult = cur_mult * cur_mult
            delta = delta >> U64(1)
        return acc_mult * np.broadcast_to(U64(state), shape) + acc_plus


def pcg_next_uint(state, inc):
    """(new state, uint32 output) of every generator in `state`."""
    with np.errstate(over="ignore"):
        new = state * PCG_MULT + U64(inc)
    xs = (((state >> U64(18)) ^ state) >> U64(27)).astype(U32)
    rot = (state >> U64(59)).astype(U32)
    return new, (xs >> rot) | (xs << ((U32(32) - rot) & U32(31)))


def pcg_next_float(state, inc):
    state, u = pcg_next_uint(state, inc)
    return state, ((u >> U32(9)) | U32(0x3F800000)).view(F) - F(1)


# ---------------------------------------------------------------------------------------------------------------- cells
def morton3d_invert(x):
    x = x.astype(U32) & U32(0x49249249)
    x = (x | (x >> U32(2))) & U32(0xC30C30C3)
    x = (x | (x >> U32(4))) & U32(0x0F00F00F)
    x = (x | (x >> U32(8))) & U32(0xFF0000FF)
    x = (x | (x >> U32(16))) & U32(0x0000FFFF)
    return x


def cell_xyz(pos_idx):
    return [morton3d_invert(pos_idx >> U32(k)) for k in range(3)]


def morton3d(x, y, z):
    def expand(v):
        v = np.asarray(v, U32)
        v = (v * U32(0x00010001)) & U32(0xFF0000FF)
        v = (v * U32(0x00000101)) & U32(0x0F00F00F)
        v = (v * U32(0x00000011)) & U32(0xC30C30C3)
        v = (v * U32(0x00000005)) & U32(0x49249249)
        return v
    with np.errstate(over="ignore"):
        return expand(x) | (expand(y) << U32(1)) | (expand(z) << U32(2))


# ---------------------------------------------------------------------------------------------------------------- the generator
def grid_samples(n, ema_step, n_cascades, thresh, state, inc, aabb_lo, aabb_hi, grid, want_break=False, only=None):
    """tvr_ngp_grid_samples: (positions [n,3] float32, indices [n] uint32 [, first j that broke, 10 where none did]).
    `only`: the samples i of the n to compute (default all of them)."""
    i = np.arange(n, dtype=U32) if only is None else np.asarray(only, U32)
    n_out = i.size
    st = pcg_advance(state, inc, (i * U32(4)).astype(U64))
    st, f = pcg_next_float(st, inc)
    level = (f * F(n_cascades)).astype(U32) % U32(n_cascades)
    with np.errstate(over="ignore"):
        h0 = (i + U32((ema_step * n) & M32)) * U32(56924617)
        idx = np.zeros(n_out, U32)
        broke = np.full(n_out, 10, np.int32)
        for j in range(10):
            cand = (h0 + U32((j * 19349663) & M32) + U32(96925573)) % U32(CELLS) + level * U32(CELLS)
            live = broke == 10
            idx = np.where(live, cand, idx)
            broke = np.where(live & (grid[cand] > F(thresh)), j, broke)
    scale = np.ldexp(F(1), level.astype(np.int32)).astype(F)
    pos = np.empty((n_out, 3), F)
    for k, c in enumerate(cell_xyz(idx % U32(CELLS))):
        st, u = pcg_next_float(st, inc)
        p = ((c.astype(F) + u) / F(G) - F(0.5)) * scale + F(0.5)
        pos[:, k] = (p - F(aabb_lo[k])) / (F(aabb_hi[k]) - F(aabb_lo[k]))
    return (pos, idx, broke) if want_break else (pos, idx)


# ---------------------------------------------------------------------------------------------------------------- mark-untrained
_cell_cache = {}


def cell_centres():
    """(pos [5*G^3, 3] float32, radius [5*G^3] float32) of every cell, computed once."""
    if "c" not in _cell_cache:
        i = np.arange(N_CELLS_ALL, dtype=U32)
        level = (i // U32(CELLS)).astype(np.int32)
        scale = np.ldexp(F(1), level).astype(F)
        pos = np.stack([((c.astype(F) + F(0.5)) / F(G) - F(0.5)) * scale + F(0.5) for c in cell_xyz(i % U32(CELLS))], 1)
        _cell_cache["c"] = (pos, F(0.5) * SQRT3 * scale / F(G))
    return _cell_cache["c"]


def cells_seen(focal_lengths, xforms, resolution):
    """bool [5*G^3]: some camera sees the cell (tvr_ngp_grid_mark_untrained's test)."""
    pos, r = cell_centres()
    seen = np.zeros(N_CELLS_ALL, bool)
    half_w, half_h = F(resolution[0]) * F(0.5), F(resolution[1]) * F(0.5)
    for fl, m in zip(np.asarray(focal_lengths, F).reshape(-1, 2), np.asarray(xforms, F).reshape(-1, 3, 4)):
        p = [pos[:, k] - m[k, 3] for k in range(3)]
        x, y, z = [(p[0] * m[0, a] + p[1] * m[1, a]) + p[2] * m[2, a] for a in range(3)]
        seen |= (z > 0) & (np.abs(x) - r < z / fl[0] * half_w) & (np.abs(y) - r < z / fl[1] * half_h)
    return seen


def mark_untrained(grid, focal_lengths, xforms, resolution):
    seen = cells_seen(focal_lengths, xforms, resolution)
    flip = (grid < 0) != ~seen
    return np.where(flip, np.where(seen, F(0), F(-1)), grid).astype(F)


# ---------------------------------------------------------------------------------------------------------------- splat and ema
def splat64(indices, raw, n_cells=N_CELLS_ALL):
    """max over the samples of each cell of exp(raw) * MIN_CONE_STEPSIZE with the exponent in fp64; cells without a sample are 0."""
    tmp = np.zeros(n_cells, np.float64)
    np.maximum.at(tmp, indices.astype(np.int64), np.exp(raw.astype(np.float64)) * float(MIN_CONE_STEPSIZE))
    return tmp


def ema(tmp, grid, decay):
    return np.where(grid < 0, grid, np.maximum(grid * F(decay), tmp)).astype(F)


# ---------------------------------------------------------------------------------------------------------------- inputs the host and GPU tests share
AABB_SCALE = 4                                     # conftest.NGP_AABB_SCALE
AABB = ([0.5 - AABB_SCALE / 2] * 3, [0.5 + AABB_SCALE / 2] * 3)
MARK_RES = (800, 800)


def mark_cameras(n=3):
    """(focal_lengths [n,2], xforms [n,3,4]): 800x800 cameras of rays.sphere_poses through ngp.matrix_nerf2ngp."""
    from jittor_myc_nerfs_amd import ngp, rays as R
    poses = R.sphere_poses(8, 4.0)
    focal = 0.5 * MARK_RES[0] / math.tan(0.5 * 0.6911)
    x = np.stack([ngp.matrix_nerf2ngp(np.asarray(poses[k], np.float32)) for k in (0, 3, 5)[:n]]).astype(F)
    return np.full((n, 2), focal, F), x


def mixed_grid(seed=7):
    """A grid that already holds -1, 0 and positive values in every cascade."""
    rng = np.random.default_rng(seed)
    g = rng.choice(np.array([-1.0, 0.0, 0.5, 2.0], F), size=N_CELLS_ALL, p=[0.3, 0.3, 0.2, 0.2])
    return g.astype(F)
