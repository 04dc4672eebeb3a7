"""The per-triangle texture atlas (include/tvr.h tvr_mesh_atlas_points / tvr_mesh_texture_sample) restated in numpy fp32, operation by operation — what the kernels of
csrc/tvr_mesh_texture.hip are held to, within 2 ulp — and the fp64 pieces the restatement itself is checked against.  Every numpy operation on float32 arrays rounds on
its own, as the kernels do (no fused multiply-add; correctly rounded division).  Pure numpy: no GPU, no library."""
import numpy as np

F32 = np.float32
PROTOTYPE_AFFINE_ERROR = 7.8e-7        # the affine-reproduction error the numpy prototype of the definition observed against fp64 for values of order 1


def layout(F, P, C):
    """(Ha, Wa) of the atlas of F triangles at patch side P, C squares per row"""
    S = (F + 1) // 2
    return max(-(-S // C), 1) * P, C * P


def default_columns(F):
    S = (F + 1) // 2
    c = 1
    while c * c < S:
        c += 1
    return c


def owners(F, P, C, idx):
    """texels with linear indices idx -> (tri, x, y): the owning triangle (-1 for none) and the local coordinates in its half"""
    Ha, Wa = layout(F, P, C)
    idx = np.asarray(idx, dtype=np.int64)
    Y, X = idx // Wa, idx % Wa
    a, b = X % P, Y % P
    s = (Y // P) * C + X // P
    h = (a + b > P - 1).astype(np.int64)
    x, y = np.where(h == 1, P - 1 - a, a), np.where(h == 1, P - 1 - b, b)
    t = 2 * s + h
    return np.where(t < F, t, -1).astype(np.int32), x, y


def restate_points(verts, faces, P, C, texel0=0, n=None):
    """tvr_mesh_atlas_points -> (pos [n,3] f32, tri [n] i32)"""
    v, f = np.asarray(verts, dtype=F32).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    Ha, Wa = layout(len(f), P, C)
    n = Ha * Wa - texel0 if n is None else n
    tri, x, y = owners(len(f), P, C, texel0 + np.arange(n, dtype=np.int64))
    own = tri >= 0
    pos = np.zeros((n, 3), dtype=F32)
    if own.any():
        L = F32(P - 4)
        b1, b2 = x[own].astype(F32) / L, y[own].astype(F32) / L
        b0 = (F32(1.0) - b1) - b2
        c = v[f[tri[own]]]                                      # [m,3 corners,3]
        pos[own] = (b0[:, None] * c[:, 0] + b1[:, None] * c[:, 1]) + b2[:, None] * c[:, 2]
    return pos, tri


def tap_texels(tri, bary, P, C, F):
    """the four taps of every hit (tri [m] >= 0, bary [m,3]) -> (e [m,4] int64 linear atlas indices in the order T00, T10, T01, T11, fx [m] f32, fy [m] f32)"""
    Ha, Wa = layout(F, P, C)
    t = np.asarray(tri, dtype=np.int64)
    b = np.asarray(bary, dtype=F32).reshape(-1, 3)
    L = F32(P - 4)
    with np.errstate(invalid="ignore"):
        x = np.fmin(np.fmax(b[:, 1] * L, F32(0.0)), L)         # fmax / fmin: a NaN becomes 0, as fmaxf makes it
        y = np.fmin(np.fmax(b[:, 2] * L, F32(0.0)), L)
    fi, fj = np.floor(x), np.floor(y)
    i, j = fi.astype(np.int64), fj.astype(np.int64)
    s, h = t >> 1, t & 1
    X0, Y0 = (s % C) * P, (s // C) * P
    e = []
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        lx, ly = i + dx, j + dy
        a, bb = np.where(h == 1, P - 1 - lx, lx), np.where(h == 1, P - 1 - ly, ly)
        e.append((Y0 + bb) * Wa + (X0 + a))
    return np.stack(e, -1), (x - fi).astype(F32), (y - fj).astype(F32)


def restate_sample(tri, bary, atlas, P, C, F):
    """tvr_mesh_texture_sample -> out [..., 3] f32; atlas [Ha,Wa,3] uint8 or f32"""
    tri = np.asarray(tri)
    shape = tri.shape
    t = tri.reshape(-1).astype(np.int64)
    b = np.asarray(bary, dtype=F32).reshape(-1, 3)
    out = np.zeros((t.size, 3), dtype=F32)
    hit = (t >= 0) & (t < F)
    if hit.any():
        tex = np.asarray(atlas).reshape(-1, 3).astype(F32)
        e, fx, fy = tap_texels(t[hit], b[hit], P, C, F)
        inside = e < len(tex)
        T = np.where(inside[..., None], tex[np.where(inside, e, 0)], F32(0.0))        # [m,4,3]
        with np.errstate(invalid="ignore", over="ignore"):
            top = T[:, 0] + fx[:, None] * (T[:, 1] - T[:, 0])
            bot = T[:, 2] + fx[:, None] * (T[:, 3] - T[:, 2])
            out[hit] = top + fy[:, None] * (bot - top)
    return out.reshape(shape + (3,))


# ---- fp64 side ----------------------------------------------------------------------------------------------------------------------------------------------------------------
AFFINE_A = np.array([[0.31, -0.22, 0.17], [-0.12, 0.27, 0.21], [0.19, 0.14, -0.33]])       # three channels, values of order 1 on the unit sphere
AFFINE_C = np.array([0.55, 0.45, 0.6])


def affine(points):
    """the affine colour field, fp64: [m,3] -> [m,3]"""
    return np.asarray(points, dtype=np.float64) @ AFFINE_A.T + AFFINE_C


def affine_atlas(verts, faces, P, C):
    """the affine field baked into the restatement's atlas, fp32 format: every owned texel holds the field at the texel's (restated, fp32) point, rounded to fp32"""
    pos, tri = restate_points(verts, faces, P, C)
    Ha, Wa = layout(len(np.asarray(faces).reshape(-1, 3)), P, C)
    return np.where((tri >= 0)[:, None], affine(pos), 0.0).astype(F32).reshape(Ha, Wa, 3)


def true_points(verts, faces, tri, bary64):
    """fp64 points of barycentric hits"""
    v, f = np.asarray(verts, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    c = v[f[np.asarray(tri, dtype=np.int64)]]
    b = np.asarray(bary64, dtype=np.float64)
    return b[:, 0:1] * c[:, 0] + b[:, 1:2] * c[:, 1] + b[:, 2:3] * c[:, 2]


def oracle_hit_points(cam, orc):
    """world points [H*W,3] fp64 of mesh_raster_common.oracle's hits (NaN where it hit nothing): o + depth * d / |d| along the pixel's ray"""
    H, W = cam["H"], cam["W"]
    c2w = cam["c2w"].astype(np.float64)
    i, j = np.arange(W, dtype=np.float64) + 0.5, np.arange(H, dtype=np.float64) + 0.5
    dcam = np.stack([np.tile(-(i - cam["cx"]) / cam["fx"], H), np.repeat((j - cam["cy"]) / cam["fy"], W), -np.ones(H * W)], -1)
    d = dcam @ c2w[:, :3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    depth = orc["depth"].reshape(-1)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(depth)[:, None], c2w[:, 3][None] + np.where(np.isfinite(depth), depth, 0.0)[:, None] * d, np.nan)


def probe_barycentrics(m, seed):
    """[m + 13, 3] fp32 barycentric probes: m random interior points, the three corners, the three edge midpoints, edge points, and points an ulp outside the triangle
    (b1 + b2 = 1 + ulp, a weight just below 0, a weight just above 1) — what the rasteriser's rounded weights can be"""
    rng = np.random.default_rng(seed)
    r = rng.random((m, 2))
    flip = r.sum(1) > 1
    r[flip] = 1.0 - r[flip]
    pts = [[1 - a - b, a, b] for a, b in r]
    pts += [[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5], [.25, .75, 0], [0, .125, .875]]
    b = np.asarray(pts, dtype=F32)
    up = np.nextafter(F32(0.5), F32(1.0))
    extra = np.asarray([[0.0, 0.5, up], [0.0, up, 0.5], [-1e-7, np.nextafter(F32(1.0), F32(2.0)), 0.0], [0.0, -1e-7, np.nextafter(F32(1.0), F32(2.0))],
                        [1.0, -1e-7, 1e-7]], dtype=F32)
    return np.concatenate([b, extra])


def small_mesh(F, seed=3):
    """F triangles over F + 2 random vertices of order 1 (a strip): (verts f32, faces i32)"""
    rng = np.random.default_rng(seed)
    v = (rng.random((F + 2, 3)) * 2.0 - 1.0).astype(F32)
    f = np.asarray([[k, k + 1, k + 2] if k % 2 == 0 else [k + 1, k, k + 2] for k in range(F)], dtype=np.int32).reshape(-1, 3)
    return v, f
