"""Shared by tests/test_ngp_geom_host.py and tests/test_gpu_ngp_geom.py: references for the density gradient and the density lattice of an Instant-NGP field
(include/tvr_ngp.h, "geometry").

  * density_gradient_ref   value and gradient of the raw density from the header's definition: cells and fp32 fractions from hash_geometry (so kernel and reference
                           agree on the cell by construction), the encoding's Jacobian as the sum over corners of (weight with factor k replaced by +-1) * value
                           times the level's scale, the network part by torch autograd with respect to the encoding.  Everything in `dtype`: fp64 is the reference,
                           the same code in fp32 the yardstick.
  * relu_margin_ok / scaled_error / cell_and_pattern   the measures the tests share.
  * occupied_np            float32 numpy restatement of tvr_ngp_density_grid's cell lookup.
  * sphere_scene           an NGP scene whose surface is known: raw = k * (trilinear interpolant of R - |p - c| on the nodes of the finest dense level).
"""
import numpy as np
import torch

from ngp_train_common import corner_weights, hash_geometry, level_table, params_t  # noqa: F401  (corner_weights: re-exported for the tests)

F = np.float32
MARGIN = 1e-5                       # a hidden unit with |h_j| < MARGIN * sum_k |W0_jk| |enc_k| may legitimately take the other ReLU branch in an fp32-class evaluation
MARGIN_CAP = 0.01                   # at most this share of the points may fail the margin


def encoding_and_jacobian(grid, levels, pos, dtype):
    """(enc [n,32], J [n,32,3] = d enc / d p) in `dtype` from the fp32 cells and fractions; `grid` is the flat table in `dtype`."""
    ent, frac, _ = hash_geometry(levels, pos)
    f = frac.to(dtype)                                                        # [n,L,3]
    tab = grid.view(-1, 2)
    scale = torch.tensor([float(s) for _, _, s, _, _ in level_table(levels)], dtype=dtype)
    n, L = ent.shape[:2]
    enc = torch.zeros(n, L, 2, dtype=dtype)
    J = torch.zeros(n, L, 2, 3, dtype=dtype)
    for idx in range(8):
        v = tab[ent[:, :, idx]]                                               # [n,L,2]
        fac = [f[..., k] if idx & (1 << k) else 1 - f[..., k] for k in range(3)]
        enc = enc + ((fac[0] * fac[1]) * fac[2])[..., None] * v
        for k in range(3):
            dw = torch.ones_like(fac[0]) if idx & (1 << k) else -torch.ones_like(fac[0])
            for m in range(3):
                if m != k:
                    dw = dw * fac[m]
            J[..., k] = J[..., k] + dw[..., None] * v
    J = J * scale[None, :, None, None]
    return enc.reshape(n, 2 * L), J.reshape(n, 2 * L, 3)


def density_gradient_ref(arrs, levels, pos, dtype):
    """pos [n,3] (fp32 numpy or torch) -> dict of numpy fp64 arrays: raw [n], grad [n,3], h [n,64], margin_ok [n] (relu_margin_ok), S [n] (the error scale
    sum_k |g_enc,k| |d enc_k / d p|_1), g_enc [n,32], J [n,32,3]."""
    pos = torch.as_tensor(np.ascontiguousarray(np.asarray(pos, np.float32)))
    p = params_t(arrs, dtype, requires_grad=False)
    enc, J = encoding_and_jacobian(p["grid"], levels, pos, dtype)
    enc = enc.detach().requires_grad_(True)
    W0, W1 = p["density_mlp.0.weight"], p["density_mlp.2.weight"]
    h = enc @ W0.t()
    raw = torch.relu(h) @ W1[0]
    (g_enc,) = torch.autograd.grad(raw.sum(), enc)
    grad = (g_enc[:, :, None] * J).sum(1)
    margin_ok = ~(h.detach().abs() < MARGIN * (enc.detach().abs() @ W0.abs().t())).any(1)
    S = (g_enc.abs() * J.abs().sum(-1)).sum(1)
    out = dict(raw=raw, grad=grad, h=h, margin_ok=margin_ok, S=S, g_enc=g_enc, J=J)
    return {k: v.detach().double().numpy() for k, v in out.items()}


GRADIENT_CASES = [(4, 4099, 1.0), (16, 1031, 1.0), (16, 1031, 4.0)]            # (aabb_scale, points, factor on the hash table's values)


def gradient_scene(ngp_scene, aabb_scale, gain=1.0):
    """(levels, arrays): the shared conftest scene at its own aabb_scale, else synthetic.make_ngp_scene_arrays on grid_levels(aabb_scale); the table times `gain`."""
    from jittor_myc_nerfs_amd import synthetic
    from oracle import ngp_oracle as N
    levels, arrs = ngp_scene
    if aabb_scale != int(round((float(levels["scale"][-1]) + 1.0) / 2048.0)):
        levels = N.grid_levels(aabb_scale)
        arrs = synthetic.make_ngp_scene_arrays(levels["offsets"])
    if gain != 1.0:
        arrs = dict(arrs, grid=(np.asarray(arrs["grid"], F) * F(gain)).astype(F))
    return levels, arrs


def relu_margin_ok(ref):
    """bool [n]: no hidden unit has |h_j| < MARGIN * sum_k |W0_jk| |enc_k| (computed by density_gradient_ref in its dtype; a unit without weights never fails)."""
    return ref["margin_ok"] > 0.5


def scaled_error(got, ref, keep):
    """max over the kept points of max_k |got - ref|_k / S (0.0 when nothing is kept)."""
    if not keep.any():
        return 0.0
    e = np.abs(np.asarray(got, np.float64)[keep] - ref["grad"][keep]).max(1) / np.maximum(ref["S"][keep], 1e-300)
    return float(e.max())


def cell_and_pattern(arrs, levels, pos):
    """(cells [n,L,3] int64, pattern [n,64] bool = h > 0) of the fp64 reference: what a finite-difference check needs to stay inside one smooth piece."""
    pos = torch.as_tensor(np.ascontiguousarray(np.asarray(pos, np.float32)))
    _, _, cells = hash_geometry(levels, pos)
    return cells.numpy(), density_gradient_ref(arrs, levels, pos, torch.float64)["h"] > 0


def sample_positions(n, seed=3, edges=True):
    """n positions uniform in [0.05, 0.95]^3 (fp32), then the eight cube corners and points with coordinates at exactly 0 and 1."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, size=(n, 3)).astype(F)
    if not edges:
        return p
    corners = np.array([[(i >> k) & 1 for k in range(3)] for i in range(8)], F)
    extra = np.array([[0.0, 0.3, 0.7], [0.4, 1.0, 0.2], [0.6, 0.1, 0.0], [1.0, 0.5, 0.5], [0.5, 0.0, 1.0]], F)
    return np.concatenate([p, corners, extra]).astype(F)


# ------------------------------------------------------------------------------------------------------------------ the lattice
def lattice_points(dims, origin, spacing):
    """[nx,ny,nz,3] fp32: fma(i, spacing, origin) per axis — the product of an fp32 and a small integer is exact in fp64 and the sum is rounded once to fp32 as long
    as it is exact in fp64, which holds for the magnitudes used here (asserted)."""
    axes = []
    for k in range(3):
        s, o = float(F(spacing[k])), float(F(origin[k]))
        # both terms are multiples of 2^-40 and the sum stays below 4: it has at most 42 significant bits, so the fp64 sum is exact and the cast rounds once
        assert all(v * 2.0 ** 40 == round(v * 2.0 ** 40) for v in (s, o)) and abs(o) + dims[k] * abs(s) < 4, "the fp64 sum must be exact for one rounding to be an fma"
        exact = np.arange(dims[k], dtype=np.float64) * s + o
        axes.append(exact.astype(F))
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    return np.stack([X, Y, Z], -1)


def in_cube(p):
    return ((p >= 0) & (p <= 1)).all(-1)


def occupied_np(p, bitfield, aabb_lo, aabb_hi):
    """bool [...]: tvr_ngp_density_grid's cell lookup for unit-cube points p [...,3] fp32 (include/tvr_ngp.h), every operation in float32."""
    from ngp_grid_common import morton3d
    p = np.asarray(p, F)
    ext = F(aabb_hi) - F(aabb_lo)
    x = (p * ext + F(aabb_lo)).astype(F)
    m = np.abs(x - F(0.5)).max(-1)
    _, e = np.frexp(m)
    mip = np.clip(e + 1, 0, 4).astype(np.int32)
    s = np.ldexp(F(1), -mip).astype(F)
    c = ((((x - F(0.5)) * s[..., None]).astype(F) + F(0.5)) * F(128)).astype(F)
    c = np.clip(c.astype(np.int32), 0, 127).astype(np.uint32)
    idx = morton3d(c[..., 0], c[..., 1], c[..., 2]).astype(np.int64)
    byte = np.asarray(bitfield, np.uint8)[idx // 8 + (128 ** 3 // 8) * mip.astype(np.int64)]
    return (byte >> (idx % 8).astype(np.uint8)) & 1 != 0


# ------------------------------------------------------------------------------------------------------------------ a scene with a known surface
def sphere_level(levels):
    """(level, scale, res) of the finest dense level."""
    tab = level_table(levels)
    l = max(i for i, t in enumerate(tab) if not t[4])
    return l, float(tab[l][2]), tab[l][3]


def sphere_scene(levels, R, k, seed=11, occupancy_margin=0.1):
    """Arrays of an NGP scene whose density's zero level is (nearly) the sphere |p - c| = R, c = (0.5, 0.5, 0.5), unit-cube units.  The grid is zero except feature 0
    of the finest dense level, whose node x holds R - |(x - 0.5) / scale - c|; density_mlp.0 rows 0 and 1 are +1 and -1 on that feature, density_mlp.2 row 0 is
    (k, -k, 0, ...): raw = k * (the trilinear interpolant of a 1-Lipschitz function).  Colour weights come from the seeded generator.  density_grid marks, in every
    cascade, the cells within R + occupancy_margin (plus a cell diagonal) of c — a solid ball, so that the empty value appears outside the surface only."""
    from ngp_grid_common import cell_xyz, CELLS, G
    l, scale, res = sphere_level(levels)
    off = int(levels["offsets"][l])
    grid = np.zeros(int(levels["offsets"][-1]) * 2, F)
    ax = (np.arange(res, dtype=np.float64) - 0.5) / scale - 0.5
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    val = R - np.sqrt(X * X + Y * Y + Z * Z)                                  # [x,y,z]
    ix, iy, iz = np.meshgrid(np.arange(res), np.arange(res), np.arange(res), indexing="ij")
    grid[2 * (off + (ix + iy * res + iz * res * res).reshape(-1))] = val.reshape(-1).astype(F)
    rng = np.random.default_rng(seed)

    def U(n_out, n_in, gain=1.0):
        b = np.sqrt(6.0 / (n_in + n_out))
        return (rng.uniform(-b, b, size=(n_out, n_in)) * gain).astype(F)
    out = {"grid": grid, "rgb_mlp.0.weight": U(64, 32, 0.25), "rgb_mlp.2.weight": U(64, 64), "rgb_mlp.4.weight": U(3, 64, 4.0)}
    w0 = np.zeros((64, 32), F)
    w0[0, 2 * l], w0[1, 2 * l] = 1.0, -1.0
    w1 = np.zeros((16, 64), F)
    w1[0, 0], w1[0, 1] = k, -k
    out["density_mlp.0.weight"], out["density_mlp.2.weight"] = w0, w1
    n_levels = len(levels["scale"])
    aabb_scale = int(round((float(levels["scale"][n_levels - 1]) + 1.0) / 2048.0))
    lo, ext = 0.5 - aabb_scale / 2, float(aabb_scale)
    dg = np.zeros(5 * CELLS, F)
    xyz = np.stack(cell_xyz(np.arange(CELLS, dtype=np.uint32)), 1).astype(np.float64)
    for c in range(5):
        size = float(1 << c)
        centre_unit = (((xyz + 0.5) / G - 0.5) * size + 0.5 - lo) / ext
        d = np.sqrt(((centre_unit - 0.5) ** 2).sum(1))
        dg[c * CELLS:(c + 1) * CELLS] = (d <= R + occupancy_margin + np.sqrt(3.0) * size / G / ext).astype(F)
    out["density_grid"] = dg
    return out
