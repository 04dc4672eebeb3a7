"""Numpy restatement of the baked appearance volume (include/tvr.h, BAKED APPEARANCE VOLUME), shared by tests/test_appearance_volume_host.py and
tests/test_gpu_appearance_volume.py: the record's channel order, the corner values, the trilinear interpolation and the factored features they must equal."""
import numpy as np

RECORD_FLOATS = 32
APP_DIM = 27


def slot_row(slot):
    """Feature row held by slot 8 g + j of a record: 4 g + j for j < 4, 16 + 4 g + (j - 4) for j >= 4 (rows 27..31 hold 0)."""
    g, j = slot >> 3, slot & 7
    return 4 * g + j if j < 4 else 16 + 4 * g + (j - 4)


SLOT_OF_ROW = {slot_row(s): s for s in range(RECORD_FLOATS)}


def factors(arrs, dtype=np.float64):
    """(planes [C, ., .], lines [C, L]) x 3 of a scene's appearance factors and basis_mat [27, 144]."""
    P = [np.asarray(arrs[f"app_plane.{i}"])[0].astype(dtype) for i in range(3)]
    Ln = [np.asarray(arrs[f"app_line.{i}"])[0, :, :, 0].astype(dtype) for i in range(3)]
    return P, Ln, np.asarray(arrs["basis_mat"]).astype(dtype)


def _rtz16(w):
    """fp16 of w rounded toward zero (v_cvt_pkrtz_f16_f32)."""
    h = w.astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(w.astype(np.float64))
    h[over] = np.nextafter(h[over], np.float16(0))
    return h


def basis_as_packed(basis32):
    """basis_mat as the render kernel's matrix operands hold it and the bake reads it: fp16 hi + fp16 lo, both truncated (tvr_mfma.h split2), summed in fp64."""
    b = np.asarray(basis32, np.float32)
    hi = _rtz16(b)
    lo = _rtz16(b - hi.astype(np.float32))             # (the residual is exact in fp32)
    return hi.astype(np.float64) + lo.astype(np.float64)


def corner_features(arrs, basis=None):
    """F[z, y, x, r] in fp64 on the grid vertices: sum_c B[r, c] P0[c,y,x] L0[c,z] + B[r, 48+c] P1[c,z,x] L1[c,y] + B[r, 96+c] P2[c,z,y] L2[c,x]
    (matMode [[0,1],[0,2],[1,2]], vecMode [2,1,0]; basis_mat's columns are the planes' channels one plane after the other)."""
    P, Ln, B = factors(arrs)
    if basis is not None:
        B = np.asarray(basis, np.float64)
    n = [p.shape[0] for p in P]
    o = np.concatenate([[0], np.cumsum(n)])
    return (np.einsum("rc,cyx,cz->zyxr", B[:, o[0]:o[1]], P[0], Ln[0]) + np.einsum("rc,czx,cy->zyxr", B[:, o[1]:o[2]], P[1], Ln[1])
            + np.einsum("rc,czy,cx->zyxr", B[:, o[2]:o[3]], P[2], Ln[2]))


def corner_magnitudes(arrs, basis):
    """sum_k |B[r, k] h_k| per vertex and row: the scale of the fp64 summation error."""
    a = {k: np.abs(np.asarray(v)) for k, v in arrs.items() if k.startswith(("app_plane", "app_line"))}
    a["basis_mat"] = np.abs(basis)
    return corner_features(a, np.abs(basis))


def records(F):
    """Corner values [gz, gy, gx, 27] -> the volume [gz+1, gy+1, gx+1, 32]: x fastest, a zero padding layer on every axis, slots in slot_row order, slots of rows >= 27 zero."""
    gz, gy, gx, _ = F.shape
    vol = np.zeros((gz + 1, gy + 1, gx + 1, RECORD_FLOATS), F.dtype)
    for s in range(RECORD_FLOATS):
        if slot_row(s) < APP_DIM:
            vol[:gz, :gy, :gx, s] = F[..., slot_row(s)]
    return vol


def rows_of(vol):
    """[..., 32] records -> [..., 27] features in row order."""
    return vol[..., [SLOT_OF_ROW[r] for r in range(APP_DIM)]]


def cells(xyz_norm, grid, dtype):
    """Cell index and weight per axis as the kernels form them: f = ((c + 1) / 2) * (g - 1), floor, f - floor — an upper face is cell g - 1 with weight 0."""
    c = np.asarray(xyz_norm, dtype)
    f = ((c + dtype(1)) / dtype(2)) * (np.asarray(grid, dtype) - dtype(1))
    f0 = np.floor(f)
    return f0.astype(np.int64), (f - f0).astype(dtype)


def trilinear(vol, xyz_norm, grid, dtype=np.float64):
    """Seven lerps a + w (b - a) per channel — x on four rows, y on two layers, z — of the eight corner records of every position; vol [gz+1, gy+1, gx+1, C]."""
    i, w = cells(xyz_norm, grid, dtype)
    x, y, z = i[:, 0], i[:, 1], i[:, 2]
    v = vol.astype(dtype)
    lerp = lambda t, a, b: a + t[:, None] * (b - a)
    layer = lambda zz: lerp(w[:, 1], lerp(w[:, 0], v[zz, y, x], v[zz, y, x + 1]), lerp(w[:, 0], v[zz, y + 1, x], v[zz, y + 1, x + 1]))
    return lerp(w[:, 2], layer(z), layer(z + 1))


def factored_features(arrs, xyz_norm, grid, dtype=np.float64):
    """basis_mat . cat_i(bilinear(plane_i) * linear(line_i)) at the positions, in `dtype` (models/tensoRF.py compute_appfeature with align_corners=True and zero padding)."""
    P, Ln, B = factors(arrs, dtype)
    i, w = cells(xyz_norm, grid, dtype)
    pad2 = lambda p: np.pad(p, ((0, 0), (0, 1), (0, 1)))
    pad1 = lambda l: np.pad(l, ((0, 0), (0, 1)))
    h = []
    for p, (ax, bx), vx in zip(range(3), ((0, 1), (0, 2), (1, 2)), (2, 1, 0)):
        pl, ln = pad2(P[p]), pad1(Ln[p])
        x0, y0, l0, wx, wy, wl = i[:, ax], i[:, bx], i[:, vx], w[:, ax], w[:, bx], w[:, vx]
        plane = ((1 - wx) * (1 - wy) * pl[:, y0, x0] + wx * (1 - wy) * pl[:, y0, x0 + 1] + (1 - wx) * wy * pl[:, y0 + 1, x0] + wx * wy * pl[:, y0 + 1, x0 + 1])
        line = (1 - wl) * ln[:, l0] + wl * ln[:, l0 + 1]
        h.append((plane * line).T)
    return np.concatenate(h, axis=1) @ B.T
