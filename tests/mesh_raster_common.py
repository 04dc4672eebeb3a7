"""Shared by tests/test_mesh_raster_host.py and tests/test_gpu_mesh_raster.py: the two references of the z-buffer rasteriser (include/tvr.h tvr_mesh_raster) and the
fixtures both are run on.

THE DEFINITION (restated from include/tvr.h; `restate` below follows it operation by operation in numpy fp32, every operation rounded on its own):
  camera    c2w 3x4 row-major = [R | o]; pixel p = j * W + i has dir = (-(((i + .5) - cx) / fx), ((j + .5) - cy) / fy, -1); a vertex goes to camera space as
            q = R^T (v - o): d = v - o, q_k = (d_0 R[0][k] + d_1 R[1][k]) + d_2 R[2][k]
  dot       a . b = (a.x b.x + a.y b.y) + a.z b.z;  cross  a x b = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x)
  coverage  n_0 = q1 x q2, n_1 = q2 x q0, n_2 = q0 x q1; det = q0 . n_0; sg = sign(det); det == 0 / NaN or a non-finite q: skipped and counted.  E_k = sg (dir . n_k);
            edge k runs from corner (k+1)%3 to corner (k+2)%3; covered iff for every k: E_k > 0, or E_k == 0 and owner_k = (index at start < index at end) XOR (sg < 0).
            cull drops det > 0.
  depth     pn = (q1 - q0) x (q2 - q0); s = (pn . q0) / (dir . pn); depth = s * sqrt(dir . dir); a covered pixel counts only if depth is finite and > near
  box       z_k = -q_k.z; all z_k <= 0: no pixel; some z_k <= 0: the whole image; else u_k = cx - fx (q_k.x / z_k), w_k = cy + fy (q_k.y / z_k) and
            i in max(ceil(min u - 1.5), 0) .. min(floor(max u + .5), W - 1), j likewise from w and H; a triangle is offered the pixels of its box only
  result    per pixel the covered triangle with the smallest depth, ties to the smallest index: depth (+inf), tri (-1), bary b_k = E_k / ((E_0 + E_1) + E_2) (zeros),
            attr_out = (b_0 a[v0] + b_1 a[v1]) + b_2 a[v2] (zeros); counts = {pixels hit, triangles skipped, triangles that covered no pixel, large path}

THE ORACLE (`oracle`) shares none of that formulation: brute-force Moeller-Trumbore ray casting in fp64 of the rays rays.get_rays makes from the same camera, nearest hit.
A pixel is AMBIGUOUS for it when some triangle that it hits, or misses by less than MARGIN of |E_0| + |E_1| + |E_2|, has its smallest |E_k| below that margin (in
barycentric terms: every b_k > -MARGIN and min |b_k| < MARGIN); such pixels are left out of mask and index comparisons."""
import math

import numpy as np

MARGIN = 1e-4
F32 = np.float32


# ---- cameras ----------------------------------------------------------------------------------------------------------------------------------------------------------
def camera(c2w, H, W, focal, center=None, near=0.0, cull=False):
    fx, fy = (focal, focal) if np.isscalar(focal) else focal
    cx, cy = (W / 2, H / 2) if center is None else center
    return dict(c2w=np.asarray(c2w, dtype=np.float32)[:3, :4].copy(), H=int(H), W=int(W), fx=float(F32(fx)), fy=float(F32(fy)), cx=float(F32(cx)), cy=float(F32(cy)),
                near=float(F32(near)), cull=bool(cull))


def sphere_camera(H, W, pose_index=1, distance=4.0, fill=0.42, **kw):
    """A rays.sphere_poses camera `distance` away from the origin whose unit sphere shows with a radius of `fill` x min(H, W) pixels."""
    from jittor_myc_nerfs_amd import rays as R
    pose = R.sphere_poses(8, distance)[pose_index] @ R.BLENDER2OPENCV
    focal = fill * min(H, W) / math.tan(math.asin(1.0 / distance))
    return camera(pose.astype(np.float32), H, W, focal, **kw)


def pixel_dirs32(cam):
    """dir per pixel, fp32, [H*W] each of dx, dy (dz = -1): rays.get_ray_directions' arithmetic."""
    i = np.arange(cam["W"], dtype=np.float32) + F32(0.5)
    j = np.arange(cam["H"], dtype=np.float32) + F32(0.5)
    dx = -((i - F32(cam["cx"])) / F32(cam["fx"]))
    dy = (j - F32(cam["cy"])) / F32(cam["fy"])
    return np.tile(dx, cam["H"]), np.repeat(dy, cam["W"])


# ---- (b) the definition in numpy fp32 ---------------------------------------------------------------------------------------------------------------------------------------
def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _cross(ax, ay, az, bx, by, bz):
    return ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx


def setup32(verts, faces, cam):
    """Per-triangle quantities of the definition, fp32: dict of n [3][3][F], pn, pq, sg, own [3][F] bool, state (0 ok / 1 skipped / 2 no pixel), box i0 i1 j0 j1."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    Rm, o = cam["c2w"][:, :3], cam["c2w"][:, 3]
    q = []
    with np.errstate(all="ignore"):
        for c in range(3):
            d = v[f[:, c]] - o[None, :]
            q.append([(d[:, 0] * Rm[0, k] + d[:, 1] * Rm[1, k]) + d[:, 2] * Rm[2, k] for k in range(3)])
        (q0, q1, q2) = q
        n = [_cross(*q1, *q2), _cross(*q2, *q0), _cross(*q0, *q1)]
        det = _dot(*q0, *n[0])
        finite = np.ones(len(f), bool)
        for c in range(3):
            for k in range(3):
                finite &= np.isfinite(q[c][k])
        ok = finite & ((det > 0) | (det < 0))
        sg = np.where(det > 0, F32(1), F32(-1)).astype(np.float32)
        neg = det < 0
        own = [(f[:, 1] < f[:, 2]) != neg, (f[:, 2] < f[:, 0]) != neg, (f[:, 0] < f[:, 1]) != neg]
        a = [q1[k] - q0[k] for k in range(3)]
        b = [q2[k] - q0[k] for k in range(3)]
        pn = _cross(*a, *b)
        pq = _dot(*pn, *q0)
        state = np.where(ok, 0, 1)
        nopix = ok & (cam["cull"] & (det > 0))
        z = [-q0[2], -q1[2], -q2[2]]
        behind = [~(zk > 0) for zk in z]
        nopix |= ok & behind[0] & behind[1] & behind[2]
        anyb = behind[0] | behind[1] | behind[2]
        fx, fy, cx, cy = F32(cam["fx"]), F32(cam["fy"]), F32(cam["cx"]), F32(cam["cy"])
        u = [cx - fx * (q[c][0] / z[c]) for c in range(3)]
        w = [cy + fy * (q[c][1] / z[c]) for c in range(3)]
        il = np.maximum(np.ceil(np.minimum(np.minimum(u[0], u[1]), u[2]) - F32(1.5)), F32(0))
        ih = np.minimum(np.floor(np.maximum(np.maximum(u[0], u[1]), u[2]) + F32(0.5)), F32(cam["W"] - 1))
        jl = np.maximum(np.ceil(np.minimum(np.minimum(w[0], w[1]), w[2]) - F32(1.5)), F32(0))
        jh = np.minimum(np.floor(np.maximum(np.maximum(w[0], w[1]), w[2]) + F32(0.5)), F32(cam["H"] - 1))
        il, jl = np.where(anyb, F32(0), il), np.where(anyb, F32(0), jl)
        ih, jh = np.where(anyb, F32(cam["W"] - 1), ih), np.where(anyb, F32(cam["H"] - 1), jh)
        nopix |= ok & ~((il <= ih) & (jl <= jh))
        state = np.where(nopix, 2, state)
        good = state == 0
        box = [np.where(good, x, y).astype(np.int64) for x, y in ((il, 0), (ih, -1), (jl, 0), (jh, -1))]
    return dict(n=n, pn=pn, pq=pq, sg=sg, own=own, state=state, i0=box[0], i1=box[1], j0=box[2], j1=box[3], faces=f)


def box_pixels(S):
    """pixels in each triangle's box (0 where it has none)"""
    return np.where(S["state"] == 0, (S["i1"] - S["i0"] + 1) * (S["j1"] - S["j0"] + 1), 0)


def restate(verts, faces, cam, attr=None, chunk=512):
    """The definition, fp32 -> dict(depth [H,W] f32, tri [H,W] i32, bary [H,W,3] f32, attr [H,W,A] or None, counts [hit, skipped, no pixel])."""
    H, W = cam["H"], cam["W"]
    S = setup32(verts, faces, cam)
    F = len(S["faces"])
    dx, dy = pixel_dirs32(cam)
    dz = np.full_like(dx, -1.0)
    pi, pj = np.tile(np.arange(W), H), np.repeat(np.arange(H), W)
    best = np.full(H * W, np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    covered_any = np.zeros(F, bool)
    dd = np.sqrt(_dot(dx, dy, dz, dx, dy, dz))
    near = F32(cam["near"])

    def edge(t, k):
        return S["sg"][t][None, :] * _dot(dx[:, None], dy[:, None], dz[:, None], S["n"][k][0][t][None, :], S["n"][k][1][t][None, :], S["n"][k][2][t][None, :])

    with np.errstate(all="ignore"):
        for t0 in range(0, F, chunk):
            t = np.arange(t0, min(F, t0 + chunk))
            inside = np.ones((H * W, len(t)), bool)
            for k in range(3):
                E = edge(t, k)
                inside &= (E > 0) | ((E == 0) & S["own"][k][t][None, :])
            s = S["pq"][t][None, :] / _dot(dx[:, None], dy[:, None], dz[:, None], S["pn"][0][t][None, :], S["pn"][1][t][None, :], S["pn"][2][t][None, :])
            depth = (s * dd[:, None]).astype(np.float32)
            inbox = (S["state"][t] == 0)[None, :] & (pi[:, None] >= S["i0"][t][None, :]) & (pi[:, None] <= S["i1"][t][None, :]) & \
                    (pj[:, None] >= S["j0"][t][None, :]) & (pj[:, None] <= S["j1"][t][None, :])
            cov = inside & inbox & np.isfinite(depth) & (depth > near)
            covered_any[t] = cov.any(0)
            key = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | t.astype(np.uint64)[None, :]
            key = np.where(cov, key, np.uint64(0xFFFFFFFFFFFFFFFF))
            best = np.minimum(best, key.min(1))
        hit = best != np.uint64(0xFFFFFFFFFFFFFFFF)
        tri = np.where(hit, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
        depth = np.where(hit, (best >> np.uint64(32)).astype(np.uint32).view(np.float32), F32(np.inf)).astype(np.float32)
        tw = np.maximum(tri, 0)
        E = [S["sg"][tw] * _dot(dx, dy, dz, S["n"][k][0][tw], S["n"][k][1][tw], S["n"][k][2][tw]) for k in range(3)] if F else [np.zeros_like(dx)] * 3
        tot = (E[0] + E[1]) + E[2]
        bary = np.stack([np.where(hit, E[k] / tot, F32(0)) for k in range(3)], -1).astype(np.float32)
        out = None
        if attr is not None:
            a = np.asarray(attr, dtype=np.float32)
            fw = S["faces"][tw] if F else np.zeros((H * W, 3), np.int64)
            out = (bary[:, 0:1] * a[fw[:, 0]] + bary[:, 1:2] * a[fw[:, 1]]) + bary[:, 2:3] * a[fw[:, 2]]
            out = np.where(hit[:, None], out, F32(0)).astype(np.float32).reshape(H, W, -1)
    counts = [int(hit.sum()), int((S["state"] == 1).sum()), int(((S["state"] == 2) | ((S["state"] == 0) & ~covered_any)).sum())]
    return dict(depth=depth.reshape(H, W), tri=tri.astype(np.int32).reshape(H, W), bary=bary.reshape(H, W, 3), attr=out, counts=counts, setup=S)


# ---- (a) the fp64 oracle ----------------------------------------------------------------------------------------------------------------------------------------------------
def oracle(verts, faces, cam, chunk=256):
    """Moeller-Trumbore, fp64 -> dict(depth [H,W] f64 (+inf), tri [H,W] (-1), ambiguous [H,W] bool, tie [H,W] bool).  tie: the two nearest hits of DIFFERENT triangles
    lie within 1e-5 relative of each other — closer than fp32 depths (4e-6 relative at a camera distance of 4) can order; only tests with crossing or coincident
    triangles have such pixels."""
    H, W = cam["H"], cam["W"]
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    c2w = cam["c2w"].astype(np.float64)
    i = np.arange(W, dtype=np.float64) + 0.5
    j = np.arange(H, dtype=np.float64) + 0.5
    dcam = np.stack([np.tile(-(i - cam["cx"]) / cam["fx"], H), np.repeat((j - cam["cy"]) / cam["fy"], W), -np.ones(H * W)], -1)
    d = dcam @ c2w[:, :3].T                                    # rays.get_rays: rays_d = directions @ R^T
    o = c2w[:, 3]
    dn = np.linalg.norm(d, axis=1)
    depth = np.full(H * W, np.inf)
    second = np.full(H * W, np.inf)
    tri = np.full(H * W, -1, np.int64)
    amb = np.zeros(H * W, bool)
    ok = np.isfinite(v[f]).all((1, 2)) if len(f) else np.zeros(0, bool)
    v0 = np.where(ok[:, None], v[f[:, 0]], 0.0) if len(f) else np.zeros((0, 3))
    e1 = np.where(ok[:, None], v[f[:, 1]], 0.0) - v0 if len(f) else np.zeros((0, 3))
    e2 = np.where(ok[:, None], v[f[:, 2]], 0.0) - v0 if len(f) else np.zeros((0, 3))
    with np.errstate(all="ignore"):
        for p0 in range(0, H * W, chunk):
            if not len(f):
                break
            D = d[p0:p0 + chunk][:, None, :]                      # [P,1,3]
            pv = np.cross(D, e2[None, :, :])
            a = (e1[None] * pv).sum(-1)                           # [P,F]
            tv = (o - v0)[None]
            u = (tv * pv).sum(-1) / a
            qv = np.cross(tv, e1[None])
            w = (D * qv).sum(-1) / a
            t = (e2[None] * qv).sum(-1) / a
            b0 = 1.0 - u - w
            dist = t * dn[p0:p0 + chunk][:, None]
            valid = ok[None, :] & np.isfinite(a) & (a != 0) & np.isfinite(dist) & (dist > cam["near"])
            if cam["cull"]:
                valid &= a > 0                                    # a = -d . (e1 x e2): the outward side faces the camera
            bmin = np.minimum(np.minimum(b0, u), w)
            babs = np.minimum(np.minimum(np.abs(b0), np.abs(u)), np.abs(w))
            amb[p0:p0 + chunk] = (valid & (bmin > -MARGIN) & (babs < MARGIN)).any(1)
            dh = np.where(valid & (bmin >= 0), dist, np.inf)
            k = dh.argmin(1)
            rows = np.arange(dh.shape[0])
            depth[p0:p0 + chunk] = dh[rows, k]
            tri[p0:p0 + chunk] = np.where(np.isfinite(dh[rows, k]), k, -1)
            dh[rows, k] = np.inf
            second[p0:p0 + chunk] = dh.min(1)
    with np.errstate(all="ignore"):
        tie = np.isfinite(second) & (second - depth <= 1e-5 * depth)
    return dict(depth=depth.reshape(H, W), tri=tri.reshape(H, W), ambiguous=amb.reshape(H, W), tie=tie.reshape(H, W))


def compare_with_oracle(res_depth, res_tri, orc):
    """-> dict(mask_diff, tri_diff: both over every pixel the oracle does not call ambiguous — nothing else is left out; ties: unambiguous pixels whose two nearest hits
    tie (see `oracle`); tri_diff_outside_ties: tri_diff without them; ambiguous, hit, max_rel_depth over pixels both hit with the same triangle).
    THE ONE EXCEPTION to "only ambiguous pixels are left out": a test whose mesh has triangles that CROSS each other compares tri_diff_outside_ties and says so —
    along the crossing line two depths agree to more digits than fp32 holds, which the ambiguity rule (about edges) does not cover.  Every other fixture asserts
    ties == 0 and the plain tri_diff."""
    hit_o, hit_r = orc["tri"] >= 0, res_tri >= 0
    clear = ~orc["ambiguous"]
    both = hit_o & hit_r & clear & (orc["tri"] == res_tri)
    rel = np.abs(res_depth.astype(np.float64)[both] - orc["depth"][both]) / orc["depth"][both]
    diff = (orc["tri"] != res_tri) & clear
    return dict(mask_diff=int(((hit_o != hit_r) & clear).sum()), tri_diff=int(diff.sum()), tri_diff_outside_ties=int((diff & ~orc["tie"]).sum()),
                ties=int((orc["tie"] & clear).sum()), ambiguous=int((orc["ambiguous"] & (hit_o | hit_r)).sum()), hit=int(hit_o.sum()),
                max_rel_depth=float(rel.max()) if rel.size else 0.0)


def ulp_diff(a, b):
    """largest distance in units of the last place between two fp32 arrays (same-sign finite values; equal infinities count 0)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.where(same, 0, np.abs(ia - ib))
    return int(d.max()) if d.size else 0


# ---- (c) fixtures -------------------------------------------------------------------------------------------------------------------------------------------------------------
def rotation(seed):
    """a proper random rotation (QR of a seeded Gaussian matrix)"""
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def latlong_sphere(stacks, slices, radius=1.0, seed=0):
    """Latitude-longitude sphere with 2 * slices * (stacks - 1) outward-facing triangles under a seeded rotation: (verts [V,3] f32, faces [F,3] i32)."""
    v = [[0.0, 0.0, radius]]
    for s in range(1, stacks):
        th = math.pi * s / stacks
        for l in range(slices):
            ph = 2 * math.pi * l / slices
            v.append([radius * math.sin(th) * math.cos(ph), radius * math.sin(th) * math.sin(ph), radius * math.cos(th)])
    v.append([0.0, 0.0, -radius])
    ring = lambda s, l: 1 + (s - 1) * slices + l % slices
    f = []
    for l in range(slices):
        f.append([0, ring(1, l), ring(1, l + 1)])
        for s in range(1, stacks - 1):
            f.append([ring(s, l), ring(s + 1, l), ring(s + 1, l + 1)])
            f.append([ring(s, l), ring(s + 1, l + 1), ring(s, l + 1)])
        f.append([len(v) - 1, ring(stacks - 1, l + 1), ring(stacks - 1, l)])
    v = np.asarray(v) @ rotation(seed).T
    return v.astype(np.float32), np.asarray(f, dtype=np.int32)


SPHERES = {"sphere960": dict(stacks=16, slices=32, seed=11, H=48, W=64), "sphere6240": dict(stacks=40, slices=80, seed=12, H=37, W=53)}


def sphere_fixture(name, **camkw):
    s = SPHERES[name]
    v, f = latlong_sphere(s["stacks"], s["slices"], 1.0, s["seed"])
    assert len(f) == int(name[len("sphere"):])
    return v, f, sphere_camera(s["H"], s["W"], **camkw)


def exact_quad(swap_labels=False, reverse=False):
    """Two triangles that share the diagonal A-C of the square (+-2, +-2, -4), seen by the identity camera at the origin with H = W = 16, fx = fy = cx = cy = 8: pixel
    directions are multiples of 1/16, every product of the definition is exact, the square's outline falls between pixel centres (it covers i, j = 4 .. 11) and its
    diagonal x = y passes through the centres of the pixels j = 15 - i.  swap_labels exchanges the vertex numbers of A and C; reverse flips both triangles."""
    A, B, Cc, D = [-2.0, -2.0, -4.0], [2.0, -2.0, -4.0], [2.0, 2.0, -4.0], [-2.0, 2.0, -4.0]
    ia, ic = (2, 0) if swap_labels else (0, 2)
    verts = np.zeros((4, 3), np.float32)
    verts[ia], verts[1], verts[ic], verts[3] = A, B, Cc, D
    faces = np.asarray([[ia, 1, ic], [ia, ic, 3]], np.int32)
    if reverse:
        faces = faces[:, ::-1].copy()
    cam = camera(np.concatenate([np.eye(3), np.zeros((3, 1))], 1), 16, 16, 8.0, (8.0, 8.0))
    return verts, faces, cam, (ia, ic)


def quad_owner(faces, verts, diag):
    """The triangle the owner rule names for a ray through the diagonal, worked out from the rule's words (exact fp64): the triangle in whose corner order the diagonal
    runs start -> end owns it iff (start < end) XOR (sg < 0)."""
    owners = []
    for t, f in enumerate(faces):
        q = verts[f].astype(np.float64)                          # identity camera: q = v
        sg_neg = np.dot(q[0], np.cross(q[1], q[2])) < 0
        for k in range(3):
            s, e = int(f[(k + 1) % 3]), int(f[(k + 2) % 3])
            if {s, e} == set(diag) and ((s < e) != sg_neg):
                owners.append(t)
    assert len(owners) == 1
    return owners[0]


def mc_sphere(device, n=24, radius=0.42, centre=(0.03, -0.02, 0.05)):
    """marching-cubes sphere (GPU): the level set |p - centre| = radius of a [n]^3 volume over [-0.5, 0.5]^3, scaled to radius 1 so the camera fixtures see it like
    the unit sphere (about 3 500 triangles)"""
    import torch
    from jittor_myc_nerfs_amd import mesh
    g = torch.linspace(-0.5, 0.5, n, dtype=torch.float64)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    vol = (radius - torch.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)).to(torch.float32).to(device)
    sp = 1.0 / (n - 1)
    verts, faces = mesh.marching_cubes(vol, 0.0, spacing=(sp, sp, sp), origin=(-0.5, -0.5, -0.5))
    return verts * (1.0 / radius), faces
