"""GPU (-m gpu): the vertex adjacency and Taubin smoothing of csrc/tvr_mesh_smooth.hip through mesh.mesh_adjacency / mesh.smooth_taubin, and the export path built on
them.  The oracle is tests/mesh_smooth_common.py (numpy, restated from the definitions in include/tvr.h); every comparison with it is exact — np.array_equal on offsets,
neighbours, edge_faces and counts, the uint32 view on positions.  There is no tolerance in this file.  (One test feeds NaN and infinity: there the NaN positions must
coincide and every other value must agree bit for bit; which NaN a processor produces is not part of IEEE arithmetic.)"""
import functools

import numpy as np
import pytest
import torch

import mesh_components_common as CM
import mesh_simplify_common as SC
import mesh_smooth_common as SM
from conftest import TINY, make_model

pytestmark = pytest.mark.gpu

ITERATIONS = (0, 1, 2, 7)
WEIGHTS = ((0.5, -0.53), (0.33, -0.34), (1.0, 0.0))
HALF_EDGES = {"two_spheres": 1716, "noise": 62604, "integer": 9720, "sphere": 3168, "torus": 3084, "slab": 1182}


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


@functools.lru_cache(maxsize=None)
def _gpu_mesh(name):
    """(verts, faces) tensors of a fixture volume from the HIP marching cubes — extracted once, shared, never written to"""
    from jittor_myc_nerfs_amd import marching_cubes
    make, level = CM.VOLUMES[name]
    return marching_cubes(torch.as_tensor(make()).cuda(), level)


@functools.lru_cache(maxsize=None)
def _simplified(name):
    from jittor_myc_nerfs_amd import mesh
    v, f = _gpu_mesh(name)
    v2, f2, _ = mesh.simplify_clustering(v, f, 2.0)
    return v2, f2


def _check_adjacency(faces_t, V):
    """mesh_adjacency against the oracle, everything exact -> ((offsets, neighbours, edge_faces) tensors, the oracle's arrays and stats)"""
    from jittor_myc_nerfs_amd import mesh
    st = {}
    off, nbr, cnt = mesh.mesh_adjacency(faces_t, V, stats=st)
    want = SM.adjacency_oracle(_np(faces_t), V)
    for t, w in zip((off, nbr, cnt), want[:3]):
        assert t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == w.shape
        assert np.array_equal(_np(t), w)
    assert st == want[3], (st, want[3])
    return (off, nbr, cnt), want


def _check_smooth(verts_t, faces_t, adjacency, want_adj, cases):
    """smooth_taubin against the oracle, bit for bit, for every (iterations, lam, mu, pin_boundary) of `cases`"""
    from jittor_myc_nerfs_amd import mesh
    v = _np(verts_t)
    for its, lam, mu, pin in cases:
        st = {}
        got = mesh.smooth_taubin(verts_t, faces_t, its, lam=lam, mu=mu, pin_boundary=pin, adjacency=adjacency, stats=st)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == tuple(verts_t.shape) and st == {"smooth_iterations": its}
        want = SM.smooth_oracle(v, want_adj[0], want_adj[1], want_adj[2], its, lam, mu, pin)
        assert SM.same_bits(_np(got), want), (its, lam, mu, pin, int((_np(got).view(np.uint32) != want.view(np.uint32)).sum()))
        if its == 0:
            assert got.data_ptr() != verts_t.data_ptr()


# ---- the adjacency ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CM.VOLUMES))
def test_adjacency_of_marching_cubes_meshes(name):
    v, f = _gpu_mesh(name)
    (off, nbr, cnt), want = _check_adjacency(f, v.shape[0])
    st = want[3]
    assert st["half_edges"] == HALF_EDGES[name]
    if name in CM.CLOSED:
        assert st["boundary_edges"] == 0 and st["nonmanifold_edges"] == 0 and bool((cnt == 2).all())
    else:
        assert st["boundary_edges"] == 78
    # the real pipeline order: after clustering rows get longer and pinches (edges with more than two sides) occur
    v2, f2 = _simplified(name)
    _, want2 = _check_adjacency(f2, v2.shape[0])
    print(f"    {name}: {st}; after simplify 2.0: {want2[3]}")


def test_adjacency_of_hand_made_meshes():
    # three triangles on one edge
    (off, nbr, cnt), want = _check_adjacency(_dev([[0, 1, 2], [1, 0, 3], [0, 1, 4]], torch.int32), 6)
    assert cnt.tolist()[:5] == [3, 1, 1, 1, 3] and want[3]["nonmanifold_edges"] == 1 and want[3]["boundary_edges"] == 6 and off.tolist() == [0, 4, 8, 10, 12, 14, 14]
    # a face listed twice, its reversal, faces with two and with three equal corners, an unused vertex at each end
    (off, nbr, cnt), want = _check_adjacency(_dev([[1, 2, 3], [1, 2, 3], [3, 2, 1], [2, 2, 3], [4, 4, 4], [4, 1, 4]], torch.int32), 6)
    assert off.tolist() == [0, 0, 3, 5, 7, 8, 8] and nbr.tolist() == [2, 3, 4, 1, 3, 1, 2, 1] and cnt.tolist() == [3, 3, 2, 3, 5, 3, 5, 2]
    # no faces; only faces without sides; nothing at all
    none = torch.zeros(0, 3, dtype=torch.int32, device="cuda")
    (off, nbr, cnt), want = _check_adjacency(none, 5)
    assert off.tolist() == [0] * 6 and nbr.numel() == 0 and want[3]["max_degree"] == 0
    (off, nbr, cnt), want = _check_adjacency(_dev([[1, 1, 1], [0, 0, 0]], torch.int32), 2)
    assert off.tolist() == [0, 0, 0]
    (off, nbr, cnt), want = _check_adjacency(none, 0)
    assert off.tolist() == [0] and want[3] == dict(half_edges=0, boundary_edges=0, nonmanifold_edges=0, max_degree=0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("hub_degree,closed", [(4096, True), (31, True), (32, True), (33, True), (33, False), (34, False), (1000, False)])
def test_adjacency_of_fans(hub_degree, closed):
    """A hub whose raw row has 2 x hub_degree entries (closed) or 2 x hub_degree - 2 (open): 8192 for the long-row sort, and 62 / 64 / 66 around the length at which a
    row passes from one thread to a workgroup; unused vertices sit at both ends of the index range."""
    from jittor_myc_nerfs_amd import mesh
    assert mesh.ADJ_SHORT_ROW == 64
    v, f = SM.fan(hub_degree, lead=3, tail=5, closed=closed)
    (off, nbr, cnt), want = _check_adjacency(_dev(f, torch.int32), len(v))
    assert want[3]["max_degree"] == hub_degree and off[3].item() == 0 and off[4].item() == hub_degree and off[-1].item() == off[-6].item()
    assert want[3]["boundary_edges"] == (hub_degree if closed else hub_degree - 1 + 2)


@pytest.mark.parametrize("V,F,crosses", [(300, 2000, False), (150, 2000, True)])
def test_adjacency_of_a_random_soup(V, F, crosses):
    """Index soups with duplicates, rotations, reversals and equal corners; the denser one has raw rows on both sides of the one-thread / one-workgroup switch."""
    rng = np.random.default_rng(5)
    _, f = SC.random_mesh(rng, V, F - 60)
    f = SM.with_equal_corners(rng, f, V, 60)
    assert f.shape == (F, 3)
    _, want = _check_adjacency(_dev(f, torch.int32), V)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    raw = np.bincount(np.concatenate((a[a != b], b[a != b])), minlength=V)                  # entries of every raw row: one per proper side at the vertex
    assert want[3]["nonmanifold_edges"] > 0 and (not crosses or raw.min() <= 64 < raw.max())


# ---- the smoothing ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CM.VOLUMES))
def test_smoothing_of_marching_cubes_meshes(name):
    v, f = _gpu_mesh(name)
    adjacency, want = _check_adjacency(f, v.shape[0])
    if name == "noise":
        cases = [(its, 0.5, -0.53, True) for its in ITERATIONS] + [(2, lam, mu, True) for lam, mu in WEIGHTS[1:]]
    else:
        cases = [(its, lam, mu, True) for its in ITERATIONS for lam, mu in WEIGHTS]
    if name == "slab":
        cases += [(its, lam, mu, False) for its in ITERATIONS for lam, mu in WEIGHTS]
    _check_smooth(v, f, adjacency, want, cases)
    if name == "slab":
        from jittor_myc_nerfs_amd import mesh
        pinned = torch.as_tensor(SM.pinned_vertices(want[0], want[2])).cuda()
        assert int(pinned.sum()) == 78
        out = mesh.smooth_taubin(v, f, 7)
        assert torch.equal(out[pinned].view(torch.int32), v[pinned].view(torch.int32)) and not torch.equal(out[~pinned], v[~pinned])
        assert not torch.equal(mesh.smooth_taubin(v, f, 7, pin_boundary=False)[pinned], v[pinned])


@pytest.mark.parametrize("name", list(CM.VOLUMES))
def test_smoothing_after_clustering(name):
    v, f = _simplified(name)
    adjacency, want = _check_adjacency(f, v.shape[0])
    its = (0, 2, 7) if name == "noise" else ITERATIONS
    _check_smooth(v, f, adjacency, want, [(i, lam, mu, pin) for i in its for lam, mu in WEIGHTS for pin in ((True, False) if name == "slab" else (True,))])


def test_smoothing_of_the_fan():
    """The hub's row of 4096 neighbours is summed in order by one thread; with pinned boundaries only the hub moves (every rim edge has one side), without them
    everything does.  The z column of a second run is -0.0 throughout: the sum starts from the first neighbour, so the mean is -0.0, not +0.0."""
    v, f = SM.fan(4096, lead=3, tail=5, closed=True)
    vt, ft = _dev(v, torch.float32), _dev(f, torch.int32)
    adjacency, want = _check_adjacency(ft, len(v))
    _check_smooth(vt, ft, adjacency, want, [(its, lam, mu, False) for its in ITERATIONS for lam, mu in WEIGHTS] + [(2, 0.5, -0.53, True), (7, 1.0, 0.0, True)])
    flat = v.copy()
    flat[:, 2] = -0.0
    _check_smooth(_dev(flat, torch.float32), ft, adjacency, want, [(1, 0.5, -0.53, False), (2, 1.0, 0.0, False)])
    small_v, small_f = SM.fan(33, lead=1, tail=2, closed=False)
    st, sf = _dev(small_v, torch.float32), _dev(small_f, torch.int32)
    adjacency, want = _check_adjacency(sf, len(small_v))
    _check_smooth(st, sf, adjacency, want, [(its, lam, mu, pin) for its in ITERATIONS for lam, mu in WEIGHTS for pin in (True, False)])


def test_non_finite_coordinates_spread():
    from jittor_myc_nerfs_amd import mesh
    v, f = _gpu_mesh("sphere")
    adjacency, want = _check_adjacency(f, v.shape[0])
    bad = v.clone()
    bad[5, 0], bad[40, 1], bad[90, 2] = float("nan"), float("inf"), float("-inf")
    for its in (1, 3):
        got = _np(mesh.smooth_taubin(bad, f, its, adjacency=adjacency))
        ref = SM.smooth_oracle(_np(bad), want[0], want[1], want[2], its)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan) and nan.any() and not nan.all()
        assert np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan])
    assert torch.equal(mesh.smooth_taubin(bad, f, 0).view(torch.int32), bad.view(torch.int32))              # iterations = 0 copies the bits, NaN included


def test_two_runs_agree_and_a_given_adjacency_changes_nothing():
    from jittor_myc_nerfs_amd import mesh
    fan_v, fan_f = SM.fan(4096, closed=True)
    for verts, faces in (_gpu_mesh("noise"), _simplified("noise"), (_dev(fan_v, torch.float32), _dev(fan_f, torch.int32))):
        V = verts.shape[0]
        a, b = mesh.mesh_adjacency(faces, V), mesh.mesh_adjacency(faces, V)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        st = {}
        s1 = mesh.smooth_taubin(verts, faces, 5, stats=st)
        s2 = mesh.smooth_taubin(verts, faces, 5)
        s3 = mesh.smooth_taubin(verts, faces, 5, adjacency=a)
        assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(s1.view(torch.int32), s3.view(torch.int32))
        assert st["smooth_iterations"] == 5 and st["half_edges"] == a[1].numel()


# ---- the fault flag ----------------------------------------------------------------------------------------------------------------------------------------------
class _Guards:
    """4 KB of 0xA5 behind every buffer allocated inside (tests/test_gpu_canaries.py's mechanism); under the TVR_GUARDS=1 sweep the guards are already there"""

    def __enter__(self):
        from jittor_myc_nerfs_amd import _lib as L
        self.keep = L.GUARD_BYTES
        self.own = self.keep <= 0
        if self.own:
            L._guarded.clear()
            L.GUARD_BYTES = 4096
        return L

    def __exit__(self, *exc):
        from jittor_myc_nerfs_amd import _lib as L
        if self.own:
            L.GUARD_BYTES = self.keep
            L._guarded.clear()


def _raw_emit(L, f, V, scratch, decl_h):
    """tvr_mesh_adjacency_emit into sentinel-filled, guarded buffers of the declared size -> (offsets, neighbours, edge_faces, flag value)"""
    lib = L.lib()
    off = L.dev_empty((V + 1,), torch.int32, "cuda", what="test offsets").fill_(-7)
    nbr = L.dev_empty((decl_h,), torch.int32, "cuda", what="test neighbours").fill_(-7)
    cnt = L.dev_empty((decl_h,), torch.int32, "cuda", what="test edge_faces").fill_(-7)
    fl = L.dev_bytes(4, "cuda", zero=True, what="test flag").view(torch.int32)
    L.check(lib.tvr_mesh_adjacency_emit(f.data_ptr(), f.shape[0], V, scratch.data_ptr(), L.nbytes(scratch), off.data_ptr(), L.nbytes(off),
                                        nbr.data_ptr() if decl_h else None, L.nbytes(nbr), cnt.data_ptr() if decl_h else None, L.nbytes(cnt), decl_h, fl.data_ptr(), None),
            "tvr_mesh_adjacency_emit")
    torch.cuda.synchronize()
    return off, nbr, cnt, int(fl.item())


def _untouched(*tensors):
    return all(bool((t == -7).all()) for t in tensors)


@pytest.mark.parametrize("bad", ["face index V", "face index -1"])
def test_bad_face_index_raises_the_flag_and_writes_nothing(bad):
    """A reported condition, not a device fault: the index is range-checked before it is used, so no access leaves a buffer."""
    from jittor_myc_nerfs_amd import mesh
    v, f = _gpu_mesh("two_spheres")
    V, F = v.shape[0], f.shape[0]
    fb = f.clone()
    fb[F // 2, 1] = V if bad.endswith("V") else -1
    with _Guards() as L:
        scratch, counts, flag = mesh.adjacency_count(fb, V)
        torch.cuda.synchronize()
        assert int(flag.item()) == 1 and counts == (0, 0, 0, 0) and L.check_guards() == []
        for decl_h in (0, HALF_EDGES["two_spheres"]):
            off, nbr, cnt, fl = _raw_emit(L, fb, V, scratch, decl_h)
            assert fl == 1 and _untouched(off, nbr, cnt) and L.check_guards() == []
    with pytest.raises(L.TvrError, match="fault flag"):
        mesh.mesh_adjacency(fb, V)
    with pytest.raises(L.TvrError, match="fault flag"):
        mesh.smooth_taubin(v, fb, 1)


def test_wrong_half_edge_count_raises_the_flag_and_writes_nothing():
    from jittor_myc_nerfs_amd import mesh
    v, f = _gpu_mesh("noise")
    V = v.shape[0]
    want = mesh.mesh_adjacency(f, V)
    with _Guards() as L:
        scratch, counts, flag = mesh.adjacency_count(f, V)
        H = counts[0]
        assert int(flag.item()) == 0 and H == HALF_EDGES["noise"] and counts[1:] == (0, 0, 19) and L.check_guards() == []
        for decl_h in (H - 1, H + 1, 0, 6 * f.shape[0]):
            off, nbr, cnt, fl = _raw_emit(L, f, V, scratch, decl_h)
            assert fl == 1 and _untouched(off, nbr, cnt), decl_h
            assert L.check_guards() == []
        off, nbr, cnt, fl = _raw_emit(L, f, V, scratch, H)           # the true count: no flag, everything written; the scratch serves again
        assert fl == 0 and L.check_guards() == []
        assert torch.equal(off, want[0]) and torch.equal(nbr, want[1]) and torch.equal(cnt, want[2])


@pytest.mark.parametrize("bad", ["decreasing offsets", "neighbour equal to V", "offsets[0] is 1", "offsets[V] is H - 1", "neighbour -1"])
@pytest.mark.parametrize("iterations", [0, 2])
def test_bad_adjacency_raises_the_flag_and_writes_nothing(bad, iterations):
    """The inputs are merely invalid: the first kernel finds them, every later one returns at once, and the gather re-checks each index it uses."""
    from jittor_myc_nerfs_amd import mesh
    v, f = _gpu_mesh("two_spheres")
    V = v.shape[0]
    off, nbr, cnt = (t.clone() for t in mesh.mesh_adjacency(f, V))
    H = nbr.numel()
    if bad == "decreasing offsets":
        off[V // 2] = off[V // 2 - 1] - 1
    elif bad == "neighbour equal to V":
        nbr[H // 3] = V
    elif bad == "neighbour -1":
        nbr[H - 1] = -1
    elif bad == "offsets[0] is 1":
        off[0] = 1
    else:
        off[V] = H - 1
    with _Guards() as L:
        lib = L.lib()
        out = L.dev_empty((V, 3), torch.float32, "cuda", what="test verts").fill_(-7.0)
        scratch = L.dev_bytes(lib.tvr_mesh_smooth_scratch_bytes(V, H), "cuda", what="test scratch")
        fl = L.dev_bytes(4, "cuda", zero=True, what="test flag").view(torch.int32)
        L.check(lib.tvr_mesh_smooth(v.data_ptr(), V, off.data_ptr(), nbr.data_ptr(), cnt.data_ptr(), H, iterations, 0.5, -0.53, 1, scratch.data_ptr(), L.nbytes(scratch),
                                    out.data_ptr(), L.nbytes(out), fl.data_ptr(), None), "tvr_mesh_smooth")
        torch.cuda.synchronize()
        assert int(fl.item()) == 1 and _untouched(out) and L.check_guards() == []
    with pytest.raises(L.TvrError, match="fault flag"):
        mesh.smooth_taubin(v, f, iterations, adjacency=(off, nbr, cnt))


# ---- through the model ------------------------------------------------------------------------------------------------------------------------------------------
def _hyper():
    from jittor_myc_nerfs_amd import synthetic
    return dict(synthetic.HYPER, near_far=TINY["near_far"], step_ratio=TINY["step_ratio"])


def _stable(stats):
    """export stats without the one entry that is a diagnostic of the order atomics landed in (include/tvr.h tvr_mesh_simplify_*)"""
    return {k: v for k, v in stats.items() if k != "max_probe"}


def test_model_export_mesh_smooths(tiny_arrays, tmp_path):
    from jittor_myc_nerfs_amd import mesh, read_ply_attributes
    m = make_model(tiny_arrays, _hyper())
    alpha = m.getDenseAlpha()[0]
    level = 0.5 * (float(alpha.min()) + float(alpha.max()))
    p0, p1, p2, p3, p4 = (str(tmp_path / f"{i}.ply") for i in range(5))
    opts = dict(level=level, simplify=2.0, keep_largest=1, normals=True, colors=True)
    m.export_mesh(p1, **opts)
    before = dict(m.mesh_export_stats)
    m.export_mesh(p0, smooth=0, **opts)
    assert open(p0, "rb").read() == open(p1, "rb").read() and _stable(m.mesh_export_stats) == _stable(before)      # 0: the file and the stats of a call without it
    assert "half_edges" not in before and "smooth_iterations" not in before
    v3, f3 = m.export_mesh(p2, smooth=3, **opts)
    st = dict(m.mesh_export_stats)
    # the composition of the public calls
    v1, f1 = m.export_mesh(p4, level=level)
    vk, fk, _ = mesh.filter_components(v1, f1, keep_largest=1)
    cell, origin = m.mesh_simplify_lattice(alpha.shape, "reference", 2.0)
    vs, fs, _ = mesh.simplify_clustering(vk, fk, cell, origin=origin)
    adj_stats = {}
    vt = mesh.smooth_taubin(vs, fs, 3, stats=adj_stats)
    assert torch.equal(v3.view(torch.int32), vt.view(torch.int32)) and torch.equal(f3, fs) and fs.shape[0] > 0 and not torch.equal(vt, vs)
    attrs = m.mesh_vertex_attributes(m.mesh_sample_positions(vt, alpha.shape, "reference"), normals=True, colors=True)
    mesh.write_ply(p3, vt, fs, normals=attrs["normals"], colors=attrs["colors"])
    assert open(p2, "rb").read() == open(p3, "rb").read()
    # against the oracle, and the attributes are those of the smoothed positions
    off, nbr, cnt, ost = SM.adjacency_oracle(_np(fs), vs.shape[0])
    assert SM.same_bits(_np(v3), SM.smooth_oracle(_np(vs), off, nbr, cnt, 3))
    rv, rf, ra = read_ply_attributes(p2)
    assert SM.same_bits(rv, _np(vt)) and np.array_equal(rf, _np(fs))
    assert np.array_equal(ra["normals"].view(np.uint32), _np(attrs["normals"]).view(np.uint32)) and np.array_equal(ra["colors"], _np(attrs["colors"]))
    unsmoothed = m.mesh_vertex_attributes(m.mesh_sample_positions(vs, alpha.shape, "reference"), normals=True, colors=False)
    assert not np.array_equal(ra["normals"], _np(unsmoothed["normals"]))
    for key, value in dict(ost, smooth_iterations=3).items():
        assert st[key] == value, key
    assert {k: st[k] for k in _stable(before)} == _stable(before) and adj_stats == dict(ost, smooth_iterations=3)
    print(f"    tiny scene, simplify 2 + smooth 3: {vs.shape[0]} vertices, {fs.shape[0]} triangles, {ost}")
    for s in (-1, 1001, 1.5):
        with pytest.raises(ValueError, match="smooth"):
            m.export_mesh(p4, level=level, smooth=s)


def test_command_line_smooths(tiny_arrays, tmp_path, capsys):
    """`--export_mesh 1 --mesh_smooth 2` on a checkpoint of the tiny scene writes the file of export_mesh(smooth=2); `--mesh_smooth 0` the file without the option."""
    from jittor_myc_nerfs_amd import reconstruct as R
    m = make_model(tiny_arrays, _hyper())
    alpha = m.getDenseAlpha()[0]
    level = 0.5 * (float(alpha.min()) + float(alpha.max()))
    ckpt = tmp_path / "tiny.th"
    m.save(str(ckpt))
    cmd = ["--export_mesh", "1", "--ckpt", str(ckpt), "--model_name", "TensorVMSplit", "--mesh_level", repr(level)]
    out = R.main(cmd)
    plain = (tmp_path / "tiny.ply").read_bytes()
    assert R.main(cmd + ["--mesh_smooth", "0"]) == out and (tmp_path / "tiny.ply").read_bytes() == plain
    capsys.readouterr()
    assert R.main(cmd + ["--mesh_smooth", "2"]) == out
    smooth = (tmp_path / "tiny.ply").read_bytes()
    assert "smoothed 2 iterations" in capsys.readouterr().out
    m.export_mesh(str(tmp_path / "direct.ply"), level=level, smooth=2)
    assert smooth == (tmp_path / "direct.ply").read_bytes() and len(smooth) == len(plain) and smooth != plain
