"""No GPU: the oracle of tests/mesh_smooth_common.py against its brute-force twin, the adjacency counts of the fixture meshes (the place where "closed" is checked),
properties of the smoothing as include/tvr.h defines it (Taubin keeps the volume where plain Laplacian smoothing loses it, the umbrella shrinks, pinned vertices stay),
the argument errors of tvr_mesh_adjacency_* / tvr_mesh_smooth (reported before any launch), the symbol list, the ValueErrors, the no-CPU-fallback rule, the command line,
and that export_mesh(smooth=0) never reaches the smoother."""
import ctypes as C
import functools
import inspect

import numpy as np
import pytest
import torch

import mesh_components_common as CM
import mesh_simplify_common as SC
import mesh_smooth_common as SM

INVALID, UNSUPPORTED = -1, -4

# half-edges, boundary edges, non-manifold edges of the fixture meshes (a numpy restatement of the definition)
FIXTURE_COUNTS = {"two_spheres": (1716, 0, 0), "noise": (62604, 0, 0), "integer": (9720, 0, 0), "sphere": (3168, 0, 0), "torus": (3084, 0, 0), "slab": (1182, 78, 0)}


@functools.lru_cache(maxsize=None)
def _adjacency(name):
    v, f = CM.cpu_mesh(name)
    return SM.adjacency_oracle(f, len(v))


@pytest.mark.parametrize("seed", range(6))
def test_oracle_equals_brute_force_on_random_soups(seed):
    rng = np.random.default_rng(seed)
    V = int(rng.integers(20, 60))
    v, f = SC.random_mesh(rng, V, int(rng.integers(10, 80)))         # duplicates, rotations, reversals
    f = SM.with_equal_corners(rng, f, V, 9)
    got, want = SM.adjacency_oracle(f, V), SM.adjacency_brute_force(f, V)
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)
    assert got[3] == want[3] and got[3]["half_edges"] == len(got[1]) == got[0][-1]
    off, nbr, cnt, _ = got
    for row in range(V):
        r = nbr[off[row]:off[row + 1]]
        assert (np.diff(r) > 0).all() and row not in r               # ascending, duplicate-free, no loop
    v[int(rng.integers(0, V))] = (np.nan, -0.0, np.inf)              # non-finite values spread as the arithmetic dictates, in both versions alike
    for its, lam, mu, pin in ((1, 0.5, -0.53, True), (3, 0.33, -0.34, False), (2, 1.0, 0.0, True), (0, 0.5, -0.53, True)):
        assert SM.same_bits(SM.smooth_oracle(v, off, nbr, cnt, its, lam, mu, pin), SM.smooth_brute_force(v, off, nbr, cnt, its, lam, mu, pin)), (its, lam, mu, pin)
    assert SM.same_bits(SM.smooth_oracle(v, off, nbr, cnt, 0), v)
    with pytest.raises(IndexError):
        SM.adjacency_oracle(np.array([[0, 1, V]]), V)
    with pytest.raises(IndexError):
        SM.adjacency_oracle(np.array([[0, -1, 1]]), V)


def test_hand_worked_adjacency():
    # three triangles on the edge {0,1}: edge_faces 3, one non-manifold edge; every other edge is a boundary
    off, nbr, cnt, st = SM.adjacency_oracle([[0, 1, 2], [1, 0, 3], [0, 1, 4]], 6)
    assert off.tolist() == [0, 4, 8, 10, 12, 14, 14] and nbr.tolist() == [1, 2, 3, 4, 0, 2, 3, 4, 0, 1, 0, 1, 0, 1]
    assert cnt.tolist() == [3, 1, 1, 1, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1]
    assert st == dict(half_edges=14, boundary_edges=6, nonmanifold_edges=1, max_degree=4)
    # a face listed twice counts twice, its reversal counts too; equal corners: (1, 1, 2) has the side {1,2} twice, (3, 3, 3) has none
    off, nbr, cnt, st = SM.adjacency_oracle([[0, 1, 2], [0, 1, 2], [2, 1, 0], [1, 1, 2], [3, 3, 3]], 4)
    assert off.tolist() == [0, 2, 4, 6, 6] and nbr.tolist() == [1, 2, 0, 2, 0, 1] and cnt.tolist() == [3, 3, 3, 5, 3, 5]
    assert st == dict(half_edges=6, boundary_edges=0, nonmanifold_edges=3, max_degree=2)
    off, nbr, cnt, st = SM.adjacency_oracle(np.zeros((0, 3), np.int64), 0)
    assert off.tolist() == [0] and len(nbr) == 0 and st == dict(half_edges=0, boundary_edges=0, nonmanifold_edges=0, max_degree=0)
    v, f = SM.fan(40, lead=2, tail=3)
    off, nbr, cnt, st = SM.adjacency_oracle(f, len(v))
    assert st == dict(half_edges=2 * (39 + 40), boundary_edges=41, nonmanifold_edges=0, max_degree=40) and off[2] == 0 and off[-1] == off[-4]


@pytest.mark.parametrize("name", list(CM.VOLUMES))
def test_adjacency_counts_of_the_fixtures(name):
    v, f = CM.cpu_mesh(name)
    off, nbr, cnt, st = _adjacency(name)
    half_edges, boundary, nonmanifold = FIXTURE_COUNTS[name]
    assert (st["half_edges"], st["boundary_edges"], st["nonmanifold_edges"]) == (half_edges, boundary, nonmanifold)
    assert int(cnt.sum()) == 6 * len(f)                              # marching cubes emits no face with equal corners: every side is counted at both ends
    if name in CM.CLOSED:
        assert (cnt == 2).all()                                      # closed and 2-manifold: checked here, promised nowhere
    if name == "noise":
        assert st["max_degree"] == 19
    if name == "slab":
        assert int(SM.pinned_vertices(off, cnt).sum()) == 78


def test_taubin_keeps_the_volume_laplace_does_not():
    for name in ("sphere", "torus", "two_spheres"):
        v, f = CM.cpu_mesh(name)
        off, nbr, cnt, _ = _adjacency(name)
        vol = SM.signed_volume(v, f)
        taubin = SM.signed_volume(SM.smooth_oracle(v, off, nbr, cnt, 10), f)
        laplace = SM.signed_volume(SM.smooth_oracle(v, off, nbr, cnt, 10, lam=0.5, mu=0.5), f)
        print(f"    {name}: volume {vol:.2f}, Taubin x 10 {100 * (taubin / vol - 1):+.2f} %, Laplace x 10 {100 * (laplace / vol - 1):+.2f} %")
        assert abs(taubin / vol - 1) < 0.02
        assert laplace / vol < 0.70


@pytest.mark.parametrize("name", list(CM.VOLUMES))
def test_the_umbrella_shrinks(name):
    v, f = CM.cpu_mesh(name)
    off, nbr, cnt, _ = _adjacency(name)
    after = SM.smooth_oracle(v, off, nbr, cnt, 10)
    assert SM.mean_umbrella(after, off, nbr) < SM.mean_umbrella(v, off, nbr)


def test_pinned_boundary_stays():
    v, f = CM.cpu_mesh("slab")
    off, nbr, cnt, _ = _adjacency("slab")
    pinned = SM.pinned_vertices(off, cnt)
    assert int(pinned.sum()) == 78
    out = SM.smooth_oracle(v, off, nbr, cnt, 5)
    assert SM.same_bits(out[pinned], v[pinned]) and not SM.same_bits(out[~pinned], v[~pinned])
    free = SM.smooth_oracle(v, off, nbr, cnt, 5, pin_boundary=False)
    assert not SM.same_bits(free[pinned], v[pinned])


def test_symbols_are_listed_and_exported():
    import jittor_myc_nerfs_amd as pkg
    from jittor_myc_nerfs_amd import _lib as L, mesh
    for name in ("tvr_mesh_adjacency_scratch_bytes", "tvr_mesh_adjacency_count", "tvr_mesh_adjacency_emit", "tvr_mesh_smooth_scratch_bytes", "tvr_mesh_smooth"):
        assert name in L.SYMBOLS
        assert hasattr(L.lib(), name)
    assert L.lib().tvr_version() == 141
    assert pkg.mesh_adjacency is mesh.mesh_adjacency and pkg.smooth_taubin is mesh.smooth_taubin
    assert callable(mesh.adjacency_count) and callable(mesh.adjacency_emit)


def test_argument_errors_without_gpu():
    from jittor_myc_nerfs_amd import _lib as L, mesh
    lib = L.lib()
    dummy = C.c_void_p(1 << 20)                                      # 256-byte aligned, never dereferenced: every check precedes the launches
    off = C.c_void_p((1 << 20) + 16)
    big = 1 << 40
    V, F, H = 1000, 3000, 6000
    top = 2 ** 31 - 1

    def refused(rc, code, what):
        assert rc == code, (what, rc, lib.tvr_last_error())
        assert what.encode() in lib.tvr_last_error(), (what, lib.tvr_last_error())

    def count(faces=dummy, nf=F, nv=V, scratch=dummy, scratch_bytes=big, counts=dummy, flag=dummy):
        return lib.tvr_mesh_adjacency_count(faces, nf, nv, scratch, scratch_bytes, counts, flag, None)

    def emit(faces=dummy, nf=F, nv=V, scratch=dummy, scratch_bytes=big, offsets=dummy, offsets_bytes=big, nbrs=dummy, nbrs_bytes=big, ef=dummy, ef_bytes=big, nh=H,
             flag=dummy):
        return lib.tvr_mesh_adjacency_emit(faces, nf, nv, scratch, scratch_bytes, offsets, offsets_bytes, nbrs, nbrs_bytes, ef, ef_bytes, nh, flag, None)

    def smooth(verts=dummy, nv=V, offsets=dummy, nbrs=dummy, ef=dummy, nh=H, its=3, lam=0.5, mu=-0.53, pin=1, scratch=dummy, scratch_bytes=big, out=dummy,
               out_bytes=12 * V, flag=dummy):
        return lib.tvr_mesh_smooth(verts, nv, offsets, nbrs, ef, nh, its, lam, mu, pin, scratch, scratch_bytes, out, out_bytes, flag, None)

    # the adjacency's scratch: a multiple of 256, linear in the counts, 0 for counts that are refused
    fn = lib.tvr_mesh_adjacency_scratch_bytes
    need = fn(V, F)
    assert need % 256 == 0 and need >= 256 + 16 * V + 48 * F
    assert fn(0, 0) > 0
    for n in (10 ** 5, 10 ** 6, 10 ** 7):
        assert fn(n, 2 * n) <= 256 * 9 + (16 + 1 + 2 * 48) * n, n
    assert 0 < fn(top, top // 6) < 30 * top
    assert fn(-1, 5) == 0 and b"negative" in lib.tvr_last_error()
    assert fn(5, -1) == 0 and b"negative" in lib.tvr_last_error()
    assert fn(top + 1, 5) == 0 and b"2^31" in lib.tvr_last_error()
    assert fn(5, top // 6 + 1) == 0 and b"2^31" in lib.tvr_last_error()
    for call in (count, emit):
        refused(call(nv=-1), INVALID, "negative")
        refused(call(nf=-1), INVALID, "negative")
        refused(call(nv=top + 1), UNSUPPORTED, "2^31")
        refused(call(nf=top // 6 + 1), UNSUPPORTED, "2^31")
        refused(call(faces=None), INVALID, "faces is NULL")
        refused(call(flag=None), INVALID, "fault_flag_dev is NULL")
        refused(call(scratch=None), INVALID, "scratch is NULL")
        refused(call(scratch=off), INVALID, "aligned")
        refused(call(scratch_bytes=need - 1), INVALID, "scratch holds")
        assert call(nv=0, nf=0, faces=None, scratch=None) == INVALID                            # empty meshes still need their (header) scratch
    refused(count(counts=None), INVALID, "counts_dev is NULL")
    for kw in ("offsets", "nbrs", "ef"):
        refused(emit(**{kw: None}), INVALID, "NULL")
    refused(emit(offsets_bytes=4 * (V + 1) - 1), INVALID, "offsets holds")
    refused(emit(nbrs_bytes=4 * H - 1), INVALID, "neighbours holds")
    refused(emit(ef_bytes=4 * H - 1), INVALID, "edge_faces holds")
    refused(emit(nh=-1), INVALID, "outside")
    refused(emit(nh=6 * F + 1), INVALID, "outside")

    # the smoothing
    fn = lib.tvr_mesh_smooth_scratch_bytes
    need = fn(V, H)
    assert need % 256 == 0 and 256 + 32 * V <= need <= 256 * 3 + 32 * V and fn(0, 0) > 0
    assert fn(-1, 5) == 0 and b"negative" in lib.tvr_last_error()
    assert fn(5, -1) == 0 and b"negative" in lib.tvr_last_error()
    assert fn(top + 1, 5) == 0 and b"2^31" in lib.tvr_last_error()
    assert fn(5, top + 1) == 0 and b"2^31" in lib.tvr_last_error()
    refused(smooth(nv=-1), INVALID, "negative")
    refused(smooth(nh=-1), INVALID, "negative")
    refused(smooth(nv=top + 1), UNSUPPORTED, "2^31")
    refused(smooth(nh=top + 1), UNSUPPORTED, "2^31")
    for its in (-1, 1001, 2 ** 31 - 1):
        refused(smooth(its=its), INVALID, "iterations")
    for bad in (float("nan"), float("inf"), float("-inf")):
        refused(smooth(lam=bad), INVALID, "finite")
        refused(smooth(mu=bad), INVALID, "finite")
    for kw in ("verts", "offsets", "nbrs", "out", "flag"):
        refused(smooth(**{kw: None}), INVALID, "NULL")
    refused(smooth(ef=None), INVALID, "edge_faces is NULL")
    for nbytes in (12 * V - 1, 12 * V + 1, 0, big):
        refused(smooth(out_bytes=nbytes), INVALID, "verts_out holds")
    refused(smooth(scratch=None), INVALID, "scratch is NULL")
    refused(smooth(scratch=off), INVALID, "aligned")
    refused(smooth(scratch_bytes=need - 1), INVALID, "scratch holds")
    assert mesh.ADJ_SHORT_ROW == 64 and mesh.SMOOTH_MAX_ITERATIONS == 1000


def test_value_errors_and_no_cpu_fallback(tiny_arrays, hyper_tiny, tmp_path):
    from conftest import make_model
    from jittor_myc_nerfs_amd import _lib as L, mesh
    v, f = torch.zeros(4, 3), torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)
    for its in (-1, 1001, 1.0, 2.5, "3", None, True, float("nan")):
        with pytest.raises(ValueError, match="iterations"):
            mesh.smooth_taubin(v, f, its)
    for lam in (0.0, -0.5, 1.0001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lam"):
            mesh.smooth_taubin(v, f, 1, lam=lam)
    for mu in (-1.0001, 1.5, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="mu"):
            mesh.smooth_taubin(v, f, 1, mu=mu)
    with pytest.raises(L.TvrError, match="no CPU fallback"):
        mesh.smooth_taubin(v, f, 1)
    with pytest.raises(L.TvrError, match="no CPU fallback"):
        mesh.smooth_taubin(v, f, 0)
    with pytest.raises(L.TvrError, match="no CPU fallback"):
        mesh.mesh_adjacency(f, 4)
    m = make_model(tiny_arrays, hyper_tiny, device="cpu")
    for s in (-1, 1001, 2.0, 0.5, float("nan"), "2", True):
        with pytest.raises(ValueError, match="smooth"):
            m.export_mesh(str(tmp_path / "x.ply"), smooth=s)
    assert not (tmp_path / "x.ply").exists()


def test_export_mesh_reaches_the_smoother_only_when_asked(tiny_arrays, hyper_tiny, tmp_path, monkeypatch):
    """Marching cubes, the simplifier and the smoother are replaced by recorders (there is no device here): smooth = 0 writes the file of a call without the keyword and
    never calls the smoother; smooth = 3 calls it once, AFTER the clustering, with Taubin's pair and pinned boundaries, and writes what it returns with the same faces."""
    from conftest import make_model
    from jittor_myc_nerfs_amd import mesh, read_ply
    m = make_model(tiny_arrays, hyper_tiny, device="cpu")
    verts = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32)
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    calls = []
    monkeypatch.setattr(m, "getDenseAlpha", lambda gridSize=None: (torch.zeros(16, 20, 24), None))
    monkeypatch.setattr(mesh, "marching_cubes", lambda *a, **k: (verts, faces))

    def simplifier(v, f, cell, origin=(0, 0, 0), stats=None):
        calls.append("simplify")
        return v[:3] + 0.25, f[:1], torch.tensor([0, 1, 2, 2], dtype=torch.int32)

    def smoother(v, f, iterations, lam=None, mu=None, pin_boundary=None, adjacency=None, stats=None):
        calls.append(("smooth", v, f, iterations, lam, mu, pin_boundary, adjacency))
        stats.update(half_edges=6, boundary_edges=3, nonmanifold_edges=0, max_degree=2, smooth_iterations=iterations)
        return v * 0.5

    monkeypatch.setattr(mesh, "simplify_clustering", simplifier)
    monkeypatch.setattr(mesh, "smooth_taubin", smoother)
    p0, p1, p2 = (str(tmp_path / f"{i}.ply") for i in range(3))
    m.export_mesh(p0)
    m.export_mesh(p1, smooth=0)
    assert calls == [] and m.mesh_export_stats == {}
    assert open(p0, "rb").read() == open(p1, "rb").read()
    v2, f2 = m.export_mesh(p2, simplify=2.0, smooth=3)
    assert calls[0] == "simplify" and len(calls) == 2
    _, v_in, f_in, its, lam, mu, pin, adjacency = calls[1]
    assert torch.equal(v_in, verts[:3] + 0.25) and torch.equal(f_in, faces[:1]) and (its, lam, mu, pin, adjacency) == (3, 0.5, -0.53, True, None)
    assert m.mesh_export_stats == dict(half_edges=6, boundary_edges=3, nonmanifold_edges=0, max_degree=2, smooth_iterations=3)
    rv, rf = read_ply(p2)
    assert np.array_equal(rv, ((verts[:3] + 0.25) * 0.5).numpy()) and np.array_equal(rf, faces[:1].numpy()) and torch.equal(f2, faces[:1])
    assert inspect.signature(type(m).export_mesh).parameters["smooth"].default == 0


def test_public_signatures():
    from jittor_myc_nerfs_amd import mesh
    p = inspect.signature(mesh.smooth_taubin).parameters
    assert list(p) == ["verts", "faces", "iterations", "lam", "mu", "pin_boundary", "adjacency", "stats"]
    assert (p["lam"].default, p["mu"].default, p["pin_boundary"].default, p["adjacency"].default, p["stats"].default) == (0.5, -0.53, True, None, None)
    assert list(inspect.signature(mesh.mesh_adjacency).parameters) == ["faces", "n_vertices", "stats"]


def test_command_line_option(tmp_path):
    from jittor_myc_nerfs_amd import reconstruct as R
    assert R.config_parser([]).mesh_smooth == 0
    a = R.config_parser(["--export_mesh", "1", "--mesh_smooth", "5", "--mesh_simplify", "2"])
    assert a.export_mesh == 1 and a.mesh_smooth == 5 and isinstance(a.mesh_smooth, int) and a.mesh_simplify == 2.0
    cfg = tmp_path / "c.txt"
    cfg.write_text("export_mesh = 1\nmesh_smooth = 3\nmesh_keep_largest = 1\n")
    a = R.config_parser(["--config", str(cfg)])
    assert a.mesh_smooth == 3 and a.mesh_keep_largest == 1
