"""CPU: the inputs and the reference of tests/test_gpu_march_backward.py, vetted without a GPU (tests/march_backward_common.py).

  * every case keeps at least 97 % of its rays after the borderline ones are dropped, and holds what it is there for (rays that end after chunk 0, after a later
    chunk, never; a chunk without a valid sample between two with some; a whole chunk behind the box);
  * the float64 reference agrees with the fp32 oracle's autograd where the two compute the same thing (eps_T = 0), and with the oracle's `sample_keep` form where a
    ray ends early;
  * the 5e-4 bar has power: each deliberate defect of the chunk loop, applied to the reference, moves a density gradient by at least ten times the bar."""
import numpy as np
import pytest
import torch

import march_backward_common as MB


@pytest.mark.parametrize("name", list(MB.KERNEL_CASES))
def test_every_case_keeps_its_rays_and_reaches_the_scene(name):
    c = MB.KERNEL_CASES[name]()
    st = c.stats()
    print(name, st)
    assert st["before"] == 768 and st["dropped"] <= MB.MAX_DROPPED * st["before"], st
    assert st["hit"] >= 256 and st["n_app"] >= 1024, st
    nc = MB.n_chunks(c.S)
    assert len(st["ends_in"]) == nc
    if c.eps_T == 0:
        assert st["never_ends"] == c.n
    else:
        assert sum(st["ends_in"]) >= 4 and st["never_ends"] >= 128, st
    r = c.ref()
    for k, g in zip(MB.DENSITY_NAMES, r["grads"]):
        assert float(g.abs().max()) > 0, f"{k}: the reference gradient is identically zero"


def test_long_ray_case_conditions():
    """at least 32 rays first end in chunk 0, at least 32 in a later chunk that is not the last; at least 128 never end and have appearance samples in two or more
    chunks"""
    st = MB.KERNEL_CASES["S192-eps0.0001-nojitter"]().stats()
    print(st)
    assert st["ends_in"][0] >= 32 and sum(st["ends_in"][1:-1]) >= 32 and st["never_ends_app_in_two_chunks"] >= 128, st
    # the finer march moves the first endings behind chunk 0
    st = MB.KERNEL_CASES["S192-eps0.0001-step0.1"]().stats()
    print(st)
    assert st["ends_in"][0] == 0 and st["ends_in"][1] >= 32, st
    # one lane in the second chunk, and its dist is 0
    c = MB.KERNEL_CASES["S65-eps0.0001-nojitter"]()
    assert MB.n_chunks(c.S) == 2 and int(c.smp["valid"][:, 64].sum()) >= 32 and float(c.ref()["w"][:, 64].abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["bits", "float"])
def test_hollow_case_conditions(kind):
    """at least 32 rays walk a chunk without a valid sample strictly between two chunks with valid samples, and at least 32 reach a whole chunk behind the box"""
    c = MB.hollow_case(kind)
    st = c.stats()
    print(st)
    assert st["skipped_between"] >= 32 and st["first_after_skip"] >= 32 and st["past_exit"] >= 32, st
    vol = torch.as_tensor(c.arrs["alpha_volume"])
    if kind == "bits":
        assert set(np.unique(vol.numpy()).tolist()) == {0.0, 1.0}
    else:
        assert int(((vol > 0) & (vol < 1)).sum()) > 100                                # only the values themselves say where alpha > 0
        assert torch.equal(vol > 0, torch.as_tensor(MB.hollow_arrays("bits")["alpha_volume"]) > 0)


def _fp32_oracle_grads(c, sample_keep=None):
    """the case's loss through oracle.tensorf_oracle.execute (fp32, autograd): density gradients, weights, acc"""
    from oracle import tensorf_oracle as TO
    sc = TO.scene_from_arrays(c.arrs, **c.hyper)
    leaves = []
    for name in ("density_plane", "density_line"):
        for t in getattr(sc, name):
            leaves.append(t.requires_grad_(True))
    d = TO.execute(sc, torch.tensor(c.rays), white_bg=True, N_samples=c.S, jitter=c.jitter, dump=True, sample_keep=sample_keep)
    loss = (d["app_mask"] * MB.g_of(d["xyz_norm"]) * d["weight"]).sum() + (c.a.float() * d["acc_map"]).sum()
    return torch.autograd.grad(loss, leaves), d


@pytest.mark.parametrize("name", ["S192-eps0-jitter", "S65-eps0-nojitter", "S192-eps0.0001-nojitter", "hollow-bits-continue-and-leftbox-break", "S192-eps0.0001-relu"])
def test_reference_agrees_with_the_fp32_oracle_autograd(name):
    """ties the float64 reference to the existing oracle: at eps_T = 0 against execute as it stands, with early exit against execute(sample_keep=...) fed with the
    reference's own mask.  fp32 against fp64 of the same formulas: the GPU tests' bars hold here too."""
    c = MB.KERNEL_CASES[name]()
    r = c.ref()
    keep = None if c.eps_T == 0 else c.keep_mask()
    grads, d = _fp32_oracle_grads(c, keep)
    assert torch.equal(d["app_mask"], r["app"]), "with the borderline rays dropped, fp32 and fp64 queue the same samples"
    assert float((d["weight"].detach().double() - r["w"]).abs().max()) < MB.BAR_FWD and float((d["acc_map"].detach().double() - r["acc"]).abs().max()) < MB.BAR_FWD
    for k, g, gr in zip(MB.DENSITY_NAMES, grads, r["grads"]):
        err = MB.rel_err(g, gr)
        print(f"{name} {k:16s} fp32 oracle vs float64 reference {err:.2e}")
        assert err < MB.BAR_GRAD, (k, err)


def test_sample_keep_default_changes_nothing(tiny_arrays, hyper_tiny, tiny_dump):
    """execute(sample_keep=None) and a mask of ones are the function as it was: bit-identical outputs"""
    from oracle import tensorf_oracle as TO
    sc = TO.scene_from_arrays(tiny_arrays, **hyper_tiny)
    rays = torch.tensor(tiny_dump["rays"])
    a = TO.execute(sc, rays, N_samples=48)
    b = TO.execute(sc, rays, N_samples=48, sample_keep=torch.ones((rays.shape[0], 48)))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("name,mutation", MB.POWER)
def test_bar_has_power(name, mutation):
    """A defect of the chunk loop, applied to the reference alone, moves some density gradient by >= 10 x the 5e-4 bar on this case: the GPU comparison on the same
    case would fail by a wide margin if the kernel had it."""
    c = MB.KERNEL_CASES[name]()
    r, m = c.ref(), c.ref(mutation)
    moved = [MB.rel_err(a, b) for a, b in zip(m["grads"], r["grads"])]
    print(name, mutation, ["%.1e" % x for x in moved])
    assert max(moved) >= 10 * MB.BAR_GRAD, (name, mutation, moved)


def test_every_mutation_is_proven_on_some_case():
    assert {m for _, m in MB.POWER} == set(MB.MUTATIONS)
    assert {n for n, _ in MB.POWER} <= set(MB.KERNEL_CASES)
