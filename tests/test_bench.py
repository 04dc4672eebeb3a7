"""bench.py's own contract: the plain run's ONE result line (the headline fields, strict JSON, short enough for a driver that keeps the tail
of stdout) and --dump-outputs (what the last timed step returned, float32, under 64 MB in all)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


def test_dump_outputs_keeps_a_frame_whole_and_samples_a_larger_batch_alike(tmp_path):
    """A frame's outputs are written whole; a batch beyond the cap (N = 8 weak scaling: 8 frames, 82 MB) keeps the same seeded rows of every
    array, in order, under 64 MB in all, and the same rows on every run."""
    import bench
    rng = np.random.default_rng(3)
    small = {"rgb": torch.from_numpy(rng.random((1000, 3), dtype=np.float32)), "depth": torch.from_numpy(rng.random(1000, dtype=np.float32))}
    bench.dump_outputs(str(tmp_path / "small"), small)
    for k, v in small.items():
        a = np.load(tmp_path / "small" / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, v.numpy())
    n = 8 * 640000
    rows = torch.arange(n, dtype=torch.float32)                                  # row i holds i (rgb) and -i (depth): exact in fp32 below 2^24
    big = {"rgb": rows[:, None].expand(n, 3).contiguous(), "depth": -rows}
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), big)
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64_000_000
    rgb, depth = np.load(tmp_path / "a" / "rgb.npy"), np.load(tmp_path / "a" / "depth.npy")
    assert rgb.dtype == depth.dtype == np.float32 and rgb.shape[1] == 3 and rgb.shape[0] == depth.shape[0] > n // 2
    assert np.all(np.diff(depth) < 0) and np.array_equal(rgb[:, 0], -depth) and np.array_equal(rgb[:, 2], -depth)    # the same rows, in order
    for k in ("rgb", "depth"):
        assert np.array_equal(np.load(tmp_path / "b" / f"{k}.npy"), np.load(tmp_path / "a" / f"{k}.npy"))


def _no_constant(c):
    raise ValueError(f"{c} is not JSON")


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_run_prints_the_headline_line_and_dumps_the_last_timed_frame(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` on a small frame: one short strict-JSON line on stdout with the headline
    fields and nothing that --full measures; DIR holds exactly the pixels of the last timed step (pose (W + K - 1) % 8) as a direct render
    of the same rays gives them."""
    import bench
    img, steps, warmup = 96, 3, 2
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--img", str(img), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and len(lines[0]) < 4096, r.stdout[-2000:]
    d = json.loads(lines[0], parse_constant=_no_constant)
    assert d["metric"] == "ray_samples_per_sec" and d["unit"] == "ray-samples/s" and d["higher_is_better"] is True and d["dtype"].startswith("f32")
    assert d["steps"] == steps and d["warmup"] == warmup and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(img * img * 512 / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert not {"roofline", "roofline_all", "effective", "arith_modes", "frame_stream_two_in_flight", "other_configs"} & set(d)
    assert d["cpu_baseline"] is None
    model, _, A = bench.build_model(torch.device("cuda"))
    rays = bench.frames(dict(A, img_wh=(img, img)))[(warmup + steps - 1) % bench.N_POSES].cuda()
    rgb, depth = model.render_rays(rays, white_bg=True, N_samples=A["N_samples"])
    for name, want in (("rgb", rgb), ("depth", depth)):
        got = np.load(out / f"{name}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, want.cpu().numpy()), name
