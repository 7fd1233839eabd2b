"""bench.py's plain run, --full and --dump-outputs: the row sampling on the CPU, and two small runs on the GPU (fresh
child processes: the command line is what is under test)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_sampling_is_whole_below_the_cap_and_a_fixed_draw_above():
    import bench

    small = torch.arange(24, dtype=torch.float64).reshape(2, 4, 3)
    out = bench._rows_sample(small, 1 << 10)
    assert out.dtype == torch.float32 and out.shape == small.shape and torch.equal(out, small.float())
    assert bench._rows_sample(torch.tensor(2.5), 4).shape == ()

    big = torch.arange(1000 * 5, dtype=torch.float32).reshape(1000, 5)
    a, b = bench._rows_sample(big, 100 * 5 * 4), bench._rows_sample(big.clone(), 100 * 5 * 4)
    assert a.shape == (100, 5) and a.numel() * 4 <= 100 * 5 * 4
    assert torch.equal(a, b)  # same shape, same rows
    assert bool((a[:, 0] % 5 == 0).all()) and bool((a[1:, 0] >= a[:-1, 0]).all())  # whole rows, in order

    img = torch.rand(40, 30, 3)
    px = bench._rows_sample(img, 200 * 3 * 4, image=True)  # an image above the cap: a sample of its pixels
    assert px.shape == (200, 3)
    assert bench._rows_sample(img, 10 * 30 * 3 * 4).shape == (10, 30, 3)  # any other array: of its rows


SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--n-splats", "2000", "--n-texels", "1e5", "--height", "96",
         "--width", "80"]


def _run_bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, "--dump-outputs", str(out_dir), *extra]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert res.returncode == 0 and len(lines) == 1, res.stderr[-2000:]
    rec = json.loads(lines[0])
    files = sorted(p.name for p in out_dir.iterdir())
    assert files == [n + ".npy" for n in rec["outputs"]]
    return rec, {n: np.load(out_dir / (n + ".npy")) for n in rec["outputs"]}


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    return _run_bench(tmp_path_factory.mktemp("plain") / "outputs")


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_one_steps_outputs(plain_run):
    rec, arrays = plain_run
    assert rec["steps"] == 3 and rec["warmup"] == 2 and len(rec["step_ms_events"]) == 3
    assert rec["unit"] == "Mpix/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(96 * 80 / (rec["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    # a plain run measures nothing beside the timed steps
    assert rec["full"] is False
    assert rec["roofline"] is None and rec["sub"] is None and rec["cpu_baseline"] is None and rec["counts"] is None

    groups = ("xyz", "features_rest", "opacity", "scaling", "rotation", "texture_dc")
    assert set(arrays) == {"loss", "rgb"} | {f"grad_{g}" for g in groups} | {f"adam_m_{g}" for g in groups}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64e6
    assert arrays["loss"].shape == () and arrays["loss"] > 0
    rgb = arrays["rgb"]
    assert rgb.shape == (96, 80, 3) and rgb.min() >= 0 and rgb.max() <= 1 and rgb.std() > 0
    assert arrays["grad_xyz"].shape == (2000, 3) and arrays["grad_features_rest"].shape == (2000, 15, 3)
    assert arrays["grad_texture_dc"].shape == arrays["adam_m_texture_dc"].shape
    assert arrays["grad_texture_dc"].shape[1] == 3
    for g in groups:
        # the dumped step starts from a fresh optimizer state: Adam's first moment is (1 - beta1) * gradient, for the
        # texels too (their deferred update has run)
        gr, m = arrays[f"grad_{g}"], arrays[f"adam_m_{g}"]
        assert np.abs(gr).max() > 0, g
        assert np.abs(m - np.float32(0.1) * gr).max() <= 1e-6 * np.abs(gr).max(), g


@pytest.mark.gpu
def test_full_run_adds_its_records_and_dumps_the_same_outputs(plain_run, tmp_path):
    """bench.py --full at small size (the sub-records have fixed sizes of their own, seconds each: --no-sub), and the
    dump of a second run with the same workload arguments.  Each run's gradients are held within 1e-5 of the fp64
    oracle (the parity tests' criterion, max-element and norm-wise), so two runs may differ by 2e-5 of an array's
    largest element at the most; the forward is held to 1e-5 per element likewise."""
    _, first = plain_run
    rec, arrays = _run_bench(tmp_path / "outputs", "--full", "--no-sub", "--cpu-crop", "32")
    assert rec["full"] is True and rec["sub"] is None
    assert rec["roofline"]["kernel"] in ("raster_fwd", "raster_bwd") and rec["roofline"]["achieved"] > 0
    assert rec["counts"]["P"] == 96 * 80 and rec["counts"]["N_v"] > 0
    assert rec["cpu_baseline"]["value"] > 0
    assert {"raster_fwd", "raster_bwd"} <= set(rec["kernel_ms"])
    assert set(arrays) == set(first)
    for name, a in arrays.items():
        b = first[name]
        assert a.shape == b.shape, name
        assert np.abs(a.astype(np.float64) - b).max() <= 2e-5 * np.abs(b).max(), name
