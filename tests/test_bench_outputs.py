"""bench.py's plain run and --dump-outputs: a plain run measures the headline
figure only (what stands beside it is null without --full), --steps is the
number of timed steps, and the dumped flows are what a caller of the timed
path receives: float32, the same from run to run, within the size limit."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("roofline", "cpu_baseline", "tolerance_mode", "pipelined", "hbm_measured_peak", "box_state",
             "gather", "max_epe_vs_oracle")


@pytest.fixture(scope="module")
def bench_mod():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_sample_is_seeded_and_float32(bench_mod, tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(bench_mod, "DUMP_SAMPLE_PIXELS", 1000)
    B, H, W = 3, 37, 53  # 5883 pixels > 1000: sampled
    out = torch.arange(B * H * W * 2, dtype=torch.float32).view(B, H, W, 2)
    info = [bench_mod.dump_outputs(str(tmp_path / d), out, 0, 1) for d in ("a", "b")]
    assert info[0]["files"] == info[1]["files"] and sorted(info[0]["files"]) == ["flow_pair0.npy", "flow_sample.npy"]
    a0, a1 = (np.load(tmp_path / d / "flow_pair0.npy") for d in ("a", "b"))
    s0, s1 = (np.load(tmp_path / d / "flow_sample.npy") for d in ("a", "b"))
    assert a0.dtype == s0.dtype == np.float32
    assert np.array_equal(a0, out[0].numpy()) and np.array_equal(a0, a1)
    assert s0.shape == (1000, 2) and np.array_equal(s0, s1)
    # every sampled vector is one (x, y) pair of `out`, each position drawn once, over all pairs
    pix = s0[:, 0].astype(np.int64) // 2
    assert np.array_equal(s0[:, 1], s0[:, 0] + 1) and len(np.unique(pix)) == 1000
    assert pix.min() < H * W and pix.max() >= 2 * H * W
    # no more pixels than the sample holds: written whole; other ranks name their files
    monkeypatch.setattr(bench_mod, "DUMP_SAMPLE_PIXELS", B * H * W)
    info = bench_mod.dump_outputs(str(tmp_path / "c"), out, 1, 2)
    assert sorted(info["files"]) == ["flow_pair0_rank1.npy", "flow_sample_rank1.npy"]
    assert np.array_equal(np.load(tmp_path / "c" / "flow_sample_rank1.npy"), out.view(-1, 2).numpy())


def test_dump_at_bench_shape_fits_64_mb(bench_mod):
    W, H = 1920, 1080  # the flagship shape; two .npy headers of 128 bytes
    assert (bench_mod.DUMP_SAMPLE_PIXELS * 2 + H * W * 2) * 4 + 2 * 128 <= 64 * 10**6


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_callers_flows(tmp_path):
    W, H, B, K = 320, 240, 2, 3
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(K), "--warmup", "1", "--warmup-floor", "0",
                        "--batch", str(B), "--width", str(W), "--height", str(H), "--dump-outputs", str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["steps"] == K and line["full"] is False and line["dtype"] == "f32" and line["higher_is_better"]
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - B / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert all(line[k] is None for k in FULL_ONLY), {k: line[k] for k in FULL_ONLY if line[k] is not None}
    pair0 = np.load(tmp_path / "flow_pair0.npy")
    sample = np.load(tmp_path / "flow_sample.npy")
    assert pair0.dtype == sample.dtype == np.float32 and pair0.shape == (H, W, 2)
    assert sample.shape == (B * H * W, 2)  # fewer pixels than the sample size: all of them
    import disflow
    eng = disflow.DenseInverseSearch(disflow.preset_params(disflow.Preset.MEDIUM, W, H), W, H, max_batch=1)
    for k in range(B):
        want = eng.calc(*disflow.synth_pair(k, W, H))
        got = sample.reshape(B, H, W, 2)[k]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
    eng.close()
    assert np.array_equal(pair0, sample.reshape(B, H, W, 2)[0])
