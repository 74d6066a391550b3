"""bench.py --dump-outputs: the arrays the last timed step computed, written so that two builds can be compared file for file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, record_err


def test_dump_outputs_writes_small_outputs_whole_and_a_fixed_sample_of_large_ones(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    small = torch.arange(12, dtype=torch.float16).reshape(3, 4)
    big = torch.randn(50, 100, dtype=torch.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big})
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (3, 4) and np.array_equal(s, small.float().numpy())
    b = np.load(tmp_path / "a" / "big.npy")
    assert b.dtype == np.float32 and b.ndim == 1 and 900 < b.size <= 1000
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))                       # the same positions in every run
    idx = np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, big.numel(), 1000))
    assert np.array_equal(b, big.reshape(-1)[idx].float().numpy())


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_refuses_a_step_count_it_cannot_time(args, monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + args)
    with pytest.raises(SystemExit) as e:
        bench.parse()
    assert e.value.code == 2


@pytest.mark.gpu
def test_dumped_outputs_are_what_the_timed_step_computed(gpu, tmp_path):
    """at a size whose outputs are written whole: the forward volume equals the CPU oracle on the bench's own seeded inputs, and a
    train step writes the volume and every gradient its caller receives"""
    import bench
    from oracle import cport
    B, S, C, V, HW = 2, 16, 256, 4, 12
    common = ["--batch", str(B), "--grid", str(S), "--channels", str(C), "--views", str(V), "--feat", str(HW),
              "--steps", "3", "--warmup", "1", "--soak-ms", "0", "--no-cpu-baseline", "--no-backward"]

    def run(extra, d):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common + extra + ["--dump-outputs", str(d)],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        line = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0

    run([], tmp_path / "fwd")
    vol = np.load(tmp_path / "fwd" / "volume.npy")
    assert vol.dtype == np.float32 and vol.shape == (B, C, S, S, S)
    torch.manual_seed(0)                                                                  # bench.py's rank-0 inputs
    feats = torch.randn(B, V, C, HW, HW, device=gpu).cpu().numpy()
    ref = cport.forward(feats, bench.ring_projections(B, V, (HW, HW), seed=0), bench.cuboid_volume(B, S), "softmax")
    record_err("bench --dump-outputs volume vs oracle", float(np.abs(vol - ref).max()), 1e-4)

    run(["--train-step"], tmp_path / "train")
    names = sorted(os.listdir(tmp_path / "train"))
    assert names == ["grad_features.npy", "grad_process_feature_0_bias.npy", "grad_process_feature_0_weight.npy", "volume.npy"]
    shapes = {"grad_features.npy": (B, V, C, HW, HW), "grad_process_feature_0_bias.npy": (C,),
              "grad_process_feature_0_weight.npy": (C, C, 1, 1), "volume.npy": (B, C, S, S, S)}
    for n in names:
        a = np.load(tmp_path / "train" / n)
        assert a.dtype == np.float32 and a.shape == shapes[n] and np.isfinite(a).all() and np.abs(a).max() > 0, n
