"""bench.py's command line and --dump-outputs writer, without a GPU (the timed run itself: tests/test_gpu_fullsize.py)."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_options_are_listed_and_steps_are_checked():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in r.stdout, opt
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr, r.stderr[-2000:]


def test_dump_writes_small_outputs_whole(tmp_path):
    t = torch.randn(2, 3, 5, 7).to(torch.bfloat16).permute(0, 1, 3, 2)            # a non-contiguous view, as a channels-last output
    got = bench.dump_outputs(t, str(tmp_path), max_values=1000)
    assert got == {"out": ([2, 3, 7, 5], 210)}
    a = np.load(tmp_path / "out.npy")
    assert a.dtype == np.float32 and a.shape == (2, 3, 7, 5)
    assert np.array_equal(a, t.float().numpy())


def test_dump_samples_large_outputs_the_same_way_every_time(tmp_path):
    t = torch.randn(1, 4, 64, 64)
    outs = []
    for run in ("a", "b"):
        got = bench.dump_outputs(t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), str(tmp_path / run), max_values=4096)
        assert got == {"out": ([1, 4, 64, 64], 4096)}
        outs.append(np.load(tmp_path / run / "out.npy"))
    assert outs[0].dtype == np.float32 and outs[0].shape == (4096,)
    assert np.array_equal(outs[0], outs[1])
    # the sample is drawn in the tensor's logical order: every value is the output's own, and they are spread over it
    g = torch.Generator().manual_seed(bench.DUMP_SEED)
    idx = torch.randint(0, t.numel(), (4096,), generator=g).sort().values
    assert np.array_equal(outs[0], t.reshape(-1)[idx].numpy())
    assert int(idx[0]) < t.numel() // 64 and int(idx[-1]) >= t.numel() - t.numel() // 64


def test_dump_of_micro_batches_stays_within_the_cap(tmp_path):
    parts = [torch.randn(2, 8, 32, 32) for _ in range(3)]
    got = bench.dump_outputs(parts, str(tmp_path), max_values=3000)
    assert sorted(got) == ["out0", "out1", "out2"] and sum(n for _, n in got.values()) <= 3000
    assert sorted(os.listdir(tmp_path)) == ["out0.npy", "out1.npy", "out2.npy"]
    assert bench.DUMP_MAX_VALUES * 4 <= 64 * 10 ** 6                               # bytes written by a default dump, in all
