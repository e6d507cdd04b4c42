"""bench.py's command line and its output dump, without a GPU: --full and --dump-outputs exist,
and dump_outputs writes float32 .npy files of bounded size whose sampled elements depend on the
buffers' lengths alone (two builds dump the same elements)."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in r.stdout


def test_dump_outputs_files_and_fixed_sample(tmp_path):
    import bench
    n = bench.DUMP_SAMPLE + 12345
    g = torch.Generator().manual_seed(0)
    arena = types.SimpleNamespace(grad=torch.randn(n, generator=g), flat=torch.randn(n, generator=g))
    logits = torch.randn(4, 3, generator=g).to(torch.bfloat16)
    loss = torch.tensor(0.75)
    bench.dump_outputs(str(tmp_path / "a"), logits, loss, arena)
    got = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["grads_sample.npy", "logits.npy", "loss.npy", "params_sample.npy"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert np.array_equal(got["logits.npy"], logits.float().numpy()) and got["loss.npy"].tolist() == [0.75]
    idx = np.sort(np.random.default_rng(0).choice(n, bench.DUMP_SAMPLE, replace=False))
    assert np.array_equal(got["grads_sample.npy"], arena.grad.numpy()[idx])
    assert np.array_equal(got["params_sample.npy"], arena.flat.numpy()[idx])
    # a buffer that fits is written whole, under its plain name
    small = types.SimpleNamespace(grad=arena.grad[:1000], flat=arena.flat[:1000])
    bench.dump_outputs(str(tmp_path / "b"), logits, loss, small)
    assert np.array_equal(np.load(tmp_path / "b" / "grads.npy"), small.grad.numpy())
    assert np.array_equal(np.load(tmp_path / "b" / "params.npy"), small.flat.numpy())
