"""bench.py's ``--dump-outputs`` writer and its ``--full`` switch, on the CPU: the writer on stand-in step outputs
(float32 / float64 ``.npy`` files, a fixed seeded sample of the large arrays, the same positions in every call), and
the command line (both options exist, ``--steps`` below 1 is refused before anything touches a GPU)."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _step_outputs(seed):
    g = torch.Generator().manual_seed(seed)
    n = bench.DUMP_SAMPLE
    logits = torch.randn(3, 7, n // 16, generator=g).to(torch.bfloat16)[:, :, :-3]  # a strided view, > the sample
    out = types.SimpleNamespace(loss=torch.tensor(2.5), loss_lm=torch.tensor(2.25), loss_emotion=None,
                                emotion_logits=torch.randn(3, 7, generator=g), logits_bf16=logits, logits=None)
    model = types.SimpleNamespace(flat=torch.randn(n // 2, generator=g))  # smaller than the sample: kept whole
    return out, model, torch.tensor([7.5, 6.75]), torch.tensor([5])


def test_dump_outputs_files_dtypes_and_fixed_sample(tmp_path):
    out, model, acc, correct = _step_outputs(1)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, out, model, acc, correct, seed=0)
    bench.dump_outputs(b, out, model, acc, correct, seed=0)
    names = sorted(os.listdir(a))
    assert names == ["emotion_logits.npy", "logits.npy", "loss.npy", "loss_lm.npy", "params.npy", "train_metrics.npy"]
    total = 0
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype in (np.float32, np.float64), (n, x.dtype)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), n
        total += x.nbytes
    assert total <= 64 << 20
    logits = np.load(os.path.join(a, "logits.npy"))
    assert logits.shape == (bench.DUMP_SAMPLE,)
    # the sample is of the logical [B,S,V] array (the padding columns of the view's storage never appear) ...
    flat = out.logits_bf16.float().reshape(-1)
    idx = torch.randint(0, flat.numel(), (bench.DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
    assert np.array_equal(logits, flat[idx].numpy())
    # ... and small outputs are whole and exact
    assert np.array_equal(np.load(os.path.join(a, "params.npy")), model.flat.numpy())
    assert np.array_equal(np.load(os.path.join(a, "emotion_logits.npy")), out.emotion_logits.numpy())
    assert np.load(os.path.join(a, "loss.npy")) == np.float32(2.5)
    assert np.array_equal(np.load(os.path.join(a, "train_metrics.npy")), np.array([7.5, 6.75, 5.0]))


def test_bench_command_line_has_full_and_dump_outputs():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs DIR" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--full", "--dump-outputs", "x", "--steps", "0"],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr, r.stderr
