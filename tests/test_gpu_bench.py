"""GPU: bench.py as later measurements call it -- a plain run (no --full) at the tiny geometry: --steps sets the timed steps, the line holds
ms_per_step and none of the --full side measurements, and --dump-outputs writes the last timed step's outputs, identical from run to run."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest
from conftest import ROOT


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--tiny", "--gpus", "1", "--steps", "2", "--warmup", "1", "--gen", "4",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_plain_run_line_and_dumped_outputs(gpu_lib, tmp_path):
    from omchat_amd.config import tiny
    cfg = tiny()
    d = _plain_run(tmp_path / "a")
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 4) < 1e-6                   # tokens/s x s per step = the 4 tokens of a step
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in d
    for k in ("configs2", "configs3", "configs4", "fp8_decode", "generate", "frontend_ms_p50", "cpu_baseline"):
        assert k not in d, k
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["image_features.npy", "prefill_logits.npy", "tokens.npy"]
    a = {f: np.load(tmp_path / "a" / f) for f in files}
    assert a["tokens.npy"].dtype == np.float64 and a["tokens.npy"].shape == (1, 4)
    assert a["prefill_logits.npy"].dtype == np.float32 and a["prefill_logits.npy"].shape == (1, cfg.text["vocab_size"])
    assert a["image_features.npy"].dtype == np.float32
    assert a["image_features.npy"].shape == (3, cfg.num_image_tokens, cfg.text["hidden_size"])
    assert all(np.isfinite(x).all() for x in a.values())
    assert a["tokens.npy"][0, 0] == np.argmax(a["prefill_logits.npy"][0])       # the first id is the greedy pick of the prefill logits
    _plain_run(tmp_path / "b")
    for f, x in a.items():
        assert np.array_equal(np.load(tmp_path / "b" / f), x), f                   # seeded inputs, deterministic kernels
