"""The long-K GEMV's counted pipeline (gemv_rows_longk_body, DESIGN.md section 17 "The long-K form's pass") computes the bits of the loop it
replaced: every case of tools/longk_golden.py -- every pass count from 2 to 8 (passes of eight chunks) and from 4 to 16 (passes of four), so
every peeled ending and both parities of the repeated part, in 16-bit bf16 and f16, e4m3, MXFP4 and bf16x12, and the real grid -- recomputed on
the loaded library against tests/golden/longk_parent_bits.npz, which the build of the commit before the pipeline wrote; the coded launch against
the 16-bit launch on the same cases; and a decode step with the MLP at 9 and at 37 chunks, tuning key 50 = 7 against 0."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from conftest import golden, ROOT
from gpu_util import randn, rnd, synth_state_dict
from omchat_amd import synth, _lib
from omchat_amd.config import tiny
from omchat_amd.engine import Engine

sys.path.insert(0, os.path.join(ROOT, "tools"))
import longk_golden as LG

_done = {}


def _bits(lib, form, N, K):
    """one launch per case and session, shared by the tests below"""
    k = LG.key(form, N, K)
    if k not in _done:
        _done[k] = LG.run(lib, form, N, K)
    return _done[k]


@pytest.mark.parametrize("form,N,K", LG.CASES, ids=[LG.key(*c) for c in LG.CASES])
def test_bits_of_the_parent(gpu_lib, form, N, K):
    g = golden("longk_parent_bits")
    assert int(g["seed"]) == LG.SEED
    want, got = g[LG.key(form, N, K)], _bits(gpu_lib, form, N, K)
    assert want.shape == (N,) and np.array_equal(want, got), np.nonzero(want != got)[0][:8].tolist()


@pytest.mark.parametrize("N,K", [(N, K) for f, N, K in LG.CASES if f == "bf16x12"])
def test_coded_rows_against_the_16_bit_launch(gpu_lib, N, K):
    """the invariant of tests/test_gpu_bf16x12_longk.py on the new pass counts; rows 10 and 16 (+inf) and 11 (-inf at weight 5) are infinite
    where the 16-bit form has no clamped chunk (K % 4096 == 0) -- an extra w * 0 term would turn them NaN"""
    y16, y12 = _bits(gpu_lib, "bf16", N, K), _bits(gpu_lib, "bf16x12", N, K)
    assert np.array_equal(y16, y12), np.nonzero(y16 != y12)[0][:8].tolist()
    y = torch.from_numpy(y12.view(np.int16).copy()).view(torch.bfloat16).float()
    assert bool(torch.isinf(y[10]))
    for r in (11, 16):
        assert bool(torch.isinf(y[r])) if K % 4096 == 0 else bool(torch.isnan(y[r]))
    keep = torch.ones(N, dtype=torch.bool)
    keep[[10, 11, 16]] = False
    assert bool(torch.isfinite(y[keep]).all())


@pytest.mark.parametrize("mlp_t", [4608, 18944])
def test_decode_step_key_50(gpu_lib, mlp_t):
    """a decode step of the tiny text geometry with the MLP at 9 and at 37 chunks, key 50 = 7 (coded down_proj) against 0 (16-bit), eager
    and captured: ids and fp32 logits bit-equal"""
    from test_gpu_graph import _run
    cfg = tiny(mlp_t=mlp_t)
    assert cfg.text["intermediate_size"] == mlp_t
    lib = _lib.lib()
    sd = synth_state_dict(cfg, 3, lambda k: not k.startswith(synth.TOWER) and "mm_projector" not in k)
    e = Engine(cfg, dtype="bf16", max_seq=256, max_batch=1, vision=False)
    e.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    x = rnd(randn((1, 10, cfg.text["hidden_size"]), 1, 0.5), "bf16")
    first = torch.tensor([5], dtype=torch.int32)
    default, n0 = e.bf16x12_stats()["roles"], e.bf16x12_stats()["launches"][1]
    runs, counts = [], []
    try:
        for k50 in (7, 0):
            lib.omchat_op_set_tuning(50, k50)
            for graph in (False, True):
                e.enable_decode_graph(graph)
                runs.append(_run(e, x, [x.shape[1]], first, 8, True))
                e.enable_decode_graph(False)
            counts.append(e.bf16x12_stats()["launches"][1])
    finally:
        lib.omchat_op_set_tuning(50, default)
    for t, l in runs[1:]:
        assert torch.equal(t, runs[0][0]) and torch.equal(l.view(torch.int32), runs[0][1].view(torch.int32))
    assert counts[0] - n0 >= 8 * cfg.text["num_hidden_layers"] and counts[1] == counts[0]      # key on: the coded launch ran; key off: it did not
    e.close()
