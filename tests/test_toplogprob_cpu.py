"""CPU: tests/toplogprob_ref.py (the restatement the device's top-n alternatives and scored ids are compared with) against torch, its tie
rule, and -- without a GPU -- the public surface of the feature and generate()'s host-side refusals.  The feature itself is tested on the
GPU in tests/test_gpu_toplogprob.py."""
import inspect
import os
import types

import numpy as np
import pytest
import torch

import logprob_ref as lr
import toplogprob_ref as tr


@pytest.mark.parametrize("V,n", [(1000, 1), (1000, 5), (1000, 20), (37, 20), (20, 20)])
def test_ref_equals_torch_topk_on_tie_free_rows(V, n):
    rng = np.random.default_rng(V + n)
    for _ in range(3):
        x = ((rng.permutation(V) / V - 0.5) * 16 + rng.normal(0, 1e-6, V)).astype(np.float32)
        assert len(set(x.tolist())) == V
        vals, ids = torch.topk(torch.log_softmax(torch.from_numpy(x).double(), -1), n)
        r_ids, r_vals = tr.top(x, n)
        assert np.array_equal(r_ids, ids.numpy())
        assert np.allclose(r_vals, vals.numpy(), rtol=1e-12, atol=1e-12)
        for i in r_ids[:3]:
            assert tr.values(x, [i])[0] == lr.log_softmax_at(x, int(i))


def test_tie_rule_on_a_row_of_8_values():
    rng = np.random.default_rng(8)
    x = np.clip(np.round(rng.standard_normal(500) * 2), -4, 3).astype(np.float32)
    x[(x == 0) & (rng.random(500) < 0.5)] = -0.0                       # both zeros: one value
    assert len(set(np.abs(x[x == 0]).tolist()) | set(x[x != 0].tolist())) == 8 and np.signbit(x[x == 0]).any()
    ids, vals = tr.top(x, 20)
    for a, b in zip(ids[:-1], ids[1:]):
        assert x[a] > x[b] or (x[a] == x[b] and a < b)                 # (== compares -0 and +0 equal)
    assert list(ids) == [int(i) for i in np.flatnonzero(x == x.max())[:20]]      # 3.0 is held by more than 20 ids: the first 20 of them
    assert np.all(np.diff(vals) <= 0)


def test_minus_inf_ranks_behind_every_finite_value_and_n_equals_V():
    x = np.array([1.0, -np.inf, 3.0, -np.inf, -2.0, 3.0], dtype=np.float32)
    ids, vals = tr.top(x, 6)
    assert list(ids) == [2, 5, 0, 4, 1, 3]
    assert np.isfinite(vals[:4]).all() and (vals[4:] == -np.inf).all()
    assert np.exp(vals[:4]).sum() == pytest.approx(1.0)
    assert list(tr.scored(x, [3, 0])) == [-np.inf, lr.log_softmax_at(x, 0)]


def test_public_surface_has_the_feature():
    from omchat_amd import _lib
    from omchat_amd.engine import Engine
    from omchat_amd.model import omchat_qwen2 as mq
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omchat_hip.h")).read()
    for name in ("omchat_set_logprobs_ex", "omchat_read_logprob_extras", "omchat_op_top_logprobs"):
        assert name in _lib._SIGS and name + "(" in header
    assert "#define OMCHAT_LP_MAX_TOP 20" in header and "#define OMCHAT_LP_MAX_SCORED 32" in header
    p = inspect.signature(Engine.set_logprobs).parameters
    assert p["top_n"].default == 0 and p["score_token_ids"].default is None
    assert callable(Engine.read_logprob_extras) and callable(Engine.logprobs_off)
    p = inspect.signature(mq.OmChatQwen2ForCausalLM.generate).parameters
    assert "top_logprobs" in p and "score_token_ids" in p
    out = mq.GenerateOutput(torch.zeros(1, 3), torch.zeros(1, 2), torch.ones(1, 2))      # the three-positional form
    for name in ("top_logprobs", "top_token_ids", "scored_logprobs"):
        assert name not in out and not hasattr(out, name)                                # present only when asked for
    t = torch.zeros(1, 2, 5)
    out.add("top_logprobs", t)
    assert out["top_logprobs"] is t and out.top_logprobs is t and "scored_logprobs" not in out


def test_host_side_refusals():
    from omchat_amd.model.omchat_qwen2 import resolve_logprob_extras as res
    gc = types.SimpleNamespace()
    V = 320
    assert res(gc, False, None, None, V) == (0, [])
    assert res(gc, True, None, None, V) == (0, [])
    assert res(gc, True, 5, [0, 7, V - 1], V) == (5, [0, 7, V - 1])
    assert res(gc, True, None, torch.tensor([3, 4]), V) == (0, [3, 4])
    assert res(types.SimpleNamespace(top_logprobs=3, score_token_ids=[9]), True, None, None, V) == (3, [9])      # generation_config
    for kw in (dict(top_logprobs=5), dict(score_token_ids=[1])):                         # either without output_logprobs=True
        with pytest.raises(ValueError):
            res(gc, False, kw.get("top_logprobs"), kw.get("score_token_ids"), V)
    for n in (0, 21, -1, 2.5, True):
        with pytest.raises(ValueError):
            res(gc, True, n, None, V)
    with pytest.raises(ValueError):
        res(gc, True, 20, None, 12)                                                      # more alternatives than the vocabulary holds
    for ids in ([], list(range(33)), [4, 4], [-1], [V], [0, V + 5]):
        with pytest.raises(ValueError):
            res(gc, True, None, ids, V)
