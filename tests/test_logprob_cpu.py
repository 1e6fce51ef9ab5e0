"""CPU: tests/logprob_ref.py (the fp64 restatement the device log-probability stage is compared with) against the installed transformers:
HF's own processors and warpers, in the order generate() builds them, then torch.log_softmax in fp64 gathered at the id -- what
compute_transition_scores(sequences, out.scores / out.logits, normalize_logits=True) returns for one step.  These tests pin the
reference only (they need no library); the feature itself is tested on the GPU in tests/test_gpu_logprob.py.  The last test checks the
public surface -- the three C symbols in the ctypes table and the header, generate()'s keyword, the output class -- without a GPU."""
import numpy as np
import pytest
import torch

import logprob_ref as lr
import sampling_ref as sr


def _hf_scores(logits, banned, temperature, top_k, top_p, seen, penalty):
    """HF's list as _get_logits_processor orders it: repetition penalty, the banning processors, then temperature, top-k, top-p"""
    from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, SuppressTokensLogitsProcessor, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper)
    s = torch.from_numpy(np.asarray(logits, dtype=np.float32))[None].clone()
    ids = torch.tensor([[i for i in seen if i >= 0] if seen else [0]], dtype=torch.long)
    if penalty != 1.0:
        s = RepetitionPenaltyLogitsProcessor(penalty=penalty)(ids, s)
    if len(banned):
        s = SuppressTokensLogitsProcessor(list(banned), device="cpu")(ids, s)
    if temperature != 1.0:
        s = TemperatureLogitsWarper(float(temperature))(ids, s)
    if top_k:
        s = TopKLogitsWarper(top_k=top_k)(ids, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(top_p=top_p)(ids, s)
    return s[0]


CASES = [
    dict(temperature=1.0, top_k=0, top_p=1.0, penalty=1.0),
    dict(temperature=0.7, top_k=0, top_p=1.0, penalty=1.0),
    dict(temperature=1.0, top_k=5, top_p=1.0, penalty=1.0),
    dict(temperature=1.0, top_k=0, top_p=0.9, penalty=1.0),
    dict(temperature=1.0, top_k=0, top_p=1.0, penalty=1.3),
    dict(temperature=0.8, top_k=50, top_p=0.9, penalty=1.3),
]


@pytest.mark.parametrize("ban", [False, True], ids=["noban", "ban"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "T{temperature}-k{top_k}-p{top_p}-r{penalty}".format(**c))
def test_ref_equals_hf_log_softmax(case, ban):
    rng = np.random.default_rng(int(case["top_k"]) * 7 + int(case["top_p"] * 100) + int(ban))
    b, V = 3, 1000
    # distinct values: no ties at the k-th value or at the nucleus edge
    logits = np.stack([((rng.permutation(V) / V - 0.5) * 16 + rng.normal(0, 1e-6, V)).astype(np.float32) for _ in range(b)])
    n_cut = 0
    for r in range(b):
        seen = sorted(set(rng.integers(0, V, 60).tolist()) | {-200})
        order = np.argsort(-logits[r])
        banned = [int(order[0]), int(order[3])] + rng.integers(0, V, 20).tolist() if ban else []
        kw = dict(banned=banned, temperature=case["temperature"], top_k=case["top_k"], top_p=case["top_p"], seen=seen, penalty=case["penalty"])
        hf = _hf_scores(logits[r], banned, case["temperature"], case["top_k"], case["top_p"], seen, case["penalty"])
        hf_proc = torch.log_softmax(hf.double(), -1).numpy()
        hf_raw = torch.log_softmax(torch.from_numpy(logits[r]).double(), -1).numpy()
        mine = lr.scores(logits[r], **kw)
        assert np.array_equal(np.isfinite(mine), np.isfinite(hf.numpy())), "kept sets differ"
        # ids: the top, a seen one, a banned one, the least likely (cut by any top-k / top-p), a few at random
        ids = [int(order[0]), int(order[1]), seen[1], int(order[-1])] + rng.integers(0, V, 8).tolist() + (banned[:2] if ban else [])
        for i in ids:
            assert lr.raw(logits[r], i) == pytest.approx(hf_raw[i], rel=1e-12, abs=1e-12)
            got = lr.processed(logits[r], i, **kw)
            if np.isinf(hf_proc[i]):
                assert got == -np.inf
                n_cut += 1
            else:
                assert got == pytest.approx(hf_proc[i], rel=1e-12, abs=1e-12)
    if ban or case["top_k"] or case["top_p"] < 1.0:
        assert n_cut > 0          # an id that was cut (or banned) was among those checked: -inf, as HF


def test_top_k_1_keeps_the_maxima_only():
    x = np.array([0.5, 2.0, -1.0, 2.0], dtype=np.float32)
    assert lr.processed(x, 1, top_k=1) == pytest.approx(-np.log(2.0))
    assert lr.processed(x, 0, top_k=1) == -np.inf
    hf = _hf_scores(x, [], 1.0, 1, 1.0, None, 1.0)
    assert torch.log_softmax(hf.double(), -1)[1].item() == pytest.approx(lr.processed(x, 1, top_k=1))


def test_device_threshold_can_replace_the_refs():
    rng = np.random.default_rng(2)
    x = rng.normal(0, 3, 500).astype(np.float32)
    thr = sr.threshold(sr.processed(x, 0.7), 20, 0.9)
    i = int(np.argmax(x))
    assert lr.processed(x, i, temperature=0.7, top_k=20, top_p=0.9) == lr.processed(x, i, temperature=0.7, thr=thr)


def test_all_minus_inf_but_one_is_exactly_zero():
    x = np.full(37, -np.inf, dtype=np.float32)
    x[11] = 3.25
    assert lr.raw(x, 11) == 0.0 and lr.raw(x, 5) == -np.inf
    assert lr.processed(np.zeros(37, dtype=np.float32), 11, banned=[i for i in range(37) if i != 11]) == 0.0


def test_public_surface_has_the_feature():
    import inspect
    import os
    from omchat_amd import _lib
    from omchat_amd.engine import Engine
    from omchat_amd.model import omchat_qwen2 as mq
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omchat_hip.h")).read()
    for name in ("omchat_set_logprobs", "omchat_read_logprobs", "omchat_op_token_logprob"):
        assert name in _lib._SIGS and name + "(" in header
    for name in ("set_logprobs", "logprobs_off", "read_logprobs"):
        assert callable(getattr(Engine, name))
    assert "output_logprobs" in inspect.signature(mq.OmChatQwen2ForCausalLM.generate).parameters
    out = mq.GenerateOutput(torch.zeros(1, 3), torch.zeros(1, 2), torch.ones(1, 2))
    assert out["logprobs"] is out.logprobs and out["processed_logprobs"] is out.processed_logprobs and out["sequences"] is out.sequences
