"""CPU: tests/sampling_ref.py (the restatement the GPU sampler is pinned to, bit for bit) against HF's own logits processors, and the draw
against the categorical it claims to sample."""
import numpy as np
import pytest
import torch

import sampling_ref as sr


def _hf(logits, temperature, top_k, top_p, seen, penalty):
    from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    s = torch.from_numpy(np.asarray(logits, dtype=np.float32))[None].clone()
    ids = torch.tensor([[i for i in seen if i >= 0] if seen else [0]], dtype=torch.long)     # HF's gather cannot take the -200 sentinel
    if penalty != 1.0:
        s = RepetitionPenaltyLogitsProcessor(penalty=penalty)(ids, s)
    if temperature != 1.0:
        s = TemperatureLogitsWarper(float(temperature))(ids, s)
    if top_k:
        s = TopKLogitsWarper(top_k=top_k)(ids, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(top_p=top_p)(ids, s)
    keep = torch.isfinite(s[0]).numpy()
    p = torch.softmax(s[0].double(), dim=-1).numpy()
    return keep, p


def _tie_free_logits(rng, V, scale):
    # distinct values spaced far beyond fp32 rounding: no ties by construction, at the k-th value nor anywhere else
    v = rng.permutation(V).astype(np.float64) / V
    return ((v - 0.5) * scale + rng.normal(0, 1e-3 / V, V)).astype(np.float32)


CASES = [
    dict(temperature=1.0, top_k=0, top_p=1.0, penalty=1.0),
    dict(temperature=0.7, top_k=0, top_p=1.0, penalty=1.0),
    dict(temperature=1.0, top_k=50, top_p=1.0, penalty=1.0),
    dict(temperature=0.8, top_k=1000, top_p=1.0, penalty=1.0),
    dict(temperature=1.0, top_k=0, top_p=0.5, penalty=1.0),
    dict(temperature=0.6, top_k=0, top_p=0.9, penalty=1.0),
    dict(temperature=1.3, top_k=0, top_p=0.999, penalty=1.0),
    dict(temperature=0.9, top_k=50, top_p=0.9, penalty=1.0),
    dict(temperature=1.0, top_k=0, top_p=1.0, penalty=1.3),
    dict(temperature=0.7, top_k=40, top_p=0.8, penalty=1.3),
]


@pytest.mark.parametrize("V", [152064, 1001, 37])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "T{temperature}-k{top_k}-p{top_p}-r{penalty}".format(**c))
def test_processed_distribution_equals_hf(V, case):
    rng = np.random.default_rng(V * 31 + int(case["top_k"]) + int(case["top_p"] * 1000))
    logits = _tie_free_logits(rng, V, 24.0)
    seen = sorted(set(rng.integers(0, V, size=min(V // 3, 200)).tolist()) | {-200})     # the image sentinel is never seen
    keep_hf, p_hf = _hf(logits, case["temperature"], case["top_k"], case["top_p"], seen, case["penalty"])
    p = sr.probs(logits, case["temperature"], case["top_k"], case["top_p"], seen, case["penalty"])
    assert np.array_equal(p > 0, keep_hf), f"kept sets differ: {np.flatnonzero((p > 0) != keep_hf)[:10]}"
    np.testing.assert_allclose(p, p_hf, rtol=1e-5, atol=1e-9)


def test_threshold_keeps_ties():
    x = np.array([3, 1, 2, 2, 2, 0, -1], dtype=np.float32)
    assert sr.kept_mask(x, top_k=2).tolist() == [True, False, True, True, True, False, False]
    # softmax mass of the top key alone is < 0.5, with the three tied 2's it reaches it: all three kept
    assert sr.kept_mask(x, top_p=0.5).tolist() == [True, False, True, True, True, False, False]
    assert sr.kept_mask(x, top_p=1e-6).tolist() == [True] + [False] * 6      # at least one token


def test_race_is_the_categorical():
    """empirical distribution of the exponential race over 40 000 (row, step) keys vs the processed categorical: fixed-seed chi-square"""
    from scipy.stats import chi2
    logits = np.array([1.5, 0.3, -0.4, 2.1, 0.9, -2.0, 1.1], dtype=np.float32)
    for kw in (dict(temperature=0.8), dict(temperature=1.2, top_k=4), dict(temperature=1.0, top_p=0.8)):
        p = sr.probs(logits, **kw)
        x = sr.processed(logits, kw.get("temperature", 1.0))
        keep = p > 0
        counts = np.zeros(len(logits))
        n = 40000
        for step in range(n // 8):
            for row in range(8):
                g = x + sr.noise(sr.row_key(1234, row, step), np.arange(len(logits)))
                counts[int(np.argmax(np.where(keep, g, -np.inf)))] += 1
        assert counts[~keep].sum() == 0
        exp = p[keep] * n
        stat = float(((counts[keep] - exp) ** 2 / exp).sum())
        assert stat < chi2.ppf(0.999, keep.sum() - 1), (kw, stat, counts, exp)


def test_sample_row_uses_global_index_and_key():
    rng = np.random.default_rng(5)
    logits = rng.normal(0, 2, 64).astype(np.float32)
    a = sr.sample_row(logits, 0, 0, 7)
    assert a == sr.sample_row(logits, 0, 0, 7)
    draws = {sr.sample_row(logits, 0, s, 7) for s in range(20)}
    assert len(draws) > 1
    # two halves at their global offsets pick what the whole row picks (the TP exchange: max of (value, index), first index on ties)
    full = sr.sample_row(logits, 3, 4, 9, top_p=0.9)
    x = sr.processed(logits)
    thr = sr.threshold(x, 0, 0.9)
    g = np.where(sr.key(x).astype(np.int64) >= thr, x + sr.noise(sr.row_key(9, 3, 4), np.arange(64)), -np.inf)
    halves = [(g[:32].max(), int(np.argmax(g[:32]))), (g[32:].max(), 32 + int(np.argmax(g[32:])))]
    assert full == (halves[1][1] if halves[1][0] > halves[0][0] else halves[0][1])
