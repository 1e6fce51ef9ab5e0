"""CPU: the interval form of the sampler's restatement (tests/sampling_ref2.py) against HF's own MinP / Typical / Epsilon / Eta warpers chained
in HF's order, hand-written edge rows, and the race drawing from the interval's distribution."""
import numpy as np
import pytest
import torch

import sampling_ref as sr
import sampling_ref2 as sr2

MARGIN = 1e-4      # no token within this relative distance of a threshold: HF decides in fp32, the restatement in fixed point

# (scale of the seeded normal logits, seed) per vocabulary size: seeds for which every case below has the margin, checked in the test
ROWS = {37: (2.0, 0), 1001: (3.0, 0), 152064: (3.0, 0)}
FILTERS = {
    "min_p": dict(min_p=0.05),
    "typical_p": dict(typical_p=0.2),
    "epsilon": dict(epsilon_cutoff=3e-3),
    "eta": dict(eta_cutoff=3e-3),
    "all4": dict(min_p=0.02, typical_p=0.6, epsilon_cutoff=1e-3, eta_cutoff=3e-3),
    "all4_behind": dict(temperature=0.7, top_k=50, top_p=0.9, min_p=0.02, typical_p=0.6, epsilon_cutoff=1e-3, eta_cutoff=3e-3),
}


def _row(V):
    scale, seed = ROWS[V]
    rng = np.random.default_rng(seed)
    x = rng.permutation(np.unique((rng.standard_normal(V + V // 8) * scale).astype(np.float32)))[:V]      # tie-free
    assert len(np.unique(x)) == V
    return x


def _far(values, thr, what):
    """the margin: no value within a relative MARGIN of thr"""
    v = values[torch.isfinite(values)].double()
    gap = float(((v - thr).abs() / abs(thr)).min())
    assert gap > MARGIN, f"{what}: a token sits within {gap:.2e} (relative) of the threshold {thr}"


def _hf_chain(x, temperature=1.0, top_k=0, top_p=1.0, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
    """HF's warper classes in the order of _get_logits_processor -> the kept mask; asserts the margin at every threshold on the way"""
    from transformers.generation import logits_process as lp
    s = torch.from_numpy(x)[None] / temperature
    if top_k:
        s = lp.TopKLogitsWarper(top_k)(None, s)
    if top_p < 1.0:
        s = lp.TopPLogitsWarper(top_p)(None, s)
    if min_p is not None:
        p = torch.softmax(s, -1)
        _far(p[0], float(min_p * p.max()), "min_p")
        s = lp.MinPLogitsWarper(min_p)(None, s)
    if typical_p is not None and typical_p < 1.0:
        norm = torch.log_softmax(s, -1)
        ent = -(norm * norm.exp()).nansum(-1, keepdim=True)
        d, idx = torch.sort(((-norm) - ent).abs(), descending=False)
        cum = s.gather(-1, idx).softmax(-1).cumsum(-1)
        last = int((cum < typical_p).sum())
        cut = float(d[0, last])
        others = torch.cat([d[0, :last], d[0, last + 1:]])
        _far(others, cut, "typical_p")
        assert abs(float(cum[0, last]) - typical_p) > 1e-5 and (last == 0 or abs(float(cum[0, last - 1]) - typical_p) > 1e-5), "typical_p mass"
        s = lp.TypicalLogitsWarper(typical_p)(None, s)
    if epsilon_cutoff is not None and 0 < epsilon_cutoff < 1:
        _far(torch.softmax(s, -1)[0], epsilon_cutoff, "epsilon_cutoff")
        s = lp.EpsilonLogitsWarper(epsilon_cutoff)(None, s)
    if eta_cutoff is not None and 0 < eta_cutoff < 1:
        ent = torch.distributions.Categorical(logits=s).entropy()
        eps = torch.tensor(float(eta_cutoff))
        _far(torch.softmax(s, -1)[0], float(torch.min(eps, torch.sqrt(eps) * torch.exp(-ent))), "eta_cutoff")
        s = lp.EtaLogitsWarper(eta_cutoff)(None, s)
    return torch.isfinite(s[0]).numpy()


@pytest.mark.parametrize("V", sorted(ROWS))
@pytest.mark.parametrize("name", sorted(FILTERS))
def test_kept_set_equals_hf_warpers(V, name):
    kw = dict(FILTERS[name])
    x = _row(V)
    keep_hf = _hf_chain(x, **kw)
    T = kw.pop("temperature", 1.0)
    keep = sr2.kept_mask(sr.processed(x, T), **kw)
    assert np.array_equal(keep, keep_hf), (np.flatnonzero(keep != keep_hf)[:10], keep.sum(), keep_hf.sum())
    # the interval is the whole story: [lo, hi] in keys selects the same tokens
    lo, hi = sr2.interval(sr.processed(x, T), **kw)
    k = sr.key(sr.processed(x, T)).astype(np.int64)
    assert np.array_equal((k >= lo) & (k <= hi), keep_hf)


def test_ties_at_a_cut_are_kept():
    # p = [.4, .2, .2, .1, .1]: min_p = 0.5 puts the threshold on the two tied .2's
    x = np.log(np.array([4, 2, 2, 1, 1], dtype=np.float32))
    assert sr2.kept_mask(x, min_p=0.4).tolist() == [True, True, True, False, False]
    # typical: two tokens at the same distance from the entropy share the cut
    y = np.array([0, 0, -3, -3, -8], dtype=np.float32)
    m = sr2.kept_mask(y, typical_p=0.3)
    assert m[0] == m[1] and m[2] == m[3] and m[:2].all()
    # epsilon between the tied pair and the rest
    assert sr2.kept_mask(x, epsilon_cutoff=0.15).tolist() == [True, True, True, False, False]


def test_typical_can_remove_the_argmax():
    # a peaked row: -log p_max is far BELOW the entropy, the mid tokens are the typical ones
    x = np.array([5.0] + [2.0 + 0.01 * i for i in range(40)], dtype=np.float32)
    keep_hf = _hf_chain(x, typical_p=0.3)
    lo, hi = sr2.interval(x, typical_p=0.3)
    assert not keep_hf[0] and hi != sr2.TOP and hi < int(sr.key(x).max())
    assert np.array_equal(sr2.kept_mask(x, typical_p=0.3), keep_hf)
    # the race then never draws the arg-max
    assert all(sr2.sample_row(x, 0, s, 5, typical_p=0.3) != 0 for s in range(200))
    # epsilon / eta behind it keep the largest SURVIVING logit, not the row's maximum
    m = sr2.kept_mask(x, typical_p=0.3, epsilon_cutoff=0.9, eta_cutoff=0.9)
    lo2, hi2 = sr2.interval(x, typical_p=0.3, epsilon_cutoff=0.9, eta_cutoff=0.9)
    assert m.sum() == 1 and hi2 == hi and lo2 == hi and not m[0]


def test_cutoff_above_every_probability_keeps_the_top_and_its_ties():
    x = np.array([1.0, 1.0, 0.5, 0.0, -1.0, 1.0], dtype=np.float32)
    for kw in (dict(epsilon_cutoff=0.9), dict(eta_cutoff=0.99), dict(epsilon_cutoff=0.9, eta_cutoff=0.9)):
        assert sr2.kept_mask(x, **kw).tolist() == [True, True, False, False, False, True], kw
        if "epsilon_cutoff" in kw:      # (eta's own threshold sqrt(eta) * exp(-H) lies below the top here: the same set, a lower key)
            assert sr2.interval(x, **kw) == (int(sr.key(x).max()), sr2.TOP)


def test_min_p_zero_keeps_everything():
    x = (np.random.default_rng(1).standard_normal(100) * 5).astype(np.float32)
    assert sr2.kept_mask(x, min_p=0.0).all()
    assert sr2.kept_mask(x, min_p=1.0).sum() == 1


def test_rows_cut_by_top_k_do_not_poison_the_entropy():
    x = (np.random.default_rng(2).standard_normal(200) * 2).astype(np.float32)
    for kw in (dict(typical_p=0.5), dict(eta_cutoff=0.05), dict(min_p=0.1, typical_p=0.7, epsilon_cutoff=0.01, eta_cutoff=0.02)):
        keep = sr2.kept_mask(x, top_k=10, **kw)
        assert keep.sum() >= 1 and not keep[np.argsort(x)[:-10]].any()
        assert np.array_equal(keep, _hf_chain(x, top_k=10, **kw)), kw
        # a row that already holds -inf (banned ids) behaves as the same row without them
        y = x.copy()
        y[::7] = -np.inf
        keep_y = sr2.kept_mask(y, **kw)
        assert np.isfinite(sr2.probs(y, **kw)).all() and not keep_y[::7].any()
        assert np.array_equal(keep_y[np.isfinite(y)], sr2.kept_mask(y[np.isfinite(y)], **kw))


def test_race_draws_from_the_interval():
    """the exponential race over a few thousand (row, step) keys vs probs of the interval form: the chi-square bound of
    test_sampling_cpu.test_race_is_the_categorical"""
    from scipy.stats import chi2
    logits = np.array([2.6, 1.5, 0.3, -0.4, 2.1, 0.9, -2.0, 1.1, 1.9, 0.0, 1.4], dtype=np.float32)
    for kw in (dict(temperature=0.8, min_p=0.1), dict(temperature=1.0, typical_p=0.5), dict(temperature=1.2, eta_cutoff=0.05),
               dict(temperature=1.0, top_k=8, min_p=0.02, typical_p=0.8, epsilon_cutoff=0.01, eta_cutoff=0.02)):
        p = sr2.probs(logits, **kw)
        T = kw.get("temperature", 1.0)
        x = sr.processed(logits, T)
        flt = {k: v for k, v in kw.items() if k != "temperature"}
        keep = sr2.kept_mask(x, **flt)
        assert np.array_equal(keep, p > 0) and 1 < keep.sum() < len(logits)
        counts = np.zeros(len(logits))
        n = 4000
        for step in range(n // 8):
            for row in range(8):
                counts[sr2.sample_row(logits, row, step, 1234, T, **flt)] += 1
        assert counts[~keep].sum() == 0
        exp = p[keep] * n
        stat = float(((counts[keep] - exp) ** 2 / exp).sum())
        assert stat < chi2.ppf(0.999, keep.sum() - 1), (kw, stat, counts, exp)
