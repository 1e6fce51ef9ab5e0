"""CPU restatement of the log-probability stage (omchat_amd/csrc/logprob.hip) in fp64 numpy, on top of
tests/sampling_ref.py (processed values, kept-set threshold, key) and tests/constraints_ref.py (ban).  raw = log_softmax(logits)[id];
processed = log_softmax(scores)[id], scores = what HF's processors leave: banned ids at -inf, repetition penalty, / T, ids outside the
top-k / top-p kept set at -inf.  The fp32 processing is sampling_ref's, bit for bit; only the softmax runs in fp64.
tests/test_logprob_cpu.py pins it to the installed transformers."""
import numpy as np

import constraints_ref as cr
import sampling_ref as sr


def log_softmax_at(x, i):
    """log_softmax(x)[i] in fp64; -inf entries contribute nothing, an id at -inf yields -inf"""
    z = np.asarray(x, dtype=np.float64)
    if z[i] == -np.inf:
        return -np.inf
    m = z.max()
    return float(z[i] - (m + np.log(np.exp(z - m).sum())))


def lse(x):
    z = np.asarray(x, dtype=np.float64)
    m = z.max()
    return float(m + np.log(np.exp(z - m).sum()))


def scores(logits, banned=(), temperature=1.0, top_k=0, top_p=1.0, seen=None, penalty=1.0, thr=None):
    """the processed row (fp32, cut ids at -inf).  seen: the ids seen BEFORE this pick.  thr: a kept-set threshold key to use instead of
    sampling_ref.threshold's (the one the device reported)"""
    l = cr.apply(np.asarray(logits, dtype=np.float32), banned)
    x = sr.processed(l, temperature, seen, penalty)
    if top_k == 1:                                   # the sampler's greedy form: only the maxima are kept
        return np.where(x == x.max(), x, np.float32(-np.inf))
    if thr is None:
        use = (1 < top_k < x.shape[0]) or top_p < 1.0
        thr = sr.threshold(x, top_k, top_p) if use else 0
    return np.where(sr.key(x).astype(np.int64) >= int(thr), x, np.float32(-np.inf))


def raw(logits, i):
    return log_softmax_at(np.asarray(logits, dtype=np.float32), i)


def processed(logits, i, **kw):
    return log_softmax_at(scores(logits, **kw), i)


def tolerance(x_id, lse_):
    """|device - ref| bound of the fp32 stage: expf at a few ulp, a summation tree of <= 18 levels at 6e-8 each, one rounding of max + log sum
    and one of the subtraction"""
    a = [1.0] + [abs(v) for v in (x_id, lse_) if np.isfinite(v)]
    return 1e-5 * max(a)
