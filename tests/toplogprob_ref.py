"""CPU restatement of the log-probability record's extras (omchat_amd/csrc/logprob.hip; DESIGN.md section 14, "Extras") in fp64 numpy on
the fp32 logits the device saw: the top_n alternatives of a row under the raw distribution -- by value descending with -0 == +0, then by id
ascending; an id at -inf has log-probability -inf and ranks behind every finite one -- and the raw log-probability of given ids.  The
values are tests/logprob_ref.py's log_softmax_at.  tests/test_toplogprob_cpu.py pins it to torch."""
import numpy as np

import logprob_ref as lr


def order(x):
    """all ids of the row in the contract's order"""
    v = np.asarray(x, dtype=np.float32) + np.float32(0.0)      # -0 + 0 = +0: one value, as the comparison sees them
    return np.lexsort((np.arange(v.shape[0]), -v.astype(np.float64)))


def values(x, ids):
    """log_softmax(x)[ids] in fp64 (logprob_ref.log_softmax_at for each id, the row's log-sum-exp taken once)"""
    z = np.asarray(x, dtype=np.float32).astype(np.float64)
    l = lr.lse(z)
    return np.array([-np.inf if z[i] == -np.inf else z[i] - l for i in ids], dtype=np.float64)


def top(x, n):
    """-> (ids int64 [n], values fp64 [n])"""
    ids = order(x)[:n].astype(np.int64)
    return ids, values(x, ids)


def scored(x, ids):
    return values(x, ids)
