"""CPU restatement of the sampler's interval form (omchat_amd/csrc/sample.hip with the four filters behind top-p), numpy only, on top of
sampling_ref: HF's MinP, Typical, Epsilon and Eta warpers in HF's order, min_tokens_to_keep = 1.  After any combination of the six filters
the kept set is a key interval [lo, hi] of the processed fp32 logits.  The same fixed-point arithmetic as the kernels: weights
w = rint(exp(x - max) * 2^32), the normaliser Z = sum w and the entropy sum E = sum w * (max - x) as integers, H = log Z + E / Z."""
import math
import numpy as np
import sampling_ref as sr

FIX = 4294967296.0
TOP = 0xFFFFFFFF


def _key_at_least(v):
    """key of the smallest fp32 >= v (fp64): a token is kept iff float64(x) >= v"""
    with np.errstate(over="ignore"):
        f = np.float32(v)
    if float(f) < v:
        f = np.nextafter(f, np.float32(np.inf))
    return int(sr.key(np.array([f], dtype=np.float32))[0])


def _stats(x, k, m, lo, hi):
    """(Z, E) over the keys in [lo, hi]: integers in units of 2^-32; a token of weight 0 (-inf among them) adds to neither"""
    sel = (k >= lo) & (k <= hi)
    xs = x[sel].astype(np.float64)
    ex = np.exp(xs - m)
    w = np.rint(ex * FIX).astype(np.int64)
    with np.errstate(invalid="ignore"):
        e = np.where(w > 0, np.rint(ex * (m - xs) * FIX), 0.0).astype(np.int64)
    return int(w.sum()), int(e[w > 0].sum())


def typ_dist(x, L32, H32):
    """|-log p - H| in fp32 as the kernels evaluate it: -log p = L - x"""
    with np.errstate(invalid="ignore"):
        return np.abs(((L32 - x).astype(np.float32) - H32).astype(np.float32))


def interval(x, top_k=0, top_p=1.0, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
    """x: processed fp32 logits of one row -> (lo, hi) keys of the kept interval; hi = 0xFFFFFFFF when the row's top token is kept.
    A filter is on under HF's rules: min_p not None, typical_p < 1, the cutoffs in (0, 1)."""
    x = np.asarray(x, dtype=np.float32)
    k = sr.key(x).astype(np.int64)
    V = x.shape[0]
    use_kp = (1 < top_k < V) or top_p < 1.0
    lo = sr.threshold(x, top_k, top_p) if use_kp else 0
    mkey = int(k.max())
    m = np.float64(sr.unkey(mkey))
    hi = mkey
    if min_p is not None:
        xt = float(sr.unkey(hi)) + (math.log(min_p) if min_p > 0 else -math.inf)
        lo = max(lo, min(_key_at_least(xt), hi))
    if typical_p is not None and typical_p < 1.0:
        Z, E = _stats(x, k, m, lo, hi)
        lz = math.log(Z * (1.0 / FIX))
        H = lz + E / Z
        L32, H32 = np.float32(m + lz), np.float32(H)
        sel = k >= lo
        xs, ks = x[sel], k[sel]
        d = typ_dist(xs, L32, H32)
        w = np.rint(np.exp(xs.astype(np.float64) - m) * FIX).astype(np.int64)
        dk = sr.key(d).astype(np.int64)
        order = np.argsort(dk, kind="stable")
        cum = np.cumsum(w[order])
        target = float(typical_p) * float(int(w.sum()))
        j = int(np.argmax(cum.astype(np.float64) >= target))
        cut = int(dk[order][j])
        kept = ks[dk <= cut]
        lo, hi = int(kept.min()), int(kept.max())
    for eps, eta in ((epsilon_cutoff, False), (eta_cutoff, True)):
        if eps is None or not 0.0 < eps < 1.0:
            continue
        Z, E = _stats(x, k, m, lo, hi)
        lz = math.log(Z * (1.0 / FIX))
        lp = math.log(eps)
        if eta:
            lp = min(lp, 0.5 * lp - (lz + E / Z))
        lo = max(lo, min(_key_at_least(float(m) + (lz + lp)), hi))
    return lo, (TOP if hi == mkey else hi)


def kept_mask(x, **kw):
    lo, hi = interval(x, **kw)
    k = sr.key(np.asarray(x, dtype=np.float32)).astype(np.int64)
    return (k >= lo) & (k <= hi)


def probs(logits, temperature=1.0, seen=None, penalty=1.0, **kw):
    """the processed distribution (fp64) the draw samples from: softmax of x over the kept interval, 0 elsewhere"""
    x = sr.processed(logits, temperature, seen, penalty)
    z = np.where(kept_mask(x, **kw), x.astype(np.float64), -np.inf)
    e = np.exp(z - z.max())
    return e / e.sum()


def logprobs(logits, temperature=1.0, seen=None, penalty=1.0, **kw):
    """log-softmax (fp64) over the kept interval, -inf elsewhere"""
    x = sr.processed(logits, temperature, seen, penalty)
    z = np.where(kept_mask(x, **kw), x.astype(np.float64), -np.inf)
    mx = z.max()
    return z - (mx + np.log(np.exp(z - mx).sum()))


def sample_row(logits, row, step, seed, temperature=1.0, seen=None, penalty=1.0, gbase=0, **kw):
    """the id omchat_op_sample_filtered picks for one row"""
    l = sr.penalised(logits, seen, penalty)
    if kw.get("top_k", 0) == 1:
        return int(np.argmax(l)) + gbase
    x = (l / np.float32(temperature)).astype(np.float32)
    keep = kept_mask(x, **kw)
    g = (x + sr.noise(sr.row_key(seed, row, step), gbase + np.arange(x.shape[0]))).astype(np.float32)
    g = np.where(keep, g, np.float32(-np.inf))
    return int(np.argmax(g)) + gbase


def sample(logits, seed, step=0, temperature=1.0, seen=None, penalty=1.0, steps=None, **kw):
    """[b, V] -> ids [b], as sampling_ref.sample"""
    logits = np.asarray(logits, dtype=np.float32)
    out = []
    for r in range(logits.shape[0]):
        st = step if steps is None else int(steps[r])
        out.append(sample_row(logits[r], r, st, seed, temperature, None if seen is None else seen[r], penalty, **kw))
    return np.array(out, dtype=np.int64)
