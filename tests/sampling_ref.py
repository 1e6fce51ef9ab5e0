"""CPU restatement of the on-device sampler (omchat_amd/csrc/sample.hip), numpy only: the same hash, the same fp32 processing, the same
fixed-point top-p mass, so picked ids compare exactly.  Order of HF's sampling path: repetition penalty, temperature, top-k, top-p, draw."""
import numpy as np

_M = np.uint64(0xFFFFFFFFFFFFFFFF)
_G = np.uint64(0x9E3779B97F4A7C15)


def mix(x):
    """splitmix64 on uint64 arrays / scalars (wrapping)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + _G
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def row_key(seed, row, step):
    inner = mix(np.uint64(((row & 0xFFFFFFFF) << 32) | (step & 0xFFFFFFFF)))
    return mix(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ inner)


def noise(rk, gidx):
    """Gumbel noise -log(-log U) of the global indices `gidx`, fp64 then rounded once to fp32"""
    with np.errstate(over="ignore"):
        h = mix(np.uint64(rk) + np.asarray(gidx, dtype=np.uint64) * _G)
    u = ((h >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52
    return (-np.log(-np.log(u))).astype(np.float32)


def key(x):
    """order-preserving uint32 key of fp32 values (-0 == +0)"""
    x = np.where(x == 0, np.float32(0), x).astype(np.float32)
    u = x.view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.uint32(k)
    u = (k & np.uint32(0x7FFFFFFF)) if k & np.uint32(0x80000000) else ~k
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def penalised(logits, seen, penalty):
    """RepetitionPenaltyLogitsProcessor in fp32: seen ids < 0 -> * p, else / p.  `seen`: iterable of ids (ids outside [0, V) ignored)"""
    l = np.asarray(logits, dtype=np.float32).copy()
    if penalty != 1.0 and seen is not None:
        ids = np.unique(np.asarray([i for i in seen if 0 <= i < l.shape[0]], dtype=np.int64))
        p = np.float32(penalty)
        v = l[ids]
        l[ids] = np.where(v < 0, v * p, v / p).astype(np.float32)
    return l


def processed(logits, temperature=1.0, seen=None, penalty=1.0):
    return (penalised(logits, seen, penalty) / np.float32(temperature)).astype(np.float32)


def threshold(x, top_k=0, top_p=1.0):
    """the kept set is key(x) >= threshold: top-k keeps every value >= the k-th largest, top-p the highest keys whose fixed-point mass
    (exp(x - max) in units of 2^-32, summed as integers over the top-k survivors) first reaches top_p of the total; ties kept"""
    k = key(x).astype(np.int64)
    V = x.shape[0]
    tk = 0
    if 1 < top_k < V:
        tk = int(np.sort(k)[::-1][top_k - 1])
    if top_p >= 1.0:
        return tk
    m = np.float64(unkey(int(k.max())))
    sel = k >= tk
    ks = k[sel]
    q = np.rint(np.exp(x[sel].astype(np.float64) - m) * 4294967296.0).astype(np.int64)
    P = float(top_p) * float(int(q.sum()))
    order = np.argsort(-ks, kind="stable")
    cum = np.cumsum(q[order])
    j = int(np.argmax(cum.astype(np.float64) >= P))
    return int(ks[order][j])


def kept_mask(x, top_k=0, top_p=1.0):
    return key(x).astype(np.int64) >= threshold(x, top_k, top_p)


def probs(logits, temperature=1.0, top_k=0, top_p=1.0, seen=None, penalty=1.0):
    """the processed distribution (fp64) the draw samples from: softmax of x over the kept set, 0 elsewhere"""
    x = processed(logits, temperature, seen, penalty)
    keep = kept_mask(x, top_k, top_p)
    z = np.where(keep, x.astype(np.float64), -np.inf)
    e = np.exp(z - z.max())
    return e / e.sum()


def sample_row(logits, row, step, seed, temperature=1.0, top_k=0, top_p=1.0, seen=None, penalty=1.0, gbase=0):
    """the id omchat_op_sample picks for one row (rank-local logits at global offset gbase)"""
    l = penalised(logits, seen, penalty)
    if top_k == 1:
        return int(np.argmax(l)) + gbase
    x = (l / np.float32(temperature)).astype(np.float32)
    use = (1 < top_k < x.shape[0]) or top_p < 1.0
    keep = kept_mask(x, top_k, top_p) if use else np.ones(x.shape[0], dtype=bool)
    g = (x + noise(row_key(seed, row, step), gbase + np.arange(x.shape[0]))).astype(np.float32)
    g = np.where(keep, g, np.float32(-np.inf))
    return int(np.argmax(g)) + gbase


def sample(logits, seed, step=0, temperature=1.0, top_k=0, top_p=1.0, seen=None, penalty=1.0, steps=None):
    """[b, V] -> ids [b]; seen: list of per-row id lists; steps: per-row step counters (default: `step` for every row)"""
    logits = np.asarray(logits, dtype=np.float32)
    out = []
    for r in range(logits.shape[0]):
        st = step if steps is None else int(steps[r])
        out.append(sample_row(logits[r], r, st, seed, temperature, top_k, top_p, None if seen is None else seen[r], penalty))
    return np.array(out, dtype=np.int64)
