"""CPU restatement of the on-device beam search (omchat_amd/csrc/beam.hip): HF's _beam_search step as the kernels
compute it -- the log-sum-exp from per-slice fixed-point sums, the tie order (accumulated desc, raw logit desc, flat index asc) and HF's
fp32 arithmetic with its -1e9 masks.  `search` drives it with a logits callback; `step` is one prompt's share of omchat_op_beam_select."""
import math
import numpy as np

NEG = np.float32(-1.0e9)
SLICE_CAP = 20480
NS_MAX = 16
FIX = 4294967296.0


def slices(V, tp=1):
    """beam.hip beam_slices: equal slices of at most SLICE_CAP ids, a multiple of 8 of them when V allows it (the same cut at TP 1..8)"""
    for n in range(1, min(V, NS_MAX) + 1):
        if V % n or V // n > SLICE_CAP:
            continue
        if (n % 8 != 0) if V % 8 == 0 else (n % tp != 0):
            continue
        if n % tp:
            continue
        return n
    raise ValueError("no vocabulary slicing")


def log_softmax(x):
    """HF's fp32 log_softmax, (x - max) - log(sum), with the sum as the kernels form it: per slice, exp(x - slice max) in units of 2^-32
    summed as integers, the slices rebased to the row max in fp64"""
    x = np.asarray(x, dtype=np.float32)
    ns = slices(x.shape[0])
    parts = x.reshape(ns, -1)
    m = parts.max(axis=1)
    M = np.float32(m.max())
    S = 0.0
    for s in range(ns):
        d = parts[s].astype(np.float64) - np.float64(m[s])
        q = int(np.rint(np.exp(d[d >= -23.0]) * FIX).astype(np.int64).sum())
        S += math.ldexp(float(q), -32) * math.exp(float(m[s]) - float(M))
    L = np.float32(math.log(S))
    return ((x - M) - L).astype(np.float32)


def denom(g, length_penalty):
    return np.float32(float(g) ** float(length_penalty))


class Prompt:
    """one prompt's beam state: running scores, finished set (score, flag, step, parent beam, token), early-stop flag, done, backpointers"""

    def __init__(self, N):
        self.N = N
        self.run = np.zeros(N, np.float32)
        self.fin = [(NEG, False, -1, 0, 0) for _ in range(N)]
        self.unsat = True
        self.done = False
        self.bp = []                       # per step: [(parent beam, token)] * N


def step(P, logits_rows, t, max_new, eos, length_penalty=1.0, early_stopping=False):
    """one beam step of one prompt.  logits_rows fp32 [rows, V] (rows = 1 at t = 0, else N).  Returns (tokens [N], parent beams [N])."""
    N = P.N
    es = 2 if early_stopping == "never" else int(bool(early_stopping))
    KB = max(2, 1 + len(eos)) * N
    last = t + 1 >= max_new
    if P.done:                             # frozen
        P.bp.append([(j, 0) for j in range(N)])
        return np.zeros(N, np.int64), np.arange(N)
    lg = np.asarray(logits_rows, dtype=np.float32)
    rows, V = lg.shape
    acc = np.stack([log_softmax(lg[j]) + (np.float32(0) if t == 0 else P.run[j]) for j in range(rows)]).astype(np.float32)
    flat = np.arange(rows * V)
    order = np.lexsort((flat, -lg.reshape(-1), -acc.reshape(-1)))[:KB]
    c_acc = acc.reshape(-1)[order]
    c_row, c_tok = order // V, order % V
    hit = np.array([last or int(v) in eos for v in c_tok])
    trl = np.where(hit, c_acc + NEG, c_acc).astype(np.float32)
    # _update_finished_beams: / generated_len ** length_penalty, then the three -1e9 masks in HF's order
    s = (c_acc / denom(t + 1, length_penalty)).astype(np.float32)
    if es == 1 and all(f[1] for f in P.fin):
        s = (s + NEG).astype(np.float32)
    if not P.unsat:
        s = (s + NEG).astype(np.float32)
    did = hit & (np.arange(KB) < N)
    s = np.where(did, s, s + NEG).astype(np.float32)
    run_sel = sorted(range(KB), key=lambda k: (-trl[k], k))[:N]
    merged = list(P.fin) + [(s[k], bool(did[k]), t, int(c_row[k]), int(c_tok[k])) for k in range(KB)]
    keep = sorted(range(N + KB), key=lambda e: (-merged[e][0], e))[:N]
    P.fin = [merged[e] for e in keep]
    P.run = trl[run_sel].astype(np.float32)
    P.bp.append([(int(c_row[k]), int(c_tok[k])) for k in run_sel])
    # _check_early_stop_heuristic
    hd = denom(max_new if (es == 2 and length_penalty > 0) else t + 1, length_penalty)
    best = np.float32(P.run[0] / hd)
    mn = min(f[0] for f in P.fin)
    any_ = any(best > (mn if f[1] else NEG) for f in P.fin)
    P.unsat = P.unsat and any_
    P.done = (not P.unsat) or (es == 1 and all(f[1] for f in P.fin)) or last
    return c_tok[run_sel].astype(np.int64), (np.arange(N) if t == 0 else c_row[run_sel].astype(np.int64))


def hypothesis(P, e):
    """generated ids of finished entry e, backtracked through the backpointers"""
    score, _, st, par, tok = P.fin[e]
    if st < 0:
        return []
    out = [int(tok)]
    beam = par
    for u in range(st - 1, -1, -1):
        beam, tk = P.bp[u][beam]
        out.append(int(tk))
    return out[::-1]


def search(logits_fn, b, N, max_new, eos=(), length_penalty=1.0, early_stopping=False, num_return=1):
    """the whole search.  logits_fn(t, tokens, parents) -> fp32 [rows, V] for step t: the b prompts' rows at t = 0 (tokens = parents = None),
    afterwards the b*N beam rows, row r fed tokens[r] and continuing row parents[r] of the previous step (at t = 1 every beam of prompt i
    continues the prompt itself: parents[r] = i*N).  Returns ([per prompt: num_return x (ids, score)], steps taken, prompt states)."""
    eos = [int(e) for e in eos]
    Ps = [Prompt(N) for _ in range(b)]
    tokens = parents = None
    t = 0
    while t < max_new:
        lg = logits_fn(t, tokens, parents)
        tk, pa = [], []
        for i, P in enumerate(Ps):
            rows = lg[i:i + 1] if t == 0 else lg[i * N:(i + 1) * N]
            a, p = step(P, rows, t, max_new, eos, length_penalty, early_stopping)
            tk += [int(x) for x in a]
            pa += [i * N + (0 if t == 0 else int(x)) for x in p]
        tokens, parents = np.array(tk), np.array(pa)
        t += 1
        if all(P.done for P in Ps):
            break
    out = [[(hypothesis(P, e), float(P.fin[e][0])) for e in range(num_return)] for P in Ps]
    return out, t, Ps
