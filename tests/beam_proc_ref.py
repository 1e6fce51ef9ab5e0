"""CPU restatement of the beam search on processed scores (omchat_amd/csrc/beam.hip behind omchat_beam_processors):
HF's _beam_search with a repetition penalty and the token bans, which HF applies to the log-probabilities of every running row -- built on
tests/beam_ref.py (the log-sum-exp as the kernels form it, HF's fp32 arithmetic and masks) and tests/constraints_ref.py (the ban set).
`process_row` is rules 1-3 of a row, `step` one prompt's share of omchat_op_beam_select_processed, `search` drives it with a logits
callback and keeps every beam's own token history."""
import numpy as np

import beam_ref as br
import constraints_ref as cr

NEG = br.NEG


def plain(params, penalty):
    """nothing changes the scores: the search is beam_ref's"""
    p = params
    no_len = not p["eos"] or not (p["min_new"] or p["min_len"])
    words = [w for w in p["bad_words"] if not (len(w) == 1 and w[0] in p["eos"])]
    return np.float32(penalty) == 1 and not p["ngram"] and not words and no_len and not p["suppress"] and not p["begin_suppress"]


def process_row(logits_row, history, params, n_generated, penalty=1.0):
    """fp32 logits [V] of a running row with token history `history` (prompt row + the ids of its path, n_generated of them) -> processed
    log-probabilities: log_softmax; RepetitionPenaltyLogitsProcessor on the ids of the history inside the vocabulary (lp < 0 ? lp * penalty
    : lp / penalty, fp32); the banned ids at -inf"""
    lp = br.log_softmax(logits_row).copy()
    V = lp.shape[0]
    pen = np.float32(penalty)
    if pen != 1:
        ids = sorted({int(i) for i in history if 0 <= int(i) < V})
        x = lp[ids]
        lp[ids] = np.where(x < 0, x * pen, x / pen).astype(np.float32)
    lp[cr.banned_ids(history, params, n_generated)] = -np.inf
    return lp


def step(P, logits_rows, histories, t, max_new, eos, params, penalty=1.0, length_penalty=1.0, early_stopping=False):
    """one beam step of one prompt on processed scores.  logits_rows fp32 [rows, V] and histories [rows] (rows = 1 at t = 0, else N).
    Returns (tokens [N], parent beams [N]).  beam_ref.step with the processed log-probability where the raw logit stood."""
    N = P.N
    es = 2 if early_stopping == "never" else int(bool(early_stopping))
    KB = max(2, 1 + len(eos)) * N
    last = t + 1 >= max_new
    if P.done:                             # frozen
        P.bp.append([(j, 0) for j in range(N)])
        return np.zeros(N, np.int64), np.arange(N)
    lg = np.asarray(logits_rows, dtype=np.float32)
    rows, V = lg.shape
    lps = np.stack([process_row(lg[j], histories[j], params, t, penalty) for j in range(rows)]).astype(np.float32)
    acc = np.stack([lps[j] + (np.float32(0) if t == 0 else P.run[j]) for j in range(rows)]).astype(np.float32)
    flat = np.arange(rows * V)
    order = np.lexsort((flat, -lps.reshape(-1), -acc.reshape(-1)))[:KB]
    c_acc = acc.reshape(-1)[order]
    assert np.isfinite(c_acc).all(), "fewer than KB finite scores: outside the contract"
    c_row, c_tok = order // V, order % V
    hit = np.array([last or int(v) in eos for v in c_tok])
    trl = np.where(hit, c_acc + NEG, c_acc).astype(np.float32)
    s = (c_acc / br.denom(t + 1, length_penalty)).astype(np.float32)
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
    hd = br.denom(max_new if (es == 2 and length_penalty > 0) else t + 1, length_penalty)
    best = np.float32(P.run[0] / hd)
    mn = min(f[0] for f in P.fin)
    any_ = any(best > (mn if f[1] else NEG) for f in P.fin)
    P.unsat = P.unsat and any_
    P.done = (not P.unsat) or (es == 1 and all(f[1] for f in P.fin)) or last
    return c_tok[run_sel].astype(np.int64), (np.arange(N) if t == 0 else c_row[run_sel].astype(np.int64))


def advance(histories, prompts, N, t, tokens, parents):
    """the b * N rows' histories for step t + 1: row r continues row parents[r] of step t (the prompt itself at t = 0) with tokens[r]"""
    if t == 0:
        return [list(prompts[r // N]) + [int(tokens[r])] for r in range(len(prompts) * N)]
    return [list(histories[int(parents[r])]) + [int(tokens[r])] for r in range(len(tokens))]


def search(logits_fn, prompts, N, max_new, eos=(), params=None, penalty=1.0, length_penalty=1.0, early_stopping=False, num_return=1):
    """the whole search; logits_fn as in beam_ref.search.  prompts: the b prompt rows as HF's processors see them.
    Returns ([per prompt: num_return x (ids, score)], steps taken, prompt states)."""
    eos = [int(e) for e in eos]
    b = len(prompts)
    V = None
    Ps = [br.Prompt(N) for _ in range(b)]
    tokens = parents = None
    hist = [list(p) for p in prompts]
    t = 0
    while t < max_new:
        lg = logits_fn(t, tokens, parents)
        V = lg.shape[1]
        prm = params if params is not None else cr.params(V, eos=eos)
        tk, pa = [], []
        for i, P in enumerate(Ps):
            sl = slice(i, i + 1) if t == 0 else slice(i * N, (i + 1) * N)
            a, p = step(P, lg[sl], hist[sl], t, max_new, eos, prm, penalty, length_penalty, early_stopping)
            tk += [int(x) for x in a]
            pa += [i * N + (0 if t == 0 else int(x)) for x in p]
        tokens, parents = np.array(tk), np.array(pa)
        hist = advance(hist, prompts, N, t, tokens, parents)
        t += 1
        if all(P.done for P in Ps):
            break
    out = [[(br.hypothesis(P, e), float(P.fin[e][0])) for e in range(num_return)] for P in Ps]
    return out, t, Ps
