"""CPU: tests/beam_proc_ref.py (the restatement of the beam search on processed scores) against HF's own generate(num_beams=N, ...) with a
repetition penalty and the token bans, on a tiny randomly initialised Qwen2ForCausalLM (fp32): the same sequences and sequences_scores
within 1e-5, and in at least half of the cases another result than the unprocessed search's (the processors were decisive).  Then the
host side: generate's arguments resolve to Engine.beam_processors' with beam_processors=True, the old refusals stand without it, and the
new refusals (tensor parallelism, a non-positive penalty, too few unbanned ids -- at the edge of the bound) are raised from host data."""
import functools
import types
import warnings
import numpy as np
import pytest
import torch

import beam_ref as br
import beam_proc_ref as bpr
import constraints_ref as cr
from omchat_amd.constraints import resolve_constraints, resolve_beam_processors

transformers = pytest.importorskip("transformers")

V = 320
NEW = 8
PROMPTS = [[3, 17, 18, 19, 20, 21], [5, 6, 11, 12, 13, 40]]
GC = types.SimpleNamespace()      # a generation_config that sets nothing


@functools.lru_cache(maxsize=None)
def _lm(seed):
    torch.manual_seed(seed)
    cfg = transformers.Qwen2Config(vocab_size=V, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=2, max_position_embeddings=64, tie_word_embeddings=False)
    m = transformers.Qwen2ForCausalLM(cfg).eval()
    with torch.no_grad():
        m.lm_head.weight.mul_(40.0)          # peaked distributions: clear margins between candidates
    return m


def _logits_fn(m, prompts, N):
    seqs = {}

    def fn(t, tokens, parents):
        nonlocal seqs
        if t == 0:
            rows = [list(p) for p in prompts]
        else:
            prev = [list(prompts[r // N]) for r in range(len(prompts) * N)] if t == 1 else seqs
            rows = [prev[int(parents[r])] + [int(tokens[r])] for r in range(len(tokens))]
        seqs = rows
        with torch.no_grad():
            out = m(input_ids=torch.tensor(rows)).logits[:, -1, :]
        return out.float().numpy()
    return fn


@functools.lru_cache(maxsize=None)
def _plain(seed, N, n_eos, lp):
    """the unprocessed search: its EOS ids (tokens the best beams emit early, so that hypotheses finish before the last step) and result"""
    m = _lm(seed)
    free, _, _ = br.search(_logits_fn(m, PROMPTS, N), 2, N, 4, num_return=N)
    cand = [free[0][0][0][1], free[1][0][0][2], free[0][N - 1][0][1], 7, 11]
    eos = []
    for c in cand:
        if c not in eos and len(eos) < n_eos:
            eos.append(int(c))
    got, _, _ = br.search(_logits_fn(m, PROMPTS, N), 2, N, NEW, eos=eos, length_penalty=lp, num_return=N)
    return tuple(eos), got


def _hf_args(mode, seed, N, n_eos, lp):
    """generate's keyword arguments of a mode; the banned ids are taken from the unprocessed result, so that they matter"""
    eos, got = _plain(seed, N, n_eos, lp)
    a, c = got[0][0][0], got[1][0][0]
    if mode == "penalty_up":
        return dict(repetition_penalty=1.3)
    if mode == "penalty_down":
        return dict(repetition_penalty=0.7)
    if mode == "ngram":
        return dict(no_repeat_ngram_size=2)
    assert mode == "all"
    words = [[a[0]]] + ([[c[0], c[1]]] if len(c) > 1 else []) + [[eos[0]]]
    return dict(repetition_penalty=1.2, no_repeat_ngram_size=3, bad_words_ids=words, min_new_tokens=3, min_length=2,
                suppress_tokens=[a[-1], 300], begin_suppress_tokens=[c[0], a[0]])


@functools.lru_cache(maxsize=None)
def _ours(mode, seed, N, n_eos, lp):
    eos, _ = _plain(seed, N, n_eos, lp)
    kw = dict(_hf_args(mode, seed, N, n_eos, lp))
    rp = kw.pop("repetition_penalty", 1.0)
    con = resolve_constraints(GC, kw, list(eos), V, N, False, beam_processors=True)
    bk = resolve_beam_processors(con, rp, N, list(eos), V, len(PROMPTS[0]), NEW)
    params = cr.params(V, ngram=bk["no_repeat_ngram_size"], bad_words=bk["bad_words_ids"], eos=list(eos), min_new=bk["min_new_tokens"],
                       min_len=bk["min_length"], suppress=bk["suppress_tokens"], begin_suppress=bk["begin_suppress_tokens"])
    got, _, _ = bpr.search(_logits_fn(_lm(seed), PROMPTS, N), PROMPTS, N, NEW, eos=list(eos), params=params, penalty=bk["repetition_penalty"],
                           length_penalty=lp, num_return=N)
    return got


MODES = ["penalty_up", "penalty_down", "ngram", "all"]
# (model seeds for which the processors change the result in most cases: test_processors_are_decisive)
CASES = [(mode, seed, N, n_eos, lp) for mode in MODES for seed, N in ((6, 2), (3, 4)) for n_eos, lp in ((1, 1.0), (2, 2.0), (1, 2.0), (2, 1.0))]


@pytest.mark.parametrize("mode,seed,N,n_eos,lp", CASES)
def test_beam_proc_ref_equals_hf(mode, seed, N, n_eos, lp):
    m = _lm(seed)
    eos, _ = _plain(seed, N, n_eos, lp)
    ids = torch.tensor(PROMPTS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hf = m.generate(ids, attention_mask=torch.ones_like(ids), do_sample=False, return_dict_in_generate=True, output_scores=True, num_beams=N,
                        max_new_tokens=NEW, eos_token_id=list(eos), pad_token_id=1, length_penalty=lp, num_return_sequences=N,
                        **_hf_args(mode, seed, N, n_eos, lp))
    got = _ours(mode, seed, N, n_eos, lp)
    P = len(PROMPTS[0])
    hyps = [h for per in got for h in per]
    gen = max(len(h[0]) for h in hyps)
    want = hf.sequences[:, P:].tolist()
    assert hf.sequences.shape[1] == P + gen
    for o, (toks, score) in enumerate(hyps):
        assert toks + [1] * (gen - len(toks)) == want[o], (o, toks, want[o])
        assert abs(score - float(hf.sequences_scores[o])) <= 1e-5, (o, score, float(hf.sequences_scores[o]))


def test_processors_are_decisive():
    """at least half of the cases return something else than the unprocessed search on the same model, and every mode does somewhere"""
    differ = {c: [h[0] for per in _ours(*c) for h in per] != [h[0] for per in _plain(*c[1:])[1] for h in per] for c in CASES}
    assert 2 * sum(differ.values()) >= len(CASES), differ
    for mode in MODES:
        assert any(v for c, v in differ.items() if c[0] == mode), mode


def test_process_row_rules():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(V) * 3).astype(np.float32)
    hist = [5, -200, 7, 5, 9, 400]
    lp0 = br.log_softmax(x)
    p = cr.params(V, ngram=2, suppress=[11], eos=[2], min_new=4)
    lp = bpr.process_row(x, hist, p, 2, 2.0)
    ban = cr.banned_ids(hist, p, 2)
    assert 11 in ban and 2 in ban
    for i in range(V):
        want = -np.inf if i in ban else (np.float32(lp0[i] * np.float32(2.0)) if i in (5, 7, 9) else lp0[i])
        assert lp[i] == want, i
    assert bpr.plain(cr.params(V, eos=[2], bad_words=[[2]]), 1.0) and not bpr.plain(cr.params(V), 1.5) and not bpr.plain(cr.params(V, ngram=1), 1.0)
    assert bpr.plain(cr.params(V, min_new=3), 1.0)          # no EOS id: HF adds no length processor


# ---------------------------------------------------------------------------------------------------------------- host resolution
def test_keyword_resolves_and_old_refusals_stand():
    kw = dict(no_repeat_ngram_size=3, suppress_tokens=[4, 5], bad_words_ids=[[7], [8, 9]], min_new_tokens=2)
    with pytest.raises(NotImplementedError, match="num_beams > 1"):
        resolve_constraints(GC, dict(kw), [7], V, 4, False)
    con = resolve_constraints(GC, dict(kw), [7], V, 4, False, beam_processors=True)
    assert con == resolve_constraints(GC, dict(kw), [7], V, 1, False)          # what the greedy path resolves
    bk = resolve_beam_processors(con, 1.05, 4, [7], V, 6, 8)
    assert bk == dict(repetition_penalty=float(np.float32(1.05)), no_repeat_ngram_size=3, bad_words_ids=[[7], [8, 9]], min_new_tokens=2,
                      min_length=0, suppress_tokens=[4, 5], begin_suppress_tokens=[])
    assert resolve_beam_processors(None, 1.0, 4, [7], V, 6, 8) is None and resolve_beam_processors(None, None, 4, [7], V, 6, 8) is None
    assert resolve_beam_processors(None, 1.2, 4, [], V, 6, 8)["no_repeat_ngram_size"] == 0
    gc = types.SimpleNamespace(no_repeat_ngram_size=2)                         # read from generation_config too
    assert resolve_constraints(gc, {}, [], V, 2, False, beam_processors=True)["no_repeat_ngram_size"] == 2
    with pytest.raises(NotImplementedError):                                   # the arguments without a kernel stay refused
        resolve_constraints(GC, dict(sequence_bias={(1,): 2.0}), [], V, 2, False, beam_processors=True)


def test_new_refusals():
    con = resolve_constraints(GC, dict(no_repeat_ngram_size=2), [], V, 2, False, beam_processors=True)
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        resolve_beam_processors(con, 1.0, 2, [], V, 6, 8, tp_size=2)
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        resolve_beam_processors(None, 1.1, 2, [], V, 6, 8, tp_size=4)
    assert resolve_beam_processors(None, 1.0, 2, [], V, 6, 8, tp_size=2) is None          # the plain search runs at every TP degree
    for bad in (0.0, -1.0, "2", True, float("nan")):
        with pytest.raises(ValueError, match="penalty"):
            resolve_beam_processors(con, bad, 2, [], V, 6, 8)
    with pytest.raises(ValueError, match="penalty"):
        resolve_beam_processors(con, float("inf"), 2, [], V, 6, 8)


@pytest.mark.parametrize("n_eos", [1, 2])
def test_unbanned_bound_at_its_edge(n_eos):
    N, P_tok, max_new = 4, 6, 8
    eos = [7, 9][:n_eos]
    KB = max(2, 1 + n_eos) * N
    words = [[7], [8, 9], [10]]          # [7] is one EOS id: HF drops it, and so does the count
    n_sup = 5
    fixed = n_sup + 2 + n_eos + P_tok + max_new          # + 2 bad words that count
    for n_bsup, ok in ((V - fixed - KB, True), (V - fixed - KB + 1, False)):
        kw = dict(bad_words_ids=[list(w) for w in words], suppress_tokens=list(range(20, 20 + n_sup)), begin_suppress_tokens=[30] * n_bsup)
        con = resolve_constraints(GC, kw, eos, V, N, False, beam_processors=True)
        if ok:          # equal to the bound: V - banned == KB
            assert resolve_beam_processors(con, 1.0, N, eos, V, P_tok, max_new) is not None
        else:           # one below
            with pytest.raises(ValueError, match=f"fewer than {KB} finite scores.* = {KB - 1}$"):
                resolve_beam_processors(con, 1.0, N, eos, V, P_tok, max_new)
