"""GPU: beam search on processed scores (omchat_amd/csrc/beam.hip behind omchat_beam_processors) -- the selection op step by step against
tests/beam_proc_ref.py with one witness per case that the plain search's raw-top-K shortcut gets wrong, plain arguments = the plain op bit
for bit, the history move against a host gather, and generate(num_beams=N, beam_processors=True, ...) on a tiny synthetic model: every step
checked against beam_proc_ref on that step's own logits, eager = decode graph, a repeated bigram that no_repeat_ngram_size=2 removes, the
keyword with nothing set = the call without it, greedy untouched, and the refusals."""
import copy
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import beam_ref as br
import beam_proc_ref as bpr
import constraints_ref as cr
from omchat_amd import synth, _lib
from omchat_amd._lib import check, ptr
from omchat_amd.config import tiny
from omchat_amd.engine import Engine


def _i32(xs):
    return torch.tensor([int(x) for x in xs] or [0], dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------------- selection op
class _Op:
    def __init__(self, lib, b, N, max_new, eos, lp, es, params, penalty):
        self.lib, self.b, self.N, self.max_new, self.eos, self.lp, self.p, self.pen = lib, b, N, max_new, list(eos), lp, params, penalty
        self.es = 2 if es == "never" else int(bool(es))
        self.state = torch.zeros(int(lib.omchat_beam_state_words(b, N, max_new)), dtype=torch.int32, device="cuda")
        self.tok = torch.empty(b * N, dtype=torch.int32, device="cuda")
        self.par = torch.empty(b * N, dtype=torch.int32, device="cuda")
        self.done = torch.zeros(1, dtype=torch.int32, device="cuda")

    def step(self, logits, t, hists, P_tok, plain=False):
        ev = _i32(self.eos)
        head = (ptr(logits), logits.shape[0], logits.shape[1], self.b, self.N, t, self.max_new, self.lp, self.es, ptr(ev), len(self.eos),
                ptr(self.state), ptr(self.tok), ptr(self.par), ptr(self.done))
        if plain:
            check(self.lib.omchat_op_beam_select(*head, _lib.cur_stream()))
        else:
            p = self.p
            words = p["bad_words"]
            off = [0]
            for w in words:
                off.append(off[-1] + len(w))
            h, hl, pl = _i32([i for r in hists for i in r]), _i32([len(r) for r in hists]), _i32([P_tok] * len(hists))
            sup, bsup, bw, bo = _i32(p["suppress"]), _i32(p["begin_suppress"]), _i32([i for w in words for i in w]), _i32(off)
            check(self.lib.omchat_op_beam_select_processed(*head, ptr(h), ptr(hl), ptr(pl), float(self.pen), p["ngram"], p["min_new"], p["min_len"],
                                                           ptr(sup), len(p["suppress"]), ptr(bsup), len(p["begin_suppress"]), ptr(bw), ptr(bo),
                                                           len(words), _lib.cur_stream()))
        torch.cuda.synchronize()
        return self.tok.cpu().numpy(), self.par.cpu().numpy(), int(self.done.item())

    def fin(self):
        s = self.state.cpu().numpy()
        bN = self.b * self.N
        return s[bN:2 * bN].view(np.float32), s[2 * bN:3 * bN], s[3 * bN:4 * bN], s[:bN].view(np.float32), s[6 * bN + self.b:6 * bN + 2 * self.b]


def _check_state(op, Ps, t):
    sc, fl, stp, run, done = op.fin()
    N = op.N
    for i, P in enumerate(Ps):
        assert bool(done[i]) == P.done, (t, i)
        for j in range(N):
            want = P.fin[j]
            assert sc[i * N + j] == want[0] and bool(fl[i * N + j]) == want[1] and stp[i * N + j] == want[2], (t, i, j, sc[i * N + j], want)
        assert np.array_equal(run[i * N:(i + 1) * N], P.run), (t, i, run[i * N:(i + 1) * N], P.run)


P_TOK = 6


def _scenario(V, b, N, witness):
    """the search's parameters and a per-step hook that plants the witness into the step's raw logits, given the rows' histories"""
    rng = np.random.default_rng(V + 10 * b + N + 97 * "abcde".index(witness))
    prompts = [[int(x) for x in rng.choice(V, P_TOK, replace=False)] for _ in range(b)]
    for p in prompts:
        p[2] = -200                                        # the image sentinel: matched like any value, ignored by the penalty
    eos = [int(x) for x in rng.choice(V, 1, replace=False)]
    KB = 2 * N
    kw, pen, es, max_new = {}, 1.0, False, 6
    plant = lambda lg, hists, t: None
    if witness == "a":                                     # the KB largest raw logits of a row are all suppressed
        kw["suppress"] = None                              # (filled from step 1's logits below)
    elif witness == "b":                                   # penalty 2, the raw argmax of every row is an id of its history
        pen = 2.0

        def plant(lg, hists, t):
            for r, h in enumerate(hists):
                lg[r, h[0]] = lg[r].max() + 0.1
    elif witness == "c":                                   # penalty 0.2 lifts a seen id from outside the raw top KB to first place
        pen = 0.2

        def plant(lg, hists, t):
            for r, h in enumerate(hists):
                lg[r, h[1]] = np.sort(lg[r])[-(KB + 4)] - np.float32(1e-3)
    elif witness == "d":                                   # min_new_tokens while EOS is the raw argmax of every row; then every prompt ends
        kw["min_new"], es, max_new = 3, True, 7

        def plant(lg, hists, t):
            lg[:, eos[0]] = lg.max(axis=1) + 1.0
    elif witness == "e":                                   # bigrams repeat inside the generated part: a few ids dominate every row
        kw["ngram"] = 2
        hot = [int(x) for x in rng.choice(V, 3, replace=False)]

        def plant(lg, hists, t):
            lg[:, hot] += 30.0
    return rng, prompts, eos, kw, pen, es, max_new, plant


@pytest.mark.parametrize("V", [152064, 1000])
@pytest.mark.parametrize("witness,b,N", [("a", 1, 2), ("b", 3, 4), ("c", 1, 8), ("d", 3, 2), ("e", 3, 4), ("e", 1, 8)])
def test_op_select_processed_equals_ref(gpu_lib, V, witness, b, N):
    rng, prompts, eos, kw, pen, es, max_new, plant = _scenario(V, b, N, witness)
    KB = 2 * N
    raw = [(rng.standard_normal((b if t == 0 else b * N, V)) * 3).astype(np.float32) for t in range(max_new)]
    if witness == "a":
        kw["suppress"] = [int(i) for i in np.argsort(-raw[1][0], kind="stable")[:KB]]
    params = cr.params(V, eos=eos, **kw)
    op = _Op(gpu_lib, b, N, max_new, eos, 1.0, es, params, pen)
    Ps = [br.Prompt(N) for _ in range(b)]
    hists = [list(p) for p in prompts]
    differs_from_plain = witnessed = moved = all_done = False
    for t in range(max_new):
        lg = raw[t]
        plant(lg, hists, t)
        tok, par, done = op.step(torch.from_numpy(lg).cuda(), t, hists, P_TOK)
        want_t, want_p = [], []
        for i, P in enumerate(Ps):
            sl = slice(i, i + 1) if t == 0 else slice(i * N, (i + 1) * N)
            shadow = None if differs_from_plain else copy.deepcopy(P)      # what the plain search would do from the same state
            a, p = bpr.step(P, lg[sl], hists[sl], t, max_new, eos, params, pen, 1.0, es)
            if shadow is not None:
                a0, p0 = br.step(shadow, lg[sl], t, max_new, eos, 1.0, es)
                differs_from_plain = not (np.array_equal(a, a0) and np.array_equal(p, p0) and np.array_equal(shadow.run, P.run) and shadow.fin == P.fin)
            moved |= t > 0 and not np.array_equal(p, np.arange(N))
            want_t += list(a)
            want_p += [i * N + int(x) for x in p]
        for i in range(b):
            sl = slice(i * N, (i + 1) * N)
            assert np.array_equal(tok[sl], np.array(want_t[sl])), (t, i, tok[sl], want_t[sl])
            assert np.array_equal(par[sl], np.array(want_p[sl])), (t, i, par[sl], want_p[sl])
        assert ((tok >= 0) & (tok < V)).all()
        _check_state(op, Ps, t)
        assert done == int(all(P.done for P in Ps))
        # the witness's premise, from the reference alone
        if witness == "a" and t == 1:
            witnessed = set(params["suppress"]) == set(int(i) for i in np.argsort(-lg[0], kind="stable")[:KB]) and not set(want_t) & set(params["suppress"])
        elif witness == "b" and t > 0:
            witnessed |= all(int(np.argmax(lg[r])) == hists[r][0] for r in range(len(hists))) and not any(hists[r][0] == want_t[r] for r in range(b * N))
        elif witness == "c":
            for r, h in enumerate(hists):
                lp = bpr.process_row(lg[r], h, params, t, pen)
                witnessed |= int(np.argmax(lp)) == h[1] and h[1] not in np.argsort(-lg[r], kind="stable")[:KB] and h[1] in want_t
        elif witness == "d" and t < 3:
            witnessed = (np.argmax(lg, axis=1) == eos[0]).all() and eos[0] not in want_t
        elif witness == "e" and t > 1:
            bans = [tuple(cr.banned_ids(h, params, t)) for h in hists]
            for i in range(b):
                mine = bans[i * N:(i + 1) * N]
                witnessed |= len(set(mine)) > 1 and any(mine)
        if done:
            all_done = True
            if t + 1 < max_new:                            # (f) a step after every prompt is done changes nothing
                before = op.state.clone()
                hists = bpr.advance(hists, prompts, N, t, np.array(want_t), np.array(want_p))
                op.step(torch.from_numpy(raw[t + 1]).cuda(), t + 1, hists, P_TOK)
                bN = b * N
                assert torch.equal(before[:6 * bN + 2 * b], op.state[:6 * bN + 2 * b]) and int(op.done.item()) == 1
                assert np.array_equal(op.par.cpu().numpy(), np.arange(bN))
            break
        hists = bpr.advance(hists, prompts, N, t, np.array(want_t), np.array(want_p))
    assert all_done and witnessed and differs_from_plain, (all_done, witnessed, differs_from_plain)
    if witness == "e":
        assert moved          # rows changed parents while their banned sets differed: a row with the wrong parent's history fails above
    if witness == "d":
        assert t + 1 < max_new          # the search ended early, so (f) ran


@pytest.mark.parametrize("V,b,N", [(152064, 1, 4), (1000, 3, 2)])
def test_op_plain_arguments_are_the_plain_op(gpu_lib, V, b, N):
    """a penalty of 1 with nothing banned: the plain op's outputs bit for bit; and with one ban that decides nothing (the lowest logit of
    every row) the processed launches still give the plain search's ids, parents and scores"""
    rng = np.random.default_rng(V + N)
    eos = [int(rng.integers(V))]
    max_new = 4
    ops = [_Op(gpu_lib, b, N, max_new, eos, 1.0, False, cr.params(V, eos=eos, bad_words=[[eos[0]]], min_new=0), 1.0),      # plain arguments
           _Op(gpu_lib, b, N, max_new, eos, 1.0, False, None, 1.0),                                                       # the plain op
           _Op(gpu_lib, b, N, max_new, eos, 1.0, False, cr.params(V, eos=eos, suppress=[V - 1]), 1.0)]                    # processed launches
    hists = [[1, 2, 3]] * b
    for t in range(max_new):
        lg = (rng.standard_normal((b if t == 0 else b * N, V)) * 3).astype(np.float32)
        lg[:, V - 1] = -50.0
        d = torch.from_numpy(lg).cuda()
        outs = [op.step(d, t, hists[:lg.shape[0]], 3, plain=op.p is None) for op in ops]
        for o, op in zip(outs[1:], ops[1:]):
            assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1]) and o[2] == outs[0][2]
            assert torch.equal(op.state, ops[0].state)
        hists = [[1, 2, 3] + [0] * (t + 1)] * (b * N)


# ---------------------------------------------------------------------------------------------------------------- history move
@pytest.mark.parametrize("case", ["identity", "cycle3", "dups", "frozen"])
def test_hist_move_equals_host_gather(gpu_lib, case):
    b, N, P, g = 2, 4, 5, 7
    ld = 16
    rows = b * N
    rng = np.random.default_rng(11)
    src = rng.integers(0, 1000, (rows, ld)).astype(np.int32)
    dst = rng.integers(0, 1000, (rows, ld)).astype(np.int32)
    par = np.arange(rows)
    if case == "cycle3":
        par[[0, 1, 2]] = [1, 2, 0]
        par[5] = 7
    elif case == "dups":
        par[:4] = 2
        par[4:] = [5, 5, 4, 4]
    elif case == "frozen":                                 # prompt 0 is frozen (parent = self, token 0) beside a live prompt
        par[4:] = [6, 4, 4, 7]
    tok = rng.integers(0, 1000, rows).astype(np.int32)
    if case == "frozen":
        tok[:4] = 0
    want = dst.copy()
    for r in range(rows):
        want[r, P:P + g] = src[par[r], P:P + g]
        want[r, P + g] = tok[r]
    d_src, d_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    d_par, d_tok = torch.from_numpy(par.astype(np.int32)).cuda(), torch.from_numpy(tok).cuda()
    d_len = torch.zeros(rows, dtype=torch.int32, device="cuda")
    bm = torch.full((2 * rows * 33,), -1, dtype=torch.int32, device="cuda")
    check(gpu_lib.omchat_op_beam_hist_move(ptr(d_src), ptr(d_dst), rows, N, ld, P, g, ptr(d_par), ptr(d_tok), ptr(d_len), ptr(bm), bm.numel() - 5,
                                           _lib.cur_stream()))
    torch.cuda.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), want)       # prompt part and the tail behind the new id untouched
    assert np.array_equal(d_src.cpu().numpy(), src)
    assert (d_len.cpu().numpy() == P + g + 1).all()
    assert not bm[:-5].any() and (bm[-5:] == -1).all()     # the bitmaps are zero again, and nothing behind them was written
    # a full row is refused before anything is enqueued
    assert gpu_lib.omchat_op_beam_hist_move(ptr(d_src), ptr(d_dst), rows, N, ld, P, ld - P, ptr(d_par), ptr(d_tok), ptr(d_len), ptr(bm), 0,
                                            _lib.cur_stream()) != 0


# ---------------------------------------------------------------------------------------------------------------- model level
def _tiny_model(b=8, seed=21, max_seq=128):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    cfg = tiny()
    e = Engine(cfg, dtype="bf16", max_seq=max_seq, max_batch=b, max_tiles=1, vision=False)
    e.load_state_dict(synth.state_dict(cfg, seed), strict=False)
    return cfg, e, OmChatQwen2ForCausalLM(cfg.clone(), e)


PROMPT = [[3, 17, 18, 19, 20, 21, 7, 9], [5, 6, 11, 12, 13, 40, 41, 42]]
V_TINY = 320


def _engine_loop(e, m, ids, N, max_new, eos, nret, bk):
    """what generate's beam branch does with beam_processors=True, one step at a time, every step's selection checked against
    beam_proc_ref on the step's own logits and the reference's own histories"""
    b = ids.shape[0]
    prompts = ids.tolist()
    params = cr.params(V_TINY, ngram=bk["no_repeat_ngram_size"], bad_words=bk["bad_words_ids"], eos=eos, min_new=bk["min_new_tokens"],
                       min_len=bk["min_length"], suppress=bk["suppress_tokens"], begin_suppress=bk["begin_suppress_tokens"])
    pen = bk["repetition_penalty"]
    out = m.forward(input_ids=ids, use_cache=True)
    e.beam_begin(b, N, 1.0, False, eos, max_new, e.kv_lengths(b)[0])
    e.beam_processors(prompts, **bk)
    Ps = [br.Prompt(N) for _ in range(b)]
    hists = [list(p) for p in prompts]
    lg = out.local_logits
    for t in range(max_new):
        l_np = lg.cpu().numpy()
        tok = e.beam_step(lg).cpu().numpy()
        want_t, want_p = [], []
        for i, Pr in enumerate(Ps):
            was_done = Pr.done
            sl = slice(i, i + 1) if t == 0 else slice(i * N, (i + 1) * N)
            a, p = bpr.step(Pr, l_np[sl], hists[sl], t, max_new, eos, params, pen)
            if not was_done:
                assert np.array_equal(tok[i * N:(i + 1) * N], a), (t, i, tok, a)
            want_t += list(a)
            want_p += [i * N + int(x) for x in p]
        if all(Pr.done for Pr in Ps):
            break
        hists = bpr.advance(hists, prompts, N, t, np.array(want_t), np.array(want_p))
        _, lg = e.decode_step(torch.from_numpy(tok).cuda(), want_logits=True)
    hyps, scores = e.beam_result(nret)
    for i, Pr in enumerate(Ps):
        for q in range(nret):
            assert hyps[i * nret + q] == br.hypothesis(Pr, q)
            assert scores[i * nret + q] == np.float32(Pr.fin[q][0])
    return hyps, scores


@pytest.mark.parametrize("b", [1, 2])
def test_generate_equals_engine_loop_and_ref(gpu_lib, b):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT[:b])
    free = m.generate(ids, num_beams=4, max_new_tokens=6)
    eos = [int(free[0, ids.shape[1] + 2])]
    T = ids.shape[1]
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, bad_words_ids=[[int(free[0, T])], [int(free[0, T]), int(free[0, T + 1])]],
              min_new_tokens=4, suppress_tokens=[int(free[-1, T + 1])], begin_suppress_tokens=[int(free[-1, T])])
    bk = dict(repetition_penalty=float(np.float32(1.3)), no_repeat_ngram_size=2, bad_words_ids=kw["bad_words_ids"], min_new_tokens=4, min_length=0,
              suppress_tokens=kw["suppress_tokens"], begin_suppress_tokens=kw["begin_suppress_tokens"])
    hyps, scores = _engine_loop(e, m, ids, 4, 10, eos, 2, bk)
    call = dict(num_beams=4, num_return_sequences=2, max_new_tokens=10, eos_token_id=eos, return_dict_in_generate=True, beam_processors=True, **kw)
    out = m.generate(ids, **call)
    gen = max(len(h) for h in hyps)
    assert out.sequences.shape == (b * 2, T + gen)
    for o, h in enumerate(hyps):
        assert out.sequences[o, T:].tolist() == h + [eos[0]] * (gen - len(h))
        assert torch.equal(out.sequences[o, :T], ids[o // 2])
    assert np.array_equal(out.sequences_scores.numpy(), scores)
    plain = m.generate(ids, num_beams=4, num_return_sequences=2, max_new_tokens=10, eos_token_id=eos, return_dict_in_generate=True)
    assert plain.sequences.shape != out.sequences.shape or not torch.equal(plain.sequences, out.sequences)      # the processors decided something
    # eager = decode graph
    e.enable_decode_graph(True)
    g = m.generate(ids, **call)
    assert e.decode_graph_stats()["replays"] > 0
    e.enable_decode_graph(False)
    assert torch.equal(g.sequences, out.sequences) and torch.equal(g.sequences_scores, out.sequences_scores)
    e.close()


def _bigrams(seq):
    return list(zip(seq, seq[1:]))


def test_no_repeat_ngram_removes_the_repeated_bigram(gpu_lib):
    """on a prompt where the plain beam call returns a hypothesis with a repeated bigram, no_repeat_ngram_size=2 returns none (prompt included)"""
    found = False
    for seed in (21, 22, 23, 24, 25, 26):
        _, e, m = _tiny_model(seed=seed)
        ids = torch.tensor(PROMPT[:1])
        kw = dict(num_beams=4, num_return_sequences=4, max_new_tokens=24)
        plain = m.generate(ids, **kw).tolist()
        if any(len(set(_bigrams(s))) < len(_bigrams(s)) for s in plain):
            found = True
            got = m.generate(ids, beam_processors=True, no_repeat_ngram_size=2, **kw).tolist()
            for s in got:
                assert len(set(_bigrams(s))) == len(_bigrams(s)), s
        e.close()
        if found:
            break
    assert found, "no seed gave a plain hypothesis with a repeated bigram: the test has no premise"


def test_keyword_with_nothing_set_and_greedy_afterwards(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    greedy = m.generate(ids, max_new_tokens=12)
    kw = dict(num_beams=4, num_return_sequences=4, max_new_tokens=10, return_dict_in_generate=True)
    a = m.generate(ids, **kw)
    bytes_plain = e.device_bytes()
    c = m.generate(ids, beam_processors=True, repetition_penalty=1.0, **kw)
    assert torch.equal(a.sequences, c.sequences) and torch.equal(a.sequences_scores, c.sequences_scores)
    assert e.device_bytes() == bytes_plain                 # the plain search: no history, no bitmaps
    # num_beams == 1: the keyword is ignored, the greedy path has its own ban stage
    assert torch.equal(m.generate(ids, beam_processors=True, no_repeat_ngram_size=2, max_new_tokens=12), m.generate(ids, no_repeat_ngram_size=2, max_new_tokens=12))
    bytes_plain = e.device_bytes()
    m.generate(ids, beam_processors=True, repetition_penalty=1.5, no_repeat_ngram_size=2, min_new_tokens=3, eos_token_id=[5], **kw)
    assert e.device_bytes() > bytes_plain                  # histories and bitmaps are counted
    assert torch.equal(m.generate(ids, max_new_tokens=12), greedy)          # a processed beam search leaves the greedy path as it was
    assert torch.equal(m.generate(ids, **kw).sequences, a.sequences)        # and the plain beam search
    e.close()


def test_refusals(gpu_lib):
    _, e, m = _tiny_model(b=4)
    ids = torch.tensor(PROMPT)
    on = dict(num_beams=2, beam_processors=True, no_repeat_ngram_size=2)
    with pytest.raises(NotImplementedError):                                   # without the keyword: as before
        m.generate(ids, num_beams=2, repetition_penalty=1.2)
    with pytest.raises(NotImplementedError, match="num_beams > 1"):
        m.generate(ids, num_beams=2, no_repeat_ngram_size=2)
    with pytest.raises(NotImplementedError):
        m.generate(ids, do_sample=True, seed=1, **on)
    with pytest.raises(NotImplementedError):
        m.generate(ids, stopping_criteria=[lambda a, b: True], **on)
    with pytest.raises(NotImplementedError):
        m.generate(ids, guidance_scale=1.5, negative_prompt_ids=ids, **on)
    with pytest.raises(NotImplementedError):
        m.generate(ids, dola_layers=[0], **on)
    from omchat_amd.fsm import TokenFSM
    with pytest.raises(NotImplementedError):
        m.generate(ids, token_fsm=TokenFSM({0: {5: 0}}), **on)
    with pytest.raises(NotImplementedError, match="b = 1"):
        m.generate(ids, attention_mask=torch.tensor([[1] * 8, [0] + [1] * 7]), **on)
    with pytest.raises(ValueError, match="penalty"):
        m.generate(ids, repetition_penalty=0.0, **on)
    with pytest.raises(ValueError, match="finite scores"):
        m.generate(ids, suppress_tokens=list(range(301)), max_new_tokens=8, **on)      # 320 - (301 + 8 + 8) = 3 < KB = 4
    # the context refuses the same things itself, and the call outside its window
    out = m.forward(input_ids=ids, use_cache=True)
    with pytest.raises(ValueError, match="between omchat_beam_begin"):
        e.beam_processors(PROMPT, no_repeat_ngram_size=2)
    e.beam_begin(2, 2, 1.0, False, [5], 8, e.kv_lengths(2)[0])
    with pytest.raises(ValueError, match="fewer finite scores"):
        e.beam_processors(PROMPT, suppress_tokens=list(range(300)))
    with pytest.raises(ValueError, match="> 0"):
        e.beam_processors(PROMPT, repetition_penalty=-1.0)
    e.beam_processors(PROMPT, no_repeat_ngram_size=2)
    e.beam_step(out.local_logits)
    with pytest.raises(ValueError, match="between omchat_beam_begin"):
        e.beam_processors(PROMPT, no_repeat_ngram_size=2)
    # nothing was left behind by a refusal: greedy still works on this model
    assert m.generate(ids[:1], max_new_tokens=3).shape == (1, 11)
    e.close()
