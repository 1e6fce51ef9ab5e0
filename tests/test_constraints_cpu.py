"""CPU (no GPU): tests/constraints_ref.py -- the restatement the device ban stage is tested against -- pinned to the installed
transformers' own logits processors, set for set; the commutation with the repetition penalty that makes one ban stage in front of the pick
exact; generate()'s resolution of the arguments and every refusal (raised before the engine is touched)."""
import os
import re
import types
import numpy as np
import pytest
import torch

import constraints_ref as cr
from omchat_amd import constraints as oc

lp = pytest.importorskip("transformers.generation.logits_process")


def _hf_banned(history, V, step, ngram=0, bad_words=(), eos=(), min_new=0, min_len=0, suppress=(), begin_suppress=()):
    ids = torch.tensor([list(history)], dtype=torch.long)
    scores = torch.zeros(1, V)
    P = len(history) - step
    procs = []
    if ngram > 0:
        procs.append(lp.NoRepeatNGramLogitsProcessor(ngram))
    if bad_words:
        procs.append(lp.NoBadWordsLogitsProcessor([list(w) for w in bad_words], list(eos) or None))
    if min_len > 0 and eos:
        procs.append(lp.MinLengthLogitsProcessor(min_len, list(eos)))
    if min_new > 0 and eos:
        procs.append(lp.MinNewTokensLengthLogitsProcessor(P, min_new, list(eos)))
    if suppress:
        procs.append(lp.SuppressTokensLogitsProcessor(list(suppress)))
    if begin_suppress:
        procs.append(lp.SuppressTokensAtBeginLogitsProcessor(list(begin_suppress), P))
    for p in procs:
        scores = p(ids, scores)
    return sorted(torch.nonzero(torch.isinf(scores[0]) & (scores[0] < 0)).view(-1).tolist())


def _looping_history(rng, V, L, span):
    """random ids from a small span: n-grams repeat"""
    lo = int(rng.integers(0, max(1, V - span)))
    return (lo + rng.integers(0, span, L)).tolist()


@pytest.mark.parametrize("V", [37, 1001, 152064])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_ngram_equals_hf(V, n):
    rng = np.random.default_rng(V + n)
    for L in (1, 2, 3, 4, 7, 40, 300):
        h = _looping_history(rng, V, L, 6)
        got = cr.banned_ids(h, cr.params(V, ngram=n), step=min(L, 3))
        assert got == _hf_banned(h, V, min(L, 3), ngram=n), (L, h[:12])
        if L + 1 < n:
            assert got == []
    assert cr.banned_ids(list(range(9)), cr.params(V, ngram=1), 0) == list(range(9))


@pytest.mark.parametrize("V", [37, 1001, 152064])
def test_bad_words_equal_hf(V):
    rng = np.random.default_rng(V)
    eos = [V - 1, 5]
    for L in (1, 2, 3, 10, 64):
        h = _looping_history(rng, V, L, 5)
        words = [[int(rng.integers(0, V))], [eos[0]], [eos[1]], [3, eos[0]]]                 # single ids; [eos] is dropped, [x, eos] is not
        words += [h[-m:] + [int(rng.integers(0, V))] for m in (1, 2, 3) if m <= L]           # words whose prefix is the tail
        words += [h[-(L):] + [7], [1] + h + [8], [9] * (L + 3)]                              # m = L + 1 and longer: skipped by HF
        words += [rng.integers(0, V, int(rng.integers(2, 5))).tolist() for _ in range(6)]
        got = cr.banned_ids(h, cr.params(V, bad_words=words, eos=eos), 0)
        assert got == _hf_banned(h, V, 0, bad_words=words, eos=eos), (L, h, words)
        assert eos[0] not in got or any(w[-1] == eos[0] and len(w) > 1 and len(w) <= L and h[L - len(w) + 1:] == w[:-1] for w in words)


@pytest.mark.parametrize("V", [37, 152064])
def test_length_and_suppress_equal_hf(V):
    rng = np.random.default_rng(V)
    eos = [2, V - 3]
    sup, bsup = [0, 11, V - 1], [4, 11]
    for P in (1, 6):
        for step in (0, 1, 3, 4, 5, 9):
            h = rng.integers(0, V, P + step).tolist()
            for kw in (dict(min_new=4, eos=eos), dict(min_len=P + 5, eos=eos), dict(min_new=4), dict(suppress=sup),
                       dict(begin_suppress=bsup), dict(min_new=2, min_len=3, eos=eos, suppress=sup, begin_suppress=bsup, ngram=2,
                                                       bad_words=[[h[-1], 20]])):
                assert cr.banned_ids(h, cr.params(V, **kw), step) == _hf_banned(h, V, step, **kw), (P, step, kw)
    # suppress ids outside the vocabulary are ignored, by HF (torch.isin over arange(V)) and here
    assert cr.banned_ids([1, 2], cr.params(37, suppress=[3, 99, -200]), 0) == _hf_banned([1, 2], 37, 0, suppress=[3, 99]) == [3]


def test_sentinel_in_history_matches_as_an_ordinary_value():
    h = [5, -200, 7, 3, 5, -200]
    assert cr.banned_ids(h, cr.params(37, ngram=3), 0) == _hf_banned(h, 37, 0, ngram=3) == [7]
    h = [-200, 9, 4, -200]
    assert cr.banned_ids(h, cr.params(37, ngram=2), 0) == _hf_banned(h, 37, 0, ngram=2) == [9]
    # an n-gram that would ban the sentinel itself: HF raises an index error, the device never bans ids outside [0, V)
    h = [3, -200, 8, 3]
    assert cr.banned_ids(h, cr.params(37, ngram=2), 0) == []
    with pytest.raises((IndexError, RuntimeError), match="out of bounds"):
        _hf_banned(h, 37, 0, ngram=2)


def test_ban_commutes_with_the_repetition_penalty():
    rng = np.random.default_rng(0)
    V = 1001
    for _ in range(8):
        h = _looping_history(rng, V, 50, 8)
        ids = torch.tensor([h])
        scores = torch.from_numpy((rng.standard_normal((1, V)) * 3).astype(np.float32))
        ban = lp.NoRepeatNGramLogitsProcessor(2)
        sup = lp.SuppressTokensLogitsProcessor([h[0], 17])
        pen = lp.RepetitionPenaltyLogitsProcessor(1.3)
        a = pen(ids, sup(ids, ban(ids, scores)))
        b = sup(ids, ban(ids, pen(ids, scores)))
        assert torch.equal(a, b)
        # and the restatement's ban applied to the raw logits is the same tensor
        banned = cr.banned_ids(h, cr.params(V, ngram=2, suppress=[h[0], 17]), 0)
        assert torch.equal(pen(ids, torch.from_numpy(cr.apply(scores[0].numpy(), banned))[None]), a)


# ---------------------------------------------------------------------------------------------------------------- host side of generate()
def _gc(**kw):
    base = dict(eos_token_id=None, pad_token_id=None, max_new_tokens=8, do_sample=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_resolution_defaults_and_hf_semantics():
    r = oc.resolve_constraints
    assert r(_gc(), {}, [], 100) is None
    assert r(_gc(no_repeat_ngram_size=0, min_length=0, min_new_tokens=None, bad_words_ids=None), {}, [7], 100) is None
    kw = dict(no_repeat_ngram_size=3, other=1)
    got = r(_gc(), kw, [7], 100)
    assert kw == dict(other=1)                                    # the constraint arguments are consumed, the rest is left
    assert got == dict(no_repeat_ngram_size=3, bad_words_ids=[], min_new_tokens=0, min_length=0, eos=[], suppress_tokens=[],
                       begin_suppress_tokens=[])                  # the eos list goes along only where it is read (length bounds, bad words)
    assert r(_gc(), dict(bad_words_ids=[[4]]), [7], 100)["eos"] == [7]
    # generation_config is the fallback, the call wins
    assert r(_gc(no_repeat_ngram_size=2), {}, [], 100)["no_repeat_ngram_size"] == 2
    assert r(_gc(no_repeat_ngram_size=2), dict(no_repeat_ngram_size=4), [], 100)["no_repeat_ngram_size"] == 4
    # HF: the length processors exist only with an EOS id; min_new_tokens replaces min_length
    assert r(_gc(), dict(min_new_tokens=5), [], 100) is None
    got = r(_gc(min_length=30), dict(min_new_tokens=5), [3, 3, 9], 100)
    assert (got["min_new_tokens"], got["min_length"], got["eos"]) == (5, 0, [3, 9])
    assert r(_gc(), dict(min_length=12), [3], 100)["min_length"] == 12
    got = r(_gc(), dict(suppress_tokens=torch.tensor([1, 2]), begin_suppress_tokens=[5], bad_words_ids=[[4], [5, 6]]), [], 100)
    assert (got["suppress_tokens"], got["begin_suppress_tokens"], got["bad_words_ids"]) == ([1, 2], [5], [[4], [5, 6]])


def test_resolution_raises_hf_messages():
    r = oc.resolve_constraints
    for bad in (-1, 2.5, "3"):
        with pytest.raises(ValueError, match="`ngram_size` has to be a strictly positive integer"):
            r(_gc(), dict(no_repeat_ngram_size=bad), [], 100)
        with pytest.raises(ValueError) as ex:
            lp.NoRepeatNGramLogitsProcessor(bad)
        assert "`ngram_size` has to be a strictly positive integer" in str(ex.value)
    for bad, msg in (([], "has to be a non-empty list"), ([3], "has to be a list of lists"), ([[1, -2]], "has to be a list of positive integers"),
                     ([[1.5]], "has to be a list of positive integers")):
        with pytest.raises(ValueError, match=msg):
            r(_gc(), dict(bad_words_ids=bad), [], 100)
        with pytest.raises(ValueError, match=msg):
            lp.NoBadWordsLogitsProcessor(bad, None)
    with pytest.raises(ValueError, match="The model vocabulary size is 100, but the following tokens were being biased"):
        r(_gc(), dict(bad_words_ids=[[1, 100]]), [], 100)
    with pytest.raises(ValueError, match="`min_length` has to be a non-negative integer"):
        r(_gc(), dict(min_length=-1), [1], 100)
    with pytest.raises(ValueError, match="`min_new_tokens` has to be a positive integer"):
        r(_gc(), dict(min_new_tokens=-1), [1], 100)


def test_resolution_refusals_and_caps():
    r = oc.resolve_constraints
    with pytest.raises(NotImplementedError, match="num_beams"):
        r(_gc(), dict(no_repeat_ngram_size=2), [], 100, num_beams=2)
    with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens"):
        r(_gc(), dict(suppress_tokens=[1]), [], 100, lookup=True)
    assert r(_gc(), {}, [], 100, num_beams=4, lookup=True) is None          # nothing set: nothing to refuse
    for name, v in (("forced_eos_token_id", 2), ("sequence_bias", [[[1], -1.0]]), ("prefix_allowed_tokens_fn", lambda b, i: [1]),
                    ("logits_processor", [object()])):
        with pytest.raises(NotImplementedError, match=name):
            r(_gc(), {name: v}, [], 100)
        if name != "logits_processor" and name != "prefix_allowed_tokens_fn":
            with pytest.raises(NotImplementedError, match=name):
                r(_gc(**{name: v}), {}, [], 100)
    assert r(_gc(), dict(logits_processor=[]), [], 100) is None              # HF's default empty list
    with pytest.raises(ValueError, match="exceeds the limit"):
        r(_gc(), dict(no_repeat_ngram_size=oc.MAX_NGRAM + 1), [], 100)
    with pytest.raises(ValueError, match="at most"):
        r(_gc(), dict(suppress_tokens=list(range(oc.MAX_SUPPRESS + 1))), [], 10 ** 6)
    # the eos cap holds only where the eos list is read: a length bound or bad_words_ids
    many = list(range(oc.MAX_EOS + 1))
    assert r(_gc(), dict(no_repeat_ngram_size=2), many, 100)["eos"] == []
    assert r(_gc(), dict(suppress_tokens=[3]), many, 100)["eos"] == []
    for kw in (dict(min_new_tokens=2), dict(min_length=2), dict(bad_words_ids=[[50]])):
        with pytest.raises(ValueError, match="eos ids exceed"):
            r(_gc(), kw, many, 100)
    with pytest.raises(ValueError, match="at most"):
        r(_gc(), dict(bad_words_ids=[[1]] * (oc.MAX_BAD_WORDS + 1)), [], 100)
    with pytest.raises(ValueError, match="at most"):
        r(_gc(), dict(bad_words_ids=[[1] * (oc.MAX_BAD_WORD_IDS + 1)]), [], 100)


def test_caps_equal_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omchat_hip.h")).read()
    caps = {k: int(v) for k, v in re.findall(r"#define OMCHAT_CON_MAX_(\w+) (\d+)", hdr)}
    assert caps == dict(NGRAM=oc.MAX_NGRAM, EOS=oc.MAX_EOS, SUPPRESS=oc.MAX_SUPPRESS, BAD_WORDS=oc.MAX_BAD_WORDS, BAD_WORD_IDS=oc.MAX_BAD_WORD_IDS)


class _Untouchable:
    """an engine generate() must not reach before its refusals: any use but host-side facts (vocabulary size, cache type) fails the test"""
    c = types.SimpleNamespace(t_vocab_total=320, max_seq=64)
    tp_size = 1
    _fp8_kv = False

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} used before the refusal")


class _Recorder:
    """a stub engine that records the constraint calls generate() makes and serves a fixed token stream"""
    c = types.SimpleNamespace(t_vocab_total=320, max_seq=64)
    tp_size = 1

    def __init__(self):
        self.calls = []

    def constraints_off(self):
        self.calls.append(("off",))

    def sampling_off(self):
        self.calls.append(("sampling_off",))

    def set_constraints(self, b, prompt, max_new, **kw):
        self.calls.append(("set", b, prompt, max_new, kw))

    def argmax(self, logits):
        self.calls.append(("pick",))
        return torch.tensor([9], dtype=torch.int32)

    def kv_lengths(self, b):
        return [4] * b

    def decode_step(self, tok, want_logits=False):
        return torch.tensor([9], dtype=torch.int32), None

    def kv_rewind(self, b, n=1):
        pass


def _stub_model(engine):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM, CausalLMOutputWithPast
    m = object.__new__(OmChatQwen2ForCausalLM)
    m.__dict__.update(generation_config=_gc(), engine=engine, config=types.SimpleNamespace(tokenizer_padding_side="right"))

    def forward(**kw):
        out = CausalLMOutputWithPast(torch.zeros(1, 1, 320), None)
        out.local_logits = torch.zeros(1, 320)
        m._padded_batch = False
        m._prefill_slots = 4
        return out
    m.forward = forward
    m._stage_buffer = lambda steps, b: (setattr(m, "_stage_event", types.SimpleNamespace(record=lambda: None, synchronize=lambda: None)),
                                        torch.empty(max(steps, 1), b, dtype=torch.int32))[1]
    return m


def test_generate_refuses_before_any_engine_work():
    m = _stub_model(_Untouchable())
    ids = torch.tensor([[1, 2, 3, 4]])
    with pytest.raises(NotImplementedError, match="num_beams"):
        m.generate(ids, num_beams=2, no_repeat_ngram_size=2)
    with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens"):
        m.generate(ids, prompt_lookup_num_tokens=4, bad_words_ids=[[5]])
    for name, v in (("forced_eos_token_id", 2), ("sequence_bias", [[[1], -1.0]]), ("prefix_allowed_tokens_fn", lambda b, i: [1]),
                    ("logits_processor", [object()])):
        with pytest.raises(NotImplementedError, match=name):
            m.generate(ids, **{name: v})
    with pytest.raises(ValueError, match="`ngram_size`"):
        m.generate(ids, no_repeat_ngram_size=-2)


def test_generate_sets_constraints_after_the_prefill_and_switches_them_off_otherwise():
    eng = _Recorder()
    m = _stub_model(eng)
    ids = torch.tensor([[1, -200, 3, 4]])
    m.generate(ids, max_new_tokens=3, eos_token_id=7, min_new_tokens=2, no_repeat_ngram_size=2, suppress_tokens=[5])
    kinds = [c[0] for c in eng.calls]
    assert "off" not in kinds and kinds.index("set") < kinds.index("pick")      # no off / on pair: equal parameters keep the decode graphs
    _, b, prompt, max_new, kw = eng.calls[kinds.index("set")]
    assert (b, prompt, max_new) == (1, [[1, -200, 3, 4]], 3)          # the prompt row as passed, sentinel included
    assert kw == dict(no_repeat_ngram_size=2, bad_words_ids=[], min_new_tokens=2, min_length=0, eos=[7], suppress_tokens=[5],
                      begin_suppress_tokens=[])
    eng.calls.clear()
    m.generate(ids, max_new_tokens=3)
    kinds = [c[0] for c in eng.calls]
    assert kinds[0] == "off" and "set" not in kinds
    # generation_config is read too
    m.generation_config.no_repeat_ngram_size = 3
    eng.calls.clear()
    m.generate(ids, max_new_tokens=2)
    assert [c for c in eng.calls if c[0] == "set"][0][4]["no_repeat_ngram_size"] == 3
