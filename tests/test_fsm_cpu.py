"""CPU: the host side of generate(token_fsm=) (omchat_amd/fsm.py) -- construction and validation of a TokenFSM, the
language of from_choices, tests/fsm_ref.py against the installed transformers' PrefixConstrainedLogitsProcessor, and generate()'s refusals,
every one raised before any engine call (the engine here is a stub whose every call fails)."""
import types

import numpy as np
import pytest
import torch

import fsm_ref as fr
from omchat_amd.config import tiny
from omchat_amd.fsm import DEAD, MAX_EDGES, MAX_STATES, TokenFSM, resolve_token_fsm
from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM

TRANS = {0: {5: 1, 9: 2, 300: 0}, 1: {7: 0, 2: 1}, 2: {2: 2, 11: 1}}


def test_construction_helpers_and_round_trip():
    f = TokenFSM(TRANS, vocab_size=320)
    assert f.n_states == 3
    off, tok, nxt = f.arrays()
    assert off == [0, 3, 5, 7] and tok == [5, 9, 300, 2, 7, 2, 11] and nxt == [1, 2, 0, 1, 0, 2, 1]
    g = TokenFSM.from_arrays(off, tok, nxt, vocab_size=320)
    assert g.transitions() == TRANS == f.transitions()
    assert TokenFSM(g.transitions()).arrays() == (off, tok, nxt)
    for s in TRANS:
        assert f.allowed(s) == fr.allowed(TRANS, s)
        for t in (0, 2, 5, 7, 9, 11, 300, 319):
            assert f.next(s, t) == fr.step(TRANS, s, t)
    assert f.allowed(DEAD) is None and f.next(DEAD, 5) == DEAD
    for ids in ([], [5], [5, 7, 9, 11, 2], [5, 5], [9, 2, 2, 11, 7, 300], [4]):
        assert f.walk(ids) == fr.walk(TRANS, ids)
    assert f.walk([5, 5]) == DEAD and f.walk([7], start=1) == 0
    # a state that only occurs as a target counts as a state
    assert TokenFSM({0: {1: 1}, 1: {2: 1}}).n_states == 2


def test_validation_errors():
    with pytest.raises(ValueError, match="non-empty dict"):
        TokenFSM({})
    with pytest.raises(ValueError, match="non-negative int"):
        TokenFSM({-1: {1: 0}})
    with pytest.raises(ValueError, match="not an int"):
        TokenFSM({0: {"a": 0}})
    with pytest.raises(ValueError, match="outside the vocabulary"):
        TokenFSM({0: {320: 0}}, vocab_size=320)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        TokenFSM.from_arrays([0, 1], [-3], [0])
    with pytest.raises(ValueError, match="outside the table"):
        TokenFSM.from_arrays([0, 1], [3], [1])
    with pytest.raises(ValueError, match="outside the table"):
        TokenFSM.from_arrays([0, 1], [3], [-1])
    with pytest.raises(ValueError, match="sorted by token"):
        TokenFSM.from_arrays([0, 2], [4, 3], [0, 0])
    with pytest.raises(ValueError, match="sorted by token"):
        TokenFSM.from_arrays([0, 2], [4, 4], [0, 0])
    with pytest.raises(ValueError, match="off must"):
        TokenFSM.from_arrays([0, 2, 1], [4, 5], [0, 0])
    with pytest.raises(ValueError, match="off must"):
        TokenFSM.from_arrays([1, 2], [4, 5], [0, 0])
    # a reachable state without an edge: the message names it and says what to do
    with pytest.raises(ValueError, match=r"state 1 can be reached and has no edge.*add an EOS edge"):
        TokenFSM({0: {4: 1}})
    with pytest.raises(ValueError, match=r"state 2 can be reached and has no edge.*add an EOS edge"):
        TokenFSM.from_arrays([0, 1, 2, 2], [4, 5], [1, 2])
    # ... an edgeless state nothing leads to is only refused as a start state
    f = TokenFSM.from_arrays([0, 1, 1], [4], [0])
    with pytest.raises(ValueError, match=r"state 1 has no edge.*add an EOS edge"):
        f.check_start(1)
    with pytest.raises(ValueError, match="at most"):
        TokenFSM.from_arrays([0] * (MAX_STATES + 2), [], [])
    assert MAX_STATES == 1 << 20 and MAX_EDGES == 1 << 26
    with pytest.raises(ValueError):
        TokenFSM.from_choices([], 2)
    with pytest.raises(ValueError):
        TokenFSM.from_choices([[1], []], 2)
    with pytest.raises(ValueError, match="EOS"):
        TokenFSM.from_choices([[1, 2]], 2)


def _language(f, eos):
    """every id sequence the automaton accepts up to and including its first EOS"""
    out, todo = [], [(0, [])]
    while todo:
        s, path = todo.pop()
        assert len(path) < 16
        for t in f.allowed(s):
            if t in eos:
                out.append(path + [t])
            else:
                todo.append((f.next(s, t), path + [t]))
    return sorted(out)


def test_from_choices_accepts_exactly_the_choices():
    choices = [[5, 6, 7], [5, 6], [5, 9, 7], [8]]                  # shared prefixes, and one choice that is a prefix of another
    f = TokenFSM.from_choices(choices, 2, vocab_size=320)
    assert _language(f, {2}) == sorted(c + [2] for c in choices)
    for c in choices:
        s = f.walk(c + [2])
        assert s != DEAD and f.allowed(s) == [2]                   # the final state loops on EOS: no reachable state is without an edge
        assert f.walk(c + [2, 0]) == DEAD                          # ... and the pad behind it ends the masking
    assert f.walk([5, 7]) == DEAD and f.walk([6]) == DEAD and f.walk([8, 8]) == DEAD
    two = TokenFSM.from_choices(choices, [2, 3])
    assert _language(two, {2, 3}) == sorted(c + [e] for c in choices for e in (2, 3))


def test_ref_equals_hf_prefix_constrained_processor():
    from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor
    V, P = 320, 6
    f = TokenFSM(TRANS, vocab_size=V)
    rng = np.random.default_rng(3)
    # the prompt part holds the image sentinel and pad ids: the callback must skip it by position, not by value
    prompt = [[3, -200, 17, 5, 9, 0], [0, 0, 0, 5, 7, 9], [-200, -200, 4, 4, 2, 11]]
    gen = [[5, 7, 9], [9, 2, 11], [5, 300, 7]]                     # row 2 is fed 300 in state 1: DEAD from there on
    starts = [0, 0, 0]
    for k in range(4):
        ids = torch.tensor([p + g[:k] for p, g in zip(prompt, gen)], dtype=torch.long)
        scores = torch.from_numpy(rng.standard_normal((3, V)).astype(np.float32))
        want = PrefixConstrainedLogitsProcessor(f.as_prefix_allowed_tokens_fn(P, starts), num_beams=1)(ids, scores.clone()).numpy()
        states = [fr.walk(TRANS, g[:k], s) for g, s in zip(gen, starts)]
        got = np.stack([fr.apply(TRANS, scores[r].numpy(), states[r]) for r in range(3)])
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        assert np.array_equal(got, want)
        assert [f.walk(g[:k], s) for g, s in zip(gen, starts)] == states
    assert states == [2, 1, DEAD] and not np.isneginf(got[2]).any() and int(np.isfinite(got[0]).sum()) == 2
    # per-row start states, and a vocabulary shard of the reference
    ids = torch.tensor([p + [9] for p in prompt], dtype=torch.long)
    want = PrefixConstrainedLogitsProcessor(f.as_prefix_allowed_tokens_fn(P, [0, 2, 1]), num_beams=1)(ids, scores.clone()).numpy()
    states = [fr.walk(TRANS, [9], s) for s in (0, 2, 1)]
    assert states == [2, DEAD, DEAD]
    got = np.stack([fr.apply(TRANS, scores[r].numpy(), states[r]) for r in range(3)])
    assert np.array_equal(got, want)
    half = np.stack([fr.apply(TRANS, scores[r].numpy()[160:], states[r], gbase=160) for r in range(3)])
    assert np.array_equal(half, want[:, 160:])


# ---------------------------------------------------------------------------------------------------------------- generate()'s refusals
class _StubEngine:
    """data attributes only: any method call (or any other attribute) is a failure of 'refused before any work'"""

    def __init__(self):
        self.c = types.SimpleNamespace(max_batch=8, t_vocab_total=320, t_vocab=320, t_heads=7, t_kv_heads=1, v_layers=0, max_seq=128,
                                       max_prefill_rows=64)
        self.tp_size, self._fp8_kv, self._fp8_prefill = 1, False, False
        self.device, self.torch_dtype = torch.device("cpu"), torch.bfloat16

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} touched before the refusal")


def test_generate_refuses_before_the_engine_is_touched():
    m = OmChatQwen2ForCausalLM(tiny().clone(), _StubEngine())
    ids = torch.tensor([[3, 17, 18, 19], [5, 6, 11, 12]])
    f = TokenFSM.from_arrays([0, 1, 1, 2], [4, 5], [0, 2], vocab_size=320)      # state 1: no edge, nothing leads there
    with pytest.raises(NotImplementedError, match="num_beams"):
        m.generate(ids, max_new_tokens=4, num_beams=2, token_fsm=f)
    with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens"):
        m.generate(ids[:1], max_new_tokens=4, prompt_lookup_num_tokens=3, token_fsm=f)
    with pytest.raises(ValueError, match="not a state"):
        m.generate(ids, max_new_tokens=4, token_fsm=f, fsm_start=3)
    with pytest.raises(ValueError, match="not a state"):
        m.generate(ids, max_new_tokens=4, token_fsm=f, fsm_start=[0, -1])
    with pytest.raises(ValueError, match="state 1 has no edge"):
        m.generate(ids, max_new_tokens=4, token_fsm=f, fsm_start=[0, 1])
    with pytest.raises(ValueError, match="one state per prompt"):
        m.generate(ids, max_new_tokens=4, token_fsm=f, fsm_start=[0, 0, 0])
    with pytest.raises(ValueError, match="fsm_start without token_fsm"):
        m.generate(ids, max_new_tokens=4, fsm_start=0)
    with pytest.raises(ValueError, match="TokenFSM"):
        m.generate(ids, max_new_tokens=4, token_fsm=TRANS)
    with pytest.raises(ValueError, match="outside the model's vocabulary"):
        m.generate(ids, max_new_tokens=4, token_fsm=TokenFSM({0: {320: 0}}))
    # HF's callback itself stays on the refused list
    with pytest.raises(NotImplementedError, match="prefix_allowed_tokens_fn"):
        m.generate(ids, max_new_tokens=4, prefix_allowed_tokens_fn=f.as_prefix_allowed_tokens_fn(4))


def test_start_states_of_the_expanded_batch():
    f = TokenFSM(TRANS)
    assert resolve_token_fsm(None, None, 2, 2, 320) is None
    assert resolve_token_fsm(f, None, 2, 2, 320) == [0, 0]
    assert resolve_token_fsm(f, 2, 2, 6, 320) == [2] * 6
    assert resolve_token_fsm(f, [1, 2], 2, 6, 320) == [1, 1, 1, 2, 2, 2]          # prompt-major, as the siblings are
    assert resolve_token_fsm(f, [0, 1, 2], 1, 3, 320) == [0, 1, 2]                # suffixes=: one prompt, a state per row
    assert resolve_token_fsm(f, [1], 1, 3, 320) == [1, 1, 1]
