"""CPU: the prompt-lookup drafter (omchat_amd/lookup.py) against HF's PromptLookupCandidateGenerator, and the host loop against the greedy
loop over a fake engine whose model is a deterministic function of the prefix (tests/lookup_ref.py)."""
import random

import pytest
import torch

import lookup_ref as lr
from omchat_amd.lookup import PromptLookupDrafter, lookup_loop


def _seqs():
    rng = random.Random(0)
    out = []
    for n in (1, 2, 3, 5, 12, 40, 120):
        out.append([rng.randrange(50) for _ in range(n)])           # random
        out.append([rng.randrange(6) for _ in range(n)])            # small alphabet: many n-gram matches
        base = [rng.randrange(1000) for _ in range(8)]
        out.append((base * (n // 8 + 2))[:n + 3])                   # repetitive
    return out


def test_drafter_matches_hf():
    pytest.importorskip("transformers")
    checked = 0
    for ids in _seqs():
        for m in (1, 2, 3, 4):
            for k in (1, 2, 5, 10, 15):
                for eos in ((), (ids[len(ids) // 2],), (3, ids[-1])):
                    for ml in (None, len(ids) + 1, len(ids) + 2, len(ids) + 4):
                        want = lr.hf_candidates(ids, k, m, eos, ml)
                        d = PromptLookupDrafter(ids, k, m, eos)
                        assert d.candidates(ml) == want, (ids, k, m, eos, ml)
                        checked += 1
    assert checked > 1000


def test_drafter_incremental_equals_fresh():
    rng = random.Random(1)
    ids = [rng.randrange(5) for _ in range(30)]
    d = PromptLookupDrafter(ids[:3], 7, 3)
    for i in range(3, len(ids)):
        assert d.candidates() == PromptLookupDrafter(ids[:i], 7, 3).candidates()
        if lr.hf_candidates(ids[:i], 7, 3) is not None:
            assert d.candidates() == lr.hf_candidates(ids[:i], 7, 3)
        d.append(ids[i])


def test_drafter_cuts_before_image_sentinel():
    # project rule on top of HF's: the draft stops before any id outside [0, vocab) (the -200 image sentinel)
    ids = [5, 6, 7, -200, 8, 9, 5, 6]
    assert PromptLookupDrafter(ids, 5, 2).candidates() == [7, -200, 8, 9, 5]       # HF's rule alone
    assert PromptLookupDrafter(ids, 5, 2, vocab=100).candidates() == [7]
    assert PromptLookupDrafter([1, -200, 3, 1], 5, 2, vocab=100).candidates() == []
    assert PromptLookupDrafter([1, 2, 3, 1], 5, 2, vocab=100).candidates() == [2, 3, 1]


def test_drafter_refuses_bad_sizes():
    with pytest.raises(ValueError):
        PromptLookupDrafter([1, 2], 0, 2)
    with pytest.raises(ValueError):
        PromptLookupDrafter([1, 2], 3, 0)


class _Streamer:
    def __init__(self):
        self.got = []

    def put(self, t):
        self.got.extend(int(x) for x in t.view(-1))

    def end(self):
        pass


def _run(model, prompt, max_new, eos, k, m=2, stop_at=None, hook=None):
    crit_a = [lambda ids, s: stop_at is not None and int(ids[0, -1]) == stop_at] if stop_at is not None else None
    crit_b = [lambda ids, s: stop_at is not None and int(ids[0, -1]) == stop_at] if stop_at is not None else None
    sa, sb = _Streamer(), _Streamer()
    want = lr.greedy_ref(model, prompt, max_new, eos, sa, crit_a)
    eng = lr.FakeEngine(model, prompt)
    got = lookup_loop(eng, torch.tensor([prompt]), model(list(prompt)), max_new, set(eos), k, m, model.V, sb, crit_b, hook)
    return want, got, eng, sa.got, sb.got


@pytest.mark.parametrize("k", [1, 2, 4, 10, 15])
@pytest.mark.parametrize("seed", range(6))
def test_loop_equals_greedy(k, seed):
    model = lr.PrefixModel(V=40, copy_every=5, seed=seed)
    rng = random.Random(seed)
    prompt = [rng.randrange(40) for _ in range(25)]
    prompt = prompt + prompt[:12] + [-200] + prompt[3:9]
    for max_new in (1, 2, 7, 60):
        want, got, eng, sa, sb = _run(model, prompt, max_new, (), k)
        assert got == want and sb == sa
        assert eng.cache == prompt + got[:-1]           # every emitted id but the last is cached, as after the greedy loop
    assert eng.accepted > 0


def test_loop_eos_mid_run_stop_and_budget():
    model = lr.PrefixModel(V=40, copy_every=50, seed=3)    # nearly always copies: long accepted runs
    prompt = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 1, 2]
    free, _, eng0, _, _ = _run(model, prompt, 30, (), 10)
    assert eng0.accepted >= 5
    # EOS in the middle of an accepted run (not a draft: drafts are cut before EOS, the pick is the EOS)
    for e in free[2:8]:
        want, got, eng, sa, sb = _run(model, prompt, 30, (e,), 10)
        assert got == want and got[-1] == e and sb == sa
        assert eng.cache == prompt + got[:-1]
    # a stopping criterion firing mid-run
    for e in free[3:9]:
        want, got, eng, sa, sb = _run(model, prompt, 30, (), 10, stop_at=e)
        assert got == want and sb == sa and eng.cache == prompt + got[:-1]
    # max_new_tokens reached inside what would be a verify step
    for max_new in range(2, 14):
        want, got, eng, sa, sb = _run(model, prompt, max_new, (), 10)
        assert got == want and len(got) == max_new and eng.cache == prompt + got[:-1]


def test_loop_forced_drafts():
    # the measurement hook: any draft (right or wrong) leaves the ids unchanged
    model = lr.PrefixModel(V=40, copy_every=3, seed=7)
    prompt = list(range(20))
    rng = random.Random(2)
    hook = lambda ids, k: [rng.randrange(40) for _ in range(k)]
    want, got, eng, _, _ = _run(model, prompt, 40, (), 8, hook=hook)
    assert got == want and eng.verify_steps > 0


def test_loop_caps_the_verify_rows():
    # max_verify (Engine.verify_max_tokens: T * n_rep <= 128) bounds every verify step, whatever k is
    model = lr.PrefixModel(V=40, copy_every=50, seed=3)
    prompt = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 1, 2]
    eng = lr.FakeEngine(model, prompt)
    seen = []
    verify = eng.decode_verify
    eng.decode_verify = lambda toks, keep_all=False: (seen.append(len(toks)), verify(toks, keep_all))[1]
    got = lookup_loop(eng, torch.tensor([prompt]), model(list(prompt)), 40, set(), 15, 2, model.V, max_verify=5)
    assert got == lr.greedy_ref(model, prompt, 40, ())
    assert seen and max(seen) <= 5
