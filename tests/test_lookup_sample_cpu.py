"""CPU: prompt-lookup decoding with do_sample=True (omchat_amd/lookup.py with sample=True; DESIGN.md section 11, "Sampling") over a fake engine
that restates the sampled verify step, its commit and its rewind: the loop returns exactly the ids of the plain sampled loop with the same
seed, and leaves the sampler's step counter and seen set as that loop leaves them."""
import numpy as np
import pytest
import torch

import lookup_sample_ref as lsr
from omchat_amd.lookup import lookup_loop

SEEDS = list(range(20))
PARAMS = {1.0: dict(temperature=0.8, top_k=20, top_p=0.9), 1.3: dict(temperature=0.8, top_k=20, top_p=0.9, repetition_penalty=1.3)}
MAX_NEW = 48


def _prompt(seed):
    rng = np.random.default_rng(1000 + seed)
    a = rng.integers(0, 50, 6).tolist()
    return a + rng.integers(0, 50, 3).tolist() + a[:4]


def _plain(seed, pen, eos=(), crit=None, streamer=None):
    prompt = _prompt(seed)
    eng = lsr.FakeSampleEngine(lsr.PrefixLogits(seed=seed), prompt, 77 + seed, PARAMS[pen])
    new = lsr.sampled_ref(eng, prompt, MAX_NEW, set(eos), streamer, crit)
    return new, eng


def _lookup(seed, pen, k, eos=(), crit=None, streamer=None, hook=None):
    prompt = _prompt(seed)
    model = lsr.PrefixLogits(seed=seed)
    eng = lsr.FakeSampleEngine(model, prompt, 77 + seed, PARAMS[pen])
    tok = eng.sample_first()
    new = lookup_loop(eng, torch.tensor([prompt]), tok, MAX_NEW, set(eos), k, 2, model.V, streamer, crit, hook, sample=True)
    return new, eng


class _Stream:
    def __init__(self):
        self.got = []

    def put(self, t):
        self.got.extend(int(x) for x in t.view(-1))


@pytest.mark.parametrize("pen", [1.0, 1.3])
@pytest.mark.parametrize("k", [1, 4, 15])
def test_lookup_sample_equals_plain_sampled_loop(k, pen):
    accepted = 0
    for seed in SEEDS:
        want, e0 = _plain(seed, pen)
        got, e1 = _lookup(seed, pen, k)
        assert got == want, (seed, got, want)
        assert e1.sampling_state() == e0.sampling_state(), seed
        assert e1.sampling_state()[0] == len(want)
        assert e1.cache == e0.cache
        accepted += e1.accepted
    assert accepted > 0


@pytest.mark.parametrize("pen", [1.0, 1.3])
@pytest.mark.parametrize("k", [1, 4, 15])
def test_stop_inside_an_accepted_run(k, pen):
    """a stopping criterion and an EOS id that fall inside an accepted run: the rest of the run is dropped and taken back (kv_rewind of picks
    a verify step committed, with the penalty on as well).  The prompt-lookup drafter cuts its drafts before an EOS id, so an EOS can sit
    inside an accepted run only with drafts from elsewhere: the EOS runs take them from the recorded plain chain through the draft hook."""
    crit_inside = eos_inside = 0
    for seed in SEEDS:
        base, _ = _plain(seed, pen)
        P = len(_prompt(seed))
        hook = lambda ids, budget: list(base[len(ids) - P:len(ids) - P + budget])
        for j in range(4, len(base) - 1, 5):          # (every fifth position, odd and even ones, keeps the test quick)
            crit = [lambda ids, s, n=P + j + 1: ids.shape[1] >= n]
            want, e0 = _plain(seed, pen, crit=crit)
            for h in (None, hook):            # the drafter's own drafts, and runs in which every draft is accepted
                got, e1 = _lookup(seed, pen, k, crit=crit, hook=h)
                assert got == want == base[:j + 1], (seed, j, h is not None)
                assert e1.sampling_state() == e0.sampling_state() and e1.cache == e0.cache, (seed, j)
                crit_inside += bool(e1.rewinds)
        for j in range(4, len(base) - 1):
            if base.index(base[j]) != j:
                continue              # the id stops the generation earlier than at j
            s0, s1 = _Stream(), _Stream()
            want, e0 = _plain(seed, pen, eos=[base[j]], streamer=s0)
            got, e2 = _lookup(seed, pen, k, eos=[base[j]], streamer=s1, hook=hook)
            assert got == want == base[:j + 1] and s0.got == s1.got, (seed, j)
            assert e2.sampling_state() == e0.sampling_state() and e2.cache == e0.cache, (seed, j)
            eos_inside += bool(e2.rewinds)
    # a rewind in the lookup loop happens only when the stop leaves emitted picks of the same verify step behind it
    assert crit_inside > 0 and eos_inside > 0, (k, pen, crit_inside, eos_inside)


def test_rejected_draft_leaves_no_trace():
    """a draft id that is rejected is in no later row's committed state: the seen set after the step holds the emitted picks only"""
    model = lsr.PrefixLogits(seed=3)
    prompt = _prompt(3)
    eng = lsr.FakeSampleEngine(model, prompt, 5, PARAMS[1.3])
    tok = eng.sample_first()
    before = set(eng.seen)
    bogus = next(i for i in range(model.V) if i not in before and i != tok)
    picks, n = eng.decode_verify([tok, bogus, bogus], sample=True)
    emitted = picks[:n + 1].tolist()
    assert set(eng.seen) == before | set(emitted)
    assert eng.step == 1 + n + 1
    for r in range(1, n + 2):
        e2 = lsr.FakeSampleEngine(model, prompt, 5, PARAMS[1.3])
        e2.sample_first()
        e2.decode_verify([tok, bogus, bogus], sample=True)
        e2.kv_rewind(1, r)
        assert e2.step == 1 + n + 1 - r and set(e2.seen) == before | set(emitted[:n + 1 - r])
