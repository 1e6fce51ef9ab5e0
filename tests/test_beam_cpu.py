"""CPU: tests/beam_ref.py (the restatement of the on-device beam search) against HF's own _beam_search on a tiny randomly initialised
Qwen2ForCausalLM (fp32): the same sequences and sequences_scores within 1e-5, over num_beams, batch, length_penalty, early_stopping, one or
two EOS ids (chosen so that beams finish early) and num_return_sequences."""
import itertools
import numpy as np
import pytest
import torch

import beam_ref as br

transformers = pytest.importorskip("transformers")

V = 320


@pytest.fixture(scope="module")
def tiny_lm():
    torch.manual_seed(0)
    cfg = transformers.Qwen2Config(vocab_size=V, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=2, max_position_embeddings=64, tie_word_embeddings=False)
    m = transformers.Qwen2ForCausalLM(cfg).eval()
    with torch.no_grad():
        m.lm_head.weight.mul_(40.0)          # peaked distributions: clear margins between candidates
    return m


PROMPTS = [[3, 17, 18, 19, 20, 21], [5, 6, 11, 12, 13, 40]]


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


def _hf(m, prompts, **kw):
    ids = torch.tensor(prompts)
    return m.generate(ids, attention_mask=torch.ones_like(ids), do_sample=False, return_dict_in_generate=True, output_scores=True, **kw)


def _eos_ids(m, prompts, N, n_eos):
    """tokens the best beams emit early, so that hypotheses finish before max_new_tokens"""
    out = _hf(m, prompts, num_beams=N, max_new_tokens=4, pad_token_id=0, eos_token_id=None, num_return_sequences=N).sequences
    P = len(prompts[0])
    cand = [int(out[0, P + 1]), int(out[min(1, out.shape[0] - 1), P + 2]), int(out[-1, P + 1])]
    picked = []
    for c in cand:
        if c not in picked:
            picked.append(c)
    return picked[:n_eos] if len(picked) >= n_eos else picked + [7, 11][:n_eos - len(picked)]


CASES = list(itertools.product([2, 4, 8], [1, 2], [False, True, "never"], [1, 2]))


@pytest.mark.parametrize("N,b,es,n_eos", CASES)
def test_beam_ref_equals_hf(tiny_lm, N, b, es, n_eos):
    prompts = PROMPTS[:b]
    eos = _eos_ids(tiny_lm, prompts, N, n_eos)
    P = len(prompts[0])
    for lp, nret in ((1.0, 1), (0.0, N), (2.0, 1), (-0.5, N)):
        hf = _hf(tiny_lm, prompts, num_beams=N, max_new_tokens=6, eos_token_id=eos, pad_token_id=1, length_penalty=lp, early_stopping=es,
                 num_return_sequences=nret)
        got, _, _ = br.search(_logits_fn(tiny_lm, prompts, N), b, N, 6, eos=eos, length_penalty=lp, early_stopping=es, num_return=nret)
        hyps = [h for per in got for h in per]
        gen = max(len(h[0]) for h in hyps)
        want = hf.sequences[:, P:].tolist()
        assert hf.sequences.shape[1] == P + gen, (lp, nret)
        for o, (ids, score) in enumerate(hyps):
            assert ids + [1] * (gen - len(ids)) == want[o], (lp, nret, o, ids, want[o])
            assert abs(score - float(hf.sequences_scores[o])) <= 1e-5, (lp, nret, o, score, float(hf.sequences_scores[o]))


def test_some_hypotheses_end_early(tiny_lm):
    """the EOS choice above makes beams finish before max_new_tokens (the grid exercises the finished set, not only max_length)"""
    eos = _eos_ids(tiny_lm, PROMPTS[:1], 4, 1)
    got, _, _ = br.search(_logits_fn(tiny_lm, PROMPTS[:1], 4), 1, 4, 6, eos=eos, num_return=4)
    assert any(len(ids) < 6 and ids[-1] in eos for ids, _ in got[0])


def test_log_softmax_matches_torch():
    rng = np.random.default_rng(0)
    for Vx in (1000, 152064, 320):
        x = (rng.standard_normal(Vx) * 4).astype(np.float32)
        # against fp64 (torch's own fp32 sum over 152064 terms is off by ~2e-5 here; the integer sum is not)
        ref = torch.log_softmax(torch.from_numpy(x).double(), -1).numpy()
        assert np.abs(br.log_softmax(x) - ref).max() <= 4e-6
    assert br.slices(152064) == 8 and br.slices(152064, 8) == 8 and br.slices(1000) == 8 and br.slices(320) == 8
