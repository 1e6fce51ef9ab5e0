"""CPU: classifier-free guidance -- tests/guidance_ref.py against the installed transformers'
UnbatchedClassifierFreeGuidanceLogitsProcessor driven with a stub model (scales, the default unconditional context, the cache growing by
one token per step), the -inf rule, and generate(guidance_scale=)'s argument resolution: every refusal raised from host data before the
engine is touched (the engine is a stub whose every call fails), None / 1 resolving to "off"."""
import types

import numpy as np
import pytest
import torch

import guidance_ref as gr
from omchat_amd import _lib
from omchat_amd.config import tiny
from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM

V = 97
SCALES = [0.0, 0.5, 1.5, 3.0]


class _StubLM:
    """returns given logits: call k gets table[k] [b, V] at the last position; records what it was called with"""

    def __init__(self, table):
        self.table, self.calls = table, []

    def __call__(self, input_ids, attention_mask=None, use_cache=None, past_key_values=None):
        k = len(self.calls)
        self.calls.append(dict(ids=input_ids.clone(), mask=attention_mask.clone(), past=past_key_values, use_cache=use_cache))
        T = input_ids.shape[1]
        logits = torch.zeros(input_ids.shape[0], T, V, dtype=torch.float32)
        logits[:, -1] = self.table[k]
        cached = (0 if past_key_values is None else past_key_values) + T
        return types.SimpleNamespace(logits=logits, get=lambda name, d=None: cached if name == "past_key_values" else d)


@pytest.mark.parametrize("neg", [False, True], ids=["default-context", "negative-prompt"])
@pytest.mark.parametrize("scale", SCALES)
def test_ref_equals_hf_processor(scale, neg):
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor as HF
    g = torch.Generator().manual_seed(int(scale * 10) + neg)
    b, steps = 3, 4
    cond = [torch.randn(b, V, generator=g) * 3 for _ in range(steps)]
    unc = [torch.randn(b, V, generator=g) * 3 for _ in range(steps)]
    lm = _StubLM(unc)
    neg_ids = torch.tensor([[7, 8, 9, 10, 11]] * b) if neg else None
    proc = HF(scale, lm, unconditional_ids=neg_ids, unconditional_attention_mask=None if not neg else torch.ones_like(neg_ids))
    ids = torch.tensor([[3, 17, 18], [5, 6, 11], [40, 41, 42]])
    for k in range(steps):
        got = proc(ids, cond[k]).numpy()
        want = gr.guide(torch.cat([cond[k], unc[k]]).numpy(), b, scale)
        assert np.abs(got - want).max() < 2e-5, (k, np.abs(got - want).max())      # HF computes in fp32
        ids = torch.cat([ids, torch.full((b, 1), 50 + k)], dim=1)
    # the unconditional context: the negative prompt, or the last prompt token alone; then one token per step over the cache
    T0 = 5 if neg else 1
    first = lm.calls[0]
    assert first["ids"].tolist() == (neg_ids.tolist() if neg else [[18], [11], [42]]) and first["past"] is None
    assert first["mask"].shape == (b, T0) and bool(first["mask"].all())
    for k in range(1, steps):
        c = lm.calls[k]
        assert c["ids"].tolist() == [[50 + k - 1]] * b and c["use_cache"] is True
        assert c["past"] == T0 + k - 1 and c["mask"].shape == (b, T0 + k)           # the cache grows one token per step


def test_ref_scale_one_is_the_conditional_log_softmax_and_the_inf_rule():
    rng = np.random.default_rng(0)
    z = (rng.standard_normal((4, V)) * 4).astype(np.float32)
    assert np.allclose(gr.guide(z, 2, 1.0), gr.log_softmax(z[:2]), atol=1e-12)
    z[0, 5] = -np.inf; z[2, 9] = -np.inf; z[1, 11] = -np.inf; z[3, 11] = -np.inf
    z[1, :4] = -np.inf
    for s in SCALES:
        out = gr.guide(z, 2, s)
        assert not np.isnan(out).any()
        assert np.isneginf(out[0, 5]) and np.isneginf(out[0, 9]) and np.isneginf(out[1, 11]) and np.isneginf(out[1, :4]).all()
        assert np.isfinite(out[0, [0, 1, 2, 6, 10]]).all()
        # the -inf entries of a row add nothing to its sum: the finite entries are those of the row without them
        keep = np.isfinite(z[0]) & np.isfinite(z[2])
        lc = z[0].astype(np.float64) - np.log(np.exp(z[0][np.isfinite(z[0])].astype(np.float64)).sum())
        lu = z[2].astype(np.float64) - np.log(np.exp(z[2][np.isfinite(z[2])].astype(np.float64)).sum())
        assert np.allclose(out[0][keep], s * (lc[keep] - lu[keep]) + lu[keep], atol=1e-10)
    # rows of nothing but -inf, and the fp32 evaluation's deviation as the GPU test measures it
    allinf = np.full((2, V), -np.inf, dtype=np.float32)
    assert np.isneginf(gr.guide(allinf, 1, 1.5)).all()
    dev, tol = gr.tolerance(z, 2, 1.5)
    assert 0 < dev < 1e-4 and tol == 8 * dev


# ---------------------------------------------------------------------------------------------------------------- generate()'s arguments
class _StubEngine:
    """data attributes only (and the host-side library for the splice plan): any method call is a failure of 'refused before any work'"""

    def __init__(self, max_batch=8, max_tiles=2, tp_size=1, fp8_kv=False, fp8_prefill=False, max_seq=128, max_prefill_rows=1024):
        self.c = types.SimpleNamespace(max_batch=max_batch, t_vocab_total=320, t_vocab=320, t_heads=7, t_kv_heads=1, v_layers=0, max_seq=max_seq,
                                       max_prefill_rows=max_prefill_rows, max_tiles=max_tiles)
        self.tp_size, self._fp8_kv, self._fp8_prefill = tp_size, fp8_kv, fp8_prefill
        self.device, self.torch_dtype = torch.device("cpu"), torch.bfloat16
        self.lib, self.ntok = _lib.lib(), 16

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} touched before the refusal")


def _model(**kw):
    return OmChatQwen2ForCausalLM(tiny().clone(), _StubEngine(**kw))


IDS = torch.tensor([[3, 17, 18, 19], [5, 6, 11, 12]])
NEG = torch.tensor([[7, 8], [9, 10]])
TILE = torch.zeros(1, 3, 4, 4)
TILE2 = torch.zeros(2, 3, 4, 4)      # (a row without a sentinel still takes a tile slot, as in the reference's splice)

REFUSALS = [
    (NotImplementedError, "num_beams", dict(num_beams=2), {}),
    (NotImplementedError, "num_return_sequences", dict(num_return_sequences=2, do_sample=True, seed=1), {}),
    (NotImplementedError, "suffixes=", dict(suffixes=[[5, 6]]), dict(rows=1)),
    (NotImplementedError, "prompt_lookup_num_tokens", dict(prompt_lookup_num_tokens=3), dict(rows=1)),
    (NotImplementedError, "reuse_cache=True", dict(reuse_cache=True), dict(rows=1)),
    (NotImplementedError, "padded batch", dict(attention_mask=torch.tensor([[1, 1, 1, 1], [1, 1, 1, 0]])), {}),
    (NotImplementedError, "rows of different spliced length", dict(images=TILE2, negative_prompt_ids=NEG), dict(ids=torch.tensor([[3, -200, 18, 19], [5, 6, 11, 12]]))),
    (NotImplementedError, "negative prompts of different spliced length", dict(negative_prompt_ids=torch.tensor([[7, -200], [9, 10]]), negative_images=TILE2), {}),
    (NotImplementedError, "negative_prompt_attention_mask with zeros", dict(negative_prompt_ids=NEG, negative_prompt_attention_mask=torch.tensor([[1, 1], [0, 1]])), {}),
    (NotImplementedError, "tensor parallelism", {}, dict(tp_size=2)),
    (NotImplementedError, "e4m3 KV cache", {}, dict(fp8_kv=True)),
    (NotImplementedError, "e4m3 KV cache", {}, dict(fp8_prefill=True)),
    (ValueError, "finite number", dict(guidance_scale=float("nan")), {}),
    (ValueError, "finite number", dict(guidance_scale=float("inf")), {}),
    (ValueError, "finite number", dict(guidance_scale="2"), {}),
    (ValueError, "finite number", dict(guidance_scale=True), {}),
    (ValueError, "one non-empty row per row", dict(negative_prompt_ids=NEG[:1]), {}),
    (ValueError, "one non-empty row per row", dict(negative_prompt_ids=torch.zeros(2, 0, dtype=torch.long)), {}),
    (ValueError, "must have the shape", dict(negative_prompt_ids=NEG, negative_prompt_attention_mask=torch.ones(2, 3)), {}),
    (ValueError, "outside the vocabulary", dict(negative_prompt_ids=torch.tensor([[7, 320], [9, 10]])), {}),
    (ValueError, "outside the vocabulary", dict(negative_prompt_ids=torch.tensor([[7, -1], [9, 10]])), {}),
    (ValueError, "negative_images is None", dict(negative_prompt_ids=torch.tensor([[7, -200], [9, -200]])), {}),
    (ValueError, "nothing would see them", dict(negative_prompt_ids=NEG, negative_images=TILE), {}),
    (ValueError, "max_batch", dict(negative_prompt_ids=NEG), dict(max_batch=3)),
    (ValueError, "max_tiles", dict(images=TILE2, negative_prompt_ids=torch.tensor([[7, -200], [9, -200]]), negative_images=TILE2),
     dict(ids=torch.tensor([[3, -200, 18, 19], [5, -200, 11, 12]]), max_tiles=3)),
    (ValueError, "do not fit", dict(negative_prompt_ids=NEG), dict(max_seq=4)),
    (ValueError, "do not fit", dict(negative_prompt_ids=NEG), dict(max_prefill_rows=15)),
]


@pytest.mark.parametrize("exc,frag,kw,env", REFUSALS, ids=[f"{i}-{r[1].split()[0]}" for i, r in enumerate(REFUSALS)])
def test_refusals_before_any_engine_call(exc, frag, kw, env):
    env = dict(env)
    ids = env.pop("ids", IDS)[:env.pop("rows", 2)]
    m = _model(**env)
    kw = dict(dict(guidance_scale=1.5), **kw)
    with pytest.raises(exc) as ei:
        m.generate(ids, max_new_tokens=4, **kw)
    assert type(ei.value) is exc and frag in str(ei.value), str(ei.value)


def test_none_and_one_resolve_to_off_and_a_scale_resolves():
    m = _model()
    args = (IDS, None, None)
    for scale in (None, 1, 1.0):
        kw = dict(guidance_scale=scale, negative_prompt_ids=NEG, negative_images=None, other=3)
        assert m._guidance_params(*args, kw, 1, None, None, False) is None
        assert kw == dict(other=3)                                   # the four keywords are taken out either way
    # off: nothing about the negative arguments is looked at, as HF adds no processor (an unusable negative prompt is not an error)
    assert m._guidance_params(*args, dict(guidance_scale=1.0, negative_prompt_ids=NEG[:1]), 2, 4, [[5]], True) is None
    gd = m._guidance_params(*args, dict(guidance_scale=3), 1, None, None, False)
    assert gd["scale"] == 3.0 and gd["neg_ids"].tolist() == [[19], [12]] and gd["neg_images"] is None      # HF's default context: the last prompt token
    gd = m._guidance_params(*args, dict(guidance_scale=np.float32(0.5), negative_prompt_ids=NEG.tolist()), 1, None, None, False)
    assert gd["scale"] == 0.5 and torch.equal(gd["neg_ids"], NEG)
    # read from generation_config when the call does not pass it
    m.generation_config.guidance_scale = 2.0
    m.generation_config.negative_prompt_ids = NEG
    gd = m._guidance_params(*args, {}, 1, None, None, False)
    assert gd["scale"] == 2.0 and torch.equal(gd["neg_ids"], NEG)
    assert m._guidance_params(*args, dict(guidance_scale=1.0), 1, None, None, False) is None               # the call's value wins
    # a one-tile negative prompt: the sentinel with its tile
    m.generation_config.guidance_scale = None
    gd = m._guidance_params(*args, dict(guidance_scale=1.5, negative_prompt_ids=torch.tensor([[-200, 7], [-200, 9]]), negative_images=TILE2),
                            1, None, None, False)
    assert gd["neg_images"].shape[0] == 2
