"""CPU: generate(do_sample=True, num_return_sequences=N) with num_beams == 1 -- the host restatement of the row
order and the seen sets, and generate()'s refusals against the restated table, every one raised before any engine call (the engine here
is a stub whose every call fails)."""
import itertools
import types

import pytest
import torch

import group_ref as gr
from omchat_amd.config import tiny
from omchat_amd.engine import group_share_refusal
from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM


class _StubEngine:
    """data attributes only: any method call (or any other attribute) is a failure of 'refused before any work'"""

    def __init__(self, max_batch=8, fp8_kv=False, tp_size=1, q_heads=7, kv_heads=1):
        self.c = types.SimpleNamespace(max_batch=max_batch, t_vocab_total=320, t_vocab=320, t_heads=q_heads, t_kv_heads=kv_heads, v_layers=0,
                                       max_seq=128)
        self.tp_size, self._fp8_kv, self._fp8_prefill = tp_size, fp8_kv, False
        self.device, self.torch_dtype = torch.device("cpu"), torch.bfloat16

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} touched before the refusal")


def _model(**kw):
    cfg = tiny()
    return OmChatQwen2ForCausalLM(cfg.clone(), _StubEngine(**kw))


def test_row_order_is_prompt_major():
    rows = [[3, -200, 5], [7, 8, 9]]
    ex = gr.expand_rows(rows, 3)
    assert ex == torch.tensor(rows).repeat_interleave(3, dim=0).tolist()
    assert [gr.prompt_of(r, 3) for r in range(6)] == [0, 0, 0, 1, 1, 1]
    assert ex[2] == rows[0] and ex[3] == rows[1]


def test_seen_sets_are_the_prompts_ids_per_sibling():
    rows = [[3, -200, 5, 5], [7, 8, 9, 0]]
    seen = gr.seen_sets(rows, 2)
    assert seen == [[3, 5, 5], [3, 5, 5], [7, 8, 9, 0], [7, 8, 9, 0]]
    seen[0].append(11)                                   # siblings own their lists
    assert seen[1] == [3, 5, 5]


@pytest.mark.parametrize("fp8_kv,tp,heads,N", list(itertools.product([False, True], [1, 2], [(7, 1), (28, 4), (64, 1), (4, 4)], [1, 2, 3, 16, 17])))
def test_share_availability_rule(fp8_kv, tp, heads, N):
    q, kv = heads
    assert (group_share_refusal(fp8_kv, tp, q, kv, N) is not None) == gr.share_refusal(fp8_kv, tp, q, kv, N)


IDS = torch.tensor([[3, 17, 18, 19], [5, 6, 11, 12]])


class _Streamer:
    def put(self, x): raise AssertionError("streamer touched")
    def end(self): raise AssertionError("streamer touched")


CASES = [
    dict(N=2, do_sample=False),
    dict(N=5, b=2, max_batch=8),
    dict(N=2, b=2, padded=True),
    dict(N=2, reuse=True),
    dict(N=2, lookup=True),
    dict(N=2, streamer=True),
    dict(N=2, share_prompt=True, fp8_kv=True),
    dict(N=2, share_prompt=True, tp_size=2),
    dict(N=16, b=1, max_batch=16, share_prompt=True, q_heads=28, kv_heads=2),
    dict(N=17, b=1, max_batch=32, share_prompt=True),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_refusals_before_any_engine_call(case):
    want = gr.refusal(**case)
    assert want is not None
    c = dict(case)
    N, b = c.pop("N"), c.pop("b", 1)
    m = _model(max_batch=c.pop("max_batch", 8), fp8_kv=c.pop("fp8_kv", False), tp_size=c.pop("tp_size", 1), q_heads=c.pop("q_heads", 7),
               kv_heads=c.pop("kv_heads", 1))
    kw = dict(do_sample=c.pop("do_sample", True), seed=1, num_return_sequences=N, max_new_tokens=4)
    ids = IDS[:b]
    if c.pop("padded", False):
        kw["attention_mask"] = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0]])
    if c.pop("reuse", False):
        kw["reuse_cache"] = True
    if c.pop("lookup", False):
        kw.update(prompt_lookup_num_tokens=4, prompt_lookup_sample=True)
    if c.pop("streamer", False):
        kw["streamer"] = _Streamer()
    if "share_prompt" in c:
        kw["share_prompt"] = c.pop("share_prompt")
    assert not c
    with pytest.raises(want):
        m.generate(ids, **kw)


def test_greedy_refusal_is_hfs_message_and_reads_generation_config():
    m = _model()
    m.generation_config.num_return_sequences = 3
    with pytest.raises(ValueError, match="Greedy methods without beam search do not support `num_return_sequences` different than 1"):
        m.generate(IDS[:1], max_new_tokens=4)
    with pytest.raises(ValueError, match="max_batch >= 12"):
        m.generate(IDS, do_sample=True, seed=1, num_return_sequences=6, max_new_tokens=4)
    with pytest.raises(NotImplementedError, match="pad the prompts to equal length or use b = 1"):
        m.generate(IDS, do_sample=True, seed=1, num_return_sequences=2, attention_mask=torch.tensor([[1, 1, 1, 1], [0, 0, 1, 1]]))
    with pytest.raises(ValueError):
        m.generate(IDS[:1], do_sample=True, seed=1, num_return_sequences=0)


def test_table_accepts_what_is_supported():
    for kw in (dict(N=1, do_sample=False), dict(N=4, num_beams=4, do_sample=False), dict(N=3), dict(N=3, share_prompt=True),
               dict(N=3, share_prompt=False, fp8_kv=True), dict(N=8, b=8)):
        assert gr.refusal(**kw) is None, kw
