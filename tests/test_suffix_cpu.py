"""CPU: generate(suffixes=[...]) / score(suffixes=[...]) -- the argument resolution and every refusal against the
restated table, each raised before any engine call (the engine here is a stub whose every call fails), the per-row histories, the padded
sequences handed to stopping criteria, the label arithmetic of the scoring form against a plain log-softmax over oracle logits, and the
fp64 attention references of the GPU tests against a dense masked softmax."""
import types

import pytest
import torch

import suffix_ref as sfr
import oracle
from omchat_amd import _lib, suffix as sx, synth
from omchat_amd.config import tiny
from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM


class _StubEngine:
    """data attributes only (and the host-side library for the splice plan): any method call is a failure of 'refused before any work'"""

    def __init__(self, max_batch=8, max_prefill_rows=1024, max_seq=128, fp8_kv=False, fp8_prefill=False, tp_size=1, q_heads=7, kv_heads=1):
        self.c = types.SimpleNamespace(max_batch=max_batch, t_vocab_total=320, t_vocab=320, t_heads=q_heads, t_kv_heads=kv_heads, v_layers=0,
                                       max_seq=max_seq, max_prefill_rows=max_prefill_rows)
        self.tp_size, self._fp8_kv, self._fp8_prefill = tp_size, fp8_kv, fp8_prefill
        self.device, self.torch_dtype = torch.device("cpu"), torch.bfloat16
        self.lib, self.ntok = _lib.lib(), 16

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} touched before the refusal")


def _model(**kw):
    return OmChatQwen2ForCausalLM(tiny().clone(), _StubEngine(**kw))


class _Streamer:
    def put(self, x): raise AssertionError("streamer touched")
    def end(self): raise AssertionError("streamer touched")


IDS = torch.tensor([[3, 17, 18, 19], [5, 6, 11, 12]])
ENGINE_KEYS = ("max_batch", "max_prefill_rows", "fp8_kv", "fp8_prefill", "tp_size", "q_heads", "kv_heads")

CASES = [
    dict(batch=2),
    dict(mask_zeros=True),
    dict(suffixes=()),
    dict(suffixes=((5, 6), ())),
    dict(suffixes=((5, -200),)),
    dict(suffixes=((5, -1),)),
    dict(suffixes=((5, 320),)),
    dict(suffixes=((5,),) * 9, max_batch=8),
    dict(suffixes=((5,) * 30, (6,) * 40, (7,)), max_prefill_rows=119),
    dict(num_beams=2),
    dict(num_return_sequences=2),
    dict(lookup=True),
    dict(reuse=True),
    dict(suffixes=((5,), (6,)), streamer=True),
    dict(fp8_kv=True),
    dict(fp8_prefill=True),
    dict(tp_size=2),
    dict(suffixes=((5,),) * 17, max_batch=32, share_prompt=True),
    dict(suffixes=((5,),) * 16, max_batch=16, share_prompt=True, q_heads=27, kv_heads=3),      # 9 query heads per kv head
    dict(suffixes=((5,),) * 16, max_batch=16, share_prompt=True, q_heads=64, kv_heads=4),      # 16 x 16 query rows
]


def _call(case):
    c = dict(case)
    m = _model(**{k: c.pop(k) for k in ENGINE_KEYS if k in c})
    kw = dict(max_new_tokens=4, suffixes=[list(s) for s in c.pop("suffixes", ((5, 6),))])
    ids = IDS[:c.pop("batch", 1)]
    if c.pop("mask_zeros", False):
        kw["attention_mask"] = torch.tensor([[1, 1, 1, 0]])
    if "num_beams" in c:
        kw["num_beams"] = c.pop("num_beams")
    if "num_return_sequences" in c:
        kw.update(num_return_sequences=c.pop("num_return_sequences"), do_sample=True, seed=1)
    if c.pop("lookup", False):
        kw["prompt_lookup_num_tokens"] = 4
    if c.pop("reuse", False):
        kw["reuse_cache"] = True
    if c.pop("streamer", False):
        kw["streamer"] = _Streamer()
    if "share_prompt" in c:
        kw["share_prompt"] = c.pop("share_prompt")
    assert not c
    return m, ids, kw


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}" for k in c))
def test_refusals_before_any_engine_call_with_their_own_messages(case):
    want = sfr.refusal(**case)
    assert want is not None
    m, ids, kw = _call(case)
    with pytest.raises(want[0]) as ei:
        m.generate(ids, **kw)
    assert type(ei.value) is want[0] and want[1] in str(ei.value), (want, str(ei.value))


def test_every_refusal_has_its_own_message():
    msgs = []
    for case in CASES:
        m, ids, kw = _call(case)
        with pytest.raises((ValueError, NotImplementedError)) as ei:
            m.generate(ids, **kw)
        msgs.append(str(ei.value).split(":")[0])
    frag = [sfr.refusal(**c)[1] for c in CASES]
    assert len(set(frag)) >= 14 and len(set(msgs)) >= 14      # (several cases share one rule: ids outside the vocabulary, the section-7 modes, sharing)


def test_score_has_the_same_refusals_where_they_apply():
    for case in CASES:
        if any(k in case for k in ("num_beams", "num_return_sequences", "lookup", "reuse", "streamer")):
            continue
        m, ids, kw = _call(case)
        want = sfr.refusal(**case)
        with pytest.raises(want[0], match=want[1].replace("(", r"\(").replace(")", r"\)")):
            m.score(ids, attention_mask=kw.get("attention_mask"), suffixes=kw["suffixes"], share_prompt=kw.get("share_prompt"))
    with pytest.raises(ValueError, match="`labels` cannot be combined"):
        _model().score(IDS[:1], suffixes=[[5]], labels=IDS[:1])


def test_room_is_refused_after_the_splice_plan_and_before_the_tower():
    """P + max S_j + 1 > max_seq: the splice plan (host integers) gives P; nothing of the engine is touched"""
    m = _model(max_seq=23)
    ids = torch.tensor([[3, -200, 17, 18]])                      # 3 text slots + 16 image slots = 19
    img = torch.zeros(1, 3, 56, 56)
    assert sfr.room_refusal(19, [[5] * 4, [6]], 23) and not sfr.room_refusal(19, [[5] * 4, [6]], 24)
    with pytest.raises(ValueError, match="exceed max_seq = 23"):
        m.generate(ids, images=img, suffixes=[[5] * 4, [6]], max_new_tokens=4)
    with pytest.raises(ValueError, match="exceed max_seq = 23"):
        m.score(ids, images=img, suffixes=[[5] * 4, [6]])
    with pytest.raises(AssertionError, match="touched"):          # one slot more room: the call goes on to the engine (the stub)
        _model(max_seq=24).generate(ids, images=img, suffixes=[[5] * 4, [6]], max_new_tokens=4)


def test_table_accepts_what_is_supported():
    for kw in (dict(), dict(suffixes=((5,),)), dict(suffixes=((5,),), streamer=True), dict(suffixes=((5,),) * 8), dict(share_prompt=True),
               dict(suffixes=((5,),) * 16, max_batch=16, share_prompt=True), dict(suffixes=((5,),) * 17, max_batch=32, share_prompt=False),
               dict(suffixes=((5,),), share_prompt=True), dict(suffixes=((5,) * 40, (6,) * 30, (7,)), max_prefill_rows=120)):
        assert sfr.refusal(**kw) is None, kw
        a = {k: v for k, v in kw.items() if k in ("max_batch", "max_prefill_rows", "share_prompt")}
        rows = sx.check_suffix_args(1, False, [list(s) for s in kw.get("suffixes", ((5, 6),))], 320, a.get("max_batch", 8), a.get("max_prefill_rows", 1024),
                                    streamer=kw.get("streamer", False), q_heads=7, kv_heads=1, share_prompt=a.get("share_prompt"))
        assert rows == [list(s) for s in kw.get("suffixes", ((5, 6),))]


def test_suffixes_as_tensors_and_mixed():
    assert sx.as_id_lists([torch.tensor([5, 6]), [7], (8, 9, 10)]) == [[5, 6], [7], [8, 9, 10]]
    assert sx.as_id_lists(torch.tensor([[5, 6], [7, 8]])) == [[5, 6], [7, 8]]
    for bad in (None, "56", 5, torch.tensor([5, 6]), [torch.tensor([[5]])], [5, 6]):
        with pytest.raises(ValueError):
            sx.as_id_lists(bad)


def test_histories_seen_sets_and_padded_sequences():
    prompt, rows = [3, -200, 17, 17], [[5, 6, 7], [8], [17, 9]]
    assert sx.histories(prompt, rows) == sfr.histories(prompt, rows) == [[3, -200, 17, 17, 5, 6, 7], [3, -200, 17, 17, 8], [3, -200, 17, 17, 17, 9]]
    seen = sx.seen_sets(prompt, rows)
    assert seen == sfr.seen_sets(prompt, rows) == [[3, 17, 17, 5, 6, 7], [3, 17, 17, 8], [3, 17, 17, 17, 9]]      # the sentinel never counts
    seen[0].append(11)
    assert sx.seen_sets(prompt, rows)[0] == [3, 17, 17, 5, 6, 7]
    new = [[40, 41], [42, 43], [44, 45]]
    for pad in (None, 0, 2):
        got = sx.padded_sequences(prompt, rows, new, pad)
        assert got == sfr.padded_sequences(prompt, rows, new, pad)
        fill = 0 if pad is None else pad
        assert got[0] == [3, -200, 17, 17, 5, 6, 7, 40, 41] and got[1] == [3, -200, 17, 17, 8, 42, 43, fill, fill]
        assert len({len(r) for r in got}) == 1
    assert sx.suffix_token_table(rows, _lib.PAD_ROW) == [[5, 6, 7], [8, _lib.PAD_ROW, _lib.PAD_ROW], [17, 9, _lib.PAD_ROW]]


def test_score_label_arithmetic_against_plain_log_softmax_over_oracle_logits():
    """what score(suffixes=) composes -- token 0 from the prompt's last position, token t + 1 from suffix row t with the shifted labels --
    equals a plain log-softmax over the oracle's logits of every concatenated sequence, read at the suffix tokens"""
    cfg = tiny()
    sdt = {k: torch.from_numpy(v) for k, v in synth.state_dict(cfg, 3).items()}
    prompt, rows = [3, 17, 18, 19, 20], [[5, 6, 7, 8], [9], [10, 11]]
    P = len(prompt)

    def logits_of(seq):
        cache = oracle.decoder.KVCache(cfg.text["num_hidden_layers"])
        h = oracle.qwen2_model(sdt["model.embed_tokens.weight"][torch.as_tensor(seq)].float()[None], sdt, cfg.text, cache)
        return oracle.lm_head(h, sdt)[0]
    full = [logits_of(prompt + r) for r in rows]
    want, want_seq, want_n = sfr.score_from_logits(full, P, rows)
    first, lab = sx.score_labels(rows)
    assert first == [5, 9, 10] and lab == [[6, 7, 8, -100], [-100] * 4, [11, -100, -100, -100]]
    S_max = max(map(len, rows))
    got = torch.zeros(len(rows), S_max, dtype=torch.float64)
    for j, r in enumerate(rows):
        lsm = torch.log_softmax(full[j].double(), dim=-1)
        got[j, 0] = lsm[P - 1, first[j]]                         # the prompt's last position (the same logits for every row)
        for t in range(S_max - 1):
            if lab[j][t] != -100:
                assert t < len(r)
                got[j, t + 1] = lsm[P + t, lab[j][t]]            # suffix row t = slot P + t
    assert torch.equal(got, want)
    assert want_n.tolist() == [4, 1, 2] and torch.allclose(want_seq, got.sum(1))
    assert bool((got[1, 1:] == 0).all()) and bool((got[2, 2:] == 0).all())
    # the prompt's last-position logits are common to all rows: the causal prefix does not see the suffix
    assert torch.allclose(full[0][P - 1], full[1][P - 1], atol=1e-5) and torch.allclose(full[0][P - 1], full[2][P - 1], atol=1e-5)


@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (7, 1)])
def test_fp64_attention_references_against_a_dense_masked_softmax(Hq, Hkv):
    g = torch.Generator().manual_seed(Hq)
    N, cap = 3, 40
    k = torch.randn(N, Hkv, cap, 128, generator=g).bfloat16()
    v = torch.randn(N, Hkv, cap, 128, generator=g).bfloat16()
    for P, lengths in ((1, [1, 3, 2]), (17, [5, 1, 20]), (20, [20, 20, 20])):
        S = max(lengths)
        q = torch.randn(N, S, Hq, 128, generator=g).bfloat16()
        a, b = sfr.attn_suffix_ref(q, k, v, P, lengths), sfr.attn_suffix_dense(q, k, v, P, lengths)
        assert torch.allclose(a, b, rtol=1e-10, atol=1e-12)
        for j, n in enumerate(lengths):
            assert bool((a[j, n:] == 0).all()) and bool(a[j, :n].abs().sum() > 0)
        # poisoning what the key set excludes changes nothing in the reference either
        kp, vp = k.clone(), v.clone()
        kp[1:, :, :P] = 7.0; vp[1:, :, :P] = -7.0
        for j, n in enumerate(lengths):
            kp[j, :, P + n:] = 7.0; vp[j, :, P + n:] = -7.0
        assert torch.equal(sfr.attn_suffix_ref(q, kp, vp, P, lengths), a)
        # the decode step that follows: one query per row at its own length, against the suffix reference's last valid row
        lens = [P + n for n in lengths]
        ql = torch.stack([q[j, n - 1] for j, n in enumerate(lengths)])
        d = sfr.attn_shared_lens_ref(ql, k, v, 1, N, P, lens)
        for j, n in enumerate(lengths):
            assert torch.allclose(d[j], a[j, n - 1], rtol=1e-10, atol=1e-12)
