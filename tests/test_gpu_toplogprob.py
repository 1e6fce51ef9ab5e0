"""GPU: the extras of the log-probability record (omchat_amd/csrc/logprob.hip; DESIGN.md section 14, "Extras") -- the top_n alternatives
and the scored ids of every pick under the raw distribution.  The op against the fp64 restatement tests/toplogprob_ref.py on the very same
fp32 logits (ids exactly, values within logprob_ref.tolerance), the records of decode steps (eager and decode graph, bit-identical; the
raw / processed record unchanged by the extras), generate(top_logprobs=, score_token_ids=) on a tiny synthetic model, the off state's
allocations, and TP = 2 / 4 against TP = 1 (rank contexts on one GPU behind a test hook)."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import logprob_ref as lr
import toplogprob_ref as tr
from omchat_amd import synth, _lib
from omchat_amd._lib import check, ptr
from omchat_amd.config import tiny
from omchat_amd.engine import Engine

KINDS = ["gauss", "ties8", "inf_block", "unaligned"]


@functools.lru_cache(maxsize=None)
def _rows(V, b, kind):
    """-> (the device buffer's host image [b, ld], the rows [b, V], their ids in the contract's order [b, min(V, 20)], their log-sum-exps)"""
    rng = np.random.default_rng(V * 7 + b + len(kind))
    x = (rng.standard_normal((b, V)) * 3).astype(np.float32)
    if kind == "ties8":                                                # 8 distinct values, both zeros among them
        x = np.clip(np.round(x / 1.5), -4, 3).astype(np.float32)
        x[(x == 0) & (rng.random((b, V)) < 0.5)] = -0.0
    elif kind == "inf_block":                                          # whole slices without a finite value, and fewer than 20 finite ids at V = 20
        x[:, V // 4:V // 4 + V // 2] = -np.inf
    buf = x
    if kind == "unaligned":
        buf = np.full((b, V + 1), np.nan, dtype=np.float32)            # ld = V + 1: the pad column must never be read
        buf[:, :V] = x
    order = np.stack([tr.order(x[r])[:min(V, 20)] for r in range(b)])
    lses = [lr.lse(x[r]) for r in range(b)]
    for a in (buf, x, order):
        a.setflags(write=False)
    return buf, x, order, lses


def _op(lib, buf, V, top_n, score_ids=()):
    b, ld = buf.shape
    dev = torch.tensor(buf).cuda()                                     # (a copy: the cached rows are read-only)
    n_s = len(score_ids)
    vals = torch.full((b, max(top_n, 1)), 7.0, device="cuda")
    ids = torch.full((b, max(top_n, 1)), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((b, max(n_s, 1)), 7.0, device="cuda")
    t_s = torch.tensor([int(i) for i in score_ids] or [0], dtype=torch.int32)
    check(lib.omchat_op_top_logprobs(ptr(dev), b, V, ld, top_n, ptr(t_s) if n_s else None, n_s, ptr(vals) if top_n else None,
                                     ptr(ids) if top_n else None, ptr(sc) if n_s else None, _lib.cur_stream()))
    torch.cuda.synchronize()
    return vals.cpu().numpy()[:, :top_n], ids.cpu().numpy()[:, :top_n].astype(np.int64), sc.cpu().numpy()[:, :n_s]


def _check_values(name, got, row, ids, l):
    """got fp32 [k] against x_id - lse in fp64 for the ids of one fp32 row"""
    assert not np.isnan(got).any(), name
    worst = 0.0
    for g, i in zip(got, ids):
        x = float(row[i])
        if x == -np.inf:
            assert g == -np.inf, (name, i, g)
            continue
        err, tol = abs(float(g) - (x - l)), lr.tolerance(x, l)
        worst = max(worst, err / tol)
        assert err <= tol, (name, i, g, x - l, err, tol)
    print(f"TOPERR {name} worst err/tol {worst:.3e}")


@pytest.mark.parametrize("V", [152064, 1000, 37, 20])
@pytest.mark.parametrize("b", [1, 5, 32])
@pytest.mark.parametrize("top_n", [1, 5, 20])
@pytest.mark.parametrize("kind", KINDS)
def test_op_top_equals_ref(gpu_lib, V, b, top_n, kind):
    if top_n > V:
        pytest.skip("top_n > V is refused")
    buf, x, order, lses = _rows(V, b, kind)
    vals, ids, _ = _op(gpu_lib, buf, V, top_n)
    assert np.array_equal(ids, order[:, :top_n]), (kind, V, b, top_n)
    for r in range(b):
        _check_values(f"op-{kind}-V{V}-b{b}-n{top_n}", vals[r], x[r], ids[r], lses[r])
    fin = np.where(np.isfinite(vals), vals, np.float32(-3e38)).astype(np.float64)
    assert np.all(np.diff(fin, axis=1) <= 0)                           # descending, the -inf entries last


@pytest.mark.parametrize("V", [152064, 1000, 37])
@pytest.mark.parametrize("b", [1, 5, 32])
@pytest.mark.parametrize("n_score", [1, 4, 32])
def test_op_scored_ids_equal_ref(gpu_lib, V, b, n_score):
    buf, x, order, lses = _rows(V, b, "inf_block")
    rng = np.random.default_rng(V + n_score)
    must = [0, V - 1, V // 4 + 1]                                      # the ends of the row and an id whose logit is -inf
    rest = [int(i) for i in rng.permutation(V) if int(i) not in must]
    lists = [[i] for i in must] if n_score == 1 else [(must + rest)[:n_score]]
    for sids in lists:
        top_n = 5 if n_score == 4 else 0                               # with and without the alternatives next to them
        vals, ids, sc = _op(gpu_lib, buf, V, top_n, sids)
        for r in range(b):
            _check_values(f"op-scored-V{V}-b{b}-k{n_score}", sc[r], x[r], sids, lses[r])
        if V // 4 + 1 in sids:
            assert (sc[:, sids.index(V // 4 + 1)] == -np.inf).all()
        if top_n:
            assert np.array_equal(ids, order[:, :top_n])


def test_op_refusals(gpu_lib):
    buf, _, _, _ = _rows(37, 1, "gauss")
    for top_n, sids in ((21, ()), (0, ()), (5, (37,)), (5, (-1,)), (0, (3, 3)), (0, tuple(range(33)))):
        with pytest.raises(ValueError):
            _op(gpu_lib, buf, 37, top_n, sids)
    with pytest.raises(ValueError):
        _op(gpu_lib, _rows(20, 1, "gauss")[0][:, :12].copy(), 12, 20)      # top_n beyond the vocabulary


# ---------------------------------------------------------------------------------------------------------------- engine level
def _tiny_model(b=2, seed=21):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    cfg = tiny()
    e = Engine(cfg, dtype="bf16", max_seq=128, max_batch=b, max_tiles=1, vision=False)
    e.load_state_dict(synth.state_dict(cfg, seed), strict=False)
    return cfg, e, OmChatQwen2ForCausalLM(cfg.clone(), e)


PROMPT = [[3, 17, 18, 19, 20, 21, 7, 9], [5, 6, 11, 12, 13, 40, 41, 42]]
V_TINY = tiny().text["vocab_size"]
SMP = dict(temperature=0.9, top_k=50, top_p=0.9, repetition_penalty=1.3)
MODES = dict(greedy={}, sampled=dict(smp=SMP), ngram=dict(ngram=2))
SIDS = [0, 17, 40, V_TINY - 1]


def _steps(e, m, ids, n, smp=None, ngram=0, graph=False, top_n=0, sids=None, seed=77):
    """n picks (the prefill's + n - 1 decode steps with want_logits) -> (ids [b, n], the n logits arrays, (raw, proc, counts), extras or None)"""
    e.enable_decode_graph(graph)
    out = m.forward(input_ids=ids, use_cache=True)
    b = ids.shape[0]
    if ngram:
        e.set_constraints(b, ids.tolist(), n, no_repeat_ngram_size=ngram)
    else:
        e.constraints_off()
    e.set_logprobs(b, n, top_n, sids)
    if smp is not None:
        e.set_sampling(b, seed=seed, seen=[[i for i in r if i >= 0] for r in ids.tolist()], **smp)
    else:
        e.sampling_off()
    lg = out.local_logits
    tok = e.sample(lg) if smp is not None else e.argmax(lg)
    toks, lgs = [], []
    for step in range(n):
        toks.append(tok.cpu().numpy().astype(np.int64)); lgs.append(lg.cpu().numpy())
        if step < n - 1:
            tok, lg = e.decode_step(tok, want_logits=True)
    raw, proc, counts = e.read_logprobs(b)
    ext = None
    if top_n or sids:
        tv, ti, sc, xc = e.read_logprob_extras(b)
        assert xc == counts
        ext = (tv.numpy(), ti.numpy(), sc.numpy())
    e.enable_decode_graph(False)
    e.constraints_off(); e.sampling_off(); e.logprobs_off()
    return np.stack(toks, 1), lgs, (raw.numpy(), proc.numpy(), counts), ext


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_decode_step_extras_equal_ref_eager_and_graph(gpu_lib, mode):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    b, n, top_n = ids.shape[0], 9, 20                                  # the prefill's pick + 8 decode steps
    kw = MODES[mode]
    off_toks, _, (off_raw, off_proc, _), none = _steps(e, m, ids, n, **kw)
    assert none is None
    toks, lgs, (raw, proc, counts), (tv, ti, sc) = _steps(e, m, ids, n, top_n=top_n, sids=SIDS, **kw)
    assert np.array_equal(toks, off_toks) and counts == [n] * b
    assert np.array_equal(_bits(raw), _bits(off_raw)) and np.array_equal(_bits(proc), _bits(off_proc))      # the extras change no bit of it
    assert tv.shape == (b, n, top_n) and ti.shape == (b, n, top_n) and sc.shape == (b, n, len(SIDS))
    hits = 0
    for t in range(n):
        for r in range(b):
            row, l = lgs[t][r], lr.lse(lgs[t][r])
            r_ids, _ = tr.top(row, top_n)
            assert np.array_equal(ti[r, t], r_ids), (mode, t, r)
            _check_values(f"engine-{mode}-top", tv[r, t], row, r_ids, l)
            _check_values(f"engine-{mode}-scored", sc[r, t], row, SIDS, l)
            tok = int(toks[r, t])
            where = np.flatnonzero(ti[r, t] == tok)
            if where.size:                                             # the picked id among the alternatives: its .logprobs value, bit for bit
                hits += 1
                assert _bits(tv[r, t, where[:1]]) == _bits(raw[r, t:t + 1])
            if tok in SIDS:
                assert _bits(sc[r, t, SIDS.index(tok):SIDS.index(tok) + 1]) == _bits(raw[r, t:t + 1])
            if mode == "greedy":
                assert ti[r, t, 0] == tok
    assert hits > 0
    g_toks, _, (g_raw, g_proc, g_counts), (g_tv, g_ti, g_sc) = _steps(e, m, ids, n, graph=True, top_n=top_n, sids=SIDS, **kw)
    assert e.decode_graph_stats()["replays"] > 0
    assert np.array_equal(g_toks, toks) and g_counts == counts
    assert np.array_equal(_bits(g_raw), _bits(raw)) and np.array_equal(_bits(g_proc), _bits(proc))
    assert np.array_equal(_bits(g_tv), _bits(tv)) and np.array_equal(g_ti, ti) and np.array_equal(_bits(g_sc), _bits(sc))
    e.close()


def test_off_state_allocates_nothing_and_changes_drop_the_graphs(gpu_lib):
    _, e, m = _tiny_model(b=1)
    _, fresh, _ = _tiny_model(b=1)
    ids = torch.tensor(PROMPT[:1])
    for eng in (e, fresh):
        eng.set_logprobs(1, 16)
    assert e.device_bytes() == fresh.device_bytes()
    with pytest.raises(ValueError):
        e.read_logprob_extras(1)                                       # refused while the extras are off
    e.set_logprobs(1, 16, top_n=5)
    with_top = e.device_bytes()
    assert with_top > fresh.device_bytes()
    e.set_logprobs(1, 16)                                              # off again: nothing shrinks, and the plain call means 0, NULL, 0
    assert e.device_bytes() == with_top
    with pytest.raises(ValueError):
        e.read_logprob_extras(1)
    fresh.set_logprobs(1, 16)
    assert fresh.device_bytes() < with_top                             # a context that never asked never pays
    # refusals of the setter: before anything changes
    for kw in (dict(top_n=21), dict(top_n=-1), dict(top_n=V_TINY + 1), dict(score_token_ids=[V_TINY]), dict(score_token_ids=[-1]),
               dict(score_token_ids=[3, 3]), dict(score_token_ids=list(range(33)))):
        with pytest.raises(ValueError):
            e.set_logprobs(1, 16, **kw)
    # another top_n or id list drops the captured decode graphs; the same values keep them
    e.enable_decode_graph(True)
    m.generate(ids, max_new_tokens=6, output_logprobs=True, return_dict_in_generate=True, top_logprobs=5)
    captures = e.decode_graph_stats()["captures"]
    m.generate(ids, max_new_tokens=6, output_logprobs=True, return_dict_in_generate=True, top_logprobs=5)
    assert e.decode_graph_stats()["captures"] == captures
    m.generate(ids, max_new_tokens=6, output_logprobs=True, return_dict_in_generate=True, top_logprobs=6)
    assert e.decode_graph_stats()["captures"] > captures
    captures = e.decode_graph_stats()["captures"]
    m.generate(ids, max_new_tokens=6, output_logprobs=True, return_dict_in_generate=True, top_logprobs=6, score_token_ids=[4])
    assert e.decode_graph_stats()["captures"] > captures
    e.enable_decode_graph(False)
    e.close(); fresh.close()


# ---------------------------------------------------------------------------------------------------------------- generate()
def test_generate_fields_eos_and_rewind(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    b, T, n = ids.shape[0], ids.shape[1], 10
    kw = dict(output_logprobs=True, return_dict_in_generate=True)
    base = m.generate(ids, max_new_tokens=n, **kw)
    free = m.generate(ids, max_new_tokens=n, top_logprobs=5, score_token_ids=SIDS, **kw)
    assert torch.equal(free.sequences, base.sequences)
    assert torch.equal(free.logprobs.view(torch.int32), base.logprobs.view(torch.int32))
    assert free.top_logprobs.shape == (b, n, 5) and free.top_logprobs.dtype == torch.float32
    assert free.top_token_ids.shape == (b, n, 5) and free.top_token_ids.dtype == torch.int64
    assert free.scored_logprobs.shape == (b, n, len(SIDS)) and free.scored_logprobs.dtype == torch.float32
    assert free["top_logprobs"] is free.top_logprobs and free["scored_logprobs"] is free.scored_logprobs
    assert torch.equal(free.top_token_ids[:, :, 0], free.sequences[:, T:])                     # greedy: the generated id leads
    assert torch.equal(free.top_logprobs[:, :, 0].view(torch.int32), free.logprobs.view(torch.int32))
    only_top = m.generate(ids, max_new_tokens=n, top_logprobs=5, **kw)
    assert "scored_logprobs" not in only_top and not hasattr(only_top, "scored_logprobs")
    assert torch.equal(only_top.top_token_ids, free.top_token_ids)
    only_sc = m.generate(ids, max_new_tokens=n, score_token_ids=SIDS, **kw)
    assert "top_logprobs" not in only_sc and "top_token_ids" not in only_sc
    assert torch.equal(only_sc.scored_logprobs.view(torch.int32), free.scored_logprobs.view(torch.int32))
    lg = m.forward(input_ids=ids, use_cache=True).local_logits.cpu().numpy()
    for r in range(b):
        r_ids, _ = tr.top(lg[r], 5)
        assert np.array_equal(free.top_token_ids[r, 0].numpy(), r_ids)
        _check_values("generate-col0-top", free.top_logprobs[r, 0].numpy(), lg[r], r_ids, lr.lse(lg[r]))
        _check_values("generate-col0-scored", free.scored_logprobs[r, 0].numpy(), lg[r], SIDS, lr.lse(lg[r]))
    # generation_config carries both keywords too
    m.generation_config.top_logprobs, m.generation_config.score_token_ids = 5, SIDS
    cfgd = m.generate(ids, max_new_tokens=n, **kw)
    assert torch.equal(cfgd.top_token_ids, free.top_token_ids) and torch.equal(cfgd.scored_logprobs, free.scored_logprobs)
    m.generation_config.top_logprobs, m.generation_config.score_token_ids = None, None
    # EOS mid-stream: row 0 ends first; behind it 0.0 / -1 / 0.0
    gen = free.sequences[:, T:].tolist()
    stop = next(i for i in range(n - 1) if gen[0][i] not in gen[0][:i] and gen[0][i] not in gen[1][:i + 1])
    eos = gen[0][stop]
    out = m.generate(ids, max_new_tokens=n, eos_token_id=eos, pad_token_id=0, top_logprobs=5, score_token_ids=SIDS, **kw)
    new = out.sequences.shape[1] - T
    assert new > stop + 1 and out.top_logprobs.shape == (b, new, 5) and out.scored_logprobs.shape == (b, new, len(SIDS))
    assert bool((out.top_logprobs[0, stop + 1:] == 0).all()) and bool((out.top_token_ids[0, stop + 1:] == -1).all())
    assert bool((out.scored_logprobs[0, stop + 1:] == 0).all())
    assert torch.equal(out.top_token_ids[0, :stop + 1], free.top_token_ids[0, :stop + 1])
    assert torch.equal(out.top_token_ids[1], free.top_token_ids[1, :new])
    assert torch.equal(out.top_logprobs[1].view(torch.int32), free.top_logprobs[1, :new].view(torch.int32))
    # b = 1: the EOS ends the call, the step enqueued ahead is taken back with its records -- exactly `new` of them
    one = ids[:1]
    free1 = m.generate(one, max_new_tokens=n, top_logprobs=5, score_token_ids=SIDS, **kw)
    gen1 = free1.sequences[0, T:].tolist()
    stop = max(i for i in range(n - 1) if gen1[i] not in gen1[:i])
    o1 = m.generate(one, max_new_tokens=n, eos_token_id=gen1[stop], top_logprobs=5, score_token_ids=SIDS, **kw)
    assert o1.top_logprobs.shape == (1, stop + 1, 5) and e.read_logprob_extras(1)[3] == [stop + 1]
    assert torch.equal(o1.top_logprobs.view(torch.int32), free1.top_logprobs[:, :stop + 1].view(torch.int32))
    assert torch.equal(o1.scored_logprobs.view(torch.int32), free1.scored_logprobs[:, :stop + 1].view(torch.int32))
    # a second call without the keywords: no extra fields, nothing recorded
    plain = m.generate(one, max_new_tokens=n, **kw)
    assert "top_logprobs" not in plain and "top_token_ids" not in plain and "scored_logprobs" not in plain
    with pytest.raises(ValueError):
        e.read_logprob_extras(1)
    # the refusals: before anything is enqueued
    kv = e.kv_lengths(1)
    for bad in (dict(top_logprobs=5), dict(score_token_ids=[1]), dict(top_logprobs=0, **kw), dict(top_logprobs=21, **kw),
                dict(score_token_ids=[], **kw), dict(score_token_ids=[1, 1], **kw), dict(score_token_ids=[V_TINY], **kw),
                dict(score_token_ids=list(range(33)), **kw)):
        with pytest.raises(ValueError):
            m.generate(one, max_new_tokens=4, **bad)
    with pytest.raises(NotImplementedError):
        m.generate(one, max_new_tokens=4, num_beams=2, top_logprobs=5, **kw)
    with pytest.raises(NotImplementedError):
        m.generate(one, max_new_tokens=4, prompt_lookup_num_tokens=3, top_logprobs=5, **kw)
    assert e.kv_lengths(1) == kv
    e.close()


def test_generate_ragged_batch_and_return_sequences(gpu_lib):
    _, e, m = _tiny_model(b=6)
    kw = dict(output_logprobs=True, return_dict_in_generate=True, top_logprobs=5, score_token_ids=SIDS)
    ids = torch.tensor([[3, 17, 18, 19, 20, 21, 7, 9], [5, 6, 11, 12, 0, 0, 0, 0]])
    mask = torch.tensor([[1] * 8, [1] * 4 + [0] * 4])
    n = 8
    out = m.generate(ids, attention_mask=mask, max_new_tokens=n, pad_token_id=0, **kw)
    assert m._padded_batch and out.top_token_ids.shape == (2, n, 5)
    assert torch.equal(out.top_token_ids[:, :, 0], out.sequences[:, 8:])
    assert torch.equal(out.top_logprobs[:, :, 0].view(torch.int32), out.logprobs.view(torch.int32))
    # the same steps by hand with the logits read back: every record against the ref
    fw = m.forward(input_ids=ids, attention_mask=mask, use_cache=True)
    e.sampling_off(); e.constraints_off(); e.logprobs_off()
    lg = fw.local_logits
    tok = e.argmax(lg)
    m1 = torch.cat([mask, torch.ones(2, 1, dtype=mask.dtype)], 1)
    _, pos1, mask1, _, _, _ = m.prepare_inputs_labels_for_multimodal(torch.zeros(2, 1, dtype=torch.long), None, m1, fw.past_key_values, None, None)
    if pos1 is None:
        pos1 = torch.full((2, 1), fw.past_key_values.get_seq_length(), dtype=torch.long)
    e.masked_decode_begin(pos1, mask1)
    for t in range(n):
        row = lg.cpu().numpy()
        for r in range(2):
            r_ids, _ = tr.top(row[r], 5)
            assert np.array_equal(out.top_token_ids[r, t].numpy(), r_ids)
            _check_values("generate-masked-top", out.top_logprobs[r, t].numpy(), row[r], r_ids, lr.lse(row[r]))
            _check_values("generate-masked-scored", out.scored_logprobs[r, t].numpy(), row[r], SIDS, lr.lse(row[r]))
        if t < n - 1:
            tok, lg = e.decode_step_masked_next(tok, want_logits=True)
    # num_return_sequences = 3: fields [b * N, ...], every sibling row its own record
    two = torch.tensor(PROMPT)
    smp = dict(do_sample=True, seed=5, num_return_sequences=3, temperature=0.9, top_k=50, top_p=0.9)
    g = m.generate(two, max_new_tokens=n, **smp, **kw)
    assert g.sequences.shape[0] == 6 and g.top_logprobs.shape == (6, n, 5) and g.top_token_ids.shape == (6, n, 5)
    assert g.scored_logprobs.shape == (6, n, len(SIDS))
    assert torch.equal(g.sequences, m.generate(two, max_new_tokens=n, **smp))
    assert bool((g.top_logprobs[:, :, :-1] >= g.top_logprobs[:, :, 1:]).all()) and bool((g.top_token_ids >= 0).all())
    lg2 = m.forward(input_ids=two, use_cache=True).local_logits.cpu().numpy()
    for r in range(6):                                                 # position 0: the prompt's own prefill logits, for each of its siblings
        r_ids, _ = tr.top(lg2[r // 3], 5)
        assert np.array_equal(g.top_token_ids[r, 0].numpy(), r_ids)
        _check_values("generate-group-top", g.top_logprobs[r, 0].numpy(), lg2[r // 3], r_ids, lr.lse(lg2[r // 3]))
    hit = g.top_token_ids == g.sequences[:, 8:].unsqueeze(-1)          # a sampled id among the alternatives: its .logprobs value
    assert bool(hit.any())
    assert torch.equal(g.top_logprobs[hit].view(torch.int32), g.logprobs.unsqueeze(-1).expand_as(hit)[hit].view(torch.int32))
    e.close()


# ---------------------------------------------------------------------------------------------------------------- tensor parallelism
class _Group:
    """all-reduce hook over rank contexts living on one GPU (tests/test_gpu_tp_single.py's pattern)"""

    def __init__(self, n):
        self.n, self.barrier, self.slots = n, threading.Barrier(n, timeout=120), [None] * n
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def hook_for(self, rank):
        def hook(user, buf, count, dtype, stream):
            torch.cuda.synchronize()
            self.slots[rank] = buf
            self.barrier.wait()
            if rank == 0:
                assert dtype == _lib.F32
                parts = []
                for b in self.slots:
                    t = torch.empty(count, dtype=torch.float32, device="cuda")
                    assert self.hip.hipMemcpy(t.data_ptr(), b, count * 4, 3) == 0
                    parts.append(t)
                s = sum(parts)
                for b in self.slots:
                    assert self.hip.hipMemcpy(b, s.data_ptr(), count * 4, 3) == 0
                torch.cuda.synchronize()
            self.barrier.wait()
            return 0
        return _lib.ALLREDUCE_FN(hook)


def _tp_steps(engines, logits_steps, top_n, sids):
    n = len(engines)
    out, err = [None] * n, [None] * n

    def work(r):
        try:
            e = engines[r]
            b = logits_steps[0].shape[0]
            e.sampling_off()
            e.set_logprobs(b, len(logits_steps), top_n, sids)
            Vl = logits_steps[0].shape[1] // n
            ids = [e.argmax(lg[:, r * Vl:(r + 1) * Vl].contiguous()).cpu().numpy() for lg in logits_steps]
            raw, _, counts = e.read_logprobs(b)
            tv, ti, sc, xc = e.read_logprob_extras(b)
            assert xc == counts
            out[r] = (np.stack(ids, 1), raw.numpy(), tv.numpy(), ti.numpy(), sc.numpy())
        except BaseException as ex:       # noqa
            err[r] = ex
    th = [threading.Thread(target=work, args=(r,)) for r in range(n)]
    for t in th: t.start()
    for t in th: t.join(timeout=300)
    for ex in err:
        if ex is not None:
            raise ex
    return out


@pytest.mark.parametrize("tp", [2, 4])
@pytest.mark.parametrize("vocab", [320, 32], ids=["V320", "V32"])      # V32: a shard holds 16 (TP = 2) or 8 (TP = 4) ids, fewer than top_n
def test_tp_extras_agree_with_tp1(gpu_lib, tp, vocab):
    cfg = tiny(vocab=vocab)
    V, b, steps, top_n = vocab, 3, 3, 20
    sids = [0, V // tp, V - 1, 5]                                      # ids of the first, the second and the last shard
    rng = np.random.default_rng(tp + vocab)
    host = [(rng.standard_normal((b, V)) * 1.5).astype(np.float32) for _ in range(steps)]
    host[1] = np.round(host[1])                                        # heavy ties, across the shards
    host[2][:, V // 2:V // 2 + 6] = -np.inf
    host[2][:, 5] = -np.inf                                            # a scored id at -inf
    logits_steps = [torch.from_numpy(h).cuda() for h in host]
    one = Engine(cfg, dtype="bf16", max_seq=16, max_batch=b, max_tiles=1, vision=False)
    ids1, raw1, tv1, ti1, sc1 = _tp_steps([one], logits_steps, top_n, sids)[0]
    grp = _Group(tp)
    engines, hooks = [], []
    for r in range(tp):
        e = Engine(cfg, dtype="bf16", max_seq=16, max_batch=b, max_tiles=1, vision=False, tp_rank=r, tp_size=tp, comm=C.c_void_p(1))
        h = grp.hook_for(r)
        check(gpu_lib.omchat_set_allreduce_hook(e.h, C.cast(h, C.c_void_p), None))
        engines.append(e); hooks.append(h)
    got = _tp_steps(engines, logits_steps, top_n, sids)
    for t, row in enumerate(host):
        for i in range(b):
            l = lr.lse(row[i])
            r_ids, _ = tr.top(row[i], top_n)
            assert np.array_equal(ti1[i, t], r_ids)
            _check_values("tp1-top", tv1[i, t], row[i], r_ids, l)
            _check_values("tp1-scored", sc1[i, t], row[i], sids, l)
            for r in range(tp):
                ids, raw, tv, ti, sc = got[r]
                assert np.array_equal(ids, ids1)
                assert np.array_equal(ti[i, t], ti1[i, t]), (r, i, t)                      # ids: TP = 1's, exactly
                for k, gid in enumerate(r_ids):
                    if row[i, gid] == -np.inf:
                        assert tv[i, t, k] == -np.inf
                    else:
                        assert abs(float(tv[i, t, k]) - float(tv1[i, t, k])) <= lr.tolerance(row[i, gid], l), (r, i, t, k)
                for k, gid in enumerate(sids):
                    if row[i, gid] == -np.inf:
                        assert sc[i, t, k] == -np.inf
                    else:
                        assert abs(float(sc[i, t, k]) - float(sc1[i, t, k])) <= lr.tolerance(row[i, gid], l), (r, i, t, k)
                assert _bits(tv[i, t, :1]) == _bits(raw[i, t:t + 1])                       # greedy: the picked id leads, bit for bit
    for r in range(1, tp):                                             # every rank holds the same bits
        for a, z in zip(got[r][1:], got[0][1:]):
            assert np.array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(z) if z.dtype == np.float32 else z)
    for e in engines + [one]:
        e.close()
