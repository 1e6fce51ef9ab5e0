"""GPU: the on-device token-FSM stage (omchat_amd/csrc/fsm.hip) -- the mark and apply passes through omchat_op_fsm
against tests/fsm_ref.py (states, the set of finite entries, their bits), then decode steps and generate(token_fsm=) on a tiny synthetic
model against a host-driven loop that applies the reference mask to the step's raw logits (eager, decode graph, sampling, constraints on
top, EOS rewind, padded batch, sampled groups, suffixes, log-probs, table reuse), and the same ids at TP = 2 / 4 as at TP = 1.  Every
comparison of ids, states and masks is exact."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import constraints_ref as cr
import fsm_ref as fr
import logprob_ref as lr
import sampling_ref as sr
from omchat_amd import synth, _lib
from omchat_amd._lib import check, ptr
from omchat_amd.config import tiny
from omchat_amd.engine import Engine
from omchat_amd.fsm import DEAD, MAX_EDGES, MAX_STATES, TokenFSM

V_BIG = 152064


def _i32(xs):
    return torch.tensor([int(x) for x in xs] or [0], dtype=torch.int32)


def _op_fsm(lib, arrays, states, fed, V, V_total, rank, logits):
    off, tok, nxt = (a if torch.is_tensor(a) else _i32(a) for a in arrays)
    b = len(states)
    st, fd = _i32(states), (None if fed is None else _i32(fed))
    out = torch.full_like(logits, 7.0)
    new = torch.full((b,), -7, dtype=torch.int32)
    check(lib.omchat_op_fsm(off.numel() - 1, ptr(off), ptr(tok), ptr(nxt), ptr(st), ptr(fd), b, V, V_total, rank, ptr(logits), ptr(out), ptr(new),
                            _lib.cur_stream()))
    torch.cuda.synchronize()
    return new.tolist(), out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _big_table():
    """states of 1, 63, 64, 65, 2 047, 2 048 and 2 049 edges, one with every id, one on the borders (ids 0 and V - 1, an apply-tile border,
    the shard borders of TP = 2 and 4) and one whose edges all lie in the first shard of TP = 4"""
    rng = np.random.default_rng(11)
    sizes = [1, 63, 64, 65, 2047, 2048, 2049]
    sets = [sorted(rng.choice(V_BIG, n, replace=False).tolist()) for n in sizes]
    sets.append(list(range(V_BIG)))
    sets.append([0, 2047, 2048, 38015, 38016, 76031, 76032, 114047, 114048, V_BIG - 1])
    sets.append(list(range(100, 164)))
    n = len(sets)
    trans = {s: {t: int((t + s) % n) for t in ids} for s, ids in enumerate(sets)}
    return trans, tuple(_i32(a) for a in TokenFSM(trans, vocab_size=V_BIG).arrays())      # (host tensors, made once)


def _absent(ids, V_total):
    have = set(ids)
    return next((t for t in (V_total - 2, 1, 5, 29) if t not in have), None)


def _check_op(lib, trans, arrays, b, tp, V_total, seed):
    V = V_total // tp
    n = len(trans)
    rng = np.random.default_rng(seed)
    states = [(seed + r) % n for r in range(b)]
    if b > 1:
        states[2 % b] = DEAD
    feds = [None]
    fd = []
    for r, s in enumerate(states):                                # first edge, last edge, absent (-> DEAD), in turn
        ids = sorted(trans[s]) if s != DEAD else [3]
        absent = _absent(ids, V_total)
        fd.append([ids[0], ids[-1], absent if absent is not None else ids[0]][r % 3])
    feds.append(fd)
    for rank in sorted({0, tp - 1}):
        lg = torch.from_numpy(rng.standard_normal((b, V)).astype(np.float32)).cuda()
        keep = lg.clone()
        for fed in feds:
            want_states = states if fed is None else [fr.step(trans, s, t) for s, t in zip(states, fed)]
            new, out = _op_fsm(lib, arrays, states, fed, V, V_total, rank, lg)
            assert new == want_states, (tp, rank, fed is None, new, want_states)
            assert torch.equal(lg, keep)                          # the input logits are never written
            raw = keep.cpu().numpy()
            for r in range(b):
                ref = fr.apply(trans, raw[r], want_states[r], gbase=rank * V)
                assert np.array_equal(np.isfinite(out[r]), np.isfinite(ref)), (tp, rank, r, want_states[r])
                assert np.array_equal(out[r].view(np.uint32), ref.view(np.uint32))      # finite entries carry the input's bits
    return states


@pytest.mark.parametrize("tp", [1, 2, 4])
@pytest.mark.parametrize("b", [1, 5, 32])
def test_op_fsm_equals_ref(gpu_lib, b, tp):
    trans, arrays = _big_table()
    n = len(trans)
    # every state comes up as a row's state over the seeds; b = 1 takes each state in turn
    for seed in (range(n) if b == 1 else (0, 3, 7)):
        _check_op(gpu_lib, trans, arrays, b, tp, V_BIG, seed)


def test_op_fsm_single_shard_state_leaves_other_ranks_all_inf(gpu_lib):
    trans, arrays = _big_table()
    s = len(trans) - 1                                            # ids 100 .. 163: rank 0's at TP = 4
    lg = torch.randn(2, V_BIG // 4, device="cuda")
    for rank in range(4):
        new, out = _op_fsm(gpu_lib, arrays, [s, s], None, V_BIG // 4, V_BIG, rank, lg)
        assert new == [s, s]
        fin = np.isfinite(out)
        assert fin.sum() == (2 * 64 if rank == 0 else 0)
        assert rank != 0 or fin[:, 100:164].all()


def test_op_fsm_small_vocab_caps_and_invalid_tables(gpu_lib):
    # V = 37: no vector path, a partial last bitmap word
    trans = {0: {0: 1, 31: 0, 32: 1, 36: 0}, 1: {5: 0, 36: 1}}
    arrays = TokenFSM(trans, vocab_size=37).arrays()
    _check_op(gpu_lib, trans, arrays, 5, 1, 37, 0)
    lg = torch.randn(1, 37, device="cuda")
    bad = [([0, 2], [4, 3], [0, 0]),                              # unsorted
           ([0, 2], [4, 4], [0, 0]),                              # duplicate
           ([0, 1], [37], [0]),                                   # id out of range
           ([0, 1], [-1], [0]),
           ([0, 1], [3], [1]),                                    # target out of range
           ([0, 1], [3], [-1]),
           ([0, 1, 1], [3], [1]),                                 # a reachable state without an edge
           ([1, 2], [3, 4], [0, 0])]                              # offsets not from 0
    for arr in bad:
        with pytest.raises(ValueError):
            _op_fsm(gpu_lib, arr, [0], None, 37, 37, 0, lg)
    with pytest.raises(ValueError, match="state 1 can be reached and has no edge.*add an EOS edge"):
        _op_fsm(gpu_lib, ([0, 1, 1], [3], [1]), [0], None, 37, 37, 0, lg)
    with pytest.raises(ValueError):                               # a row in a state without an edge
        _op_fsm(gpu_lib, ([0, 1, 1], [3], [0]), [1], None, 37, 37, 0, lg)
    with pytest.raises(ValueError):
        _op_fsm(gpu_lib, arrays, [2], None, 37, 37, 0, lg)
    # above the caps: refused from n_states / the offsets alone, before an edge is read
    z = _i32([0, 0])
    new, out = torch.zeros(1, dtype=torch.int32), torch.empty_like(lg)
    with pytest.raises(ValueError, match="n_states"):
        check(gpu_lib.omchat_op_fsm(MAX_STATES + 1, ptr(z), ptr(z), ptr(z), ptr(z), None, 1, 37, 37, 0, ptr(lg), ptr(out), ptr(new), _lib.cur_stream()))
    over = _i32([0, MAX_EDGES + 1])
    with pytest.raises(ValueError, match="edges"):
        check(gpu_lib.omchat_op_fsm(1, ptr(over), ptr(z), ptr(z), ptr(z), None, 1, 37, 37, 0, ptr(lg), ptr(out), ptr(new), _lib.cur_stream()))


# ---------------------------------------------------------------------------------------------------------------- model level
def _tiny_model(b=2, seed=21, max_seq=128):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    cfg = tiny()
    e = Engine(cfg, dtype="bf16", max_seq=max_seq, max_batch=b, max_tiles=1, vision=False)
    e.load_state_dict(synth.state_dict(cfg, seed), strict=False)
    return cfg, e, OmChatQwen2ForCausalLM(cfg.clone(), e)


PROMPT = [[3, 17, 18, 19, 20, 21, 7, 9], [5, 6, 11, 12, 13, 40, 41, 42]]
V_TINY = tiny().text["vocab_size"]
SMP = dict(temperature=0.9, top_k=50, top_p=0.9, repetition_penalty=1.3)
K_CYCLE = 4


def _cyclic(free):
    """state i allows two thirds of the vocabulary, minus every id the free run picks at the positions i mod K -- so the constrained run
    cannot repeat the free one, from position 0 on -- and leads to state i + 1"""
    trans = {}
    for i in range(K_CYCLE):
        out = {int(row[t]) for row in free for t in range(i, len(row), K_CYCLE)}
        trans[i] = {t: (i + 1) % K_CYCLE for t in range(V_TINY) if (t * 7 + i) % 3 != 0 and t not in out}
        assert trans[i]
    return trans, TokenFSM(trans, vocab_size=V_TINY)


def _con_kw(p):
    return dict(no_repeat_ngram_size=p["ngram"], bad_words_ids=p["bad_words"], min_new_tokens=p["min_new"], min_length=p["min_len"], eos=p["eos"],
                suppress_tokens=p["suppress"], begin_suppress_tokens=p["begin_suppress"])


def _ref_pick(lg, trans, states, hist, p, step, smp, seed):
    out = []
    for r in range(lg.shape[0]):
        l = fr.apply(trans, lg[r], states[r])
        if p is not None:
            l = cr.apply(l, cr.banned_ids(hist[r], p, step))
        assert np.isfinite(l).any()
        if smp is None:
            out.append(int(np.argmax(l)))
        else:
            out.append(sr.sample_row(l, r, step, seed, smp["temperature"], smp["top_k"], smp["top_p"], [i for i in hist[r] if i >= 0],
                                     smp["repetition_penalty"]))
    return out


def _host_loop(e, m, ids, n, trans, f, starts=None, graph=False, smp=None, seed=5, p=None, logprobs=False):
    """the device's constrained picks, each checked against the reference mask applied on the host to the step's RAW logits"""
    e.enable_decode_graph(graph)
    out = m.forward(input_ids=ids, use_cache=True)
    b = ids.shape[0]
    hist = [list(r) for r in ids.tolist()]
    states = list(starts) if starts is not None else [0] * b
    e.load_token_fsm(f)
    e.token_fsm_begin(b, states, n)
    if p is not None:
        e.set_constraints(b, hist, n, **_con_kw(p))
    if logprobs:
        e.set_logprobs(b, n)
    if smp is not None:
        e.set_sampling(b, seed=seed, seen=[[i for i in r if i >= 0] for r in hist], **smp)
    else:
        e.sampling_off()
    lg = out.local_logits
    tok = e.sample(lg) if smp is not None else e.argmax(lg)
    got, raws, sts = [], [], []
    for step in range(n):
        raw = lg.cpu().numpy()
        assert np.isfinite(raw).all()                              # the logits handed back stay the raw ones
        ref = _ref_pick(raw, trans, states, hist, p, step, smp, seed)
        assert tok.tolist() == ref, (step, tok.tolist(), ref)
        assert e.token_fsm_states(b) == states, (step, states)
        got.append(ref); raws.append(raw); sts.append(list(states))
        for r in range(b):
            hist[r].append(ref[r])
            states[r] = fr.step(trans, states[r], ref[r])
        if step < n - 1:
            tok, lg = e.decode_step(tok, want_logits=True)
    rec = e.read_logprobs(b) if logprobs else None
    e.enable_decode_graph(False)
    e.constraints_off(); e.sampling_off(); e.token_fsm_off()
    if logprobs:
        e.logprobs_off()
    return np.array(got).T, raws, sts, rec


def _new(m, ids, n, **kw):
    return m.generate(ids, max_new_tokens=n, **kw)[:, ids.shape[1]:]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("smp", [None, SMP], ids=["greedy", "sampled"])
def test_decode_steps_pick_what_the_ref_picks(gpu_lib, smp, graph):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    kw = dict(do_sample=True, seed=77, **SMP) if smp else {}
    free = _new(m, ids, 48, **kw).tolist()
    trans, f = _cyclic(free)
    got, _, _, _ = _host_loop(e, m, ids, 48, trans, f, graph=graph, smp=smp, seed=77)
    if graph:
        assert e.decode_graph_stats()["replays"] > 0
    assert all(got[r, 0] != free[r][0] for r in range(2)) and got.tolist() != free      # the automaton bit
    for r in range(2):
        assert fr.walk(trans, got[r]) != DEAD
    e.enable_decode_graph(graph)
    out = m.generate(ids, max_new_tokens=48, token_fsm=f, return_dict_in_generate=True, **kw)
    assert np.array_equal(out.sequences[:, ids.shape[1]:].numpy(), got)
    assert out.fsm_states.tolist() == [fr.walk(trans, got[r]) for r in range(2)]
    # a call without the keyword is unconstrained again
    assert _new(m, ids, 48, **kw).tolist() == free
    e.close()


def test_choices_end_with_eos_then_pad_and_report_dead(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    choices = [[17, 18], [17, 19, 20], [40], [17, 18, 21]]
    f = TokenFSM.from_choices(choices, 7, vocab_size=V_TINY)
    out = m.generate(ids, max_new_tokens=8, eos_token_id=7, pad_token_id=0, token_fsm=f, return_dict_in_generate=True)
    for r in range(2):
        row = out.sequences[r, ids.shape[1]:].tolist()
        k = row.index(7)
        assert row[:k] in choices and all(t == 0 for t in row[k + 1:])
    assert out.fsm_states.tolist() == [DEAD, DEAD]
    # cut by max_new_tokens inside a choice: the state the reference walks to
    long = TokenFSM.from_choices([[17, 18, 19, 20], [40, 41, 42]], 7, vocab_size=V_TINY)
    out = m.generate(ids, max_new_tokens=2, eos_token_id=7, pad_token_id=0, token_fsm=long, return_dict_in_generate=True)
    new = out.sequences[:, ids.shape[1]:].tolist()
    want = [fr.walk(long.transitions(), row) for row in new]
    assert out.fsm_states.tolist() == want and DEAD not in want
    assert all(row in ([17, 18], [40, 41]) for row in new)
    # per-row start states: row 1 begins behind 17
    s17 = f.next(0, 17)
    out = m.generate(ids, max_new_tokens=8, eos_token_id=7, pad_token_id=0, token_fsm=f, fsm_start=[0, s17], return_dict_in_generate=True)
    row = out.sequences[1, ids.shape[1]:].tolist()
    assert [17] + row[:row.index(7)] in choices
    # both KV cache types
    e.enable_fp8_kv(True)
    row = m.generate(ids, max_new_tokens=8, eos_token_id=7, pad_token_id=0, token_fsm=f)[0, ids.shape[1]:].tolist()
    assert row[:row.index(7)] in choices
    e.enable_fp8_kv(False)
    e.close()


def test_eos_rewind_takes_the_trail_back(gpu_lib):
    _, e, m = _tiny_model(b=1)
    ids = torch.tensor(PROMPT[:1])
    trans, f = _cyclic(_new(m, ids, 16).tolist())
    free = _new(m, ids, 16, token_fsm=f)[0].tolist()
    stop = next(i for i in range(3, 14) if free[i] not in free[:i])
    eos = free[stop]
    out = _new(m, ids, 16, eos_token_id=eos, token_fsm=f)[0].tolist()
    assert out == free[:stop + 1]
    # generate enqueued one step ahead of the EOS and took it back: the device is behind out[:-1], a follow-up step feeds the EOS
    assert e.token_fsm_states(1) == [fr.walk(trans, out[:-1])]
    nxt, lg = e.decode_step(torch.tensor([eos]), want_logits=True)
    st = fr.walk(trans, out)
    assert e.token_fsm_states(1) == [st]
    assert int(nxt[0]) == int(np.argmax(fr.apply(trans, lg.cpu().numpy()[0], st))) == free[stop + 1]
    e.kv_rewind(1, 1)
    other = next(t for t in sorted(trans[fr.walk(trans, out[:-1])]) if t != eos)
    nxt2, lg2 = e.decode_step(torch.tensor([other]), want_logits=True)
    st2 = fr.walk(trans, out[:-1] + [other])
    assert st2 != DEAD and e.token_fsm_states(1) == [st2]
    assert int(nxt2[0]) == int(np.argmax(fr.apply(trans, lg2.cpu().numpy()[0], st2)))
    # a token without an edge kills the row: the next pick is the raw argmax
    e.kv_rewind(1, 1)
    none = next(t for t in range(V_TINY) if t not in trans[fr.walk(trans, out[:-1])])
    nxt3, lg3 = e.decode_step(torch.tensor([none]), want_logits=True)
    assert e.token_fsm_states(1) == [DEAD] and int(nxt3[0]) == int(np.argmax(lg3.cpu().numpy()[0]))
    e.close()


def test_composition_with_no_repeat_ngram(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    trans, f = _cyclic(_new(m, ids, 48).tolist())
    p = cr.params(V_TINY, ngram=2)
    alone, _, _, _ = _host_loop(e, m, ids, 48, trans, f)
    both, _, _, _ = _host_loop(e, m, ids, 48, trans, f, p=p)
    both_g, _, _, _ = _host_loop(e, m, ids, 48, trans, f, p=p, graph=True)
    assert np.array_equal(both, both_g)
    out = _new(m, ids, 48, token_fsm=f, no_repeat_ngram_size=2).numpy()
    assert np.array_equal(out, both)
    for r in range(2):
        row = PROMPT[r] + both[r].tolist()
        bg = list(zip(row[:-1], row[1:]))
        assert len(bg) == len(set(bg)) and fr.walk(trans, both[r]) != DEAD
    assert np.array_equal(_new(m, ids, 48, token_fsm=f).numpy(), alone)
    e.close()


def test_batch_forms_stay_inside_the_automaton(gpu_lib):
    _, e, m = _tiny_model(b=8)
    ids = torch.tensor(PROMPT)
    trans, f = _cyclic(_new(m, ids, 24).tolist())
    # a padded batch through the masked path
    pids = torch.tensor([[3, 17, 18, 19, 20, 21, 7, 9], [5, 6, 11, 12, 0, 0, 0, 0]])
    mask = torch.tensor([[1] * 8, [1] * 4 + [0] * 4])
    got = m.generate(pids, attention_mask=mask, max_new_tokens=24, pad_token_id=0, token_fsm=f)[:, 8:]
    assert m._padded_batch
    assert all(fr.walk(trans, row) != DEAD for row in got.tolist())
    assert not torch.equal(got, m.generate(pids, attention_mask=mask, max_new_tokens=24, pad_token_id=0)[:, 8:])
    # sampled groups: the per-prompt start state is repeated for the siblings
    out = m.generate(ids, max_new_tokens=24, do_sample=True, seed=3, num_return_sequences=4, token_fsm=f, fsm_start=[0, 2],
                     return_dict_in_generate=True, **SMP)
    rows = out.sequences[:, ids.shape[1]:].tolist()
    assert len(rows) == 8 and len({tuple(r) for r in rows}) > 2
    ends = [fr.walk(trans, row, start=0 if i < 4 else 2) for i, row in enumerate(rows)]
    assert DEAD not in ends and out.fsm_states.tolist() == ends
    # suffixes of different lengths: a state per row
    sfx = [[5, 6], [7, 8, 9], [11]]
    rows = m.generate(ids[:1], max_new_tokens=24, suffixes=sfx, token_fsm=f, fsm_start=[0, 1, 3]).tolist()
    assert [fr.walk(trans, row, start=s) != DEAD for row, s in zip(rows, (0, 1, 3))] == [True] * 3
    assert rows != m.generate(ids[:1], max_new_tokens=24, suffixes=sfx).tolist()
    e.close()


def test_reuse_cache_second_turn_and_mxfp4_decode(gpu_lib):
    _, e, m = _tiny_model(b=1)
    ids = torch.tensor(PROMPT[:1])
    trans, f = _cyclic(_new(m, ids, 24).tolist())
    first = m.generate(ids, max_new_tokens=12, reuse_cache=True, token_fsm=f)
    assert fr.walk(trans, first[0, ids.shape[1]:].tolist()) != DEAD
    # the second turn begins in its own start state over the kept cache
    turn2 = torch.cat([first, torch.tensor([[44, 45, 46]])], dim=1)
    got = m.generate(turn2, max_new_tokens=12, reuse_cache=True, token_fsm=f, fsm_start=2)[0, turn2.shape[1]:].tolist()
    assert e.extend_stats()["kept_slots"] > 0
    assert fr.walk(trans, got, start=2) != DEAD
    e.enable_mxfp4_decode(True)
    assert fr.walk(trans, _new(m, ids, 24, token_fsm=f)[0].tolist()) != DEAD
    e.enable_mxfp4_decode(False)
    e.close()


def test_logprobs_processed_is_over_the_allowed_set(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    trans, f = _cyclic(_new(m, ids, 24).tolist())
    got, raws, sts, rec = _host_loop(e, m, ids, 24, trans, f, logprobs=True)
    raw_lp, proc_lp, counts = rec
    assert counts == [24, 24]
    for t in range(24):
        for r in range(2):
            z, i = raws[t][r], int(got[r, t])
            masked = fr.apply(trans, z, sts[t][r])
            want_raw, want_proc = lr.raw(z, i), lr.log_softmax_at(masked, i)
            assert abs(float(raw_lp[r, t]) - want_raw) <= lr.tolerance(z[i], lr.lse(z))
            assert abs(float(proc_lp[r, t]) - want_proc) <= lr.tolerance(z[i], lr.lse(masked[np.isfinite(masked)]))
            assert want_proc > want_raw
    out = m.generate(ids, max_new_tokens=24, token_fsm=f, output_logprobs=True, return_dict_in_generate=True)
    assert np.array_equal(out.sequences[:, ids.shape[1]:].numpy(), got)
    assert torch.equal(out.logprobs, raw_lp) and torch.equal(out.processed_logprobs, proc_lp)
    e.close()


def test_table_reuse_device_bytes_and_bounds(gpu_lib):
    _, e, m = _tiny_model(b=1)
    ids = torch.tensor(PROMPT[:1])
    free = _new(m, ids, 24)
    trans, f = _cyclic(free.tolist())
    eager = _new(m, ids, 24, token_fsm=f)
    e.enable_decode_graph(True)
    one = _new(m, ids, 24, token_fsm=f)
    st1 = e.decode_graph_stats()
    assert st1["captures"] > 0 and st1["replays"] > 0
    two = _new(m, ids, 24, token_fsm=f)
    st2 = e.decode_graph_stats()
    assert st2["captures"] == st1["captures"] and st2["replays"] > st1["replays"]      # the same table: replayed, not recaptured
    assert torch.equal(one, eager) and torch.equal(two, eager)
    other = TokenFSM({s: {t: n for t, n in ed.items() if t != int(eager[0, 0])} for s, ed in trans.items()}, vocab_size=V_TINY)
    three = _new(m, ids, 24, token_fsm=other)
    assert e.decode_graph_stats()["captures"] > st2["captures"]                         # another table recaptures
    assert int(three[0, 0]) != int(eager[0, 0])
    e.enable_decode_graph(False)
    assert torch.equal(three, _new(m, ids, 24, token_fsm=other))
    assert torch.equal(_new(m, ids, 24), free)                                          # off again without the keyword
    e.close()
    # device bytes: the table, then the trail, grown on demand and never shrunk; a step beyond max_new is refused before it is enqueued
    _, e, m = _tiny_model(b=1)
    out = m.forward(input_ids=ids, use_cache=True)
    before = e.device_bytes()
    e.load_token_fsm(f)
    loaded = e.device_bytes()
    edges = sum(len(v) for v in trans.values())
    assert loaded - before >= (K_CYCLE + 1 + 2 * edges) * 4
    e.load_token_fsm(f)
    assert e.device_bytes() == loaded
    e.token_fsm_begin(1, 0, 4)
    begun = e.device_bytes()
    assert begun - loaded >= 5 * 4
    e.token_fsm_begin(1, 0, 4)
    assert e.device_bytes() == begun
    e.token_fsm_begin(1, 0, 64)
    grown = e.device_bytes()
    assert grown - begun >= 60 * 4
    e.token_fsm_begin(1, 0, 4)
    assert e.device_bytes() == grown
    tok = e.argmax(out.local_logits)
    for _ in range(4):
        tok, _ = e.decode_step(tok)
    lens = e.kv_lengths(1)
    with pytest.raises(ValueError, match="max_new"):
        e.decode_step(tok)
    assert e.kv_lengths(1) == lens                                                       # nothing was enqueued
    e.kv_rewind(1, 1)
    tok, _ = e.decode_step(tok)                                                          # the rewind gave the step's room back
    with pytest.raises(ValueError):
        e.token_fsm_begin(1, K_CYCLE, 4)                                                 # start state out of range
    e.close()


# ---------------------------------------------------------------------------------------------------------------- tensor parallelism
class _Group:
    """all-reduce hook over rank contexts living on one GPU (tests/test_gpu_constraints.py's pattern)"""

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


TP_SEED = 424242


def _fsm_steps(engines, logits_steps, prompt, trans, f, starts, smp):
    n = len(engines)
    out, err = [None] * n, [None] * n

    def work(r):
        try:
            e = engines[r]
            b = logits_steps[0].shape[0]
            e.load_token_fsm(f)
            if smp is not None:
                e.set_sampling(b, seed=TP_SEED, seen=[[i for i in row if i >= 0] for row in prompt], **smp)
            Vl = logits_steps[0].shape[1] // n
            states = list(starts)
            ids = []
            for lg in logits_steps:
                # no decoder weights here: the state a decode step would have walked to is handed over with each begin, as
                # tests/test_gpu_constraints.py hands the history over.  So this test checks the shard offset of the mark pass and the
                # picks over shards that are entirely -inf; the advance itself is rank-local and covered at TP = 1
                e.token_fsm_begin(b, states, 2)
                shard = lg[:, r * Vl:(r + 1) * Vl].contiguous()
                pick = (e.sample(shard) if smp is not None else e.argmax(shard)).cpu().numpy()
                ids.append(pick)
                states = [fr.step(trans, s, int(t)) for s, t in zip(states, pick)]
            out[r] = np.stack(ids, 1)
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
@pytest.mark.parametrize("smp", [None, dict(temperature=0.9, top_k=200, top_p=0.95, repetition_penalty=1.3)], ids=["greedy", "sampled"])
def test_tp_ids_equal_tp1(gpu_lib, tp, smp):
    cfg = tiny()
    V, b, steps = cfg.text["vocab_size"], 3, 8
    rng = np.random.default_rng(tp)
    logits_steps = [torch.from_numpy((rng.standard_normal((b, V)) * 2).astype(np.float32)).cuda() for _ in range(steps)]
    prompt = [rng.integers(0, V, 12).tolist() + [-200] for _ in range(b)]
    q = V // 4
    # state 1: ids of the first quarter only, state 2: of the last quarter only -- one shard at TP = 2 and at TP = 4 holds every
    # allowed id, the others are -inf throughout; states 0 and 3 spread over all shards
    sets = [[t for t in range(V) if t % 3 == 0], list(range(5, q - 3)), list(range(3 * q + 2, V)), [t for t in range(V) if t % 5 != 1]]
    trans = {s: {t: (s + 1) % 4 for t in ids} for s, ids in enumerate(sets)}
    f = TokenFSM(trans, vocab_size=V)
    starts = [0, 1, 2]
    one = Engine(cfg, dtype="bf16", max_seq=16, max_batch=b, max_tiles=1, vision=False)
    ref = _fsm_steps([one], logits_steps, prompt, trans, f, starts, smp)[0]
    grp = _Group(tp)
    engines, hooks = [], []
    for r in range(tp):
        e = Engine(cfg, dtype="bf16", max_seq=16, max_batch=b, max_tiles=1, vision=False, tp_rank=r, tp_size=tp, comm=C.c_void_p(1))
        h = grp.hook_for(r)
        check(gpu_lib.omchat_set_allreduce_hook(e.h, C.cast(h, C.c_void_p), None))
        engines.append(e); hooks.append(h)
    got = _fsm_steps(engines, logits_steps, prompt, trans, f, starts, smp)
    for r in range(tp):
        assert np.array_equal(got[r], ref), (r, got[r], ref)
    # and the CPU restatement over the whole vocabulary
    states, seen = list(starts), [[t for t in row if t >= 0] for row in prompt]
    for k, lg in enumerate(logits_steps):
        want = []
        for i in range(b):
            l = fr.apply(trans, lg[i].cpu().numpy(), states[i])
            want.append(int(np.argmax(l)) if smp is None else
                        sr.sample_row(l, i, k, TP_SEED, smp["temperature"], smp["top_k"], smp["top_p"], seen[i], smp["repetition_penalty"]))
        assert ref[:, k].tolist() == want, (k, ref[:, k], want)
        for i in range(b):
            seen[i].append(want[i])
            states[i] = fr.step(trans, states[i], want[i])
    for e in engines + [one]:
        e.close()
