"""GPU: the on-device HF logits constraints (omchat_amd/csrc/constrain.hip) -- the ban pass against
tests/constraints_ref.py set for set, decode steps and generate() on a tiny synthetic model against a host-driven loop that applies the
reference ban to the step's raw logits (eager, decode graph, padded batch, sampling, EOS rewind, reuse_cache), the same ids at TP = 2 / 4
as at TP = 1, and one case at full depth.  Every comparison is exact."""
import ctypes as C
import threading
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import constraints_ref as cr
import sampling_ref as sr
import fulldepth_sample as fs
from omchat_amd import synth, _lib
from omchat_amd._lib import check, ptr
from omchat_amd.config import tiny, omchat13b
from omchat_amd.engine import Engine


def _i32(xs):
    return torch.tensor([int(x) for x in xs] or [0], dtype=torch.int32)


def _op_constrain(lib, hist, plen, V, V_total, rank, p, fed):
    b = len(hist)
    bmw = (V + 31) // 32
    out = torch.full((b, bmw), -1, dtype=torch.int32, device="cuda")
    words = p["bad_words"]
    off = [0]
    for w in words:
        off.append(off[-1] + len(w))
    t = [_i32([i for r in hist for i in r]), _i32([len(r) for r in hist]), _i32(plen), _i32(p["eos"]), _i32(p["suppress"]),
         _i32(p["begin_suppress"]), _i32([i for w in words for i in w]), _i32(off)]
    check(lib.omchat_op_constrain(ptr(t[0]), ptr(t[1]), ptr(t[2]), b, V, V_total, rank, int(fed), p["ngram"], p["min_new"], p["min_len"],
                                  ptr(t[3]), len(p["eos"]), ptr(t[4]), len(p["suppress"]), ptr(t[5]), len(p["begin_suppress"]), ptr(t[6]),
                                  ptr(t[7]), len(words), ptr(out), _lib.cur_stream()))
    torch.cuda.synchronize()
    bits = np.unpackbits(out.cpu().numpy().view(np.uint8), axis=1, bitorder="little")[:, :V]
    return [sorted((np.flatnonzero(bits[r]) + rank * V).tolist()) for r in range(b)]


def _histories(rng, b, L, V):
    """looping rows (ids from a small span, so n-grams repeat) with a sentinel and a few far ids"""
    rows = []
    for r in range(b):
        lo = int(rng.integers(0, V - 8))
        h = (lo + rng.integers(0, 7, L)).tolist()
        if L > 4:
            h[int(rng.integers(0, L - 2))] = -200
            h[int(rng.integers(0, L - 2))] = int(rng.integers(0, V))
        rows.append(h)
    return rows


@pytest.mark.parametrize("tp", [1, 2, 4])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 4096, 33000])
@pytest.mark.parametrize("b", [1, 5, 32])
def test_op_constrain_equals_ref(gpu_lib, b, L, tp):
    V_total = 152064
    V = V_total // tp
    rng = np.random.default_rng(b * 131 + L + tp)
    hist = _histories(rng, b, L, V_total)
    step = min(L - 1, 3)
    plen = [L - step] * b
    tail = hist[0][-3:]
    words = [[int(x)] for x in rng.integers(0, V_total, 8)] + [[V_total - 1]] + [tail[-2:] + [77], tail + [V // 2 + 5]] + ([hist[0] + [7], [1] + hist[0] + [9]] if L <= 65 else [])
    words += [rng.integers(0, V_total, int(rng.integers(2, 5))).tolist() for _ in range(52)]
    eos = [V_total - 1, 11]
    sup = rng.integers(0, V_total, 40).tolist() + [0, V - 1, V, V_total - 1]
    cases = [cr.params(V_total, ngram=1), cr.params(V_total, ngram=2), cr.params(V_total, ngram=3), cr.params(V_total, ngram=5),
             cr.params(V_total, bad_words=words, eos=eos), cr.params(V_total, min_new=step + 1, eos=eos), cr.params(V_total, min_new=step, eos=eos),
             cr.params(V_total, min_len=L + 1, eos=eos), cr.params(V_total, suppress=sup), cr.params(V_total, begin_suppress=sup[:5]),
             cr.params(V_total, ngram=3, bad_words=words, eos=eos, min_new=step + 1, min_len=3, suppress=sup, begin_suppress=[4, 5])]
    for p in cases:
        want = [cr.banned_ids(h, p, step) for h in hist]
        for rank in sorted({0, tp - 1}):
            mine = [[i for i in w if rank * V <= i < (rank + 1) * V] for w in want]
            for fed in ((False, True) if L > 1 else (False,)):
                got = _op_constrain(gpu_lib, hist, plen, V, V_total, rank, p, fed)
                assert got == mine, (p["ngram"], rank, fed, [len(g) for g in got][:4], [len(m) for m in mine][:4])
    # the first generated position: begin_suppress applies there only
    p = cr.params(V_total, begin_suppress=[4, 5])
    assert _op_constrain(gpu_lib, hist, [L] * b, V, V_total, 0, p, False) == [[4, 5]] * b


def test_op_constrain_small_vocab_and_caps(gpu_lib):
    p = cr.params(37, ngram=2, suppress=[36, 37, -200], bad_words=[[3]])
    hist = [[5, 6, 5], [1, 2, 3]]
    assert _op_constrain(gpu_lib, hist, [3, 3], 37, 37, 0, p, False) == [cr.banned_ids(h, p, 0) for h in hist] == [[3, 6, 36], [3, 36]]
    with pytest.raises(ValueError):
        _op_constrain(gpu_lib, hist, [3, 3], 37, 37, 0, cr.params(37, ngram=65), False)
    with pytest.raises(ValueError):
        _op_constrain(gpu_lib, hist, [3, 3], 37, 37, 0, cr.params(37, suppress=list(range(1025))), False)
    with pytest.raises(ValueError):
        _op_constrain(gpu_lib, hist, [3, 3], 37, 37, 0, cr.params(37, bad_words=[[1]] * 1025), False)


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


def _engine_kw(p):
    return dict(no_repeat_ngram_size=p["ngram"], bad_words_ids=p["bad_words"], min_new_tokens=p["min_new"], min_length=p["min_len"], eos=p["eos"],
                suppress_tokens=p["suppress"], begin_suppress_tokens=p["begin_suppress"])


def _ref_pick(lg, hist, p, step, smp=None, seed=0):
    out = []
    for r in range(lg.shape[0]):
        l = cr.apply(lg[r], cr.banned_ids(hist[r], p, step))
        if smp is None:
            out.append(int(np.argmax(l)))
        else:
            out.append(sr.sample_row(l, r, step, seed, smp["temperature"], smp["top_k"], smp["top_p"], [i for i in hist[r] if i >= 0],
                                     smp["repetition_penalty"]))
    return out


def _host_loop(e, m, ids, n, p, graph=False, smp=None, seed=5, prefill=None):
    """the device's constrained picks, each checked against the reference ban applied on the host to the step's RAW logits"""
    e.enable_decode_graph(graph)
    out = prefill(ids) if prefill is not None else m.forward(input_ids=ids, use_cache=True)
    b = ids.shape[0]
    hist = [list(r) for r in ids.tolist()]
    e.set_constraints(b, hist, n, **_engine_kw(p))
    if smp is not None:
        e.set_sampling(b, seed=seed, seen=[[i for i in r if i >= 0] for r in hist], **smp)
    else:
        e.sampling_off()
    lg = out.local_logits
    tok = e.sample(lg) if smp is not None else e.argmax(lg)
    got = []
    for step in range(n):
        raw = lg.cpu().numpy()
        assert np.isfinite(raw).all()                              # the logits handed back stay the raw ones
        ref = _ref_pick(raw, hist, p, step, smp, seed)
        assert tok.tolist() == ref, (step, tok.tolist(), ref)
        got.append(ref)
        for r in range(b):
            hist[r].append(ref[r])
        if step < n - 1:
            tok, lg = e.decode_step(tok, want_logits=True)
    e.enable_decode_graph(False)
    e.constraints_off(); e.sampling_off()
    return np.array(got).T


def _free(m, ids, n, **kw):
    return m.generate(ids, max_new_tokens=n, **kw)[:, ids.shape[1]:]


def _bigrams_repeat(row):
    bg = list(zip(row[:-1], row[1:]))
    return len(bg) != len(set(bg))


CASES = {
    "ngram2": lambda free: cr.params(V_TINY, ngram=2),
    "ngram1": lambda free: cr.params(V_TINY, ngram=1),
    "ngram4": lambda free: cr.params(V_TINY, ngram=4),
    "bad_words": lambda free: cr.params(V_TINY, bad_words=[[free[0][2]], free[0][3:5], free[1][1:4], [free[1][0]]]),
    "min_new": lambda free: cr.params(V_TINY, min_new=20, eos=sorted({free[0][0], free[1][0], free[0][5]})),
    "min_len": lambda free: cr.params(V_TINY, min_len=len(PROMPT[0]) + 9, eos=[free[0][0], free[1][0]]),
    "suppress": lambda free: cr.params(V_TINY, suppress=sorted(set(free[0][:6] + free[1][:6]))),
    "begin_suppress": lambda free: cr.params(V_TINY, begin_suppress=[free[0][0], free[1][0], free[0][1]]),
    "all": lambda free: cr.params(V_TINY, ngram=3, bad_words=[[free[0][2]], free[1][1:3]], min_new=12, eos=[free[0][0], free[1][3]],
                                  suppress=[free[0][1]], begin_suppress=[free[1][0]]),
}


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_decode_steps_pick_what_the_ref_picks(gpu_lib, case, graph):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    free = _free(m, ids, 48).tolist()
    p = CASES[case](free)
    got = _host_loop(e, m, ids, 48, p, graph=graph)
    if graph:
        assert e.decode_graph_stats()["replays"] > 0
    if not case.startswith("ngram"):
        assert got.tolist() != free                               # the constraint bit
    # generate drives the same seam (its EOS handling aside: no eos_token_id is passed here, the constraint's eos list only bans)
    if not p["eos"]:
        out = m.generate(ids, max_new_tokens=48, **{k: v for k, v in _engine_kw(p).items() if k != "eos" and v})
        assert np.array_equal(out[:, ids.shape[1]:].numpy(), got)
    e.close()


def test_sampling_with_top_k_top_p_penalty_and_constraints(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    p = cr.params(V_TINY, ngram=2, suppress=[7, 9, 17], bad_words=[[18, 19], [40]], begin_suppress=[3])
    eager = _host_loop(e, m, ids, 48, p, smp=SMP, seed=77)
    assert np.array_equal(_host_loop(e, m, ids, 48, p, graph=True, smp=SMP, seed=77), eager)
    out = m.generate(ids, do_sample=True, seed=77, max_new_tokens=48, no_repeat_ngram_size=2, suppress_tokens=[7, 9, 17],
                     bad_words_ids=[[18, 19], [40]], begin_suppress_tokens=[3], **SMP)
    assert np.array_equal(out[:, ids.shape[1]:].numpy(), eager)
    assert not np.array_equal(m.generate(ids, do_sample=True, seed=77, max_new_tokens=48, **SMP)[:, ids.shape[1]:].numpy(), eager)
    e.close()


def test_generate_end_to_end(gpu_lib):
    ids = torch.tensor(PROMPT[:1])
    found = None
    for seed in range(21, 29):                                    # a synthetic model whose greedy output loops
        _, e, m = _tiny_model(b=1, seed=seed)
        free = _free(m, ids, 32)[0].tolist()
        if _bigrams_repeat(free):
            found = seed
            break
        e.close()
    assert found is not None, "no synthetic seed whose unconstrained greedy output repeats a bigram"
    parent = m.generate(ids, max_new_tokens=32)
    # no_repeat_ngram_size = 2: no bigram of prompt + output repeats, and the ids are the host-driven loop's
    out = m.generate(ids, max_new_tokens=32, no_repeat_ngram_size=2)
    assert not _bigrams_repeat(out[0].tolist())
    assert np.array_equal(out[:, ids.shape[1]:].numpy(), _host_loop(e, m, ids, 32, cr.params(V_TINY, ngram=2)))
    # min_new_tokens against an EOS that is the unconstrained first pick
    assert m.generate(ids, max_new_tokens=32, eos_token_id=free[0]).shape[1] == ids.shape[1] + 1
    out = m.generate(ids, max_new_tokens=32, eos_token_id=free[0], min_new_tokens=8)
    new = out[0, ids.shape[1]:].tolist()
    assert len(new) >= 8 and free[0] not in new[:8]
    out = m.generate(ids, max_new_tokens=32, eos_token_id=free[0], min_length=ids.shape[1] + 5)
    assert out.shape[1] >= ids.shape[1] + 5
    # a bad word taken from the unconstrained output never appears
    word = free[3:5]
    new = m.generate(ids, max_new_tokens=32, bad_words_ids=[word])[0].tolist()
    assert not any(new[i:i + 2] == word for i in range(len(new) - 1))
    one = m.generate(ids, max_new_tokens=32, bad_words_ids=[[free[0]]])[0, ids.shape[1]:].tolist()
    assert free[0] not in one
    # begin_suppress_tokens changes the first pick, and nothing when it names another id
    assert m.generate(ids, max_new_tokens=8, begin_suppress_tokens=[free[0]])[0, ids.shape[1]] != free[0]
    other = next(t for t in range(V_TINY) if t not in free)
    assert torch.equal(m.generate(ids, max_new_tokens=32, begin_suppress_tokens=[other]), parent)
    assert torch.equal(m.generate(ids, max_new_tokens=32, suppress_tokens=[other]), parent)
    # constraints are sticky context state: a call without the arguments returns the parent's ids
    assert torch.equal(m.generate(ids, max_new_tokens=32), parent)
    # both KV cache types
    e.enable_fp8_kv(True)
    out8 = m.generate(ids, max_new_tokens=24, no_repeat_ngram_size=2)
    assert not _bigrams_repeat(out8[0].tolist())
    e.enable_fp8_kv(False)
    with pytest.raises(NotImplementedError):
        m.generate(ids, max_new_tokens=4, num_beams=2, no_repeat_ngram_size=2)
    with pytest.raises(NotImplementedError):
        m.generate(ids, max_new_tokens=4, prompt_lookup_num_tokens=3, no_repeat_ngram_size=2)
    with pytest.raises(NotImplementedError):
        m.generate(ids, max_new_tokens=4, forced_eos_token_id=3)
    assert torch.equal(m.generate(ids, max_new_tokens=32), parent)
    e.close()


def test_equal_parameters_keep_the_decode_graphs_between_generate_calls(gpu_lib):
    _, e, m = _tiny_model(b=1)
    ids = torch.tensor(PROMPT[:1])
    eager = m.generate(ids, max_new_tokens=24, no_repeat_ngram_size=2)
    e.enable_decode_graph(True)
    one = m.generate(ids, max_new_tokens=24, no_repeat_ngram_size=2)
    st1 = e.decode_graph_stats()
    assert st1["captures"] > 0 and st1["replays"] > 0
    two = m.generate(ids, max_new_tokens=24, no_repeat_ngram_size=2)
    st2 = e.decode_graph_stats()
    assert st2["captures"] == st1["captures"] and st2["replays"] > st1["replays"]      # same parameters: replayed, not recaptured
    assert torch.equal(one, eager) and torch.equal(two, eager)                          # the re-seeded history is what the replays read
    three = m.generate(ids, max_new_tokens=24, no_repeat_ngram_size=3)
    assert e.decode_graph_stats()["captures"] > st2["captures"]                         # a parameter change drops the graphs
    e.enable_decode_graph(False)
    assert torch.equal(three, m.generate(ids, max_new_tokens=24, no_repeat_ngram_size=3))
    e.close()


def test_device_bytes_count_the_history_and_steps_beyond_max_new_are_refused(gpu_lib):
    _, e, m = _tiny_model(b=1)
    ids = torch.tensor(PROMPT[:1])
    out = m.forward(input_ids=ids, use_cache=True)
    before = e.device_bytes()
    e.set_constraints(1, ids.tolist(), 4, no_repeat_ngram_size=2)
    mid = e.device_bytes()
    assert mid > before
    e.set_constraints(1, ids.tolist(), 4, no_repeat_ngram_size=2)
    assert e.device_bytes() == mid                                # kept, not re-allocated
    e.set_constraints(1, ids.tolist(), 64, no_repeat_ngram_size=2)
    assert e.device_bytes() > mid                                 # grown on demand
    e.set_constraints(1, ids.tolist(), 2, no_repeat_ngram_size=2)
    tok = e.argmax(out.local_logits)
    for _ in range(64):                                           # never shrunk: 64 steps still fit
        tok, _ = e.decode_step(tok)
    with pytest.raises(ValueError):
        for _ in range(8):
            tok, _ = e.decode_step(tok)
    e.close()


def test_padded_batch_through_the_masked_path(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor([[3, 17, 18, 19, 20, 21, 7, 9], [5, 6, 11, 12, 0, 0, 0, 0]])
    mask = torch.tensor([[1] * 8, [1] * 4 + [0] * 4])
    n = 24
    p = cr.params(V_TINY, ngram=2, suppress=[17])
    got = m.generate(ids, attention_mask=mask, max_new_tokens=n, pad_token_id=0, no_repeat_ngram_size=2, suppress_tokens=[17])
    assert m._padded_batch
    e.constraints_off()
    # the loop HF drives, on the host: forward() per step, the reference ban on its raw logits, argmax.  The pad ids of row 1 are part of
    # the history HF's processors see.
    out = m.forward(input_ids=ids, attention_mask=mask, use_cache=True)
    hist = [list(r) for r in ids.tolist()]
    lg, cur = out.logits[:, 0].cpu().numpy(), mask
    for step in range(n):
        pick = _ref_pick(lg, hist, p, step)
        for r in range(2):
            hist[r].append(pick[r])
        if step == n - 1:
            break
        cur = torch.cat([cur, torch.ones(2, 1, dtype=cur.dtype)], dim=1)
        out = m.forward(input_ids=torch.tensor(pick)[:, None], attention_mask=cur, past_key_values=out.past_key_values)
        lg = out.logits[:, 0].cpu().numpy()
    assert got.tolist() == hist
    assert not torch.equal(got, m.generate(ids, attention_mask=mask, max_new_tokens=n, pad_token_id=0))
    e.close()


def test_eos_rewind_restores_the_history(gpu_lib):
    _, e, m = _tiny_model(b=1)
    ids = torch.tensor(PROMPT[:1])
    p = cr.params(V_TINY, ngram=2)
    free = m.generate(ids, max_new_tokens=16, no_repeat_ngram_size=2)[0, ids.shape[1]:].tolist()
    stop = next(i for i in range(3, 14) if free[i] not in free[:i])
    eos = free[stop]
    out = m.generate(ids, max_new_tokens=16, eos_token_id=eos, no_repeat_ngram_size=2)[0, ids.shape[1]:].tolist()
    assert out == free[:stop + 1]
    # generate enqueued one step ahead of the EOS and took it back: a follow-up step sees prompt + out, as a fresh run does
    nxt, lg = e.decode_step(torch.tensor([eos]), want_logits=True)
    hist = [PROMPT[0] + out]
    assert int(nxt[0]) == _ref_pick(lg.cpu().numpy(), hist, p, stop + 1)[0] == free[stop + 1]
    e.kv_rewind(1, 1)
    other = next(t for t in PROMPT[0] if t != eos)
    nxt2, lg2 = e.decode_step(torch.tensor([other]), want_logits=True)
    assert int(nxt2[0]) == _ref_pick(lg2.cpu().numpy(), [PROMPT[0] + out[:-1] + [other]], p, stop + 1)[0]
    e.close()


def test_reuse_cache_second_turn(gpu_lib):
    # two contexts with the same weights run the same first turn, so their caches hold the same bits; on the second turn one goes through
    # generate(), the other through the host-driven loop over the same kept-cache prefill, every pick checked against the reference ban
    # over the WHOLE second-turn prompt (the kept prefix included, not the prefilled suffix alone)
    ids = torch.tensor(PROMPT[:1])
    p = cr.params(V_TINY, ngram=2)
    _, e, m = _tiny_model(b=1)
    first = m.generate(ids, max_new_tokens=12, reuse_cache=True, no_repeat_ngram_size=2)
    # the suffix ends on an id of the first turn: the bigrams that ban the second turn's first picks lie in the kept prefix
    turn2 = torch.cat([first, torch.tensor([[44, 45, int(first[0, 9])]])], dim=1)
    got = m.generate(turn2, max_new_tokens=24, reuse_cache=True, no_repeat_ngram_size=2)
    assert e.extend_stats()["kept_slots"] > 0
    assert not _bigrams_repeat(got[0].tolist())
    e.close()
    _, e2, m2 = _tiny_model(b=1)
    assert torch.equal(m2.generate(ids, max_new_tokens=12, reuse_cache=True, no_repeat_ngram_size=2), first)
    loop = _host_loop(e2, m2, turn2, 24, p, prefill=lambda t: m2._forward_reuse(t, None)[0])
    assert e2.extend_stats()["kept_slots"] > 0
    assert np.array_equal(got[:, turn2.shape[1]:].numpy(), loop)
    e2.close()


# ---------------------------------------------------------------------------------------------------------------- tensor parallelism
class _Group:
    """all-reduce hook over rank contexts living on one GPU (tests/test_gpu_sampling.py's pattern)"""

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


def _constrained_steps(engines, logits_steps, prompt, p, smp):
    n = len(engines)
    out, err = [None] * n, [None] * n

    def work(r):
        try:
            e = engines[r]
            b = logits_steps[0].shape[0]
            if smp is not None:
                e.set_sampling(b, seed=424242, seen=[[i for i in row if i >= 0] for row in prompt], **smp)
            Vl = logits_steps[0].shape[1] // n
            hist = [list(row) for row in prompt]
            ids = []
            for lg in logits_steps:
                # no decoder weights here: the history a decode step would have grown is handed over with each begin, as a prompt with 0
                # generated ids.  So this test checks the ban pass's shard offset under TP alone; the on-device append, the step counting
                # (min_new_tokens expiring, begin_suppress_tokens switching off after the first position) and kv_rewind -- all rank-local
                # and the same code at every TP degree -- are covered at TP = 1 only (the decode-step tests above)
                e.set_constraints(b, hist, 2, **_engine_kw(p))
                shard = lg[:, r * Vl:(r + 1) * Vl].contiguous()
                pick = (e.sample(shard) if smp is not None else e.argmax(shard)).cpu().numpy()
                ids.append(pick)
                for i in range(b):
                    hist[i].append(int(pick[i]))
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
    # a few ids far above the rest, spread over the shards: greedy without the ban would repeat them
    base = (rng.standard_normal((b, V)) * 0.5).astype(np.float32)
    hot = [5, V // 2 + 3, V - 2, V // 4 + 1]
    base[:, hot] += np.array([9.0, 8.0, 7.0, 6.0], dtype=np.float32)
    logits_steps = [torch.from_numpy(base + (rng.standard_normal((b, V)) * 0.1).astype(np.float32)).cuda() for _ in range(steps)]
    prompt = [rng.integers(0, V, 12).tolist() + [-200, hot[0]] for _ in range(b)]
    p = cr.params(V, ngram=1, suppress=[hot[1]], bad_words=[[hot[0], hot[2]]], begin_suppress=[hot[3]], min_new=3, eos=[V - 1, 0])
    one = Engine(cfg, dtype="bf16", max_seq=16, max_batch=b, max_tiles=1, vision=False)
    ref = _constrained_steps([one], logits_steps, prompt, p, smp)[0]
    grp = _Group(tp)
    engines, hooks = [], []
    for r in range(tp):
        e = Engine(cfg, dtype="bf16", max_seq=16, max_batch=b, max_tiles=1, vision=False, tp_rank=r, tp_size=tp, comm=C.c_void_p(1))
        h = grp.hook_for(r)
        check(gpu_lib.omchat_set_allreduce_hook(e.h, C.cast(h, C.c_void_p), None))
        engines.append(e); hooks.append(h)
    got = _constrained_steps(engines, logits_steps, prompt, p, smp)
    for r in range(tp):
        assert np.array_equal(got[r], ref), (r, got[r], ref)
    # and the CPU restatement over the whole vocabulary (every begin above hands the grown history over as a prompt: 0 generated ids
    # for the ban; the sampler's own step counter runs on)
    hist = [list(row) for row in prompt]
    for k, lg in enumerate(logits_steps):
        want = []
        for i in range(b):
            l = cr.apply(lg[i].cpu().numpy(), cr.banned_ids(hist[i], p, 0))
            want.append(int(np.argmax(l)) if smp is None else
                        sr.sample_row(l, i, k, 424242, smp["temperature"], smp["top_k"], smp["top_p"], [t for t in hist[i] if t >= 0],
                                      smp["repetition_penalty"]))
        assert ref[:, k].tolist() == want, (k, ref[:, k], want)
        for i in range(b):
            hist[i].append(want[i])
    for e in engines + [one]:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- full depth
def test_full_depth_no_repeat_ngram_3(gpu_lib):
    cfg = omchat13b()
    S = fs.N_TILES * 1024 + fs.N_TEXT
    n = 16
    e = Engine(cfg, dtype="bf16", max_seq=S + n + 8, max_batch=1, max_tiles=fs.N_TILES, max_prefill_rows=S + 8)
    e.fill_synthetic(0)
    px, ids = fs.sample()
    embeds, lengths, _ = e.splice(ids, None, e.encode_images(px))
    logits, _ = e.prefill(embeds, [S])
    hist = [ids[0].tolist()]                                       # the prompt row as passed: 512 text ids and the three sentinels
    p = cr.params(cfg.text["vocab_size"], ngram=3)
    e.set_constraints(1, hist, n, **_engine_kw(p))
    lg = logits
    tok = e.argmax(lg)
    for step in range(n):
        ref = _ref_pick(lg.cpu().numpy(), hist, p, step)
        assert tok.tolist() == ref, (step, tok.tolist(), ref)
        hist[0].append(ref[0])
        if step < n - 1:
            tok, lg = e.decode_step(tok, want_logits=True)
    e.close()
    del e
    torch.cuda.empty_cache()
