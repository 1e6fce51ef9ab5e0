"""GPU: per-token log-probabilities of the picked ids (omchat_amd/csrc/logprob.hip) -- the op against the fp64
restatement tests/logprob_ref.py on the very same fp32 logits, the records of decode steps (eager and decode graph, bit-identical) and of
generate(output_logprobs=True) on a tiny synthetic model, and TP = 2 / 4 against TP = 1 (rank contexts on one GPU behind a test hook).
Tolerance everywhere: logprob_ref.tolerance = 1e-5 * max(1, |x_id|, |lse|).  Every comparison prints `LPERR name err tol`."""
import ctypes as C
import threading
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import constraints_ref as cr
import logprob_ref as lr
import sampling_ref as sr
from omchat_amd import synth, _lib
from omchat_amd._lib import check, ptr
from omchat_amd.config import tiny
from omchat_amd.engine import Engine


def _i32(xs):
    return torch.tensor([int(x) for x in xs] or [0], dtype=torch.int32)


def _op(lib, dev, V, ids, ban=None, T=1.0, pen=1.0, seen=None, newly=None, thr=None):
    """dev: device fp32 [b, ld] -> (raw [b], processed [b]) fp32 numpy"""
    b, ld = dev.shape
    raw = torch.full((b,), 7.0, device="cuda")
    proc = torch.full((b,), 7.0, device="cuda")
    d_ban = d_thr = None
    if ban is not None:
        bmw = (V + 31) // 32
        bits = np.zeros((b, bmw * 32), dtype=np.uint8)
        for r in range(b):
            bits[r, list(ban[r])] = 1
        d_ban = torch.from_numpy(np.packbits(bits, axis=1, bitorder="little").view(np.int32).copy()).cuda()
    if thr is not None:
        d_thr = torch.from_numpy(np.asarray(thr, dtype=np.uint32).view(np.int32).copy()).cuda()
    seen = seen if seen is not None else [[] for _ in range(b)]
    t_ids, t_seen, t_n = _i32(ids), _i32([i for r in seen for i in r]), _i32([len(r) for r in seen])      # host arrays alive over the call
    t_new = _i32(newly) if newly is not None else None
    check(lib.omchat_op_token_logprob(ptr(dev), b, V, ld, ptr(t_ids), ptr(d_ban), T, pen, ptr(t_seen), ptr(t_n), ptr(t_new), ptr(d_thr),
                                      ptr(raw), ptr(proc), _lib.cur_stream()))
    torch.cuda.synchronize()
    return raw.cpu().numpy(), proc.cpu().numpy()


def _close(name, got, x_id, z):
    """got (fp32) against log_softmax(z)[id] = x_id - lse(z) in fp64, z the fp32 row the device saw"""
    assert not np.isnan(got), name
    if x_id == -np.inf:
        assert got == -np.inf, (name, got)
        return
    l = lr.lse(z)
    err, tol = abs(float(got) - (float(x_id) - l)), lr.tolerance(x_id, l)
    print(f"LPERR {name} {err:.3e} {tol:.3e}")
    assert err <= tol, (name, got, float(x_id) - l, err, tol)


def _ids_mixed(rng, logits):
    """even rows pick their argmax, odd rows a random id"""
    b, V = logits.shape
    return [int(np.argmax(logits[r])) if r % 2 == 0 else int(rng.integers(0, V)) for r in range(b)]


OP_CASES = ["raw", "ban", "one_left", "T0.7", "top_k5", "top_p0.9", "pen_new", "pen_old", "spike", "inf_slice", "cut"]


@pytest.mark.parametrize("V", [152064, 1000, 37])
@pytest.mark.parametrize("b", [1, 5, 32])
@pytest.mark.parametrize("case", OP_CASES)
def test_op_token_logprob_equals_ref(gpu_lib, b, V, case):
    rng = np.random.default_rng(b * 13 + V + len(case))
    logits = (rng.standard_normal((b, V)) * 3).astype(np.float32)
    ids = _ids_mixed(rng, logits)
    kw, ref_kw = {}, [dict() for _ in range(b)]
    if case == "ban":
        ban = [sorted(set(rng.integers(0, V, 50).tolist()) - ({ids[r]} if r else set()) | ({ids[0]} if r == 0 else set())) for r in range(b)]
        kw["ban"] = ban                                                # row 0's own id is banned: -inf
        ref_kw = [dict(banned=ban[r]) for r in range(b)]
    elif case == "one_left":
        kw["ban"] = [[i for i in range(V) if i != ids[r]] for r in range(b)]
        ref_kw = [dict(banned=kw["ban"][r]) for r in range(b)]
    elif case == "T0.7":
        kw["T"] = 0.7
        ref_kw = [dict(temperature=0.7) for _ in range(b)]
    elif case in ("top_k5", "top_p0.9", "cut"):
        k, p = (5, 1.0) if case != "top_p0.9" else (0, 0.9)
        T = 0.8 if case == "cut" else 1.0
        thr = [sr.threshold(sr.processed(logits[r], T), k, p) for r in range(b)]
        if case == "cut":
            ids = [int(np.argmin(logits[r])) for r in range(b)]        # outside every kept set
        kw.update(thr=thr, T=T)
        ref_kw = [dict(temperature=T, thr=thr[r]) for r in range(b)]
    elif case in ("pen_new", "pen_old"):
        seen = [sorted(set(rng.integers(0, V, 64).tolist())) + [-200] for _ in range(b)]
        if case == "pen_new":      # the pick set its own bit: HF scored it unseen
            kw.update(pen=1.3, seen=seen, newly=[1] * b, T=0.9)
            ref_kw = [dict(temperature=0.9, penalty=1.3, seen=[i for i in seen[r] if i != ids[r]]) for r in range(b)]
        else:
            seen = [s + [ids[r]] for r, s in enumerate(seen)]
            kw.update(pen=1.3, seen=seen, newly=[0] * b, T=0.9)
            ref_kw = [dict(temperature=0.9, penalty=1.3, seen=seen[r]) for r in range(b)]
    elif case == "spike":
        logits[:] = -80.0
        for r in range(b):
            logits[r, ids[r]] = 80.0
    elif case == "inf_slice":
        logits[:, :V // 2] = -np.inf                                   # whole workgroup slices without a finite value
        ids = [V // 2 + int(rng.integers(0, V - V // 2)) for _ in range(b)]
        if b > 1:
            ids[1] = 0                                                 # and an id inside them: -inf
    raw, proc = _op(gpu_lib, torch.from_numpy(logits).cuda(), V, ids, **kw)
    assert not np.isnan(raw).any() and not np.isnan(proc).any()
    for r in range(b):
        _close(f"op-{case}-V{V}-b{b}-raw", raw[r], logits[r, ids[r]], logits[r])
        sc = lr.scores(logits[r], **ref_kw[r])
        _close(f"op-{case}-V{V}-b{b}-proc", proc[r], sc[ids[r]], sc)
    if case in ("raw", "spike", "inf_slice"):
        assert np.array_equal(raw.view(np.uint32), proc.view(np.uint32))          # nothing to process: one pass and a copy
    if case == "spike":
        assert (raw == 0.0).all()
    if case == "one_left":
        assert (proc == 0.0).all()
    if case == "ban":
        assert proc[0] == -np.inf and np.isfinite(raw[0])
    if case == "cut":
        assert (proc == -np.inf).all() and np.isfinite(raw).all()
    if case == "inf_slice" and b > 1:
        assert raw[1] == -np.inf


@pytest.mark.parametrize("V", [152064, 1000, 37])
def test_op_rows_that_are_not_16_byte_aligned(gpu_lib, V):
    rng = np.random.default_rng(V)
    b = 5
    buf = np.full((b, V + 1), np.nan, dtype=np.float32)                # ld = V + 1: the pad column must never be read
    buf[:, :V] = (rng.standard_normal((b, V)) * 3).astype(np.float32)
    logits = buf[:, :V]
    ids = _ids_mixed(rng, logits)
    raw, proc = _op(gpu_lib, torch.from_numpy(buf).cuda(), V, ids, T=0.7)
    for r in range(b):
        _close(f"op-ld-V{V}-raw", raw[r], logits[r, ids[r]], logits[r])
        sc = lr.scores(logits[r], temperature=0.7)
        _close(f"op-ld-V{V}-proc", proc[r], sc[ids[r]], sc)


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


def _steps(e, m, ids, n, smp=None, ngram=0, graph=False, logprobs=True, seed=77):
    """n picks (the prefill's + n - 1 decode steps with want_logits) -> (ids [b, n], the n logits arrays, (raw, proc, counts) or None)"""
    e.enable_decode_graph(graph)
    out = m.forward(input_ids=ids, use_cache=True)
    b = ids.shape[0]
    if ngram:
        e.set_constraints(b, ids.tolist(), n, no_repeat_ngram_size=ngram)
    else:
        e.constraints_off()
    if logprobs:
        e.set_logprobs(b, n)
    else:
        e.logprobs_off()
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
    rec = None
    if logprobs:
        raw, proc, counts = e.read_logprobs(b)
        rec = (raw.numpy(), proc.numpy(), counts)
    e.enable_decode_graph(False)
    e.constraints_off(); e.sampling_off(); e.logprobs_off()
    return np.stack(toks, 1), lgs, rec


@pytest.mark.parametrize("mode", sorted(MODES))
def test_decode_step_records_equal_ref_eager_and_graph(gpu_lib, mode):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    b, n = ids.shape[0], 9                                             # the prefill's pick + 8 decode steps
    kw = MODES[mode]
    smp, ngram = kw.get("smp"), kw.get("ngram", 0)
    off, _, _ = _steps(e, m, ids, n, logprobs=False, **kw)
    toks, lgs, (raw, proc, counts) = _steps(e, m, ids, n, **kw)
    assert np.array_equal(toks, off)                                   # recording changes no pick
    assert counts == [n] * b and raw.shape == (b, n) and proc.shape == (b, n)
    hist = [list(r) for r in ids.tolist()]
    for t in range(n):
        for r in range(b):
            i, row = int(toks[r, t]), lgs[t][r]
            _close(f"engine-{mode}-raw", raw[r, t], row[i], row)
            banned = cr.banned_ids(hist[r], cr.params(V_TINY, ngram=ngram), t) if ngram else []
            pk = dict(temperature=smp["temperature"], top_k=smp["top_k"], top_p=smp["top_p"], penalty=smp["repetition_penalty"],
                      seen=list(hist[r])) if smp else {}
            sc = lr.scores(row, banned=banned, **pk)
            assert np.isfinite(sc[i])                                  # a picked id is never cut
            _close(f"engine-{mode}-proc", proc[r, t], sc[i], sc)
        for r in range(b):
            hist[r].append(int(toks[r, t]))
    if mode == "greedy":
        assert np.array_equal(raw.view(np.uint32), proc.view(np.uint32))
    g_toks, _, (g_raw, g_proc, g_counts) = _steps(e, m, ids, n, graph=True, **kw)
    assert e.decode_graph_stats()["replays"] > 0
    assert np.array_equal(g_toks, toks) and g_counts == counts
    assert np.array_equal(g_raw.view(np.uint32), raw.view(np.uint32)) and np.array_equal(g_proc.view(np.uint32), proc.view(np.uint32))
    e.close()


def test_record_capacity_rewind_device_bytes_and_refusals(gpu_lib):
    _, e, m = _tiny_model(b=1)
    ids = torch.tensor(PROMPT[:1])
    out = m.forward(input_ids=ids, use_cache=True)
    e.sampling_off(); e.constraints_off()
    before = e.device_bytes()
    e.set_logprobs(1, 3)
    assert e.device_bytes() > before
    grown = e.device_bytes()
    tok = e.argmax(out.local_logits)
    tok, _ = e.decode_step(tok)
    tok, _ = e.decode_step(tok)
    kv = e.kv_lengths(1)
    with pytest.raises(ValueError):
        e.decode_step(tok)                                             # a fourth pick: refused before anything is enqueued
    assert e.kv_lengths(1) == kv
    raw3, _, counts = e.read_logprobs(1)
    assert counts == [3]
    e.kv_rewind(1, 1)
    assert e.read_logprobs(1)[2] == [2]
    tok2, _ = e.decode_step(tok)                                       # room again: the step lands in line 2, lines 0 and 1 are untouched
    raw3b, _, counts = e.read_logprobs(1)
    assert counts == [3] and torch.equal(raw3b[:, :2], raw3[:, :2])
    with pytest.raises(ValueError):
        e.decode_verify([int(tok2[0]), 5, 6])
    with pytest.raises(ValueError):
        e.beam_begin(1, 2, max_new=4)
    e.set_logprobs(1, 2)                                               # smaller: nothing shrinks, the counters restart
    assert e.device_bytes() == grown and e.read_logprobs(1)[2] == [0]
    e.logprobs_off()
    e.close()


LP_FULL = "more picks than the max_new given to omchat_set_logprobs"
CON_FULL = "more decode steps than the max_new given to omchat_set_constraints"


def _steps_until_refused(step, tok, message, limit=32):
    """decode steps that succeed before one is refused with `message` -> (their number, the last token)"""
    for n in range(limit):
        try:
            tok, _ = step(tok)
        except ValueError as ex:
            assert message in str(ex), str(ex)
            return n, tok
    raise AssertionError("no refusal within %d steps" % limit)


@pytest.mark.parametrize("path", ["decode_step", "decode_step_masked_next"])
def test_refused_pick_leaves_the_history_room_and_the_kv_lengths(gpu_lib, path):
    """The admission of a step: the record's room (omchat_set_logprobs) is checked before the history's (omchat_set_constraints), and a
    refused step moves no counter -- the history's budget, measured first without a record, is all still there after the refusal."""
    _, e, m = _tiny_model()
    if path == "decode_step":
        ids, kw, step = torch.tensor([[3, 17, 18, 19], [5, 6, 11, 12]]), {}, e.decode_step
    else:
        ids, step = torch.tensor([[3, 17, 18, 19], [5, 6, 0, 0]]), e.decode_step_masked_next
        kw = dict(attention_mask=torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0]]))

    def begin(logprobs):
        fw = m.forward(input_ids=ids, use_cache=True, **kw)
        e.sampling_off()
        e.set_constraints(2, ids.tolist(), 6, no_repeat_ngram_size=2)
        if logprobs:
            e.set_logprobs(2, 2)
        else:
            e.logprobs_off()
        if kw:      # positions and key mask of the first step as generate() takes them from the reference's decode branch
            m1 = torch.cat([kw["attention_mask"], torch.ones(2, 1, dtype=torch.long)], 1)
            _, pos1, mask1, _, _, _ = m.prepare_inputs_labels_for_multimodal(torch.zeros(2, 1, dtype=torch.long), None, m1, fw.past_key_values,
                                                                             None, None)
            if pos1 is None:
                pos1 = torch.full((2, 1), fw.past_key_values.get_seq_length(), dtype=torch.long)
            e.masked_decode_begin(pos1, mask1)
        return e.argmax(fw.local_logits)

    budget, _ = _steps_until_refused(step, begin(False), CON_FULL)      # the history's room in decode steps
    assert budget >= 6
    tok = begin(True)                                                   # the record's first line: the prefill's pick
    taken, tok = _steps_until_refused(step, tok, LP_FULL)
    assert taken == 1
    kv = e.kv_lengths(2)
    with pytest.raises(ValueError, match=LP_FULL):
        step(tok)
    assert e.kv_lengths(2) == kv and e.read_logprobs(2)[2] == [2, 2]
    e.logprobs_off()
    more, _ = _steps_until_refused(step, tok, CON_FULL)
    assert more == budget - taken, (more, budget, taken)
    assert e.kv_lengths(2) == [n + more for n in kv]
    e.constraints_off()
    e.close()


# ---------------------------------------------------------------------------------------------------------------- generate()
def test_generate_output_logprobs(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    b, T, n = ids.shape[0], ids.shape[1], 10
    plain = m.generate(ids, max_new_tokens=n)
    out = m.generate(ids, max_new_tokens=n, output_logprobs=True, return_dict_in_generate=True)
    assert torch.equal(out.sequences, plain) and torch.equal(out["sequences"], plain)
    assert out.logprobs.shape == (b, n) and out.processed_logprobs.shape == (b, n)
    assert out.logprobs.dtype == torch.float32 and bool((out.logprobs < 0).all())
    assert torch.equal(out.logprobs.view(torch.int32), out.processed_logprobs.view(torch.int32))      # greedy, no constraints: bit for bit
    lg = m.forward(input_ids=ids, use_cache=True).local_logits.cpu().numpy()
    for r in range(b):
        _close("generate-col0-raw", out.logprobs[r, 0].numpy(), lg[r, int(plain[r, T])], lg[r])
    # without the keyword nothing changes, and HF's full-vocabulary outputs are still dropped
    assert torch.equal(m.generate(ids, max_new_tokens=n), plain)
    dropped = m.generate(ids, max_new_tokens=n, output_scores=True, output_logits=True, return_dict_in_generate=True)
    assert isinstance(dropped, torch.Tensor) and torch.equal(dropped, plain)
    # sampled: same ids as the plain sampled call; the picked ids are kept ones
    s_plain = m.generate(ids, max_new_tokens=n, do_sample=True, seed=5, **SMP)
    s_out = m.generate(ids, max_new_tokens=n, do_sample=True, seed=5, output_logprobs=True, return_dict_in_generate=True, **SMP)
    assert torch.equal(s_out.sequences, s_plain)
    assert bool(torch.isfinite(s_out.processed_logprobs).all()) and bool((s_out.processed_logprobs <= 0).all())
    assert not torch.equal(s_out.processed_logprobs, s_out.logprobs)
    # generation_config carries the keyword too
    m.generation_config.output_logprobs = True
    assert torch.equal(m.generate(ids, max_new_tokens=n, return_dict_in_generate=True).logprobs, out.logprobs)
    m.generation_config.output_logprobs = False
    # another max_new_tokens within the record's capacity keeps the captured decode graphs, and the replayed records are the eager ones
    e.enable_decode_graph(True)
    m.generate(ids, max_new_tokens=n, output_logprobs=True, return_dict_in_generate=True)
    captures = e.decode_graph_stats()["captures"]
    g = m.generate(ids, max_new_tokens=n - 3, output_logprobs=True, return_dict_in_generate=True)
    assert e.decode_graph_stats()["captures"] == captures and e.decode_graph_stats()["replays"] > 0
    assert torch.equal(g.logprobs.view(torch.int32), out.logprobs[:, :n - 3].view(torch.int32))
    e.enable_decode_graph(False)
    e.close()


def test_generate_bad_words_first_token(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    b, T, n = ids.shape[0], ids.shape[1], 6
    first = int(m.generate(ids, max_new_tokens=1)[0, T])
    plain = m.generate(ids, max_new_tokens=n, bad_words_ids=[[first]])
    out = m.generate(ids, max_new_tokens=n, bad_words_ids=[[first]], output_logprobs=True, return_dict_in_generate=True)
    assert torch.equal(out.sequences, plain) and int(plain[0, T]) != first
    assert out.processed_logprobs[0, 0] != out.logprobs[0, 0]
    lg = m.forward(input_ids=ids, use_cache=True).local_logits.cpu().numpy()
    for r in range(b):
        i = int(plain[r, T])
        _close("generate-badwords-raw", out.logprobs[r, 0].numpy(), lg[r, i], lg[r])
        sc = lr.scores(lg[r], banned=[first])
        _close("generate-badwords-proc", out.processed_logprobs[r, 0].numpy(), sc[i], sc)
    e.close()


def test_generate_eos_mid_stream(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    T, n = ids.shape[1], 10
    free = m.generate(ids, max_new_tokens=n, output_logprobs=True, return_dict_in_generate=True)
    gen = free.sequences[:, T:].tolist()
    # an id whose first appearance in row 0 lies before the last step and that row 1 emits later or never: row 0 ends first
    stop = next(i for i in range(n - 1) if gen[0][i] not in gen[0][:i] and gen[0][i] not in gen[1][:i + 1])
    eos = gen[0][stop]
    stop1 = gen[1].index(eos) if eos in gen[1] else n - 1
    out = m.generate(ids, max_new_tokens=n, eos_token_id=eos, pad_token_id=0, output_logprobs=True, return_dict_in_generate=True)
    new = out.sequences.shape[1] - T
    assert new == stop1 + 1 and out.logprobs.shape == (2, new)         # the batch runs until row 1 ends too (or to max_new_tokens)
    assert out.sequences[0, T:].tolist() == gen[0][:stop + 1] + [0] * (new - stop - 1)
    assert out.sequences[1, T:].tolist() == gen[1][:new]
    assert torch.equal(out.logprobs[0, :stop + 1], free.logprobs[0, :stop + 1])
    assert torch.equal(out.logprobs[1].view(torch.int32), free.logprobs[1, :new].view(torch.int32))
    assert new > stop + 1
    assert bool((out.logprobs[0, stop + 1:] == 0).all()) and bool((out.processed_logprobs[0, stop + 1:] == 0).all())
    assert bool((out.logprobs[1] < 0).all())
    # b = 1: the EOS ends the call, the step enqueued ahead is taken back with its record -- exactly `new` records, and the next call is clean
    one = ids[:1]
    free1 = m.generate(one, max_new_tokens=n, output_logprobs=True, return_dict_in_generate=True)      # (batch 1 takes other GEMV forms)
    gen1 = free1.sequences[0, T:].tolist()
    stop = max(i for i in range(n - 1) if gen1[i] not in gen1[:i])
    eos = gen1[stop]
    kv = None
    for _ in range(2):
        o1 = m.generate(one, max_new_tokens=n, eos_token_id=eos, output_logprobs=True, return_dict_in_generate=True)
        assert o1.sequences[0, T:].tolist() == gen1[:stop + 1] and o1.logprobs.shape == (1, stop + 1)
        assert e.read_logprobs(1)[2] == [stop + 1]
        assert torch.equal(o1.logprobs[0].view(torch.int32), free1.logprobs[0, :stop + 1].view(torch.int32))
        kv = e.kv_lengths(1)
    # the three refusals: before anything is enqueued
    with pytest.raises(ValueError):
        m.generate(one, max_new_tokens=4, output_logprobs=True)
    with pytest.raises(NotImplementedError):
        m.generate(one, max_new_tokens=4, num_beams=2, output_logprobs=True, return_dict_in_generate=True)
    with pytest.raises(NotImplementedError):
        m.generate(one, max_new_tokens=4, prompt_lookup_num_tokens=3, output_logprobs=True, return_dict_in_generate=True)
    assert e.kv_lengths(1) == kv
    e.close()


def test_generate_ragged_batch_through_the_masked_path(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor([[3, 17, 18, 19, 20, 21, 7, 9], [5, 6, 11, 12, 0, 0, 0, 0]])
    mask = torch.tensor([[1] * 8, [1] * 4 + [0] * 4])
    n = 8
    plain = m.generate(ids, attention_mask=mask, max_new_tokens=n, pad_token_id=0)
    out = m.generate(ids, attention_mask=mask, max_new_tokens=n, pad_token_id=0, output_logprobs=True, return_dict_in_generate=True)
    assert m._padded_batch
    assert torch.equal(out.sequences, plain) and out.logprobs.shape == (2, n)
    assert torch.equal(out.logprobs.view(torch.int32), out.processed_logprobs.view(torch.int32))
    # the same steps by hand with the logits read back: every record against the ref
    fw = m.forward(input_ids=ids, attention_mask=mask, use_cache=True)
    e.sampling_off(); e.constraints_off(); e.logprobs_off()
    lg = fw.local_logits
    tok = e.argmax(lg)
    # positions and key mask of the first step exactly as generate() takes them from the reference's decode branch
    m1 = torch.cat([mask, torch.ones(2, 1, dtype=mask.dtype)], 1)
    _, pos1, mask1, _, _, _ = m.prepare_inputs_labels_for_multimodal(torch.zeros(2, 1, dtype=torch.long), None, m1, fw.past_key_values, None, None)
    if pos1 is None:
        pos1 = torch.full((2, 1), fw.past_key_values.get_seq_length(), dtype=torch.long)
    e.masked_decode_begin(pos1, mask1)
    for t in range(n):
        row = lg.cpu().numpy()
        for r in range(2):
            i = int(plain[r, 8 + t])
            assert int(tok[r]) == i
            _close("generate-masked-raw", out.logprobs[r, t].numpy(), row[r, i], row[r])
        if t < n - 1:
            tok, lg = e.decode_step_masked_next(tok, want_logits=True)
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


def _tp_steps(engines, logits_steps, seen, p):
    n = len(engines)
    out, err = [None] * n, [None] * n

    def work(r):
        try:
            e = engines[r]
            b = logits_steps[0].shape[0]
            if p is not None:
                e.set_sampling(b, seed=424242, seen=seen, **p)
            else:
                e.sampling_off()
            e.set_logprobs(b, len(logits_steps))
            Vl = logits_steps[0].shape[1] // n
            ids = []
            for lg in logits_steps:
                part = lg[:, r * Vl:(r + 1) * Vl].contiguous()
                ids.append((e.sample(part) if p is not None else e.argmax(part)).cpu().numpy())
            raw, proc, counts = e.read_logprobs(b)
            out[r] = (np.stack(ids, 1), raw.numpy(), proc.numpy(), counts)
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
@pytest.mark.parametrize("p", [None, dict(temperature=0.9, top_k=200, top_p=0.95, repetition_penalty=1.3),
                               dict(temperature=0.5, top_k=1, top_p=1.0, repetition_penalty=1.3)], ids=["greedy", "sampled", "top_k1"])
def test_tp_records_agree_with_tp1(gpu_lib, tp, p):
    cfg = tiny()
    V, b, steps = cfg.text["vocab_size"], 3, 4
    rng = np.random.default_rng(tp)
    logits_steps = [torch.from_numpy((rng.standard_normal((b, V)) * 1.5).astype(np.float32)).cuda() for _ in range(steps)]
    seen = [rng.integers(0, V, 20).tolist() + [-200] for _ in range(b)]
    one = Engine(cfg, dtype="bf16", max_seq=16, max_batch=b, max_tiles=1, vision=False)
    ids1, raw1, proc1, counts1 = _tp_steps([one], logits_steps, seen, p)[0]
    assert counts1 == [steps] * b
    grp = _Group(tp)
    engines, hooks = [], []
    for r in range(tp):
        e = Engine(cfg, dtype="bf16", max_seq=16, max_batch=b, max_tiles=1, vision=False, tp_rank=r, tp_size=tp, comm=C.c_void_p(1))
        h = grp.hook_for(r)
        check(gpu_lib.omchat_set_allreduce_hook(e.h, C.cast(h, C.c_void_p), None))
        engines.append(e); hooks.append(h)
    got = _tp_steps(engines, logits_steps, seen, p)
    kw = dict(temperature=p["temperature"], top_k=p["top_k"], top_p=p["top_p"], penalty=p["repetition_penalty"]) if p else {}
    sn = [[i for i in s if i >= 0] for s in seen]
    for t, lg in enumerate(logits_steps):
        row = lg.cpu().numpy()
        for i in range(b):
            tok = int(ids1[i, t])
            sc = lr.scores(row[i], seen=list(sn[i]), **kw) if p else row[i]
            _close("tp1-raw", raw1[i, t], row[i, tok], row[i])
            _close("tp1-proc", proc1[i, t], sc[tok], sc)
            tol_raw, tol_proc = lr.tolerance(row[i, tok], lr.lse(row[i])), lr.tolerance(sc[tok], lr.lse(sc))
            for r in range(tp):
                ids, raw, proc, counts = got[r]
                assert np.array_equal(ids, ids1) and counts == counts1
                assert abs(float(raw[i, t]) - float(raw1[i, t])) <= tol_raw, (r, i, t, raw[i, t], raw1[i, t])
                assert abs(float(proc[i, t]) - float(proc1[i, t])) <= tol_proc, (r, i, t, proc[i, t], proc1[i, t])
                assert np.array_equal(raw.view(np.uint32), got[0][1].view(np.uint32))      # every rank holds the same number
                assert np.array_equal(proc.view(np.uint32), got[0][2].view(np.uint32))
        for i in range(b):
            sn[i].append(int(ids1[i, t]))
    for e in engines + [one]:
        e.close()
