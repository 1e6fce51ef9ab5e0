"""GPU: min_p, typical_p, epsilon_cutoff and eta_cutoff on the device (omchat_amd/csrc/sample.hip, the interval form) -- the op against
tests/sampling_ref2.py with ids and both interval ends equal exactly, decode steps (eager, decode graph), generate(), EOS rewind, TP = 2 / 4
against TP = 1 and the processed log-probabilities over the interval."""
import ctypes as C
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import logprob_ref as lr
import sampling_ref as sr
import sampling_ref2 as sr2
from omchat_amd import _lib
from omchat_amd._lib import check, ptr
from omchat_amd.config import tiny
from omchat_amd.engine import Engine
from test_gpu_sampling import _tiny_model, _op_sample, _Group, PROMPT

ALL4 = dict(min_p=0.02, typical_p=0.6, epsilon_cutoff=1e-3, eta_cutoff=3e-3)
GRID = [
    dict(temperature=1.0, min_p=0.05),
    dict(temperature=1.0, typical_p=0.2),
    dict(temperature=1.0, typical_p=0.9),
    dict(temperature=1.0, epsilon_cutoff=3e-3),
    dict(temperature=1.0, eta_cutoff=3e-3),
    dict(temperature=1.0, **ALL4),
    dict(temperature=0.7, top_k=50, top_p=0.9, **ALL4),
]


def _c(kw):
    """(min_p, typical_p, epsilon, eta) as the C entry takes them"""
    cut = lambda v: 1.0 if v is None or not 0.0 < v < 1.0 else float(v)
    return (-1.0 if kw.get("min_p") is None else float(kw["min_p"]), cut(kw.get("typical_p")), cut(kw.get("epsilon_cutoff")),
            cut(kw.get("eta_cutoff")))


def _op(lib, logits, seed, step=0, temperature=1.0, top_k=0, top_p=1.0, **flt):
    """omchat_op_sample_filtered -> (ids, lo, hi)"""
    b, V = logits.shape
    out = torch.empty(b, dtype=torch.int32, device="cuda")
    lo = torch.zeros(b, dtype=torch.int32, device="cuda")
    hi = torch.zeros(b, dtype=torch.int32, device="cuda")
    n = torch.zeros(b, dtype=torch.int32)
    flat = torch.zeros(1, dtype=torch.int32)
    check(lib.omchat_op_sample_filtered(ptr(logits), b, V, seed, temperature, top_k, top_p, 1.0, *_c(flt), ptr(flat), ptr(n), step, ptr(out),
                                        ptr(lo), ptr(hi), _lib.cur_stream()))
    torch.cuda.synchronize()
    u = lambda t: t.cpu().numpy().view(np.uint32).astype(np.int64)
    return out.cpu().numpy().astype(np.int64), u(lo), u(hi)


_ROWS = {}


def _rows(b, V):
    if (b, V) not in _ROWS:
        _ROWS[b, V] = (np.random.default_rng(b * 7 + V).standard_normal((b, V)) * 3).astype(np.float32)
    return _ROWS[b, V]


def _check_rows(lib, logits, kw):
    kw = dict(kw)
    T = kw.pop("temperature", 1.0)
    want = [sr2.interval(sr.processed(row, T), **kw) for row in logits]
    dev = torch.from_numpy(logits).cuda()
    for seed, step in ((11, 0), (12345678901, 7)):
        ids, lo, hi = _op(lib, dev, seed, step, temperature=T, **kw)
        assert lo.tolist() == [w[0] for w in want] and hi.tolist() == [w[1] for w in want], (lo, hi, want)
        ref = sr2.sample(logits, seed, step, temperature=T, **kw)
        assert np.array_equal(ids, ref), (seed, step, ids, ref)


@pytest.mark.parametrize("V", [1000, 152064])
@pytest.mark.parametrize("b", [1, 5])
@pytest.mark.parametrize("case", GRID, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_op_equals_ref(gpu_lib, b, V, case):
    _check_rows(gpu_lib, _rows(b, V), case)


EDGE = {
    "ties_min_p": (np.log(np.array([4, 2, 2, 1, 1], dtype=np.float32)), dict(min_p=0.4)),
    "ties_typical": (np.array([0, 0, -3, -3, -8], dtype=np.float32), dict(typical_p=0.3)),
    "ties_epsilon": (np.log(np.array([4, 2, 2, 1, 1], dtype=np.float32)), dict(epsilon_cutoff=0.15)),
    "typical_cuts_argmax": (np.array([5.0] + [2.0 + 0.01 * i for i in range(40)], dtype=np.float32), dict(typical_p=0.3)),
    "typical_cuts_argmax_then_cutoffs": (np.array([5.0] + [2.0 + 0.01 * i for i in range(40)], dtype=np.float32),
                                         dict(typical_p=0.3, epsilon_cutoff=0.9, eta_cutoff=0.9)),
    "epsilon_above_all": (np.array([1.0, 1.0, 0.5, 0.0, -1.0, 1.0], dtype=np.float32), dict(epsilon_cutoff=0.9)),
    "eta_above_all": (np.array([1.0, 1.0, 0.5, 0.0, -1.0, 1.0], dtype=np.float32), dict(epsilon_cutoff=0.9, eta_cutoff=0.9)),
    "min_p_zero": ((np.random.default_rng(1).standard_normal(100) * 5).astype(np.float32), dict(min_p=0.0)),
    "min_p_one": ((np.random.default_rng(1).standard_normal(100) * 5).astype(np.float32), dict(min_p=1.0)),
    "behind_top_k": ((np.random.default_rng(2).standard_normal(200) * 2).astype(np.float32),
                     dict(top_k=10, min_p=0.1, typical_p=0.7, epsilon_cutoff=0.01, eta_cutoff=0.02)),
    "minus_inf_entries": (np.where(np.arange(200) % 7 == 0, -np.inf, np.random.default_rng(2).standard_normal(200) * 2).astype(np.float32),
                          dict(typical_p=0.5, eta_cutoff=0.05)),
}


@pytest.mark.parametrize("name", sorted(EDGE))
def test_op_edge_rows(gpu_lib, name):
    row, kw = EDGE[name]
    _check_rows(gpu_lib, np.stack([row, row[::-1].copy()]), kw)
    if name.startswith("typical_cuts_argmax"):
        assert sr2.interval(row, **kw)[1] != sr2.TOP


@pytest.mark.parametrize("V", [1000, 152064])
@pytest.mark.parametrize("kw", [dict(temperature=1.0), dict(temperature=0.8, top_k=50), dict(temperature=0.9, top_k=50, top_p=0.9),
                                dict(temperature=0.5, top_k=1)], ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_filters_off_is_op_sample_bit_for_bit(gpu_lib, V, kw):
    dev = torch.from_numpy(_rows(5, V)).cuda()
    ids0, thr0 = _op_sample(gpu_lib, dev, 99, 3, want_thr=True, **kw)
    ids, lo, hi = _op(gpu_lib, dev, 99, 3, **kw)
    assert np.array_equal(ids, ids0) and np.array_equal(lo, thr0) and (hi == sr2.TOP).all()
    # top_k = 1 stays the greedy pick whatever the filters say
    if kw.get("top_k") == 1:
        assert np.array_equal(_op(gpu_lib, dev, 99, 3, **kw, **ALL4)[0], ids0)


# ---------------------------------------------------------------------------------------------------------------- model level
SETS = {"min_p": dict(temperature=0.9, top_k=0, top_p=1.0, repetition_penalty=1.3, min_p=0.2),
        "typical_eta": dict(temperature=1.1, top_k=100, top_p=0.95, repetition_penalty=1.0, typical_p=0.5, eta_cutoff=0.02)}


def _ref_kw(p):
    kw = {k: v for k, v in p.items() if k != "repetition_penalty"}
    kw["penalty"] = p.get("repetition_penalty", 1.0)
    return kw


def _engine_loop(e, m, ids, n, seed, graph=False, **p):
    """generate's sampled path one step at a time, every pick checked against sampling_ref2 on the step's own logits"""
    e.enable_decode_graph(graph)
    out = m.forward(input_ids=ids, use_cache=True)
    b = ids.shape[0]
    seen = [[int(i) for i in r if i >= 0] for r in ids.tolist()]
    e.set_sampling(b, seed=seed, seen=seen, **p)
    lg = out.local_logits
    tok = e.sample(lg)
    got = []
    for step in range(n):
        ref = sr2.sample(lg.cpu().numpy(), seed, step, seen=seen, **_ref_kw(p))
        assert np.array_equal(tok.cpu().numpy(), ref), (step, tok.tolist(), ref)
        got.append(ref)
        for r in range(b):
            seen[r].append(int(ref[r]))
        tok, lg = e.decode_step(tok, want_logits=True)
    e.enable_decode_graph(False)
    return np.stack(got, 1)


@pytest.mark.parametrize("name", sorted(SETS))
def test_decode_steps_pick_what_the_ref_picks(gpu_lib, name):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    eager = _engine_loop(e, m, ids, 8, 77, **SETS[name])
    g = _engine_loop(e, m, ids, 8, 77, graph=True, **SETS[name])
    assert np.array_equal(g, eager) and e.decode_graph_stats()["replays"] > 0
    out = m.generate(ids, do_sample=True, seed=77, max_new_tokens=8, **SETS[name])
    assert np.array_equal(out[:, ids.shape[1]:].numpy(), eager)
    e.close()


def _walk(m, ids, out):
    """the logits (numpy [b, V]) every generated position of `out` was picked from, by teacher-forcing the sequence through the model"""
    m.engine.sampling_off()
    if getattr(m.engine, "_logprobs_on", False):
        m.engine.logprobs_off()
    new = out[:, ids.shape[1]:]
    lg = m.forward(input_ids=ids, use_cache=True).local_logits
    for step in range(new.shape[1]):
        yield step, lg.cpu().numpy()
        if step + 1 < new.shape[1]:
            _, lg = m.engine.decode_step(new[:, step].to(torch.int32).cuda(), want_logits=True)


def _replay(m, ids, out, seed, **p):
    """the reference replayed on the logits the model returns for the generated sequence"""
    b, T = ids.shape
    seen = [[int(i) for i in r if i >= 0] for r in ids.tolist()]
    for step, lg in _walk(m, ids, out):
        ref = sr2.sample(lg, seed, step, seen=seen, **_ref_kw(p))
        assert ref.tolist() == out[:, T + step].tolist(), (step, ref, out[:, T + step])
        for r in range(b):
            seen[r].append(int(ref[r]))


def test_generate_min_p(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    n, T = 12, ids.shape[1]
    # a seed for which the reference says the two runs must part at the very first pick (same logits, same noise: the unfiltered draw lies
    # outside min_p's kept set)
    lg0 = m.forward(input_ids=ids, use_cache=True).local_logits.cpu().numpy()
    seed = next(s for s in range(1, 400) if not np.array_equal(sr2.sample(lg0, s, 0), sr2.sample(lg0, s, 0, min_p=0.2)))
    a = m.generate(ids, do_sample=True, seed=seed, max_new_tokens=n, min_p=0.2, top_k=0)
    assert torch.equal(a, m.generate(ids, do_sample=True, seed=seed, max_new_tokens=n, min_p=0.2, top_k=0))
    plain = m.generate(ids, do_sample=True, seed=seed, max_new_tokens=n, top_k=0)
    assert not torch.equal(a[:, T], plain[:, T])
    _replay(m, ids, plain, seed, temperature=1.0)
    _replay(m, ids, a, seed, temperature=1.0, min_p=0.2)
    # generation_config carries the parameters too
    m.generation_config.min_p = 0.2
    assert torch.equal(m.generate(ids, do_sample=True, seed=seed, max_new_tokens=n, top_k=0), a)
    m.generation_config.min_p = None
    assert torch.equal(m.generate(ids, do_sample=True, seed=seed, max_new_tokens=n, top_k=0), plain)
    with pytest.raises(ValueError, match="min_p"):
        m.generate(ids, do_sample=True, seed=1, min_p=1.5)
    with pytest.raises(ValueError, match="typical_p"):
        m.generate(ids, do_sample=True, seed=1, typical_p=0)
    greedy = m.generate(ids, max_new_tokens=n)
    assert torch.equal(m.generate(ids, max_new_tokens=n, min_p=0.2, typical_p=0.5, epsilon_cutoff=0.01, eta_cutoff=0.01), greedy)
    assert torch.equal(m.generate(ids, do_sample=True, seed=3, top_k=1, max_new_tokens=n, **ALL4), greedy)
    e.close()


def test_eos_rewind_restores_step_with_filters(gpu_lib):
    P = SETS["typical_eta"] | dict(repetition_penalty=1.3)
    _, e, m = _tiny_model(b=1)
    ids = torch.tensor(PROMPT[:1])
    free = m.generate(ids, do_sample=True, seed=31, max_new_tokens=10, **P)[0, ids.shape[1]:].tolist()
    stop = next(i for i in range(2, 10) if free[i] not in free[:i])
    eos = free[stop]
    out = m.generate(ids, do_sample=True, seed=31, max_new_tokens=10, eos_token_id=eos, **P)[0, ids.shape[1]:].tolist()
    assert out == free[:stop + 1]
    # the step enqueued ahead of the EOS was taken back: the next pick is keyed by step stop + 1 with the seen set of prompt + out
    nxt, lg = e.decode_step(torch.tensor([eos]), want_logits=True)
    seen = PROMPT[0] + out
    assert int(nxt[0]) == int(sr2.sample(lg.cpu().numpy(), 31, stop + 1, seen=[seen], **_ref_kw(P))[0])
    e.kv_rewind(1, 1)
    other = next(t for t in range(320) if t != eos)
    nxt2, lg2 = e.decode_step(torch.tensor([other]), want_logits=True)
    assert int(nxt2[0]) == int(sr2.sample(lg2.cpu().numpy(), 31, stop + 1, seen=[seen], **_ref_kw(P))[0])
    e.close()


def test_reuse_cache_with_filters(gpu_lib):
    _, e, m = _tiny_model(b=1)
    ids = torch.tensor(PROMPT[:1])
    p = dict(do_sample=True, seed=9, max_new_tokens=6, top_k=0, **ALL4)
    a = m.generate(ids, reuse_cache=True, **p)
    m.reset_cache()
    assert torch.equal(a, m.generate(ids, **p))
    e.close()


# ---------------------------------------------------------------------------------------------------------------- tensor parallelism
@pytest.mark.parametrize("tp", [2, 4])
def test_tp_ids_equal_tp1(gpu_lib, tp):
    from test_gpu_sampling import _sample_steps
    p = dict(temperature=0.9, top_k=200, top_p=0.95, repetition_penalty=1.3, min_p=0.01, typical_p=0.7, epsilon_cutoff=1e-3, eta_cutoff=3e-3)
    cfg = tiny()
    V, b, steps = cfg.text["vocab_size"], 3, 4
    rng = np.random.default_rng(tp)
    logits_steps = [torch.from_numpy((rng.standard_normal((b, V)) * 1.5).astype(np.float32)).cuda() for _ in range(steps)]
    seen = [rng.integers(0, V, 20).tolist() + [-200] for _ in range(b)]
    one = Engine(cfg, dtype="bf16", max_seq=16, max_batch=b, max_tiles=1, vision=False)
    ref = _sample_steps([one], logits_steps, seen, p)[0]
    grp = _Group(tp)
    engines, hooks = [], []
    for r in range(tp):
        e = Engine(cfg, dtype="bf16", max_seq=16, max_batch=b, max_tiles=1, vision=False, tp_rank=r, tp_size=tp, comm=C.c_void_p(1))
        h = grp.hook_for(r)
        check(gpu_lib.omchat_set_allreduce_hook(e.h, C.cast(h, C.c_void_p), None))
        engines.append(e); hooks.append(h)
    got = _sample_steps(engines, logits_steps, seen, p)
    for r in range(tp):
        assert np.array_equal(got[r], ref), (r, got[r], ref)
    sn = [list(s) for s in seen]
    for k, lg in enumerate(logits_steps):
        want = sr2.sample(lg.cpu().numpy(), 424242, k, seen=sn, **_ref_kw(p))
        assert np.array_equal(ref[:, k], want), (k, ref[:, k], want)
        for i in range(b):
            sn[i].append(int(want[i]))
    for e in engines + [one]:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- log-probabilities
def test_op_token_logprob_interval(gpu_lib):
    """an id above the interval's upper end records -inf; inside, the log-softmax over the interval"""
    row = EDGE["typical_cuts_argmax"][0]
    lo, hi = sr2.interval(row, typical_p=0.3)
    want = sr2.logprobs(row, typical_p=0.3)
    ids = [0, 20, int(np.flatnonzero(np.isfinite(want))[0])]
    dev = torch.from_numpy(np.stack([row] * 3)).cuda()
    raw = torch.zeros(3, device="cuda")
    proc = torch.zeros(3, device="cuda")
    t_ids = torch.tensor(ids, dtype=torch.int32)
    u = lambda v: torch.from_numpy(np.full(3, v, dtype=np.uint32).view(np.int32).copy()).cuda()
    d_lo, d_hi = u(lo), u(hi)
    check(gpu_lib.omchat_op_token_logprob_interval(ptr(dev), 3, len(row), len(row), ptr(t_ids), None, 1.0, 1.0, None, None, None, ptr(d_lo),
                                                   ptr(d_hi), ptr(raw), ptr(proc), _lib.cur_stream()))
    torch.cuda.synchronize()
    proc = proc.cpu().numpy()
    assert proc[0] == -np.inf and want[0] == -np.inf
    z = np.where(np.isfinite(want), row, -np.inf)
    for j in (1, 2):
        assert np.isfinite(want[ids[j]]) == np.isfinite(proc[j])
        if np.isfinite(want[ids[j]]):
            l = lr.lse(z)
            assert abs(float(proc[j]) - want[ids[j]]) <= lr.tolerance(row[ids[j]], l), (j, proc[j], want[ids[j]])


def test_generate_output_logprobs_with_typical_p(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    b, T, n = ids.shape[0], ids.shape[1], 8
    p = dict(temperature=0.9, top_k=0, typical_p=0.5)
    kw = dict(do_sample=True, seed=5, max_new_tokens=n, output_logprobs=True, return_dict_in_generate=True, temperature=0.9, top_k=0)
    out = m.generate(ids, typical_p=0.5, **kw)
    off = m.generate(ids, **kw)
    assert torch.equal(out.sequences, m.generate(ids, do_sample=True, seed=5, max_new_tokens=n, **p))
    new = out.sequences[:, T:]
    for step, rows in _walk(m, ids, out.sequences):
        for r in range(b):
            tok = int(new[r, step])
            x = sr.processed(rows[r], 0.9)
            z = np.where(sr2.kept_mask(x, typical_p=0.5), x, np.float32(-np.inf))
            want, l = lr.log_softmax_at(z, tok), lr.lse(z)
            got = float(out.processed_logprobs[r, step])
            err, tol = abs(got - want), lr.tolerance(x[tok], l)
            print(f"LPERR typical-proc {err:.3e} {tol:.3e}")
            assert np.isfinite(want) and err <= tol, (r, step, got, want, tol)
            want_raw = lr.raw(rows[r], tok)
            assert abs(float(out.logprobs[r, step]) - want_raw) <= lr.tolerance(rows[r, tok], lr.lse(rows[r]))
    assert not torch.equal(out.logprobs, out.processed_logprobs)
    # .logprobs is the run's without the filter: while a row's ids agree the two runs saw the same logits, and the raw values are the same bits
    same = 0
    for r in range(b):
        for step in range(n):
            if int(off.sequences[r, T + step]) != int(new[r, step]):
                break
            assert out.logprobs[r, step].view(torch.int32) == off.logprobs[r, step].view(torch.int32), (r, step)
            same += 1
    print("positions compared with the unfiltered run:", same)
    assert same >= 2, "this seed leaves no common prefix with the unfiltered run: pick another"
    e.close()
