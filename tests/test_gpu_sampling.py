"""GPU: the on-device sampler (omchat_amd/csrc/sample.hip) -- op level bit for bit against tests/sampling_ref.py, the decode steps and
generate(do_sample=True) on a tiny synthetic model (eager, decode graph, padded batch, EOS rewind), and the same ids at TP = 2 / 4 as at TP = 1
(rank contexts on one GPU, all-reduces served by a test hook)."""
import ctypes as C
import threading
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import sampling_ref as sr
from omchat_amd import synth, _lib
from omchat_amd._lib import check, ptr
from omchat_amd.config import tiny
from omchat_amd.engine import Engine


def _op_sample(lib, logits, seed, step=0, temperature=1.0, top_k=0, top_p=1.0, penalty=1.0, seen=None, want_thr=False):
    b, V = logits.shape
    out = torch.empty(b, dtype=torch.int32, device="cuda")
    thr = torch.zeros(b, dtype=torch.int32, device="cuda") if want_thr else None
    seen = seen if seen is not None else [[] for _ in range(b)]
    n = torch.tensor([len(r) for r in seen], dtype=torch.int32)
    flat = torch.tensor([i for r in seen for i in r] or [0], dtype=torch.int32)
    check(lib.omchat_op_sample(ptr(logits), b, V, seed, temperature, top_k, top_p, penalty, ptr(flat), ptr(n), step, ptr(out), ptr(thr),
                               _lib.cur_stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64), (thr.cpu().numpy().view(np.uint32).astype(np.int64) if want_thr else None)


GRID = [
    dict(temperature=1.0),
    dict(temperature=0.7),
    dict(temperature=1.0, top_k=1),
    dict(temperature=0.8, top_k=50),
    dict(temperature=1.0, top_k=1000),
    dict(temperature=1.0, top_p=0.5),
    dict(temperature=0.7, top_p=0.9),
    dict(temperature=1.2, top_p=0.999),
    dict(temperature=0.9, top_k=50, top_p=0.9),
    dict(temperature=1.0, penalty=1.0, seen=True),
    dict(temperature=0.8, penalty=1.3, seen=True),
    dict(temperature=0.8, top_k=50, top_p=0.9, penalty=1.3, seen=True),
]


@pytest.mark.parametrize("V", [152064, 1000])
@pytest.mark.parametrize("b", [1, 5, 32])
@pytest.mark.parametrize("case", GRID, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_op_sample_equals_ref(gpu_lib, b, V, case):
    rng = np.random.default_rng(b * 7 + V)
    logits = (rng.standard_normal((b, V)) * 3).astype(np.float32)
    kw = dict(case)
    seen = None
    if kw.pop("seen", False):
        seen = [sorted(set(rng.integers(0, V, 64).tolist())) + [-200] for _ in range(b)]
    pen = kw.pop("penalty", 1.0)
    for seed, step in ((11, 0), (12345678901, 7)):
        ids, thr = _op_sample(gpu_lib, torch.from_numpy(logits).cuda(), seed, step, penalty=pen, seen=seen, want_thr=True, **kw)
        ref = sr.sample(logits, seed, step, seen=seen, penalty=pen, **kw)
        assert np.array_equal(ids, ref), (seed, step, np.flatnonzero(ids != ref)[:8], ids[:8], ref[:8])
        k, p = kw.get("top_k", 0), kw.get("top_p", 1.0)
        if (1 < k < V) or p < 1.0:
            want = [sr.threshold(sr.processed(logits[r], kw["temperature"], None if seen is None else seen[r], pen), k, p) for r in range(b)]
            assert np.array_equal(thr, np.array(want)), (thr[:4], want[:4])


def test_top_k_1_is_argmax(gpu_lib):
    rng = np.random.default_rng(3)
    lg = torch.from_numpy((rng.standard_normal((32, 152064)) * 2).astype(np.float32)).cuda()
    lg[3, 100] = lg[3, 200] = lg[3].max() + 1          # a tie: the first index wins, as in greedy
    am = torch.empty(32, dtype=torch.int32, device="cuda")
    check(gpu_lib.omchat_op_argmax(ptr(lg), 32, 152064, ptr(am), _lib.cur_stream()))
    ids, _ = _op_sample(gpu_lib, lg, 99, 3, temperature=0.5, top_k=1)
    assert np.array_equal(ids, am.cpu().numpy()) and ids[3] == 100


def test_seed_and_step_key_the_draw(gpu_lib):
    lg = torch.zeros(32, 1000, device="cuda")
    a, _ = _op_sample(gpu_lib, lg, 5, 0)
    assert np.array_equal(a, _op_sample(gpu_lib, lg, 5, 0)[0])
    assert not np.array_equal(a, _op_sample(gpu_lib, lg, 6, 0)[0])
    assert not np.array_equal(a, _op_sample(gpu_lib, lg, 5, 1)[0])
    assert len(set(a.tolist())) > 16                     # rows draw independently


# ---------------------------------------------------------------------------------------------------------------- model level
def _tiny_model(b=2, seed=21):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    cfg = tiny()
    e = Engine(cfg, dtype="bf16", max_seq=128, max_batch=b, max_tiles=1, vision=False)
    e.load_state_dict(synth.state_dict(cfg, seed), strict=False)
    return cfg, e, OmChatQwen2ForCausalLM(cfg.clone(), e)


PROMPT = [[3, 17, 18, 19, 20, 21, 7, 9], [5, 6, 11, 12, 13, 40, 41, 42]]
P = dict(temperature=0.9, top_k=50, top_p=0.9, repetition_penalty=1.3)


def _engine_loop(e, m, ids, n, seed, graph=False, **p):
    """what generate's sampled path does, one step at a time, every pick checked against sampling_ref on the step's own logits"""
    e.enable_decode_graph(graph)
    out = m.forward(input_ids=ids, use_cache=True)
    b = ids.shape[0]
    seen = [[int(i) for i in r if i >= 0] for r in ids.tolist()]
    kw = dict(temperature=p["temperature"], top_k=p["top_k"], top_p=p["top_p"], penalty=p["repetition_penalty"])
    e.set_sampling(b, seed=seed, seen=seen, **p)
    lg = out.local_logits
    tok = e.sample(lg)
    got = []
    for step in range(n):
        ref = sr.sample(lg.cpu().numpy(), seed, step, seen=seen, **kw)
        assert np.array_equal(tok.cpu().numpy(), ref), (step, tok.tolist(), ref)
        got.append(tok.cpu().numpy().astype(np.int64))
        for r in range(b):
            seen[r].append(int(ref[r]))
        tok, lg = e.decode_step(tok, want_logits=True)
    e.enable_decode_graph(False)
    return np.stack(got, 1)


@pytest.mark.parametrize("graph", [False, True])
def test_decode_steps_pick_what_the_ref_picks(gpu_lib, graph):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    eager = _engine_loop(e, m, ids, 10, 77, **P)
    if graph:
        g = _engine_loop(e, m, ids, 10, 77, graph=True, **P)
        assert np.array_equal(g, eager)
        assert e.decode_graph_stats()["replays"] > 0
    # generate drives the same seam: the same ids
    out = m.generate(ids, do_sample=True, seed=77, max_new_tokens=10, **P)
    assert np.array_equal(out[:, ids.shape[1]:].numpy(), eager)
    e.close()


def test_generate_sampling_is_reproducible_and_greedy_unchanged(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    greedy = m.generate(ids, max_new_tokens=12)
    a = m.generate(ids, do_sample=True, seed=1, max_new_tokens=12, temperature=1.0, top_k=0)
    assert torch.equal(a, m.generate(ids, do_sample=True, seed=1, max_new_tokens=12, temperature=1.0, top_k=0))
    assert not torch.equal(a, m.generate(ids, do_sample=True, seed=2, max_new_tokens=12, temperature=1.0, top_k=0))
    g = torch.Generator().manual_seed(4)
    b1 = m.generate(ids, do_sample=True, generator=g, max_new_tokens=6)
    assert torch.equal(b1, m.generate(ids, do_sample=True, generator=torch.Generator().manual_seed(4), max_new_tokens=6))
    # top_k = 1 is the greedy pick; do_sample=False after sampling is greedy again, bit for bit
    assert torch.equal(m.generate(ids, do_sample=True, seed=3, top_k=1, max_new_tokens=12), greedy)
    assert torch.equal(m.generate(ids, max_new_tokens=12), greedy)
    with pytest.raises(ValueError):
        m.generate(ids, do_sample=True, seed=1, temperature=0.0)
    with pytest.raises(NotImplementedError):
        m.generate(ids, do_sample=True)                   # no seed source: the device sampler never reads torch's global RNG
    e.close()


def test_padded_batch_samples_through_the_masked_path(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor([[3, 17, 18, 19, 20, 21, 7, 9], [5, 6, 11, 12, 0, 0, 0, 0]])
    mask = torch.tensor([[1] * 8, [1] * 4 + [0] * 4])
    greedy = m.generate(ids, attention_mask=mask, max_new_tokens=8, pad_token_id=0)
    assert m._padded_batch
    assert torch.equal(m.generate(ids, attention_mask=mask, do_sample=True, seed=8, top_k=1, max_new_tokens=8, pad_token_id=0), greedy)
    a = m.generate(ids, attention_mask=mask, do_sample=True, seed=8, max_new_tokens=8, pad_token_id=0, **P)
    assert m._padded_batch
    assert torch.equal(a, m.generate(ids, attention_mask=mask, do_sample=True, seed=8, max_new_tokens=8, pad_token_id=0, **P))
    assert int(a.max()) < 320 and int(a.min()) >= 0
    e.close()


def test_eos_rewind_restores_step_and_seen_set(gpu_lib):
    _, e, m = _tiny_model(b=1)
    ids = torch.tensor(PROMPT[:1])
    free = m.generate(ids, do_sample=True, seed=31, max_new_tokens=10, **P)[0, ids.shape[1]:].tolist()
    stop = next(i for i in range(2, 10) if free[i] not in free[:i])      # a token whose pick set a new seen bit
    eos = free[stop]
    out = m.generate(ids, do_sample=True, seed=31, max_new_tokens=10, eos_token_id=eos, **P)[0, ids.shape[1]:].tolist()
    assert out == free[:stop + 1]
    # generate enqueued one step ahead of the EOS and took it back: the next step must be keyed by step stop + 1 with the seen set of
    # prompt + out (the ahead pick's bit cleared), and it must see the EOS token as its input
    nxt, lg = e.decode_step(torch.tensor([eos]), want_logits=True)
    seen = PROMPT[0] + out
    ref = sr.sample(lg.cpu().numpy(), 31, stop + 1, seen=[seen], temperature=P["temperature"], top_k=P["top_k"], top_p=P["top_p"],
                    penalty=P["repetition_penalty"])
    assert int(nxt[0]) == int(ref[0])
    # take that pick back by hand and feed another token: its seen bit must be gone, the step the same
    e.kv_rewind(1, 1)
    other = next(t for t in range(320) if t != eos)
    nxt2, lg2 = e.decode_step(torch.tensor([other]), want_logits=True)
    ref2 = sr.sample(lg2.cpu().numpy(), 31, stop + 1, seen=[seen], temperature=P["temperature"], top_k=P["top_k"], top_p=P["top_p"],
                     penalty=P["repetition_penalty"])
    assert int(nxt2[0]) == int(ref2[0])
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


def _sample_steps(engines, logits_steps, seen, p):
    n = len(engines)
    out = [None] * n
    err = [None] * n

    def work(r):
        try:
            e = engines[r]
            e.set_sampling(logits_steps[0].shape[0], seed=424242, seen=seen, **p)
            Vl = logits_steps[0].shape[1] // n
            ids = []
            for lg in logits_steps:
                ids.append(e.sample(lg[:, r * Vl:(r + 1) * Vl].contiguous()).cpu().numpy())
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
@pytest.mark.parametrize("p", [dict(temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0),
                               dict(temperature=0.7, top_k=50, top_p=1.0, repetition_penalty=1.0),
                               dict(temperature=1.0, top_k=0, top_p=0.9, repetition_penalty=1.0),
                               dict(temperature=0.9, top_k=200, top_p=0.95, repetition_penalty=1.3),
                               dict(temperature=0.5, top_k=1, top_p=1.0, repetition_penalty=1.3)],
                         ids=lambda p: "T{temperature}-k{top_k}-p{top_p}-r{repetition_penalty}".format(**p))
def test_tp_ids_equal_tp1(gpu_lib, tp, p):
    cfg = tiny()
    V, b, steps = cfg.text["vocab_size"], 3, 6
    rng = np.random.default_rng(tp)
    # flat-ish logits: the top-p nucleus spans every shard
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
    # and the CPU restatement of the whole-vocabulary draw (seen set grown by every pick)
    kw = dict(temperature=p["temperature"], top_k=p["top_k"], top_p=p["top_p"], penalty=p["repetition_penalty"])
    sn = [list(s) for s in seen]
    for k, lg in enumerate(logits_steps):
        want = sr.sample(lg.cpu().numpy(), 424242, k, seen=sn, **kw)
        assert np.array_equal(ref[:, k], want), (k, ref[:, k], want)
        for i in range(b):
            sn[i].append(int(want[i]))
    for e in engines + [one]:
        e.close()
