"""GPU: on-device beam search (omchat_amd/csrc/beam.hip) -- the selection op step by step against tests/beam_ref.py, the same decisions at
TP = 2 / 4 as at TP = 1 (rank contexts on one GPU, all-reduces served by a test hook), the KV gather against a torch gather bit for bit,
and generate(num_beams=N) on a tiny synthetic model: every step checked against beam_ref on that step's own logits, eager = decode graph,
the returned hypotheses rescored by a fresh teacher-forced pass (16-bit and e4m3 KV cache), num_beams=1 = greedy, and the refusals."""
import ctypes as C
import threading
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import beam_ref as br
from omchat_amd import synth, _lib
from omchat_amd._lib import check, ptr
from omchat_amd.config import tiny
from omchat_amd.engine import Engine


# ---------------------------------------------------------------------------------------------------------------- selection op
class _OpSearch:
    def __init__(self, lib, b, N, max_new, eos, lp, es):
        self.lib, self.b, self.N, self.max_new, self.eos, self.lp = lib, b, N, max_new, list(eos), lp
        self.es = 2 if es == "never" else int(bool(es))
        self.state = torch.zeros(int(lib.omchat_beam_state_words(b, N, max_new)), dtype=torch.int32, device="cuda")
        self.tok = torch.empty(b * N, dtype=torch.int32, device="cuda")
        self.par = torch.empty(b * N, dtype=torch.int32, device="cuda")
        self.done = torch.zeros(1, dtype=torch.int32, device="cuda")

    def step(self, logits, t):
        ev = torch.tensor(self.eos or [0], dtype=torch.int32)
        check(self.lib.omchat_op_beam_select(ptr(logits), logits.shape[0], logits.shape[1], self.b, self.N, t, self.max_new, self.lp, self.es,
                                             ptr(ev), len(self.eos), ptr(self.state), ptr(self.tok), ptr(self.par), ptr(self.done),
                                             _lib.cur_stream()))
        torch.cuda.synchronize()
        return self.tok.cpu().numpy(), self.par.cpu().numpy(), int(self.done.item())

    def fin(self):
        s = self.state.cpu().numpy()
        bN = self.b * self.N
        return s[bN:2 * bN].view(np.float32), s[2 * bN:3 * bN], s[3 * bN:4 * bN], s[:bN].view(np.float32), s[6 * bN + self.b:6 * bN + 2 * self.b]


def _check_state(op, Ps, t):
    sc, fl, stp, run, done = op.fin()
    N = op.N
    for i, P in enumerate(Ps):
        assert bool(done[i]) == P.done, (t, i)
        for j in range(N):
            want = P.fin[j]
            assert sc[i * N + j] == want[0] and bool(fl[i * N + j]) == want[1] and stp[i * N + j] == want[2], (t, i, j, sc[i * N + j], want)
        assert np.array_equal(run[i * N:(i + 1) * N], P.run), (t, i, run[i * N:(i + 1) * N], P.run)


@pytest.mark.parametrize("V", [152064, 1000])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("N", [2, 4, 8])
@pytest.mark.parametrize("n_eos,lp,es", [(1, 1.0, False), (2, 2.0, "never"), (1, -0.5, True), (0, 0.0, False)])
def test_op_select_equals_ref(gpu_lib, V, b, N, n_eos, lp, es):
    rng = np.random.default_rng(V + 10 * b + N + n_eos)
    max_new = 7
    eos = [int(x) for x in rng.choice(V, n_eos, replace=False)]
    op = _OpSearch(gpu_lib, b, N, max_new, eos, lp, es)
    Ps = [br.Prompt(N) for _ in range(b)]
    all_done = False
    for t in range(max_new):
        rows = b if t == 0 else b * N
        lg = (rng.standard_normal((rows, V)) * 3).astype(np.float32)
        if eos and t in (1, 2, 4):                        # forced EOS hits: a candidate ends in EOS among the top beams
            for r in range(0, rows, 2):
                lg[r, eos[t % len(eos)]] = lg[r].max() + 0.5 + 0.01 * r
        tok, par, done = op.step(torch.from_numpy(lg).cuda(), t)
        want_t, want_p = [], []
        for i, P in enumerate(Ps):
            a, p = br.step(P, lg[i:i + 1] if t == 0 else lg[i * N:(i + 1) * N], t, max_new, eos, lp, es)
            want_t += list(a)
            want_p += [i * N + int(x) for x in p]          # a row's own index at t = 0 and for a frozen prompt
        for i, P in enumerate(Ps):
            sl = slice(i * N, (i + 1) * N)
            assert np.array_equal(tok[sl], np.array(want_t[sl])), (t, i, tok[sl], want_t[sl])
            assert np.array_equal(par[sl], np.array(want_p[sl])), (t, i, par[sl], want_p[sl])
        _check_state(op, Ps, t)
        assert done == int(all(P.done for P in Ps))
        if done:
            all_done = True
            if t + 1 < max_new:                           # a step after every prompt is done is a no-op
                before = op.state.clone()
                lg2 = torch.from_numpy((rng.standard_normal((b * N, V)) * 3).astype(np.float32)).cuda()
                tok2, par2, done2 = op.step(lg2, t + 1)
                s0, s1 = before.cpu().numpy(), op.state.cpu().numpy()
                bN = b * N
                assert np.array_equal(s0[:6 * bN + 2 * b], s1[:6 * bN + 2 * b]) and done2 == 1
                assert np.array_equal(par2, np.arange(bN))
            break
    assert all_done


# ---------------------------------------------------------------------------------------------------------------- tensor parallelism
class _Group:
    """fp32 all-reduce hook over rank contexts living on one GPU (tests/test_gpu_tp_single.py's pattern)"""

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


def _beam_steps(engines, logits_steps, b, N, eos):
    n = len(engines)
    out, err = [None] * n, [None] * n

    def work(r):
        try:
            e = engines[r]
            e.beam_begin(b, N, 1.0, False, eos, len(logits_steps), prompt_len=4)
            Vl = logits_steps[0].shape[1] // n
            toks = []
            for lg in logits_steps:
                toks.append(e.beam_step(lg[:, r * Vl:(r + 1) * Vl].contiguous()).cpu().numpy())
                if int(e.beam_done.item()):
                    break
            hyps, scores = e.beam_result(N)
            out[r] = (toks, hyps, scores)
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
@pytest.mark.parametrize("vocab", [320, 152064])
def test_tp_select_equals_tp1(gpu_lib, tp, vocab):
    cfg = tiny(vocab=vocab)
    b, N, steps = 2, 4, 5
    rng = np.random.default_rng(tp + vocab)
    logits_steps = [torch.from_numpy((rng.standard_normal((b if k == 0 else b * N, vocab)) * 2).astype(np.float32)).cuda()
                    for k in range(steps)]
    eos = [int(rng.integers(vocab))]
    for k in (1, 3):
        logits_steps[k][0, eos[0]] = logits_steps[k][0].max() + 1
    one = Engine(cfg, dtype="bf16", max_seq=16, max_batch=b * N, max_tiles=1, vision=False)
    ref = _beam_steps([one], logits_steps, b, N, eos)[0]
    grp = _Group(tp)
    engines, hooks = [], []
    for r in range(tp):
        e = Engine(cfg, dtype="bf16", max_seq=16, max_batch=b * N, max_tiles=1, vision=False, tp_rank=r, tp_size=tp, comm=C.c_void_p(1))
        h = grp.hook_for(r)
        check(gpu_lib.omchat_set_allreduce_hook(e.h, C.cast(h, C.c_void_p), None))
        engines.append(e); hooks.append(h)
    got = _beam_steps(engines, logits_steps, b, N, eos)
    for r in range(tp):
        assert len(got[r][0]) == len(ref[0])
        for a, w in zip(got[r][0], ref[0]):
            assert np.array_equal(a, w)
        assert got[r][1] == ref[1] and np.array_equal(got[r][2], ref[2])
    for e in engines + [one]:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- KV gather
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("case", ["identity", "cycle3", "dups", "fork"])
def test_kv_gather_equals_torch(gpu_lib, fp8, case):
    L, R, H, S = 2, 8, 3, 40
    lo, hi = 5, 29
    g = torch.Generator(device="cuda").manual_seed(5)
    k = torch.randn(L, R, H, S, 128, device="cuda", generator=g).to(torch.bfloat16)
    v = torch.randn(L, R, H, S, 128, device="cuda", generator=g).to(torch.bfloat16)
    k8 = torch.randint(0, 256, (L, R, H, S, 128), dtype=torch.uint8, device="cuda", generator=g) if fp8 else None
    v8 = torch.randint(0, 256, (L, R, H, S, 128), dtype=torch.uint8, device="cuda", generator=g) if fp8 else None
    ks = torch.rand(L, R, H, S, device="cuda", generator=g) if fp8 else None
    vs = torch.rand(L, R, H, S, device="cuda", generator=g) if fp8 else None
    row0, nrows = 1, 6
    par = list(range(R))
    fork_src = -1
    if case == "cycle3":
        par[1], par[2], par[3] = 2, 3, 1          # 1 <- 2 <- 3 <- 1
        par[5] = 4
    elif case == "dups":
        par[1] = par[2] = par[3] = 4
        par[6] = 3
    elif case == "fork":
        fork_src = 2
        par = [2 if row0 <= r < row0 + nrows else r for r in range(R)]
    bufs = [t for t in (k, v, k8, v8, ks, vs) if t is not None]
    want = [t.clone() for t in bufs]
    src = [t.clone() for t in bufs]
    for r in range(row0, row0 + nrows):
        if par[r] != r:
            for w, s_ in zip(want, src):
                w[:, r, :, lo:hi] = s_[:, par[r], :, lo:hi]
    pd = torch.tensor(par, dtype=torch.int32, device="cuda")
    check(gpu_lib.omchat_op_kv_gather(_lib.BF16, ptr(k), ptr(v), ptr(k8), ptr(v8), ptr(ks), ptr(vs), L, R, H, S,
                                      None if case == "fork" else ptr(pd), row0, nrows, fork_src, lo, hi, _lib.cur_stream()))
    torch.cuda.synchronize()
    for got, w in zip(bufs, want):
        assert torch.equal(got.view(torch.uint8) if got.dtype != torch.uint8 else got, w.view(torch.uint8) if w.dtype != torch.uint8 else w)


# ---------------------------------------------------------------------------------------------------------------- model level
def _tiny_model(b=8, seed=21, max_seq=128):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    cfg = tiny()
    e = Engine(cfg, dtype="bf16", max_seq=max_seq, max_batch=b, max_tiles=1, vision=False)
    e.load_state_dict(synth.state_dict(cfg, seed), strict=False)
    return cfg, e, OmChatQwen2ForCausalLM(cfg.clone(), e)


PROMPT = [[3, 17, 18, 19, 20, 21, 7, 9], [5, 6, 11, 12, 13, 40, 41, 42]]


def _engine_loop(e, m, ids, N, max_new, eos, nret, lp=1.0, es=False):
    """what generate's beam branch does, one step at a time, every step's selection checked against beam_ref on the step's own logits"""
    b = ids.shape[0]
    out = m.forward(input_ids=ids, use_cache=True)
    P = e.kv_lengths(b)[0]
    e.beam_begin(b, N, lp, es, eos, max_new, P)
    Ps = [br.Prompt(N) for _ in range(b)]
    lg = out.local_logits
    for t in range(max_new):
        l_np = lg.cpu().numpy()
        tok = e.beam_step(lg).cpu().numpy()
        for i, Pr in enumerate(Ps):
            was_done = Pr.done
            a, _ = br.step(Pr, l_np[i:i + 1] if t == 0 else l_np[i * N:(i + 1) * N], t, max_new, eos, lp, es)
            if not was_done:
                assert np.array_equal(tok[i * N:(i + 1) * N], a), (t, i, tok, a)
        if all(Pr.done for Pr in Ps):
            break
        _, lg = e.decode_step(torch.from_numpy(tok).cuda(), want_logits=True)
    hyps, scores = e.beam_result(nret)
    for i, Pr in enumerate(Ps):
        for q in range(nret):
            assert hyps[i * nret + q] == br.hypothesis(Pr, q)
            assert scores[i * nret + q] == np.float32(Pr.fin[q][0])
    return hyps, scores


def _eos_for(m, ids, N):
    free = m.generate(ids, num_beams=N, max_new_tokens=6)
    return [int(free[0, ids.shape[1] + 2])]


@pytest.mark.parametrize("b", [1, 2])
def test_generate_equals_engine_loop_and_ref(gpu_lib, b):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT[:b])
    eos = _eos_for(m, ids, 4)
    hyps, scores = _engine_loop(e, m, ids, 4, 10, eos, 2)
    out = m.generate(ids, num_beams=4, num_return_sequences=2, max_new_tokens=10, eos_token_id=eos, return_dict_in_generate=True)
    T = ids.shape[1]
    gen = max(len(h) for h in hyps)
    assert out.sequences.shape == (b * 2, T + gen)
    for o, h in enumerate(hyps):
        assert out.sequences[o, T:].tolist() == h + [eos[0]] * (gen - len(h))      # HF pads with eos[0] when no pad id is set
        assert torch.equal(out.sequences[o, :T], ids[o // 2])
    assert np.array_equal(out.sequences_scores.numpy(), scores)
    assert any(len(h) < 10 for h in hyps)                                      # a hypothesis ended on EOS
    e.close()


def test_decode_graph_equals_eager(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    kw = dict(num_beams=4, num_return_sequences=4, max_new_tokens=12, return_dict_in_generate=True, length_penalty=0.5)
    eager = m.generate(ids, **kw)
    e.enable_decode_graph(True)
    g = m.generate(ids, **kw)
    assert e.decode_graph_stats()["replays"] > 0
    e.enable_decode_graph(False)
    assert torch.equal(g.sequences, eager.sequences) and torch.equal(g.sequences_scores, eager.sequences_scores)
    e.close()


def _rescore(e, m, prompt, cont, lp, fed=None):
    """fresh prefill of the prompt, then the continuation teacher-forced through batch-1 decode steps: sum of fp64 log-probs / len ** lp.
    fed (negative control): the tokens written into the cache instead of cont's -- what a row continuing the wrong parent would hold"""
    fed = cont if fed is None else fed
    out = m.forward(input_ids=torch.tensor([prompt]), use_cache=True)
    lg = out.local_logits[0].double()
    s = 0.0
    for k, tk in enumerate(cont):
        s += float(torch.log_softmax(lg, -1)[tk])
        if k + 1 < len(cont):
            _, l2 = e.decode_step(torch.tensor([fed[k]]), want_logits=True)
            lg = l2[0].double()
    return s / (len(cont) ** lp)


@pytest.mark.parametrize("fp8", [False, True])
def test_rescoring_proves_the_cache_moves(gpu_lib, fp8):
    _, e, m = _tiny_model()
    if fp8:
        e.enable_fp8_kv(True)
    ids = torch.tensor(PROMPT)
    lp = 1.0
    out = m.generate(ids, num_beams=4, num_return_sequences=4, max_new_tokens=16, return_dict_in_generate=True, length_penalty=lp)
    T = ids.shape[1]
    # measured: the rescoring agrees to <= 3e-5 of |score| (batch-1 against batched decode kernels, same cache format); a cache slot that
    # holds another history moves it by >= 1e-3
    tol = 2e-4
    errs, wrong = [], []
    for o in range(out.sequences.shape[0]):
        cont = out.sequences[o, T:].tolist()
        got = _rescore(e, m, PROMPT[o // 4], cont, lp)
        want = float(out.sequences_scores[o])
        errs.append(abs(got - want) / max(1.0, abs(want)))
        # negative control: the same tokens scored over the cache of another beam of the same prompt for the first half (a wrong parent
        # row between finish and gather) must move the score by more than the tolerance
        h = len(cont) // 2
        others = [out.sequences[(o // 4) * 4 + q, T:].tolist() for q in range(4)]
        other = next((x for x in others if x[:h] != cont[:h]), None)
        fed = other[:h] + cont[h:] if other is not None else [(cont[0] + 1) % 320] + cont[1:]
        wrong.append(abs(_rescore(e, m, PROMPT[o // 4], cont, lp, fed=fed) - want) / max(1.0, abs(want)))
    assert max(errs) <= tol, errs
    assert min(wrong) > tol, (wrong, errs)
    e.close()


def test_num_beams_1_is_greedy(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    greedy = m.generate(ids, max_new_tokens=12)
    assert torch.equal(m.generate(ids, num_beams=1, max_new_tokens=12), greedy)
    m.generate(ids, num_beams=4, max_new_tokens=5)
    assert torch.equal(m.generate(ids, max_new_tokens=12), greedy)          # a beam search leaves the greedy path as it was
    e.close()


def test_refusals(gpu_lib):
    _, e, m = _tiny_model(b=4)
    ids = torch.tensor(PROMPT)
    with pytest.raises(NotImplementedError):
        m.generate(ids, num_beams=2, do_sample=True, seed=1)
    with pytest.raises(ValueError, match="streamer"):
        m.generate(ids, num_beams=2, streamer=object())
    with pytest.raises(NotImplementedError):
        m.generate(ids, num_beams=2, stopping_criteria=[lambda a, b: True])
    with pytest.raises(NotImplementedError):
        m.generate(ids, num_beams=2, repetition_penalty=1.2)
    with pytest.raises(NotImplementedError, match="b = 1"):
        m.generate(ids, num_beams=2, attention_mask=torch.tensor([[1] * 8, [0] + [1] * 7]))
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.generate(ids, num_beams=2, num_return_sequences=3)
    with pytest.raises(NotImplementedError, match="b = 1"):       # same prompt length, different spliced length (one image vs two)
        m.generate(torch.tensor([[3, -200, 17, 18, -200], [3, -200, 17, 18, 19]]), images=torch.zeros(3, 3, 56, 56).half().cuda(), num_beams=2)
    with pytest.raises(ValueError, match="max_batch >= 8"):
        m.generate(ids, num_beams=4)
    # nothing was enqueued by a refusal: greedy still works on this model
    assert m.generate(ids[:1], max_new_tokens=3).shape == (1, 11)
    e.close()
