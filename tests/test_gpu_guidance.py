"""GPU: classifier-free guidance on the device (omchat_amd/csrc/guidance.hip) -- the stage through omchat_op_guidance
against tests/guidance_ref.py (fp64) within 8 times the deviation of an fp32 numpy evaluation of the same formula on the same inputs, its
-inf rule and bit-for-bit repeatability; then decode steps over 2b rows and generate(guidance_scale=) on a tiny synthetic model against a
host-driven loop that runs the stage on the step's raw [2b, V] logits and applies the CPU references of the stages behind it (exact ids:
greedy and sampled, eager and decode graph), the log-prob record, the composition with the bans, the automaton, the EOS rewind and MXFP4
decode, the tower with negative_images, and the refusals of the C ABI."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import constraints_ref as cr
import fsm_ref as fr
import guidance_ref as gr
import logprob_ref as lr
import sampling_ref as sr
from gpu_util import rel, TOL_DEEP
from omchat_amd import synth, _lib
from omchat_amd._lib import check, ptr
from omchat_amd.config import tiny
from omchat_amd.engine import Engine
from omchat_amd.fsm import DEAD, TokenFSM

V_BIG = 152064
V_TINY = tiny().text["vocab_size"]
SCALES = [0.0, 0.5, 1.5, 3.0]


# ---------------------------------------------------------------------------------------------------------------- the stage alone
def _inputs(b, V, seed):
    """[2b, V] fp32: row 0 (conditional) with a maximum above 100 -- exp without the max subtraction overflows --, the last twin row and
    the last conditional row with -inf entries, one id -inf in both"""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((2 * b, V)) * 3).astype(np.float32)
    z[0, V // 3] = 131.0
    z[0, V - 1] = 104.5
    z[2 * b - 1, ::7] = -np.inf
    z[b - 1, 3::11] = -np.inf
    z[b - 1, V // 2] = -np.inf
    z[2 * b - 1, V // 2] = -np.inf
    return z


def _op(lib, z, b, V, ld, scale, ld_out=None):
    """the stage on rows of stride ld (the columns behind V hold a sentinel that must not be read as a logit) -> (scores [b, V], the whole
    output buffer [b, ld_out])"""
    ld_out = ld_out or V
    buf = torch.full((2 * b, ld), 1e30, dtype=torch.float32)
    buf[:, :V] = torch.from_numpy(z)
    lg = buf.cuda()
    out = torch.full((b, ld_out), 7.0, dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.omchat_op_guidance_ws(b, V)), dtype=torch.uint8, device="cuda")
    check(lib.omchat_op_guidance(ptr(lg), ld, b, V, float(scale), ptr(ws), ptr(out), ld_out, _lib.cur_stream()))
    torch.cuda.synchronize()
    assert torch.equal(lg.cpu(), buf)                                # the input logits are never written
    full = out.cpu().numpy()
    return full[:, :V], full


def _check_op(lib, b, V, ld, seed, ld_out=None):
    z = _inputs(b, V, seed)
    for scale in SCALES:
        ref = gr.guide(z, b, scale)
        dev32, tol = gr.tolerance(z, b, scale)
        got, full = _op(lib, z, b, V, ld, scale, ld_out)
        assert not np.isnan(got).any()
        assert np.array_equal(np.isfinite(got), np.isfinite(ref))    # -inf exactly where either logit is -inf, finite elsewhere
        assert (got[~np.isfinite(got)] == -np.inf).all()
        fin = np.isfinite(ref)
        err = float(np.abs(got[fin].astype(np.float64) - ref[fin]).max())
        print(f"guidance op b={b} V={V} ld={ld} scale={scale}: device {err:.3e}, fp32 numpy {dev32:.3e}, bound {tol:.3e}")
        assert err <= tol, (b, V, ld, scale, err, dev32, tol)
        assert (full[:, V:] == 7.0).all()                            # nothing is written behind a row's V ids
        again, _ = _op(lib, z, b, V, ld, scale, ld_out)
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32))      # the same input bits give the same output bits


# (V, ld): the tiny vocabulary; widths that are no multiple of 4 nor of the 2048-logit tile, one and two tiles wide; ld > V with
# 16-byte-aligned rows (vector pieces, scalar tail) and with unaligned rows (scalar throughout)
WIDTHS = [(V_TINY, V_TINY), (2049, 2049), (4099, 4099), (2049, 2052), (V_TINY, V_TINY + 3)]


@pytest.mark.parametrize("V,ld", WIDTHS, ids=[f"V{v}-ld{l}" for v, l in WIDTHS])
@pytest.mark.parametrize("b", [1, 5, 16])
def test_op_guidance_equals_ref(gpu_lib, b, V, ld):
    _check_op(gpu_lib, b, V, ld, seed=b * 31 + V)


def test_op_guidance_full_vocabulary_and_padded_output(gpu_lib):
    _check_op(gpu_lib, 1, V_BIG, V_BIG, seed=3)
    _check_op(gpu_lib, 5, 4099, 4100, seed=4, ld_out=4104)           # the output rows wider than V too
    z = np.full((2, 2049), -np.inf, dtype=np.float32)                # rows of nothing but -inf: -inf, never NaN
    got, _ = _op(gpu_lib, z, 1, 2049, 2049, 1.5)
    assert (got == -np.inf).all()
    lg = torch.zeros(2, 64, device="cuda")
    out, ws = torch.empty(1, 64, device="cuda"), torch.empty(64, dtype=torch.uint8, device="cuda")
    for bad in (dict(ld=63), dict(ld_out=63), dict(scale=float("nan")), dict(b=0)):
        a = dict(dict(ld=64, b=1, scale=1.5, ld_out=64), **bad)
        with pytest.raises(ValueError):
            check(gpu_lib.omchat_op_guidance(ptr(lg), a["ld"], a["b"], 64, a["scale"], ptr(ws), ptr(out), a["ld_out"], _lib.cur_stream()))


# ---------------------------------------------------------------------------------------------------------------- model level
def _tiny_model(max_batch=4, seed=22, max_seq=128, vision=False, **kw):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    cfg = tiny()
    e = Engine(cfg, dtype="bf16", max_seq=max_seq, max_batch=max_batch, max_tiles=2, vision=vision, **kw)
    e.load_state_dict(synth.state_dict(cfg, seed), strict=not vision)
    return cfg, e, OmChatQwen2ForCausalLM(cfg.clone(), e)


PROMPT = [[3, 17, 18, 19, 20, 21, 7, 9], [5, 6, 11, 12, 13, 40, 41, 42]]
# the model seed and the negative prompts are chosen so that the guided ids leave the unguided ones early, greedy and sampled
NEG = {"shorter": [[1, 2, 4], [300, 301, 302]], "longer": [list(range(250, 261)), list(range(60, 71))]}
SMP = dict(temperature=0.9, top_k=50, top_p=0.9, repetition_penalty=1.3)
SCALE = 1.5
N = 24


def _con_kw(p):
    return dict(no_repeat_ngram_size=p["ngram"], bad_words_ids=p["bad_words"], min_new_tokens=p["min_new"], min_length=p["min_len"], eos=p["eos"],
                suppress_tokens=p["suppress"], begin_suppress_tokens=p["begin_suppress"])


def _host_loop(e, m, ids, neg, n, scale=SCALE, graph=False, smp=None, seed=5, p=None, fsm=None, logprobs=False, images=None, neg_images=None):
    """decode steps over 2b rows, the device's picks each checked against the CPU references applied to the stage's output on the step's RAW
    [2b, V] logits (omchat_op_guidance is deterministic: those are the bits the step's pick saw) -> (ids [b, n], raw logits per step,
    guided scores per step, the record)"""
    e.enable_decode_graph(graph)
    b = ids.shape[0]
    out = m._forward_guided(ids, images, dict(scale=scale, neg_ids=torch.tensor(neg), neg_images=neg_images))
    lens0 = e.kv_lengths(2 * b)
    hist = [list(r) for r in ids.tolist()]
    trans, states = (fsm[0], [0] * b) if fsm is not None else (None, None)
    if fsm is not None:
        e.load_token_fsm(fsm[1])
        e.token_fsm_begin(b, states, n)
    if p is not None:
        e.set_constraints(b, hist, n, **_con_kw(p))
    if logprobs:
        e.set_logprobs(b, n)
    if smp is not None:
        e.set_sampling(b, seed=seed, seen=[[i for i in r if i >= 0] for r in hist], **smp)
    else:
        e.sampling_off()
    e.set_guidance(b, scale)
    lg = out.local_logits
    assert tuple(lg.shape) == (2 * b, e.c.t_vocab)
    tok = e.sample(lg) if smp is not None else e.argmax(lg)
    got, raws, guided = [], [], []
    for step in range(n):
        raw = lg.cpu().numpy()
        assert np.isfinite(raw).all()                                # the logits handed back stay the raw ones
        g = e.guidance(lg, b, scale).cpu().numpy()
        ref = []
        for r in range(b):
            l = g[r]
            if p is not None:
                l = cr.apply(l, cr.banned_ids(hist[r], p, step))
            if trans is not None:
                l = fr.apply(trans, l, states[r])
            assert np.isfinite(l).any()
            ref.append(int(np.argmax(l)) if smp is None else
                       sr.sample_row(l, r, step, seed, smp["temperature"], smp["top_k"], smp["top_p"], [i for i in hist[r] if i >= 0],
                                     smp["repetition_penalty"]))
        assert tok.tolist() == ref + ref, (step, tok.tolist(), ref)      # the twins' ids are their rows'
        assert e.kv_lengths(2 * b) == [L + step for L in lens0], (step, e.kv_lengths(2 * b), lens0)
        got.append(ref); raws.append(raw); guided.append(g)
        for r in range(b):
            hist[r].append(ref[r])
            if trans is not None:
                states[r] = fr.step(trans, states[r], ref[r])
        if step < n - 1:
            tok, lg = e.decode_step(tok, want_logits=True)
    rec = e.read_logprobs(b) if logprobs else None
    e.enable_decode_graph(False)
    e.constraints_off(); e.sampling_off(); e.token_fsm_off(); e.guidance_off()
    if logprobs:
        e.logprobs_off()
    return np.array(got).T, raws, guided, rec


def _new(m, ids, n, **kw):
    return m.generate(ids, max_new_tokens=n, **kw)[:, ids.shape[1]:]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("smp", [None, SMP], ids=["greedy", "sampled"])
@pytest.mark.parametrize("neg", ["shorter", "longer"])
def test_decode_steps_pick_what_the_ref_picks_and_generate_returns_them(gpu_lib, neg, smp, graph):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    kw = dict(do_sample=True, seed=77, **SMP) if smp else {}
    free = _new(m, ids, N, **kw).tolist()
    assert e.kv_lengths(4)[2:] == [0, 0]                             # an unguided call has no twin rows
    got, _, _, _ = _host_loop(e, m, ids, NEG[neg], N, graph=graph, smp=smp, seed=77)
    if graph:
        assert e.decode_graph_stats()["replays"] > 0
    # guidance bit: both rows leave the unguided run early
    first = [next(t for t in range(N) if got[r, t] != free[r][t]) for r in range(2)]
    print(f"guided rows leave the unguided ids at positions {first}")
    assert max(first) < 8, first
    e.enable_decode_graph(graph)
    out = m.generate(ids, max_new_tokens=N, guidance_scale=SCALE, negative_prompt_ids=torch.tensor(NEG[neg]), **kw)
    assert torch.equal(out[:, :ids.shape[1]], ids) and tuple(out.shape) == (2, ids.shape[1] + N)      # the twins appear in no output
    assert np.array_equal(out[:, ids.shape[1]:].numpy(), got)
    assert e.kv_lengths(4) == [8 + N - 1] * 2 + [len(NEG[neg][0]) + N - 1] * 2
    # a call without the keyword is unguided again; so is a scale of 1
    e.enable_decode_graph(False)
    assert _new(m, ids, N, **kw).tolist() == free
    assert _new(m, ids, N, guidance_scale=1.0, negative_prompt_ids=torch.tensor(NEG[neg]), **kw).tolist() == free
    e.close()


def test_scale_one_allocates_no_twin_rows_and_the_default_context(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    plain = _new(m, ids, 8)                                          # (the first batched step builds what every later one reuses)
    before = e.device_bytes()
    one = _new(m, ids, 8, guidance_scale=1.0, negative_prompt_ids=torch.tensor(NEG["longer"]))
    assert e.kv_lengths(4) == [8 + 7, 8 + 7, 0, 0] and e.device_bytes() == before
    assert torch.equal(one, plain)
    # negative_prompt_ids=None: the twin's context is the last prompt token alone, as HF's processor takes it
    got, _, _, _ = _host_loop(e, m, ids, [[9], [42]], 8)
    out = _new(m, ids, 8, guidance_scale=SCALE)
    assert np.array_equal(out.numpy(), got) and e.kv_lengths(4) == [15, 15, 8, 8]
    assert e.device_bytes() > before                                 # the workspace and the copy are the context's, and counted
    grown = e.device_bytes()
    _new(m, ids, 8, guidance_scale=3.0)
    assert e.device_bytes() == grown
    # read from generation_config; the call's own value wins
    m.generation_config.guidance_scale = SCALE
    assert np.array_equal(_new(m, ids, 8).numpy(), got)
    assert torch.equal(_new(m, ids, 8, guidance_scale=1), one)
    m.generation_config.guidance_scale = None
    # the captured graphs survive a call with the same b and scale, and are dropped by another scale
    e.enable_decode_graph(True)
    a = _new(m, ids, 8, guidance_scale=SCALE)
    st1 = e.decode_graph_stats()
    b2 = _new(m, ids, 8, guidance_scale=SCALE)
    st2 = e.decode_graph_stats()
    assert st2["captures"] == st1["captures"] and st2["replays"] > st1["replays"]
    assert np.array_equal(a.numpy(), got) and torch.equal(a, b2)
    _new(m, ids, 8, guidance_scale=3.0)
    assert e.decode_graph_stats()["captures"] > st2["captures"]
    e.enable_decode_graph(False)
    e.close()


@pytest.mark.parametrize("smp", [None, dict(temperature=0.7, top_k=0, top_p=1.0, repetition_penalty=1.0)], ids=["greedy", "sampled"])
def test_logprobs_raw_is_the_conditional_row_processed_the_guided_scores(gpu_lib, smp):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    got, raws, guided, rec = _host_loop(e, m, ids, NEG["shorter"], N, smp=smp, seed=9, logprobs=True)
    raw_lp, proc_lp, counts = rec
    assert counts == [N, N]
    for t in range(N):
        for r in range(2):
            z, g, i = raws[t][r], guided[t][r], int(got[r, t])
            want_raw = lr.raw(z, i)
            want_proc = lr.log_softmax_at(g, i) if smp is None else lr.processed(g, i, temperature=smp["temperature"])
            assert abs(float(raw_lp[r, t]) - want_raw) <= lr.tolerance(z[i], lr.lse(z))
            scaled = g if smp is None else g / np.float32(smp["temperature"])
            assert abs(float(proc_lp[r, t]) - want_proc) <= lr.tolerance(scaled[i], lr.lse(scaled))
    kw = dict(do_sample=True, seed=9, **smp) if smp else {}
    out = m.generate(ids, max_new_tokens=N, guidance_scale=SCALE, negative_prompt_ids=torch.tensor(NEG["shorter"]), output_logprobs=True,
                     return_dict_in_generate=True, **kw)
    assert np.array_equal(out.sequences[:, ids.shape[1]:].numpy(), got)
    assert torch.equal(out.logprobs, raw_lp) and torch.equal(out.processed_logprobs, proc_lp)
    e.close()


def _cyclic(avoid, k=4):
    """state i allows two thirds of the vocabulary, minus every id `avoid` holds at the positions i mod k, and leads to state i + 1"""
    trans = {}
    for i in range(k):
        out = {int(row[t]) for row in avoid for t in range(i, len(row), k)}
        trans[i] = {t: (i + 1) % k for t in range(V_TINY) if (t * 7 + i) % 3 != 0 and t not in out}
    return trans, TokenFSM(trans, vocab_size=V_TINY)


def test_composition_with_no_repeat_ngram_and_token_fsm(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    neg = NEG["shorter"]
    alone, _, _, _ = _host_loop(e, m, ids, neg, N)
    fsm = _cyclic(alone.tolist())
    p = cr.params(V_TINY, ngram=2)
    both, _, _, _ = _host_loop(e, m, ids, neg, N, p=p, fsm=fsm)
    both_g, _, _, _ = _host_loop(e, m, ids, neg, N, p=p, fsm=fsm, graph=True)
    assert np.array_equal(both, both_g) and not np.array_equal(both, alone)
    for r in range(2):
        row = PROMPT[r] + both[r].tolist()
        bg = list(zip(row[:-1], row[1:]))
        assert len(bg) == len(set(bg)) and fr.walk(fsm[0], both[r]) != DEAD
    out = m.generate(ids, max_new_tokens=N, guidance_scale=SCALE, negative_prompt_ids=torch.tensor(neg), token_fsm=fsm[1], no_repeat_ngram_size=2,
                     return_dict_in_generate=True)
    assert np.array_equal(out.sequences[:, ids.shape[1]:].numpy(), both)
    assert out.fsm_states.tolist() == [fr.walk(fsm[0], both[r]) for r in range(2)]
    kw = dict(guidance_scale=SCALE, negative_prompt_ids=torch.tensor(neg))
    assert np.array_equal(_new(m, ids, N, **kw).numpy(), alone)      # the other stages are off again without their keywords
    e.close()


def test_eos_rewind_takes_both_twins_back_and_mxfp4_batched(gpu_lib):
    _, e, m = _tiny_model(max_batch=2)
    ids = torch.tensor(PROMPT[:1])
    neg = torch.tensor(NEG["longer"][:1])
    kw = dict(guidance_scale=SCALE, negative_prompt_ids=neg)
    free = _new(m, ids, 16, **kw)[0].tolist()
    stop = next(i for i in range(3, 14) if free[i] not in free[:i])
    out = _new(m, ids, 16, eos_token_id=free[stop], pad_token_id=0, **kw)[0].tolist()
    assert out == free[:stop + 1]
    # generate enqueued one step ahead of the EOS and took it back on both rows: `stop` steps behind the prefill
    assert e.kv_lengths(2) == [8 + stop, 11 + stop]
    assert _new(m, ids, 16, **kw)[0].tolist() == free                # the next call is clean
    # a streamer at b = 1 sees the prompt and the conditional row's ids
    class _S:
        def __init__(self): self.got, self.ended = [], False
        def put(self, x): self.got.append(x.view(-1).tolist())
        def end(self): self.ended = True
    s = _S()
    _new(m, ids, 16, streamer=s, **kw)
    assert s.ended and s.got[0] == PROMPT[0] and [t[0] for t in s.got[1:]] == free
    # stopping criteria see the conditional rows alone
    seen = []
    crit = lambda seq, _: (seen.append(tuple(seq.shape)), seq.shape[1] >= 8 + 5)[1]
    assert _new(m, ids, 16, stopping_criteria=[crit], **kw)[0].tolist() == free[:5] and all(sh[0] == 1 for sh in seen)
    # MXFP4 mode 2: the 2-row step of a guided b = 1 call is a batched step
    e.enable_mxfp4_decode(True, batched=True)
    got, _, _, _ = _host_loop(e, m, ids, neg.tolist(), 16)
    assert _new(m, ids, 16, **kw)[0].tolist() == got[0].tolist()
    e.enable_mxfp4_decode(False)
    e.close()


def test_tower_negative_images(gpu_lib):
    cfg, e, m = _tiny_model(max_batch=2, max_seq=256, vision=True)
    img = torch.from_numpy(synth.pixels(1, 56, 3)).to(torch.bfloat16).cuda()
    other = torch.from_numpy(synth.pixels(1, 56, 8)).to(torch.bfloat16).cuda()
    ids = torch.tensor([[3, -200, 17, 18, 19]])
    plain = m.forward(input_ids=ids, images=img, use_cache=True).local_logits.clone()
    S = 4 + e.ntok
    # the twin text-only, as HF's processor runs it (it calls the model without `images`)
    e.encode_stats(reset=True)
    text = m.generate(ids, images=img, max_new_tokens=8, guidance_scale=SCALE, negative_prompt_ids=torch.tensor([[3, 17, 18, 19]]))
    assert e.encode_stats() == dict(calls=1, tiles=1) and e.kv_lengths(2) == [S + 7, 4 + 7]
    # the same question over another picture: one tower pass over both tiles
    e.encode_stats(reset=True)
    vis = m.generate(ids, images=img, max_new_tokens=8, guidance_scale=SCALE, negative_prompt_ids=ids, negative_images=other)
    assert e.encode_stats() == dict(calls=1, tiles=2) and e.kv_lengths(2) == [S + 7, S + 7]
    assert not torch.equal(text, vis)
    # the conditional row of the 2-row ragged prefill is the plain prefill's, to rounding
    out = m._forward_guided(ids, img, dict(scale=SCALE, neg_ids=torch.tensor([[3, 17, 18, 19]]), neg_images=None))
    assert rel(out.local_logits[0], plain[0]) < TOL_DEEP["bf16"]
    got, _, _, _ = _host_loop(e, m, ids, ids.tolist(), 8, images=img, neg_images=other)
    assert np.array_equal(vis[:, ids.shape[1]:].numpy(), got)
    e.close()


def test_abi_refusals_leave_the_cache_untouched(gpu_lib):
    _, e, m = _tiny_model()
    lib = gpu_lib
    ids = torch.tensor(PROMPT)
    out = m._forward_guided(ids, None, dict(scale=SCALE, neg_ids=torch.tensor(NEG["shorter"]), neg_images=None))
    e.set_guidance(2, SCALE)
    lens = e.kv_lengths(4)
    lg = out.local_logits
    tok4 = e.argmax(lg)
    s = _lib.cur_stream()

    def refused(call, frag):
        with pytest.raises(ValueError, match=frag):
            call()
        assert frag in lib.omchat_last_error().decode() and e.kv_lengths(4) == lens

    refused(lambda: e.argmax(lg[:2]), "2b rows")
    refused(lambda: e.argmax(lg[:3]), "2b rows")
    e.set_sampling(2, seed=1)
    refused(lambda: e.sample(lg[:2]), "2b rows")
    e.sampling_off()
    refused(lambda: e.decode_step(tok4[:2]), "2b rows")
    refused(lambda: e.decode_step(tok4[:3]), "2b rows")
    refused(lambda: e.kv_rewind(2, 1), "2b rows")
    refused(lambda: e.beam_begin(1, 2, max_new=4, prompt_len=8), "guidance is on")
    refused(lambda: e.decode_verify(torch.tensor([1, 2, 3])), "guidance is on")
    refused(lambda: e.group_begin(1, 2, prompt_len=8), "guidance is on")
    refused(lambda: e.decode_step_masked(tok4, torch.full((4, 1), 8), torch.ones(4, 12, dtype=torch.long)), "guidance is on")
    refused(lambda: e.masked_decode_begin(torch.full((4, 1), 8), torch.ones(4, 12, dtype=torch.long)), "guidance is on")
    refused(lambda: e.decode_step_masked_next(tok4), "guidance is on")
    with pytest.raises(ValueError, match="max_batch"):
        e.set_guidance(3, SCALE)
    with pytest.raises(ValueError, match="finite"):
        e.set_guidance(2, float("inf"))
    # still on, and in step: a step of 2b rows runs, the rewind takes 2b cache rows back
    nxt, _ = e.decode_step(tok4)
    assert nxt[:2].tolist() == nxt[2:].tolist() and e.kv_lengths(4) == [L + 1 for L in lens]
    e.kv_rewind(4, 1)
    assert e.kv_lengths(4) == lens
    again, _ = e.decode_step(tok4)
    assert torch.equal(again, nxt)
    e.guidance_off()
    e.kv_rewind(2, 1)                                                # off: any row count again
    assert e.kv_lengths(4) == lens[:2] + [L + 1 for L in lens[2:]]
    e.close()
