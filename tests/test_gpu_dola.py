"""GPU: layer-contrastive decoding on the device (omchat_amd/csrc/dola.hip) -- the stage through omchat_op_dola against
tests/dola_ref.py (fp64): the scores within 8 times the deviation of an fp32 numpy evaluation of the same formulas on the same inputs (the bound
of the guidance op, tests/test_gpu_guidance.py), the -inf set and the picked positions exactly, on inputs whose margins tests/test_dola_cpu.py
asserts; its witnesses (tie, strict threshold, underflow, identical candidate, graph replay); then a 4-layer tiny decoder: the context's rows
against the oracle's per-layer hidden rows through the head, the picks, ids and layer record against the fp64 stage applied to the device's OWN
rows at every step (teacher-forced), greedy and sampled, eager and decode graph, log-probs, EOS, dola_layers=None and every refusal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import dola_ref as dr
import logprob_ref as lr
import sampling_ref as sr
from gpu_util import rel, rnd, TOL_DEEP
import oracle
from omchat_amd import synth, _lib
from omchat_amd._lib import check, ptr
from omchat_amd.config import tiny
from omchat_amd.engine import Engine


# ---------------------------------------------------------------------------------------------------------------- the stage alone
def _op(lib, z, b, k, ld, rt, ld_out=None, graph=False):
    """the stage on rows of stride ld, the columns behind V poisoned with NaN (they must not be read as logits) -> (scores [b, V], the
    whole output buffer [b, ld_out], picked [b])"""
    V = z.shape[1]
    ld_out = ld_out or V
    buf = torch.full(((k + 1) * b, ld), float("nan"), dtype=torch.float32)
    buf[:, :V] = torch.from_numpy(z)
    lg = buf.cuda()
    out = torch.full((b, ld_out), 7.0, dtype=torch.float32, device="cuda")
    picked = torch.full((b,), -5, dtype=torch.int32, device="cuda")
    n = int(lib.omchat_op_dola_ws(b, k, V))
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")

    def run():
        check(lib.omchat_op_dola(ptr(lg), ld, V, b, k, float(rt), ptr(out), ld_out, ptr(picked), ptr(ws), n, _lib.cur_stream()))
    if graph:
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            run()
        g.replay()
    else:
        run()
    torch.cuda.synchronize()
    assert torch.equal(lg.cpu().nan_to_num(nan=1e30), buf.nan_to_num(nan=1e30))      # the input rows are never written
    full = out.cpu().numpy()
    return full[:, :V].copy(), full, picked.cpu().numpy()


def _check_op(lib, z, b, k, ld, rt, ld_out=None):
    ref, want = dr.stage(z, b, k, rt)
    dev32, tol = dr.tolerance(z, b, k, rt, want)
    got, full, picked = _op(lib, z, b, k, ld, rt, ld_out)
    V = z.shape[1]
    assert not np.isnan(got).any()
    assert picked.tolist() == want.tolist(), (picked, want)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))          # the filtered set, exactly
    assert (got[~np.isfinite(got)] == -np.inf).all()
    fin = np.isfinite(ref)
    err = float(np.abs(got[fin].astype(np.float64) - ref[fin]).max())
    print(f"dola op b={b} k={k} V={V} ld={ld} rt={rt}: device {err:.3e}, fp32 numpy {dev32:.3e}, bound {tol:.3e}")
    assert err <= tol, (b, k, V, ld, err, dev32, tol)
    assert (full[:, V:] == 7.0).all()                                  # nothing is written behind a row's V ids
    again, _, p2 = _op(lib, z, b, k, ld, rt, ld_out)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32)) and p2.tolist() == picked.tolist()
    return got, picked


@pytest.mark.parametrize("k", dr.OP_K)
@pytest.mark.parametrize("b", dr.OP_B)
@pytest.mark.parametrize("V", sorted(dr.OP_V))
def test_op_dola_equals_ref(gpu_lib, V, b, k):
    _check_op(gpu_lib, dr.op_inputs(b, k, V), b, k, dr.OP_V[V], dr.OP_RT, ld_out=V + (V % 3))


def test_op_tie_between_identical_candidates_goes_to_the_lower_position(gpu_lib):
    z = dr.op_inputs(1, 2, 2049)                                      # rows: final, c0, c1
    jf = int(np.argmax(dr.divergences(z, 1, 2)[0]))
    far, near = z[1 + jf], z[2 - jf]
    rows = np.stack([z[0], near, far, near, far])                     # k = 4: positions 1 and 3 are bit-identical and the maximum
    assert dr.stage(rows, 1, 4, 0.1)[1].tolist() == [1]
    got, _, picked = _op(gpu_lib, rows, 1, 4, 2052, 0.1)
    assert picked.tolist() == [1]
    only, _, _ = _op(gpu_lib, np.stack([z[0], far]), 1, 1, 2052, 0.1)
    assert np.array_equal(got.view(np.uint32), only.view(np.uint32))


def test_op_relative_top_one_keeps_exactly_the_maxima(gpu_lib):
    z = dr.op_inputs(1, 2, 4100).copy()
    top = float(z[0].max()) + 1.0
    keep = [5, 2047, 4099]                                            # the maximum three times, in both tiles and in the scalar tail
    z[0, keep] = top
    got, _, _ = _op(gpu_lib, z, 1, 2, 4103, 1.0)
    assert np.flatnonzero(np.isfinite(got[0])).tolist() == keep       # strict <: an id AT the threshold survives
    assert (got[0][~np.isfinite(got[0])] == -np.inf).all()


def test_op_underflowing_candidate_and_identical_candidate(gpu_lib):
    rng = np.random.default_rng(11)
    f = (rng.standard_normal(2049) * 2).astype(np.float32)
    spread = f.copy(); spread[::2] -= 200.0                           # half of its probabilities underflow in fp32
    spread2 = (f * 30).astype(np.float32)
    z = np.stack([f, spread, spread2])
    assert dr.margins_ok(z, 1, 2, 0.1)
    got, _ = _check_op(gpu_lib, z, 1, 2, 2052, 0.1)
    assert not np.isnan(got).any()
    # a candidate identical to the final row has no divergence from it: the other one is picked, whichever position it has
    other = (rng.standard_normal(2049) * 2).astype(np.float32)
    for rows, want in ((np.stack([f, f, other]), 1), (np.stack([f, other, f]), 0)):
        _, _, picked = _op(gpu_lib, rows, 1, 2, 2049, 0.1)
        assert picked.tolist() == [want] == dr.stage(rows, 1, 2, 0.1)[1].tolist()
    # ... and contrasted with it alone every kept id scores exactly 0
    got, _, _ = _op(gpu_lib, np.stack([f, f]), 1, 1, 2049, 0.1)
    assert np.isfinite(got).any() and (got[np.isfinite(got)] == 0).all()


def test_op_graph_replay_gives_the_eager_bits_and_bad_arguments_are_refused(gpu_lib):
    for b, k, V in ((3, 16, 2049), (1, 1, 4100)):
        z = dr.op_inputs(b, k, V)
        eager, _, p = _op(gpu_lib, z, b, k, dr.OP_V[V], 0.1)
        replay, _, pg = _op(gpu_lib, z, b, k, dr.OP_V[V], 0.1, graph=True)
        assert np.array_equal(eager.view(np.uint32), replay.view(np.uint32)) and p.tolist() == pg.tolist()
    lg, out = torch.zeros(2, 64, device="cuda"), torch.empty(1, 64, device="cuda")
    ws = torch.empty(4096, dtype=torch.uint8, device="cuda")
    for bad in (dict(ld=63), dict(ld_out=63), dict(rt=0.0), dict(rt=1.5), dict(rt=float("nan")), dict(b=0), dict(k=0), dict(k=17), dict(n=8)):
        a = dict(dict(ld=64, b=1, k=1, rt=0.1, ld_out=64, n=4096), **bad)
        with pytest.raises(ValueError):
            check(gpu_lib.omchat_op_dola(ptr(lg), a["ld"], 64, a["b"], a["k"], a["rt"], ptr(out), a["ld_out"], None, ptr(ws), a["n"], _lib.cur_stream()))


# ---------------------------------------------------------------------------------------------------------------- model level
LAYERS_T = 4
PROMPT = [[3, 17, 18, 19, 20, 21, 7, 9], [5, 6, 11, 12, 13, 40, 41, 42]]
SMP = dict(temperature=0.9, top_k=50, top_p=0.9, repetition_penalty=1.3)
N = 4                                                                  # the prefill's pick and 3 decode steps


def _tiny_model(dt="bf16", max_batch=8, seed=22, **kw):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    cfg = tiny(layers_t=LAYERS_T)
    e = Engine(cfg, dtype=dt, max_seq=64, max_batch=max_batch, max_tiles=2, vision=False, **kw)
    e.load_state_dict(synth.state_dict(cfg, seed), strict=False)
    return cfg, e, OmChatQwen2ForCausalLM(cfg.clone(), e)


def _host_loop(e, m, ids, layers, n=N, rt=0.1, norm=False, graph=False, smp=None, seed=5, logprobs=False):
    """prefill + n - 1 decode steps with the stage on; at every pick the device's ids against the fp64 stage (then the argmax, or the CPU
    sampler) applied to the device's own rows -> (ids [b, n], rows per step, scores per step, picked HF layers [b, n], the record)"""
    e.enable_decode_graph(graph)
    b, k = ids.shape[0], len(layers)
    e.set_dola(b, layers, rt, norm)
    out = m.forward(input_ids=ids, use_cache=True)
    lens0 = e.kv_lengths(b)
    hist = [list(r) for r in ids.tolist()]
    if logprobs:
        e.set_logprobs(b, n)
    if smp is not None:
        e.set_sampling(b, seed=seed, seen=hist, **smp)
    else:
        e.sampling_off()
    lg = out.local_logits
    tok = e.sample(lg) if smp is not None else e.argmax(lg)
    got, rows_all, outs, lay = [], [], [], []                          # (outs: the fp64 scores; with logprobs the stage's own fp32 ones)
    for step in range(n):
        rows = e.dola_rows().numpy()
        assert rows.shape == ((k + 1) * b, e.c.t_vocab) and np.isfinite(rows).all()
        assert np.array_equal(lg.cpu().numpy(), rows[:b])               # the logits handed back are the final rows, raw
        ref, picked = dr.stage(rows, b, k, rt)
        ids_ref = []
        for r in range(b):
            l = ref[r].astype(np.float32)
            ids_ref.append(int(np.argmax(ref[r])) if smp is None else
                           sr.sample_row(l, r, step, seed, smp["temperature"], smp["top_k"], smp["top_p"], hist[r], smp["repetition_penalty"]))
        assert tok.tolist() == ids_ref, (step, tok.tolist(), ids_ref)
        assert e.kv_lengths(b) == [L + step for L in lens0]
        if logprobs:
            # the stage's own fp32 scores for the record's comparison (deterministic: the op gives the bits the step's stage gave).  Eager
            # runs only: a pageable host-to-device copy between two replays of a captured sampled step disturbs the next replay (LOG.md)
            dev_out, dev_pick = e.dola(torch.from_numpy(rows).cuda(), b, k, rt)
            assert dev_pick.tolist() == picked.tolist()
            ref = dev_out.cpu().numpy()
        got.append(ids_ref); rows_all.append(rows); outs.append(ref); lay.append([layers[int(p)] for p in picked])
        for r in range(b):
            hist[r].append(ids_ref[r])
        if step < n - 1:
            tok, lg = e.decode_step(tok, want_logits=True)
    assert e.dola_record(b, n).tolist() == np.array(lay).T.tolist()
    rec = e.read_logprobs(b) if logprobs else None
    e.enable_decode_graph(False)
    e.sampling_off(); e.dola_off()
    if logprobs:
        e.logprobs_off()
    return np.array(got).T, rows_all, outs, np.array(lay).T, rec


def _new(m, ids, n, **kw):
    return m.generate(ids, max_new_tokens=n, **kw)[:, ids.shape[1]:]


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "norm"])
@pytest.mark.parametrize("layers", [[0], [1, 3], "high"], ids=["l0", "l13", "high"])
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_rows_equal_the_oracles_hidden_rows_through_the_head(gpu_lib, dt, b, layers, norm):
    cfg, e, m = _tiny_model(dt)
    ids = torch.tensor(PROMPT[:b])
    ls = layers if isinstance(layers, list) else [2]                   # 'high' at N = 4: range(2, 4, 2)
    from omchat_amd import dola
    assert dola.resolve_layers(layers, LAYERS_T) == ls
    got, rows_all, _, _, _ = _host_loop(e, m, ids, ls, norm=norm)
    sd = {k_: rnd(v, dt) for k_, v in synth.state_dict(cfg, 22).items() if k_.startswith(("model.layers", "model.norm", "model.embed", "lm_head"))}
    k = len(ls)
    for r in range(b):
        cache = oracle.KVCache(LAYERS_T)
        feed = ids[r:r + 1]
        for step in range(N):
            h = dr.hidden_rows(oracle, sd["model.embed_tokens.weight"][feed], sd, cfg.text, cache, ls, norm)
            ref = oracle.lm_head(h, sd)                                # [k + 1, V]
            for j in range(k + 1):
                dev_row = torch.from_numpy(rows_all[step][j * b + r])
                assert rel(dev_row, ref[j]) < TOL_DEEP[dt], (step, r, j, rel(dev_row, ref[j]))
            feed = torch.tensor([[int(got[r, step])]])                 # teacher-forced with the device's ids
    e.close()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("smp", [None, SMP], ids=["greedy", "sampled"])
def test_generate_returns_the_loops_ids_and_layers(gpu_lib, smp, graph):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    n = 8
    kw = dict(do_sample=True, seed=77, **SMP) if smp else {}
    free = _new(m, ids, n, **kw)
    lens_free = e.kv_lengths(2)
    rt = 1e-3                                                          # a wide kept set: the contrast, not the final row alone, decides
    got, rows_all, outs, lay, _ = _host_loop(e, m, ids, [1, 3], n=n, rt=rt, graph=graph, smp=smp, seed=77)
    if graph:
        assert e.decode_graph_stats()["replays"] > 0
    e.enable_decode_graph(graph)
    out = m.generate(ids, max_new_tokens=n, dola_layers=[1, 3], dola_relative_top=rt, return_dict_in_generate=True, **kw)
    assert torch.equal(out.sequences[:, :ids.shape[1]], ids)
    assert np.array_equal(out.sequences[:, ids.shape[1]:].numpy(), got)
    assert np.array_equal(out.dola_premature_layers.numpy(), lay)
    # where the contrast's argmax leaves the final row's, the greedy ids leave the plain call's
    moved = [t for t in range(n) if (outs[t].argmax(axis=1) != rows_all[t][:2].argmax(axis=1)).any()]
    print(f"the contrast moves the argmax at steps {moved}; ids equal to the plain call's: {np.array_equal(got, free.numpy())}")
    if smp is None and moved:
        assert not np.array_equal(got, free.numpy())
    # the other graph mode gives the same ids; a call without the keyword, or with None, is the plain call again
    e.enable_decode_graph(not graph)
    assert np.array_equal(_new(m, ids, n, dola_layers=[1, 3], dola_relative_top=rt, **kw).numpy(), got)
    e.enable_decode_graph(False)
    assert torch.equal(_new(m, ids, n, **kw), free) and e.kv_lengths(2) == lens_free
    assert torch.equal(_new(m, ids, n, dola_layers=None, **kw), free) and e.kv_lengths(2) == lens_free
    e.close()


@pytest.mark.parametrize("smp", [None, dict(temperature=0.7, top_k=0, top_p=1.0, repetition_penalty=1.0)], ids=["greedy", "sampled"])
def test_logprobs_raw_is_the_final_row_processed_the_contrast(gpu_lib, smp):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    n = 6
    got, rows_all, outs, lay, rec = _host_loop(e, m, ids, [0, 2], n=n, smp=smp, seed=9, logprobs=True)
    raw_lp, proc_lp, counts = rec
    assert counts == [n, n]
    for t in range(n):
        for r in range(2):
            z, g, i = rows_all[t][r], outs[t][r], int(got[r, t])
            assert abs(float(raw_lp[r, t]) - lr.raw(z, i)) <= lr.tolerance(z[i], lr.lse(z))
            want = lr.log_softmax_at(g, i) if smp is None else lr.processed(g, i, temperature=smp["temperature"])
            scaled = g if smp is None else g / np.float32(smp["temperature"])
            assert abs(float(proc_lp[r, t]) - want) <= lr.tolerance(scaled[i], lr.lse(scaled))
    kw = dict(do_sample=True, seed=9, **smp) if smp else {}
    out = m.generate(ids, max_new_tokens=n, dola_layers=[0, 2], output_logprobs=True, return_dict_in_generate=True, **kw)
    assert np.array_equal(out.sequences[:, ids.shape[1]:].numpy(), got)
    assert torch.equal(out.logprobs, raw_lp) and torch.equal(out.processed_logprobs, proc_lp)
    assert np.array_equal(out.dola_premature_layers.numpy(), lay)
    e.close()


def test_eos_row_records_minus_one_behind_it(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor(PROMPT)
    n = 8
    base = m.generate(ids, max_new_tokens=n, dola_layers=[1, 3], return_dict_in_generate=True)
    new = base.sequences[:, ids.shape[1]:]
    # the first id of row 0 (behind its first) that neither row produced before: the EOS of the second call
    t = next(t for t in range(1, n - 1) if int(new[0, t]) not in new[0, :t].tolist() and int(new[0, t]) not in new[1].tolist())
    eos = int(new[0, t])
    out = m.generate(ids, max_new_tokens=n, dola_layers=[1, 3], return_dict_in_generate=True, eos_token_id=eos, pad_token_id=0)
    got, rec = out.sequences[:, ids.shape[1]:], out.dola_premature_layers
    assert got[0].tolist() == new[0, :t + 1].tolist() + [0] * (n - t - 1) and torch.equal(got[1], new[1])
    assert rec[0, :t + 1].tolist() == base.dola_premature_layers[0, :t + 1].tolist() and rec[0, t + 1:].tolist() == [-1] * (n - t - 1)
    assert torch.equal(rec[1], base.dola_premature_layers[1]) and set(rec[1].tolist()) <= {1, 3}
    # a batch of one whose row ends: the step enqueued ahead is taken back, with its line of the record
    alone = m.generate(ids[:1], max_new_tokens=n, dola_layers=[1, 3])[0, ids.shape[1]:]
    t = next(t for t in range(1, n - 1) if int(alone[t]) not in alone[:t].tolist())
    out = m.generate(ids[:1], max_new_tokens=n, dola_layers=[1, 3], return_dict_in_generate=True, eos_token_id=int(alone[t]))
    assert out.sequences[0, ids.shape[1]:].tolist() == alone[:t + 1].tolist() and out.dola_premature_layers.shape == (1, t + 1)
    assert (e.dola_record(1, t + 2)[0] >= 0).tolist() == [True] * (t + 1) + [False]
    e.close()


def test_generate_refusals_and_value_errors_before_any_work(gpu_lib):
    _, e, m = _tiny_model(max_batch=4)
    ids = torch.tensor(PROMPT)
    _new(m, ids, 2)
    lens = e.kv_lengths(4)
    one = ids[:1]
    for kw in (dict(num_beams=2), dict(guidance_scale=1.5), dict(num_return_sequences=2, do_sample=True), dict(suffixes=[[1, 2], [3]]),
               dict(prompt_lookup_num_tokens=3), dict(reuse_cache=True)):
        with pytest.raises(NotImplementedError, match="dola_layers with"):
            m.generate(one, max_new_tokens=2, dola_layers=[1], **kw)
        assert e.kv_lengths(4) == lens
    with pytest.raises(NotImplementedError, match="padded"):
        m.generate(ids, max_new_tokens=2, dola_layers=[1], attention_mask=torch.tensor([[1] * 8, [1] * 6 + [0] * 2]))
    e.enable_mxfp4_decode(True)
    with pytest.raises(NotImplementedError, match="MXFP4"):
        m.generate(one, max_new_tokens=2, dola_layers=[1])
    e.enable_mxfp4_decode(False)
    e.enable_fp8_decode(True)
    with pytest.raises(NotImplementedError, match="fp8"):
        m.generate(one, max_new_tokens=2, dola_layers=[1])
    e.enable_fp8_decode(False)
    for kw in (dict(dola_layers="middle"), dict(dola_layers=[-1]), dict(dola_layers=[4, 7]), dict(dola_layers=[]), dict(dola_layers=[1], dola_relative_top=0.0),
               dict(dola_layers=[1], dola_relative_top=1.5), dict(dola_layers=[0, 1, 2])):      # (the last: (3 + 1) * 2 rows > max_batch = 4)
        with pytest.raises(ValueError):
            m.generate(ids, max_new_tokens=2, **kw)
        assert e.kv_lengths(4) == lens
    m.generation_config.dola_layers = [1, 3]                          # read from generation_config too
    a = m.generate(one, max_new_tokens=4, return_dict_in_generate=True)
    m.generation_config.dola_layers = None
    assert set(a.dola_premature_layers[0].tolist()) <= {1, 3} and a.dola_premature_layers.shape == (1, 4)
    assert torch.equal(a.sequences[:, 8:], _new(m, one, 4, dola_layers=[1, 3]))
    assert not hasattr(m.generate(one, max_new_tokens=4, output_logprobs=True, return_dict_in_generate=True), "dola_premature_layers")
    e.close()


def test_abi_refusals_leave_the_cache_untouched(gpu_lib):
    _, e, m = _tiny_model(max_batch=4)
    lib = gpu_lib
    ids = torch.tensor(PROMPT[:1])
    plain = _new(m, ids, 3)
    e.set_dola(1, [1, 3])
    out = m.forward(input_ids=ids, use_cache=True)
    lg = out.local_logits
    tok = e.argmax(lg)
    lens = e.kv_lengths(4)

    def refused(call, frag):
        with pytest.raises(ValueError, match=frag):
            call()
        assert frag in lib.omchat_last_error().decode() and e.kv_lengths(4) == lens

    on = "layer-contrastive decoding is on"
    refused(lambda: e.argmax(torch.cat([lg, lg])), on)
    refused(lambda: e.decode_step(torch.cat([tok, tok])), on)
    refused(lambda: e.kv_rewind(2, 1), on)
    refused(lambda: e.beam_begin(1, 2, max_new=4, prompt_len=8), on)
    refused(lambda: e.set_guidance(1, 1.5), on)
    refused(lambda: e.group_begin(1, 2, prompt_len=8), on)
    refused(lambda: e.decode_verify(torch.tensor([1, 2, 3])), on)
    refused(lambda: e.decode_step_masked(tok, torch.full((1, 1), 8), torch.ones(1, 12, dtype=torch.long)), on)
    refused(lambda: e.masked_decode_begin(torch.full((1, 1), 8), torch.ones(1, 12, dtype=torch.long)), on)
    refused(lambda: e.decode_step_masked_next(tok), on)
    emb = torch.zeros(1, 2, 256, dtype=torch.bfloat16, device="cuda")
    refused(lambda: e.prefill_extend(emb, 8), on)
    refused(lambda: e.prefill_suffixes(emb, [2], 8), on)
    refused(lambda: e.prefill(emb, [2], padding_side="left"), on)
    refused(lambda: e.prefill(torch.cat([emb, emb]), [2, 2]), on)
    refused(lambda: e.enable_fp8_decode(True), on)
    refused(lambda: e.enable_mxfp4_decode(True), on)
    for bad, frag in ((dict(b=2, layers=[1, 3]), "rows go through the head"), (dict(layers=[4]), "outside"), (dict(layers=[-1]), "outside"),
                      (dict(layers=[1, 1]), "distinct"), (dict(layers=[]), "candidate layers"), (dict(relative_top=0.0), "relative_top"),
                      (dict(relative_top=1.01), "relative_top")):
        a = dict(dict(b=1, layers=[1, 3], relative_top=0.1), **bad)
        refused(lambda: e.set_dola(a["b"], a["layers"], a["relative_top"]), frag)
    # still on, and in step: a step runs, a rewind takes it back with its line of the record, and the same step gives the same id
    nxt, _ = e.decode_step(tok)
    assert e.kv_lengths(1) == [lens[0] + 1] and (e.dola_record(1, 3)[0] >= 0).tolist() == [True, True, False]
    e.kv_rewind(1, 1)
    assert e.kv_lengths(1) == [lens[0]] and (e.dola_record(1, 3)[0] >= 0).tolist() == [True, False, False]
    again, _ = e.decode_step(tok)
    assert torch.equal(again, nxt)
    # b = 0 restores the plain picks
    e.dola_off()
    assert torch.equal(_new(m, ids, 3), plain)
    # refused at the setter while another mode holds the context
    e.set_guidance(1, 1.5)
    with pytest.raises(ValueError, match="guidance is on"):
        e.set_dola(1, [1])
    e.guidance_off()
    e.enable_mxfp4_decode(True)
    with pytest.raises(ValueError, match="MXFP4"):
        e.set_dola(1, [1])
    e.enable_mxfp4_decode(False)
    e.enable_fp8_decode(True)
    with pytest.raises(ValueError, match="e4m3"):
        e.set_dola(1, [1])
    e.enable_fp8_decode(False)
    e.close()
