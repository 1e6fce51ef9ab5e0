"""GPU: contrastive search on the device (omchat_amd/csrc/contrastive.hip).  The four launches through their test hooks
against tests/contrastive_ref.py (fp64): penalties and probabilities within 8 times the deviation of an fp32 numpy evaluation of the same
formulas on the same inputs (the op bound of tests/test_gpu_guidance.py / test_gpu_dola.py), top-k ids exact with ties, witnesses on every
chunk edge of the plan, inputs never written, nothing read behind V, the same bits twice and in a captured graph.  Then a 4-layer tiny decoder,
text-only and with an image: at every step the device's record against the fp64 stage applied to the device's OWN logits and hidden rows
(teacher-forced), the free-running ids against the reference loop over the CPU oracle (near-tie rule), share_prompt and decode-graph modes,
EOS / max_new_tokens / stopping criterion / streamer, the one-slot commit, the mode rule and every refusal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import contrastive_ref as cr
from gpu_util import DT, TOL_DEEP
import oracle
from omchat_amd import synth, _lib
from omchat_amd._lib import check, ptr
from omchat_amd.config import tiny
from omchat_amd.engine import Engine

ALPHA = cr.ALPHA


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _op_engine():
    """an engine for the op wrappers only (they read nothing of its context but the device)"""
    return Engine(tiny(), dtype="bf16", max_seq=32, max_batch=1, max_tiles=1, vision=False)


def _packed(cand, nb):
    """[k, H] -> the packed x layout of common.h (packed_x_index), rows beyond k poisoned with NaN"""
    k, H = cand.shape
    out = np.full(nb * 16 * H, np.nan, np.float32)
    kk = np.arange(H)
    for r in range(k):
        idx = ((((kk >> 6) * 2 + ((kk >> 5) & 1)) * nb + (r >> 4)) * 64 + (r & 15) + 16 * ((kk >> 3) & 3)) * 8 + (kk & 7)
        out[idx] = cand[r]
    return out


def _penalty(e, hist, cand, dt="bf16", nb=0):
    h = torch.from_numpy(hist).to("cuda", DT[dt])
    c = torch.from_numpy(_packed(cand, nb) if nb else cand).to("cuda", DT[dt])
    h0, c0 = h.clone(), c.clone()
    part, cinv, inv = e.contrastive_penalty(h, c, cand_nb=nb, k=cand.shape[0])
    torch.cuda.synchronize()
    assert torch.equal(h.view(torch.int16), h0.view(torch.int16)) and torch.equal(c.view(torch.int16), c0.view(torch.int16))      # inputs are never written
    part = part.cpu().numpy()
    k = cand.shape[0]
    assert part.shape[0] == cr.plan(hist.shape[0], _cus())[0]
    assert np.isnan(part[:, k:]).all() and not np.isnan(part[:, :k]).any()      # nothing is written for a candidate at or beyond k
    return part, cinv.cpu().numpy(), inv.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- ops
def test_plan_hook_equals_the_restatement(gpu_lib):
    e = _op_engine()
    for L in list(cr.OP_L) + [16, 17, 4096, 16384, 16385, cr.OP_L_TWO_GROUPS]:
        assert e.contrastive_plan(L) == cr.plan(L, _cus()), L
    e.close()


# (the two-group length at H = 128 only: 118 MB of rows at H = 3584 would reach no other branch)
@pytest.mark.parametrize("H,L", [(H, L) for H in cr.OP_H for L in cr.OP_L] + [(128, cr.OP_L_TWO_GROUPS)])
def test_op_penalty_witness_on_every_chunk_edge(gpu_lib, H, L):
    e = _op_engine()
    k = cr.OP_K[L % len(cr.OP_K)]
    worst = 0.0
    for n, row in enumerate(cr.edge_rows(L, _cus(), every=H == 128 and L <= 1025)):      # (both sides of EVERY edge where that is cheap)
        i = n % k
        hist, cand = cr.witness_inputs(H, L, k, row, i)
        ref = cr.penalties(hist, cand)
        dev32, tol = cr.penalty_bound(hist, cand)
        part, cinv, inv = _penalty(e, hist, cand)
        got = part[:, :k].max(axis=0)
        err = float(np.abs(got.astype(np.float64) - ref).max())
        print(f"penalty H={H} L={L} k={k} witness row {row} -> candidate {i}: device {err:.3e}, fp32 numpy {dev32:.3e}, bound {tol:.3e}")
        assert got[i] >= 0.999
        assert err <= tol, (H, L, row, err, dev32, tol)
        # the witness's chunk, and only it, holds the 1 of its candidate
        chunks, rpc = cr.plan(L, _cus())
        assert int(np.argmax(part[:, i])) == row // rpc and (np.delete(part[:, i], row // rpc) < 0.9).all()
        # the norm tables in fp32
        assert np.abs(inv.astype(np.float64) * np.linalg.norm(hist.astype(np.float64), axis=1) - 1).max() < 1e-6
        assert np.abs(cinv[:k].astype(np.float64) * np.linalg.norm(cand.astype(np.float64), axis=1) - 1).max() < 1e-6
        worst = max(worst, err)
        if n == 0:
            again, _, _ = _penalty(e, hist, cand)
            assert np.array_equal(again[:, :k].view(np.uint32), part[:, :k].view(np.uint32))      # the same bits twice
    e.close()


@pytest.mark.parametrize("dt,nb", [("f16", 0), ("bf16", 1), ("f16", 2)])
def test_op_penalty_f16_and_packed_candidates(gpu_lib, dt, nb):
    e = _op_engine()
    H, L, k = 256, 257, 5
    for row in cr.edge_rows(L, _cus())[:4]:
        hist, cand = cr.witness_inputs(H, L, k, row, 3)
        if dt == "f16":
            hist, cand = (torch.from_numpy(a).to(torch.float16).float().numpy() for a in (hist, cand))
            hist[row] = 2.0 * cand[3]
        ref = cr.penalties(hist, cand)
        dev32, tol = cr.penalty_bound(hist, cand)
        part, _, _ = _penalty(e, hist, cand, dt, nb)
        err = float(np.abs(part[:, :k].max(axis=0).astype(np.float64) - ref).max())
        print(f"penalty {dt} packed blocks {nb} witness row {row}: device {err:.3e}, fp32 numpy {dev32:.3e}, bound {tol:.3e}")
        assert err <= tol and part[:, 3].max() >= 0.999
    e.close()


def _topk(e, z, ld, k, row=None, rows=2):
    V = z.shape[0]
    buf = torch.full((rows, ld), float("nan"), dtype=torch.float32)
    r = 0 if row is None else row
    buf[:, :V] = torch.from_numpy(z)[None] - 100.0      # the other rows: the same order, other values
    buf[r, :V] = torch.from_numpy(z)
    lg = buf.cuda()
    sel = None if row is None else torch.tensor([row], dtype=torch.int32, device="cuda")
    ids, probs = e.contrastive_topk(lg, V, k, sel)
    assert torch.equal(lg.cpu().nan_to_num(nan=1e30), buf.nan_to_num(nan=1e30))      # the input rows are never written
    return ids.cpu().numpy(), probs.cpu().numpy()


@pytest.mark.parametrize("k", cr.OP_K)
@pytest.mark.parametrize("V", sorted(cr.OP_V))
def test_op_topk_ids_exact_with_ties_and_probabilities(gpu_lib, V, k):
    e = _op_engine()
    z = cr.logits_inputs(V, k)
    want, ref = cr.topk_probs(z, k)
    dev32, tol = cr.probs_bound(z, k)
    for ld, row in ((cr.OP_V[V], None), (cr.OP_V[V], 1), (V + 4 - V % 4 if V % 4 else V + 4, 1)):      # NaN behind V; a misaligned and an aligned row 1
        ids, probs = _topk(e, z, ld, k, row)
        assert ids.tolist() == want.tolist(), (ld, row, ids, want)
        assert np.isfinite(probs).all()                                      # nothing behind V was read
        err = float(np.abs(probs.astype(np.float64) - ref).max())
        print(f"top-k V={V} ld={ld} row={row} k={k}: device {err:.3e}, fp32 numpy {dev32:.3e}, bound {tol:.3e}")
        assert err <= tol, (V, ld, k, err, dev32, tol)
        again = _topk(e, z, ld, k, row)
        assert again[0].tolist() == ids.tolist() and np.array_equal(again[1].view(np.uint32), probs.view(np.uint32))
    e.close()


def test_op_topk_all_equal_row_and_bad_arguments(gpu_lib):
    e = _op_engine()
    ids, probs = _topk(e, np.zeros(4100, np.float32), 4103, 16)
    assert ids.tolist() == list(range(16)) and np.allclose(probs, 1 / 4100, rtol=1e-6)
    z = np.full(2049, -np.inf, np.float32); z[[2048, 5]] = 1.0
    ids, probs = _topk(e, z, 2052, 4)
    assert ids.tolist() == [5, 2048, 0, 1] and probs.tolist() == [0.5, 0.5, 0.0, 0.0]
    lg = torch.zeros(1, 64, device="cuda")
    for bad in (dict(k=0), dict(k=17), dict(V=8, k=9), dict(ld=63)):
        a = dict(dict(V=64, k=2, ld=64), **bad)
        with pytest.raises(ValueError):
            e.contrastive_topk(lg.as_strided((1, 64), (a["ld"], 1)), a["V"], a["k"])
    e.close()


def test_op_select_commits_and_the_appended_row_is_seen(gpu_lib):
    e = _op_engine()
    H, L, k = 128, 65, 5
    hist, cand = cr.witness_inputs(H, L, k, 0, 0)
    cap = torch.zeros(L + 1, H, dtype=torch.bfloat16, device="cuda")
    cap[:L] = torch.from_numpy(hist).to(torch.bfloat16)
    c = torch.from_numpy(cand).to("cuda", torch.bfloat16)
    part, cinv, inv = e.contrastive_penalty(cap[:L], c)
    inv_cap = torch.zeros(L + 1, dtype=torch.float32, device="cuda"); inv_cap[:L] = inv
    ids = torch.tensor([40, 41, 42, 43, 44], dtype=torch.int32, device="cuda")
    p = np.array([0.05, 0.30, 0.20, 0.30, 0.15], np.float32)
    probs = torch.from_numpy(p).cuda()
    pen = cr.penalties(hist, cand)
    want, margin = cr.pick(p, pen, ALPHA)
    assert margin > 1e-3 and want != 0                                       # candidate 0 is the witness: the likeliest unpenalised id wins
    out = e.contrastive_select(part, k, ALPHA, ids, probs, cinv, cand=c, hist=cap, inv=inv_cap, n_hist=L, eos=[43, 40 + want])
    torch.cuda.synchronize()
    rec = cs_unpack(out["rec"], k)
    assert rec["pick"].tolist() == [want] and rec["token"].tolist() == [40 + want] and rec["ids"][0].tolist() == [40, 41, 42, 43, 44]
    assert np.array_equal(rec["probs"][0], p) and np.abs(rec["penalties"][0].astype(np.float64) - pen).max() <= cr.penalty_bound(hist, cand)[1]
    assert rec["chunks"].tolist() == [part.shape[0]] and rec["rows"].tolist() == [L]
    assert out["parents"].tolist() == [want] * k and out["sel"].tolist() == [want] and out["token"].tolist() == [40 + want] and out["done"].tolist() == [1]
    assert torch.equal(cap[L].view(torch.int16), c[want].view(torch.int16)) and torch.equal(cap[:L].cpu(), torch.from_numpy(hist).to(torch.bfloat16))
    assert float(inv_cap[L]) == float(cinv[want])
    # the row appended by the previous step is a row of the next penalty: its own candidate finds it
    part2, _, _ = e.contrastive_penalty(cap, c, inv=inv_cap)
    got2 = part2.cpu().numpy()[:, :k].max(axis=0)
    assert got2[want] >= 0.999 and int(np.argmax(part2.cpu().numpy()[:, want])) == cr.plan(L + 1, _cus())[0] - 1
    # ties go to the lower rank; no EOS, not the last: done = 0; `last` sets it
    flat = torch.full((1, 16), 0.25, dtype=torch.float32, device="cuda")
    same = torch.full((k,), 0.2, dtype=torch.float32, device="cuda")
    o = e.contrastive_select(flat, k, ALPHA, ids, same, cinv)
    assert o["sel"].tolist() == [0] and o["done"].tolist() == [0]
    assert e.contrastive_select(flat, k, ALPHA, ids, same, cinv, last=True)["done"].tolist() == [1]
    with pytest.raises(ValueError):
        e.contrastive_select(flat, 17, ALPHA, ids, same, cinv)
    e.close()


def cs_unpack(rec, k):
    from omchat_amd.contrastive import unpack_record
    return unpack_record(rec.cpu().numpy(), k)


def test_op_graph_replay_gives_the_eager_bits(gpu_lib):
    e = _op_engine()
    H, L, k, V = 128, 257, 5, 2049
    hist, cand = cr.witness_inputs(H, L, k, 128, 2)
    h = torch.from_numpy(hist).to("cuda", torch.bfloat16)
    c = torch.from_numpy(cand).to("cuda", torch.bfloat16)
    z = torch.from_numpy(cr.logits_inputs(V, k)).cuda().view(1, V)
    chunks, _ = e.contrastive_plan(L)
    lib = gpu_lib
    ws = torch.empty(int(lib.omchat_op_contrastive_topk_ws(V)), dtype=torch.uint8, device="cuda")

    def run():
        part = torch.zeros(chunks, 16, device="cuda"); cinv = torch.zeros(16, device="cuda"); inv = torch.zeros(L, device="cuda")
        ids = torch.zeros(k, dtype=torch.int32, device="cuda"); probs = torch.zeros(k, device="cuda")
        rec = torch.zeros(52, dtype=torch.int32, device="cuda")
        def go():
            check(lib.omchat_op_contrastive_topk(ptr(z), V, None, V, k, ptr(ids), ptr(probs), ptr(ws), _lib.cur_stream()))
            check(lib.omchat_op_contrastive_penalty(_lib.BF16, ptr(h), ptr(inv), 1, L, H, ptr(c), 0, k, ptr(part), ptr(cinv), _lib.cur_stream()))
            check(lib.omchat_op_contrastive_select(_lib.BF16, ptr(part), chunks, k, ALPHA, ptr(ids), ptr(probs), ptr(cinv), None, 0, 0, None, None, 0,
                                                   None, 0, 0, ptr(rec), None, None, None, None, _lib.cur_stream()))
        return go, (part, cinv, inv, ids, probs, rec)
    go, eager = run()
    go()
    torch.cuda.synchronize()
    go2, replay = run()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(g, stream=s):
        go2()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, replay):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert cs_unpack(eager[5], k)["pick"][0] >= 0 and eager[2].min() > 0
    e.close()


# ---------------------------------------------------------------------------------------------------------------- model level
K, NEW = cr.TINY_K, cr.TINY_NEW
PROMPT = cr.TINY_PROMPT
IMG_PROMPT = [3, -200, 17, 18, 19, 20, 21, 7, 9]
VERIFY_BOUND = {"bf16": 8e-3, "f16": 1.2e-3}      # tests/test_gpu_lookup.py: rows of a batched step against batch-1 steps, max |logit| difference


def _tiny_model(dt="bf16", max_batch=8, vision=False, max_seq=96, **kw):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    cfg = tiny(layers_t=cr.TINY_LAYERS)
    e = Engine(cfg, dtype=dt, max_seq=max_seq, max_batch=max_batch, max_tiles=2, vision=vision, **kw)
    e.load_state_dict(synth.state_dict(cfg, cr.TINY_SEED), strict=False)
    return cfg, e, OmChatQwen2ForCausalLM(cfg.clone(), e)


def _img():
    return torch.from_numpy(synth.pixels(1, 56, 3)).cuda()


def _new(m, ids, n=NEW, **kw):
    return m.generate(ids, max_new_tokens=n, **kw)[0, ids.shape[1]:].tolist()


def _cs(m, ids, n=NEW, k=K, **kw):
    return _new(m, ids, n, penalty_alpha=ALPHA, top_k=k, **kw)


def _host_loop(e, m, ids, images=None, k=K, n=NEW, share=False, graph=False, dt="bf16"):
    """the engine calls generate() makes, with the device's own logits and hidden rows read back at every step: the record against the fp64
    stage on them.  -> (ids, near ties, history rows at the end, the fp64 top-two score margin of every pick, the trace: per step the
    candidates' ids, the record's probabilities and penalties, the candidates' hidden rows and the pick)"""
    e.enable_decode_graph(graph)
    e.sampling_off()
    e.set_contrastive(k, ALPHA, n, share)
    out = m.forward(input_ids=ids, images=images, use_cache=True)
    P = e.kv_lengths(1)[0]
    z = out.local_logits[0].cpu().numpy()
    cand = e.contrastive_step(out.local_logits)
    assert cand.tolist()[k] == -1 and e.kv_lengths(k) == [P] * k
    hist, inv, _ = e.contrastive_rows(0, P, want_cand=False)
    assert np.abs(inv.double().numpy() * np.linalg.norm(hist.double().numpy(), axis=1) - 1).max() < 1e-6
    hist = hist.float().numpy()
    got, near, margins, trace = [], 0, [], []
    for t in range(n):
        want_ids, want_p = cr.topk_probs(z, k)
        assert cand.tolist()[:k] == want_ids.tolist(), (t, cand.tolist(), want_ids)
        _, lg = e.decode_step(cand[:k], want_logits=True)
        cand = e.contrastive_step(lg)
        rec = e.contrastive_record(t + 1)
        h_all, inv_all, rows = e.contrastive_rows(0, P + t + 1)
        rows = rows.float().numpy()
        assert np.array_equal(h_all[:P + t].float().numpy(), hist)                                 # the history is only appended to
        assert rec["ids"][t].tolist() == want_ids.tolist() and rec["rows"][t] == P + t
        p_tol = cr.probs_bound(z, k)[1]
        assert np.abs(rec["probs"][t].astype(np.float64) - want_p).max() <= p_tol
        pen = cr.penalties(hist, rows)
        pen_tol = cr.penalty_bound(hist, rows)[1]
        err = float(np.abs(rec["penalties"][t].astype(np.float64) - pen).max())
        assert err <= pen_tol, (t, err, pen_tol)
        want, margin = cr.pick(want_p, pen, ALPHA)
        margins.append(margin)
        i = int(rec["pick"][t])
        if i != want:                                                     # only where the two best scores are closer than the ops may deviate
            assert margin < 2 * ((1 - ALPHA) * p_tol + ALPHA * pen_tol), (t, i, want, margin)
            near += 1
        assert rec["token"][t] == want_ids[i] == cand.tolist()[k]
        assert np.array_equal(h_all[P + t].float().numpy(), rows[i]) and abs(float(inv_all[P + t]) * np.linalg.norm(rows[i].astype(np.float64)) - 1) < 1e-6
        assert e.kv_lengths(k) == [P + t + 1] * k
        assert int(e.contrastive_done[0]) == (1 if t == n - 1 else 0)
        got.append(int(want_ids[i]))
        trace.append(dict(ids=want_ids.tolist(), probs=rec["probs"][t].astype(np.float64), pens=rec["penalties"][t].astype(np.float64), rows=rows, pick=i))
        hist = np.concatenate([hist, rows[i][None]])
        z = lg[i].cpu().numpy()
    e.group_end(); e.contrastive_off()
    e.enable_decode_graph(False)
    return got, near, hist, margins, trace


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("share", [False, True], ids=["fork", "share"])
@pytest.mark.parametrize("image", [False, True], ids=["text", "image"])
def test_record_equals_the_fp64_stage_on_the_devices_own_rows(gpu_lib, image, share, graph):
    cfg, e, m = _tiny_model(vision=image)
    ids = torch.tensor([IMG_PROMPT if image else PROMPT])
    img = _img() if image else None
    got, near, hist, _, _ = _host_loop(e, m, ids, img, share=share, graph=graph)
    print(f"teacher-forced image={image} share={share} graph={graph}: ids {got}, near ties {near}")
    assert hist.shape[0] == (len(IMG_PROMPT) - 1 + 16 if image else len(PROMPT)) + NEW      # image rows included
    if graph:
        assert e.decode_graph_stats()["replays"] > 0
    e.enable_decode_graph(graph)
    out = m.generate(ids, images=img, max_new_tokens=NEW, penalty_alpha=ALPHA, top_k=K, share_prompt=share, return_dict_in_generate=True)
    assert out.sequences[0, ids.shape[1]:].tolist() == got and torch.equal(out.sequences[:, :ids.shape[1]], ids)
    assert out.contrastive_ranks.shape == (1, NEW) and out.degeneration_penalties.shape == (1, NEW)
    if not image:
        assert any(r > 0 for r in out.contrastive_ranks[0].tolist())      # (tests/test_contrastive_cpu.py asserts it of the reference on this prompt)
    e.enable_decode_graph(False)
    e.close()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _same_path(base, other, margins, what):
    """two traces of one search: while the ids agree the two runs scored the same candidates, so the score of a candidate differs between
    them by at most dev = (1 - alpha) |dp| + alpha |dpen| as MEASURED on that step, and the pick may differ only where the base run's two
    best scores are closer than 2 dev.  -> the number of steps compared exactly"""
    exact = 0
    for t, (a, o) in enumerate(zip(base, other)):
        assert a["ids"] == o["ids"], (what, t)
        dev = (1 - ALPHA) * float(np.abs(a["probs"] - o["probs"]).max()) + ALPHA * float(np.abs(a["pens"] - o["pens"]).max())
        if margins[t] > 2 * dev:
            assert a["pick"] == o["pick"], (what, t, margins[t], dev)
            exact += 1
        else:
            print(f"{what}: near tie at {t} (margin {margins[t]:.3e}, measured score deviation {dev:.3e})")
        if a["pick"] != o["pick"]:
            break                                                          # behind a near tie the two runs are different searches
    return exact


@pytest.mark.parametrize("image", [False, True], ids=["text", "image"])
def test_free_running_against_the_oracle_and_between_the_forms(gpu_lib, image):
    dt = "bf16"
    cfg, e, m = _tiny_model(dt, vision=image)
    ids = torch.tensor([IMG_PROMPT if image else PROMPT])
    img = _img() if image else None
    sd = {k_: torch.from_numpy(v_).to(DT[dt]).float() for k_, v_ in synth.state_dict(cfg, cr.TINY_SEED).items()}
    model = cr.oracle_model(oracle, sd, cfg, ids, None if img is None else img.float().cpu())
    greedy = _new(m, ids, images=img)
    base, _, hist, margins, trace = _host_loop(e, m, ids, img)
    assert _cs(m, ids, images=img) == base
    print(f"device    {base}\ngreedy    {greedy}")
    assert base != greedy                                                  # the asserted prompt: contrastive search leaves the greedy ids
    # ---- against the CPU oracle, along the device's own ids.  The history rows behind the prefill (image rows included) and every
    # candidate's hidden row against the oracle's post-final-norm rows, within the project's bound for several layers
    H0, z = model([])
    P = H0.shape[0]
    assert hist.shape[0] == P + NEW
    worst_rows = max(_rel(hist[j], H0[j]) for j in range(P))
    assert worst_rows < TOL_DEEP[dt], worst_rows
    # ... and the pick: the oracle scores the device's candidates; a device score deviates from the oracle's by at most
    # dev = (1 - alpha) |dp| + alpha |dpen| as measured on that step, so the picks may differ only where the oracle's two best scores are
    # closer than 2 dev -- and most steps must be farther apart than that, so that they are compared exactly
    H_ctx, exact, worst_dev = H0, 0, 0.0
    for t, st in enumerate(trace):
        want_ids, _ = cr.topk_probs(z, K)
        x = z.astype(np.float64)
        p_all = np.exp(x - x.max()); p_all /= p_all.sum()
        if sorted(want_ids.tolist()) != sorted(st["ids"]):                 # the k-th and (k + 1)-th logits closer than the device's deviate
            print(f"oracle: step {t}: candidate sets differ ({want_ids.tolist()} against {st['ids']})")
        hs, zs = zip(*[(lambda o: (o[0][-1], o[1]))(model(base[:t] + [c])) for c in st["ids"]])
        for i in range(K):
            r = _rel(st["rows"][i], hs[i])
            worst_rows = max(worst_rows, r)
            assert r < TOL_DEEP[dt], (t, i, r)
        p_or, pen_or = p_all[st["ids"]], cr.penalties(H_ctx, np.stack(hs))
        dev = (1 - ALPHA) * float(np.abs(st["probs"] - p_or).max()) + ALPHA * float(np.abs(st["pens"] - pen_or).max())
        worst_dev = max(worst_dev, dev)
        want, margin = cr.pick(p_or, pen_or, ALPHA)
        print(f"oracle: step {t}: margin {margin:.3e}, measured score deviation {dev:.3e}, picks {want} / {st['pick']}")
        if margin > 2 * dev:
            assert st["pick"] == want, (t, margin, dev)
            exact += 1
        H_ctx = np.concatenate([H_ctx, hs[st["pick"]][None]])
        z = zs[st["pick"]]
    print(f"oracle: {exact} of {NEW} steps compared exactly; rows within {worst_rows:.3e} (bound {TOL_DEEP[dt]}), scores within {worst_dev:.3e}")
    assert exact > NEW // 2
    # ---- the same search for every way to run it: the decode graph replays the eager launches; the shared-prompt attention sums a row's
    # keys in another order than the forked rows' attention, so its rows may differ in the last bits
    for graph in (False, True):
        for share in (False, True):
            if not graph and not share:
                continue
            got, _, _, _, tr = _host_loop(e, m, ids, img, share=share, graph=graph)
            what = f"graph={graph} share={share}"
            n_exact = _same_path(trace, tr, margins, what)
            print(f"{what}: {n_exact} steps compared exactly, ids {'equal' if got == base else 'differ'}")
            if got == base:
                assert n_exact > NEW // 2                                  # (a run that left the base run did so at a measured near tie)
            if not share:
                assert got == base and n_exact == NEW                      # the graph replays the eager launches: the same bits
            e.enable_decode_graph(graph)
            assert _cs(m, ids, images=img, share_prompt=share) == got
            e.enable_decode_graph(False)
    assert _new(m, ids, images=img) == greedy
    e.close()


def test_f16_and_k16_and_mxfp4_batched(gpu_lib):
    cfg, e, m = _tiny_model("f16", max_batch=16)
    ids = torch.tensor([PROMPT])
    got, near, _, _, _ = _host_loop(e, m, ids, k=16, n=5, dt="f16")
    assert _cs(m, ids, 5, k=16) == got
    got2, _, _, _, _ = _host_loop(e, m, ids, k=2, n=5, share=True, dt="f16")
    assert _cs(m, ids, 5, k=2, share_prompt=True) == got2
    e.close()
    cfg, e, m = _tiny_model("bf16")
    e.enable_mxfp4_decode(True, batched=True)
    got, near, _, _, _ = _host_loop(e, m, ids, n=5)
    assert _cs(m, ids, 5) == got
    e.enable_mxfp4_decode(False)
    e.close()


def test_eos_max_new_stopping_criterion_and_streamer(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor([PROMPT])
    base = _cs(m, ids)
    assert len(base) == NEW and _cs(m, ids, 3) == base[:3] and _cs(m, ids, 1) == base[:1]
    t = next(t for t in range(1, NEW - 1) if base[t] not in base[:t])
    assert _cs(m, ids, eos_token_id=base[t]) == base[:t + 1]
    assert _cs(m, ids, eos_token_id=[999999, base[t]]) == base[:t + 1]

    class Stop:
        def __call__(self, seq, scores):
            return seq.shape[1] >= len(PROMPT) + 4
    assert _cs(m, ids, stopping_criteria=[Stop()]) == base[:4]

    class Streamer:
        def __init__(self): self.got, self.ended = [], False
        def put(self, t): self.got.append(t.view(-1).tolist())
        def end(self): self.ended = True
    s = Streamer()
    assert _cs(m, ids, 6, streamer=s) == base[:6]
    assert s.ended and s.got[0] == PROMPT and [x[0] for x in s.got[1:]] == base[:6]
    # the plain call afterwards is the plain call
    m.generation_config.penalty_alpha, m.generation_config.top_k = ALPHA, K      # read from generation_config too
    assert _new(m, ids) == base
    m.generation_config.penalty_alpha, m.generation_config.top_k = None, 50
    assert _new(m, ids) != base
    e.close()


@pytest.mark.parametrize("share", [False, True], ids=["fork", "share"])
def test_one_slot_commit_leaves_row_0_with_the_generated_sequence(gpu_lib, share):
    _, e, m = _tiny_model()
    ids = torch.tensor([PROMPT])
    n = 7
    gen = _cs(m, ids, n, share_prompt=share)
    assert e.kv_lengths(1) == [len(PROMPT) + n]                             # every emitted id is cached
    e.kv_rewind(1, 1)
    _, lg = e.decode_step(torch.tensor([gen[-1]]), want_logits=True)         # a plain step on row 0 over the committed slots
    torch.cuda.synchronize()
    fresh = m.forward(input_ids=torch.tensor([PROMPT + gen]), use_cache=True).local_logits
    d = float((lg[0] - fresh[0]).abs().max())
    print(f"share={share}: plain step over the committed slots against a fresh prefill: max |logit diff| {d:.3e} (bound {VERIFY_BOUND['bf16']})")
    assert d < VERIFY_BOUND["bf16"]
    e.close()


def test_mode_rule_other_values_give_the_plain_calls_ids(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor([PROMPT])
    greedy = _new(m, ids)
    lens = e.kv_lengths(1)
    for kw in (dict(penalty_alpha=None, top_k=4), dict(penalty_alpha=0, top_k=4), dict(penalty_alpha=0.0, top_k=4), dict(penalty_alpha=ALPHA, top_k=1),
               dict(penalty_alpha=-0.5, top_k=4), dict(top_k=4)):
        assert _new(m, ids, **kw) == greedy and e.kv_lengths(1) == lens, kw
    smp = dict(do_sample=True, seed=5, temperature=0.9, top_k=4)
    assert _new(m, ids, penalty_alpha=ALPHA, **smp) == _new(m, ids, **smp)
    assert _new(m, ids, penalty_alpha=ALPHA, top_k=4, num_beams=2) == _new(m, ids, num_beams=2)
    e.close()


def test_generate_refusals_before_any_work(gpu_lib):
    _, e, m = _tiny_model(max_batch=4)
    ids = torch.tensor([PROMPT])
    _new(m, ids, 2)
    lens = e.kv_lengths(4)
    from omchat_amd.fsm import TokenFSM
    cs = dict(penalty_alpha=ALPHA, top_k=4)
    two = torch.tensor([PROMPT, PROMPT])
    for kw in (dict(num_return_sequences=2), dict(suffixes=[[1, 2], [3]]), dict(prompt_lookup_num_tokens=3), dict(reuse_cache=True),
               dict(guidance_scale=1.5), dict(dola_layers=[1]), dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[5]]), dict(min_new_tokens=2, eos_token_id=5),
               dict(repetition_penalty=1.2), dict(output_logprobs=True, return_dict_in_generate=True),
               dict(token_fsm=TokenFSM({0: {5: 0, 6: 0}}, 320)),
               dict(attention_mask=torch.tensor([[1] * 6 + [0] * 2]))):
        with pytest.raises(NotImplementedError, match="contrastive search"):
            m.generate(ids, max_new_tokens=2, **cs, **kw)
        assert e.kv_lengths(4) == lens, kw
    with pytest.raises(NotImplementedError, match="b > 1"):
        m.generate(two, max_new_tokens=2, **cs)
    e.enable_mxfp4_decode(True)
    with pytest.raises(NotImplementedError, match="MXFP4"):
        m.generate(ids, max_new_tokens=2, **cs)
    e.enable_mxfp4_decode(False)
    e.enable_fp8_kv(True)
    with pytest.raises(NotImplementedError, match="e4m3"):
        m.generate(ids, max_new_tokens=2, **cs)
    e.enable_fp8_kv(False)
    e.enable_fp8_prefill(True)
    with pytest.raises(NotImplementedError, match="fp8 x fp8"):
        m.generate(ids, max_new_tokens=2, **cs)
    e.enable_fp8_prefill(False)
    for kw, frag in ((dict(penalty_alpha=1.5, top_k=4), "penalty_alpha"), (dict(penalty_alpha=ALPHA, top_k=5), "top_k=5"),
                     (dict(penalty_alpha=ALPHA, top_k=17), "top_k=17"), (dict(penalty_alpha=ALPHA, top_k=4, eos_token_id=list(range(9))), "eos_token_id"), (dict(penalty_alpha=ALPHA, top_k=4, max_new_tokens=96 - len(PROMPT) + 1), "max_seq")):
        with pytest.raises(ValueError, match=frag):
            m.generate(ids, **dict(dict(max_new_tokens=2), **kw))
        assert e.kv_lengths(4) == lens, kw
    assert m.generation_config.top_k == 50                                # HF's default: the message names the cap
    with pytest.raises(ValueError, match="default to 50"):
        m.generate(ids, max_new_tokens=2, penalty_alpha=ALPHA)
    assert e.kv_lengths(4) == lens
    assert len(_cs(m, ids, 3)) == 3                                          # and the mode still runs
    e.close()


def test_abi_refusals_leave_the_state_untouched(gpu_lib):
    _, e, m = _tiny_model(max_batch=4)
    lib = gpu_lib
    ids = torch.tensor([PROMPT])
    plain = _new(m, ids, 3)
    base = _cs(m, ids, 3)
    P = len(PROMPT)

    def refused(call, frag):
        with pytest.raises(ValueError, match=frag):
            call()
        assert frag in lib.omchat_last_error().decode()

    # the setter's own refusals, while another mode holds the context or for bad values: nothing changes
    for bad, frag in ((dict(k=1), "top_k"), (dict(k=5), "top_k"), (dict(k=17), "top_k"), (dict(alpha=0.0), "penalty_alpha"), (dict(alpha=1.01), "penalty_alpha"),
                      (dict(max_new=0), "max_new"), (dict(eos=list(range(9))), "eos")):
        a = dict(dict(k=4, alpha=ALPHA, max_new=8, eos=[]), **bad)
        refused(lambda: e.set_contrastive(a["k"], a["alpha"], a["max_new"], False, a["eos"]), frag)
    for on, off, frag in ((lambda: e.set_guidance(1, 1.5), e.guidance_off, "guidance is on"), (lambda: e.set_dola(1, [1]), e.dola_off, "layer-contrastive"),
                          (lambda: e.set_logprobs(1, 4), e.logprobs_off, "logprobs are on"),
                          (lambda: e.set_sampling(1, seed=1), e.sampling_off, "sampling is on"),
                          (lambda: e.enable_mxfp4_decode(True), lambda: e.enable_mxfp4_decode(False), "MXFP4"),
                          (lambda: e.enable_fp8_kv(True), lambda: e.enable_fp8_kv(False), "e4m3"),
                          (lambda: e.enable_fp8_prefill(True), lambda: e.enable_fp8_prefill(False), "fp8 x fp8")):
        on()
        refused(lambda: e.set_contrastive(4, ALPHA, 8), frag)
        off()
    # ... a beam search, a token FSM, constraints, a sampled group
    from omchat_amd.fsm import TokenFSM
    m.forward(input_ids=ids, use_cache=True)
    e.load_token_fsm(TokenFSM({0: {5: 0, 6: 0}}, 320))
    for on, off, frag in ((lambda: e.token_fsm_begin(1, 0, 4), e.token_fsm_off, "token FSM is on"),
                          (lambda: e.set_constraints(1, [PROMPT], 4, no_repeat_ngram_size=2), e.constraints_off, "constraints are on"),
                          (lambda: e.group_begin(1, 2, prompt_len=len(PROMPT), share=True), e.group_end, "sampled group"),
                          (lambda: e.beam_begin(1, 2, max_new=4, prompt_len=len(PROMPT)), lambda: m.forward(input_ids=ids, use_cache=True), "beam search is active")):
        on()
        lens_on = e.kv_lengths(4)
        refused(lambda: e.set_contrastive(4, ALPHA, 8), frag)
        assert e.kv_lengths(4) == lens_on
        off()
    e.load_token_fsm(None)
    assert _new(m, ids, 3) == plain
    # while the mode is on
    e.set_contrastive(4, ALPHA, 8)
    on = "contrastive search is on"
    emb = torch.zeros(1, 2, 256, dtype=torch.bfloat16, device="cuda")
    refused(lambda: e.prefill(torch.cat([emb, emb]), [2, 2]), on)
    refused(lambda: e.prefill(emb, [2], padding_side="left"), on)
    refused(lambda: e.prefill(torch.zeros(1, 90, 256, dtype=torch.bfloat16, device="cuda"), [90]), "exceed max_seq")
    refused(lambda: e.contrastive_step(torch.zeros(1, 320, device="cuda")), "no b = 1 prefill")
    out = m.forward(input_ids=ids, use_cache=True)
    lens = e.kv_lengths(4)
    tok = torch.tensor([5], dtype=torch.int32, device="cuda")

    def still(call, frag):
        refused(call, frag)
        assert e.kv_lengths(4) == lens

    still(lambda: e.decode_step(tok), on)                                    # before the fork no step runs
    still(lambda: e.contrastive_step(torch.zeros(4, 320, device="cuda")), "rows = 1")
    still(lambda: e.beam_begin(1, 2, max_new=4, prompt_len=P), on)
    still(lambda: e.set_guidance(1, 1.5), on)
    still(lambda: e.set_dola(1, [1]), on)
    still(lambda: e.set_logprobs(1, 4), on)
    still(lambda: e.set_sampling(1, seed=1), on)
    still(lambda: e.set_constraints(1, [PROMPT], 4, no_repeat_ngram_size=2), on)
    still(lambda: e.token_fsm_begin(1, 0, 4), on)                            # (refused before it looks for a table)
    still(lambda: e.group_begin(1, 2, prompt_len=P), on)
    still(lambda: e.decode_verify(torch.tensor([1, 2, 3])), on)
    still(lambda: e.decode_step_masked(tok, torch.full((1, 1), P), torch.ones(1, 12, dtype=torch.long)), on)
    still(lambda: e.masked_decode_begin(torch.full((1, 1), P), torch.ones(1, 12, dtype=torch.long)), on)
    still(lambda: e.prefill_extend(emb, P), on)
    still(lambda: e.prefill_suffixes(emb, [2], P), on)
    still(lambda: e.kv_rewind(1, 1), on)
    cand = e.contrastive_step(out.local_logits)
    lens = e.kv_lengths(4)
    assert lens == [P] * 4
    still(lambda: e.decode_step(tok), on)                                    # ... and behind it only k-row steps
    still(lambda: e.contrastive_step(out.local_logits), "rows = 1")
    still(lambda: e.contrastive_step(torch.zeros(4, 320, device="cuda")), "one k-row decode step")
    # still in step: the run goes on and gives the ids of generate()
    got = []
    for t in range(3):
        _, lg = e.decode_step(cand[:4], want_logits=True)
        cand = e.contrastive_step(lg)
        got.append(cand.tolist()[4])
    assert got == base
    e.group_end(); e.contrastive_off()
    assert _new(m, ids, 3) == plain
    e.close()
