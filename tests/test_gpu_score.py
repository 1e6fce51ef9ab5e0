"""GPU: teacher-forced scoring.  The op -- the MFMA GEMM with the EPI_LSE epilogue and its finishing kernel
(omchat_op_lse_label) -- against fp64 on the CPU from the same 16-bit inputs, and forward(labels=...) / score() of a tiny model against the
existing path (prefill's hidden rows through Engine.lm_head, softmax in fp64) and against the reference's own forward
(tests/golden/score_tiny.npz).  Every comparison prints `SCERR name err tol`.

Op tolerance (tests/score_ref.py: op_tolerance): the products of 16-bit inputs are exact in fp32, so only the summation differs:
2 K 2^-24 max_n sum_k |a_k w_nk| (worst-case fp32 summation, for the logit and for the log-sum-exp) + logprob_ref.tolerance(x_id, lse)."""
import ctypes as C
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import logprob_ref as lr
import score_ref as sf
from conftest import golden
from gpu_util import CODE, DT, dev
from omchat_amd import synth, _lib
from omchat_amd._lib import check, ptr, cur_stream
from omchat_amd.config import tiny
from omchat_amd.engine import Engine

IGN = -100


# ---------------------------------------------------------------------------------------------------------------- the op
def _op(lib, dt, a, w, labels, want_lse=True):
    """a [M, K], w [N, K] device 16-bit, labels list -> (logprob, lse|None) fp32 numpy; outputs start at 7.0"""
    M, K = a.shape
    N = w.shape[0]
    lab = torch.tensor(labels, dtype=torch.int32, device="cuda")
    lp = torch.full((M,), 7.0, device="cuda")
    lse = torch.full((M,), 7.0, device="cuda") if want_lse else None
    nb = lib.omchat_op_lse_label_ws(M, N)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    rc = lib.omchat_op_lse_label(CODE[dt], ptr(a), K, ptr(w), K, M, N, K, ptr(lab), ptr(lp), ptr(lse), ptr(ws), nb, cur_stream())
    torch.cuda.synchronize()
    out = (lp.cpu().numpy(), None if lse is None else lse.cpu().numpy())
    check(rc)
    return out


def _special_labels(N):
    """0, N - 1, the ids around the 64- and 256-column tile edges where they exist, one id of the last partial 64-column block"""
    s = [0, N - 1] + [c for c in (63, 64, 255, 256) if c < N]
    if N % 64:
        s.append(N - N % 64 + (N % 64) // 2)
    return s


SHAPES = [(1, 320, 256), (17, 36, 64), (17, 1000, 3584), (257, 1000, 256), (33, 152064, 64)]


@pytest.mark.parametrize("big", [False, True], ids=["unit", "pm80"])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_op_lse_label_equals_fp64(gpu_lib, M, N, K, dt, big):
    rng = np.random.default_rng(M * 7 + N + K + big)
    # row plan: ignored rows, the special labels, an all-zero hidden row (scored and ignored), random labels; as many calls of M rows as it takes
    plan = [(IGN, False)] + [(l, False) for l in _special_labels(N)] + [(5 % N, True), (IGN, True)]
    calls = -(-len(plan) // M)
    while len(plan) < calls * M:
        plan.append((IGN if len(plan) % 7 == 3 else int(rng.integers(0, N)), False))
    # W scaled so that the logits are ~ N(0, 1), or ~ N(0, 30^2): they reach +-80 and beyond, so the online max is needed (exp(x - m) underflows)
    sw = (30.0 if big else 1.0) / np.sqrt(K)
    w = dev((rng.standard_normal((N, K)) * sw).astype(np.float32), dt)
    w64 = w.float().cpu().numpy().astype(np.float64)
    worst_err = z_max = 0.0
    for c in range(calls):
        rows = plan[c * M:(c + 1) * M]
        a32 = rng.standard_normal((M, K)).astype(np.float32)
        for r, (_, zero) in enumerate(rows):
            if zero:
                a32[r] = 0.0
        a = dev(a32, dt)
        labels = [l for l, _ in rows]
        lp, lse = _op(gpu_lib, dt, a, w, labels)
        lp2, lse2 = _op(gpu_lib, dt, a, w, labels)
        assert np.array_equal(lp.view(np.uint32), lp2.view(np.uint32)) and np.array_equal(lse.view(np.uint32), lse2.view(np.uint32))
        lp3, none = _op(gpu_lib, dt, a, w, labels, want_lse=False)
        assert none is None and np.array_equal(lp.view(np.uint32), lp3.view(np.uint32))
        a64 = a.float().cpu().numpy().astype(np.float64)
        z = a64 @ w64.T                                   # exact products, fp64 sums
        worst = (np.abs(a64) @ np.abs(w64).T).max(axis=1)
        z_max = max(z_max, float(np.abs(z).max()))
        for r, (lab, zero) in enumerate(rows):
            l_ref = lr.lse(z[r])
            x_id = 0.0 if lab == IGN else z[r, lab]
            tol = 2.0 * K * 2.0 ** -24 * worst[r] + lr.tolerance(x_id, l_ref)
            assert abs(tol - sf.op_tolerance(a64[r], w64, x_id, l_ref)) <= 1e-12 * tol
            e_lse = abs(float(lse[r]) - l_ref)
            assert not np.isnan(lse[r]) and e_lse <= tol, (M, N, K, dt, r, lse[r], l_ref, tol)
            if lab == IGN:
                assert lp[r] == 0.0
                continue
            err = abs(float(lp[r]) - (x_id - l_ref))
            worst_err = max(worst_err, err / tol)
            assert not np.isnan(lp[r]) and err <= tol, (M, N, K, dt, r, lab, lp[r], x_id - l_ref, err, tol)
            if zero:      # every logit is exactly 0: log(1 / N), so the padded columns of the last tile counted nothing
                assert abs(float(lp[r]) + np.log(N)) <= tol and abs(float(lse[r]) - np.log(N)) <= tol
    assert z_max > 80.0 or not big
    print(f"SCERR op-{M}x{N}x{K}-{dt}-{'pm80' if big else 'unit'} worst err/tol {worst_err:.3e} 1")


def test_op_refusals_enqueue_nothing(gpu_lib):
    rng = np.random.default_rng(3)
    a = dev(rng.standard_normal((5, 64)).astype(np.float32), "bf16")
    w = dev(rng.standard_normal((40, 64)).astype(np.float32), "bf16")
    ok, _ = _op(gpu_lib, "bf16", a, w, [0, 39, IGN, 7, 8])
    assert ok[2] == 0.0 and np.all(ok[[0, 1, 3, 4]] < 0)
    for bad in ([0, 40, IGN, 7, 8], [0, -1, IGN, 7, 8], [0, 39, -101, 7, 8]):
        lab = torch.tensor(bad, dtype=torch.int32, device="cuda")
        lp = torch.full((5,), 7.0, device="cuda"); lse = torch.full((5,), 7.0, device="cuda")
        nb = gpu_lib.omchat_op_lse_label_ws(5, 40)
        ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        rc = gpu_lib.omchat_op_lse_label(CODE["bf16"], ptr(a), 64, ptr(w), 64, 5, 40, 64, ptr(lab), ptr(lp), ptr(lse), ptr(ws), nb, cur_stream())
        torch.cuda.synchronize()
        assert rc == 1 and b"label" in gpu_lib.omchat_last_error()
        assert bool((lp == 7.0).all()) and bool((lse == 7.0).all()) and int(ws.count_nonzero()) == 0
    # N % 4 != 0, K % 64 != 0, a workspace that is too small
    w38 = w[:38].contiguous()
    lab = torch.tensor([0, 1, 2, 3, IGN], dtype=torch.int32, device="cuda")
    for (wt, N, K, cut) in ((w38, 38, 64, 0), (w, 40, 32, 0), (w, 40, 64, 16)):
        lp = torch.full((5,), 7.0, device="cuda")
        nb = gpu_lib.omchat_op_lse_label_ws(5, 40)
        ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        rc = gpu_lib.omchat_op_lse_label(CODE["bf16"], ptr(a), 64, ptr(wt), 64, 5, N, K, ptr(lab), ptr(lp), None, ptr(ws), nb - cut, cur_stream())
        torch.cuda.synchronize()
        assert rc == 1, (N, K, cut)
        assert bool((lp == 7.0).all()) and int(ws.count_nonzero()) == 0


# ---------------------------------------------------------------------------------------------------------------- the model
CASES = ["A", "B", "C", "D", "E"]


@pytest.fixture(scope="module")
def models():
    g = golden("score_tiny")
    cache = {}

    def get(dt, vocab):
        if (dt, vocab) not in cache:
            from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
            cfg = tiny(vocab=vocab)
            sd = synth.state_dict(cfg, seed=int(g["seed"]))
            e = Engine(cfg, dtype=dt, max_seq=128, max_batch=2, max_tiles=2)
            e.load_state_dict(sd)
            cache[(dt, vocab)] = (cfg, e, OmChatQwen2ForCausalLM(cfg.clone(), e), sd["lm_head.weight"].astype(np.float64))
        return cache[(dt, vocab)]
    yield get
    for _, e, _, _ in cache.values():
        e.close()


def _forward(m, cfg, g, name, labels="fixture", **kw):
    """forward() of a fixture case: the reference run's feature rows in place of the tower, its padding side and length cut"""
    ids, mask, lab, n_tiles, side, ml, _ = sf.case_inputs(g, name)
    feats = sf.case_feats(name, n_tiles, cfg.num_image_tokens, cfg.text["hidden_size"])
    m.config.tokenizer_padding_side, m.config.tokenizer_model_max_length = side, ml
    images = None
    if feats is not None:
        m.encode_images = lambda images: feats.to(device=m.device, dtype=m.dtype)
        images = torch.zeros(n_tiles, 3, 56, 56)
    try:
        if labels == "score":
            return m.score(ids, images=images, attention_mask=mask, **kw)
        return m.forward(input_ids=ids, attention_mask=mask, images=images, labels=lab if labels == "fixture" else labels, **kw)
    finally:
        if feats is not None:
            del m.encode_images
        m.config.tokenizer_padding_side, m.config.tokenizer_model_max_length = "right", None


def _exist(e, hidden, new_labels, w64):
    """the existing path: Engine.lm_head on prefill's hidden rows, log-softmax in fp64 -> (token_logprobs fp64, per-slot op tolerance)"""
    L = e.lm_head(hidden).cpu().numpy()
    tl = sf.token_logprobs(L, new_labels)
    h64 = hidden.float().cpu().numpy().astype(np.float64)
    b, S, H = h64.shape
    worst = (np.abs(h64).reshape(b * S, H) @ np.abs(w64).T).max(axis=1).reshape(b, S)
    tol = np.zeros((b, S))
    for i in range(b):
        for t in range(1, S):
            if new_labels[i, t] != IGN:
                z = L[i, t - 1].astype(np.float64)
                tol[i, t] = 2.0 * H * 2.0 ** -24 * worst[i, t - 1] + lr.tolerance(z[new_labels[i, t]], lr.lse(z))
    return tl, tol


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("name", CASES)
def test_forward_labels_equals_existing_path_and_reference(gpu_lib, models, name, dt):
    g = golden("score_tiny")
    cfg, e, m, w64 = models(dt, int(g[f"{name}_vocab"]))
    w64 = torch.from_numpy(w64).to(DT[dt]).double().numpy()              # the 16-bit lm_head the device holds
    out = _forward(m, cfg, g, name)
    plain = _forward(m, cfg, g, name, labels=None, output_hidden_states=True)
    torch.cuda.synchronize()
    # without labels: today's object
    assert plain.loss is None and plain["loss"] is None and not hasattr(plain, "token_logprobs") and "labels" not in plain
    assert torch.equal(out.logits, plain.logits) and out.logits.shape == (out.labels.shape[0], 1, cfg.text["vocab_size"])
    new_labels = out.labels.numpy()
    assert out.labels.dtype == torch.int64 and np.array_equal(new_labels, g[f"{name}_new_labels"])
    assert out.loss.dtype == torch.float32 and out.loss.dim() == 0 and out.loss.is_cuda
    tl = out.token_logprobs.cpu().numpy().astype(np.float64)
    assert out.token_logprobs.dtype == torch.float32 and tl.shape == new_labels.shape
    scored = new_labels != IGN
    scored[:, 0] = False
    assert np.all(tl[~scored] == 0.0) and not np.isnan(tl).any() and np.all(tl[scored] < 0.0)
    exist, tol = _exist(e, plain.hidden_states[0], new_labels, w64)
    gold = g[f"{name}_token_logprobs"].astype(np.float64)
    d_new = np.abs(tl - exist)[scored]
    d_ref = float(np.abs(exist - gold)[scored].max())
    print(f"SCERR model-{name}-{dt} new-vs-existing {d_new.max():.3e} tol {tol[scored].min():.3e}   max|exist - golden| {d_ref:.3e}")
    assert np.all(d_new <= tol[scored]), (name, dt, d_new.max(), tol[scored].min())
    assert np.all(np.abs(tl - gold)[scored] <= d_ref + tol[scored])
    n = int(scored.sum())
    loss_exist = -exist[scored].sum() / n
    assert abs(float(out.loss) - loss_exist) <= tol[scored].mean()
    assert abs(float(out.loss) - float(g[f"{name}_loss"])) <= d_ref + tol[scored].mean()
    # a second run: the same bits
    again = _forward(m, cfg, g, name)
    assert torch.equal(again.token_logprobs, out.token_logprobs) and torch.equal(again.loss, out.loss)


@pytest.mark.parametrize("name", ["A", "B", "C", "E"])
def test_score_equals_forward_with_ids_as_labels(gpu_lib, models, name):
    g = golden("score_tiny")
    cfg, e, m, _ = models("bf16", int(g[f"{name}_vocab"]))
    ids = sf.case_inputs(g, name)[0]
    out = _forward(m, cfg, g, name, labels=ids)
    sc = _forward(m, cfg, g, name, labels="score")
    assert torch.equal(sc["token_logprobs"], out.token_logprobs) and torch.equal(sc["loss"], out.loss) and torch.equal(sc["labels"], out.labels)
    tl = sc["token_logprobs"].cpu().numpy().astype(np.float64)
    lab = sc["labels"].numpy()
    scored = lab != IGN
    scored[:, 0] = False
    # every text token but a row's first is scored; image rows and padding are not
    mask = g[f"{name}_mask"]
    n_text = [(int((ids[i] != -200).sum()) if mask.size == 0 else int(((ids[i] != -200) & (torch.from_numpy(mask[i]) != 0)).sum())) for i in range(ids.shape[0])]
    first_col_scored = [int(lab[i, 0] != IGN) for i in range(ids.shape[0])]
    n_tok = sc["num_tokens"].cpu().numpy()
    assert sc["num_tokens"].dtype == torch.int64 and list(n_tok) == [int(scored[i].sum()) for i in range(ids.shape[0])]
    assert list(n_tok) == [n_text[i] - first_col_scored[i] for i in range(ids.shape[0])]
    seq = sc["sequence_logprobs"].cpu().numpy().astype(np.float64)
    for i in range(ids.shape[0]):
        s = tl[i][scored[i]].sum()
        assert abs(seq[i] - s) <= 1e-6 * max(1.0, abs(s)) * n_tok[i]          # fp32 sums of n_tok[i] terms, another order
        assert abs(float(sc["perplexity"][i]) - np.exp(-seq[i] / n_tok[i])) <= 1e-5 * np.exp(-seq[i] / n_tok[i])
    total = -tl[scored].sum() / scored.sum()
    assert abs(float(sc["loss"]) - total) <= 1e-6 * abs(total) * scored.sum()


def test_score_agrees_with_generate_logprobs(gpu_lib, models):
    """section 14 cross-check: the raw log-probabilities generate() records for its greedy ids (decode steps) and the scored values of
    prompt + generated (one prefill, the lm_head epilogue) are two paths to the same numbers.  Each is held to its own tolerance against
    fp64 values from its OWN logits -- the logits of the same greedy steps run by hand (forward, then decode steps with want_logits), and
    Engine.lm_head of the prefill's hidden rows -- and their difference to the sum of the two measured distances: prefill and decode agree."""
    g = golden("score_tiny")
    cfg, e, m, w64 = models("bf16", 320)
    w64 = torch.from_numpy(w64).to(DT["bf16"]).double().numpy()
    prompt = torch.tensor([[3, 17, 18, 19, 20, 21, 7, 9]])
    P, n = prompt.shape[1], 8
    gen = m.generate(input_ids=prompt, max_new_tokens=n, do_sample=False, return_dict_in_generate=True, output_logprobs=True)
    seq = gen.sequences.cpu()
    assert seq.shape == (1, P + n)
    rec = gen.logprobs[0].cpu().numpy().astype(np.float64)
    # the generate path's own logits: the same greedy steps by hand
    e.logprobs_off(); e.sampling_off(); e.constraints_off()      # (generate() leaves its record stage on)
    out = m.forward(input_ids=prompt, use_cache=True)
    lg, toks, own = out.local_logits, [], []
    for step in range(n):
        tok = e.argmax(lg)
        toks.append(int(tok[0])); own.append(lg[0].cpu().numpy())
        if step < n - 1:
            tok, lg = e.decode_step(tok, want_logits=True)
    assert toks == seq[0, P:].tolist()
    d_gen = tol_gen = 0.0
    for t in range(n):
        z = own[t].astype(np.float64)
        ref = z[toks[t]] - lr.lse(z)
        d_gen, tol_gen = max(d_gen, abs(rec[t] - ref)), max(tol_gen, lr.tolerance(z[toks[t]], lr.lse(z)))
        assert abs(rec[t] - ref) <= lr.tolerance(z[toks[t]], lr.lse(z)), (t, rec[t], ref)
    # the scoring path's own logits: Engine.lm_head of the prefill's hidden rows
    plain = m.forward(input_ids=seq, output_hidden_states=True)
    sc = m.score(seq)
    got = sc["token_logprobs"][0].cpu().numpy().astype(np.float64)
    exist, tol = _exist(e, plain.hidden_states[0], seq.numpy(), w64)
    d_sc = float(np.abs(got - exist)[0, P:].max())
    assert np.all(np.abs(got - exist)[0, P:] <= tol[0, P:])
    delta = float(np.abs(got[P:] - rec).max())
    print(f"SCERR generate-vs-score |delta| {delta:.3e}   generate-vs-own-logits {d_gen:.3e} tol {tol_gen:.3e}   "
          f"score-vs-own-logits {d_sc:.3e} tol {tol[0, P:].min():.3e}")
    assert delta <= d_gen + d_sc, (delta, d_gen, d_sc)


def test_persistent_gemm_form_gives_the_same_bits(gpu_lib):
    """tuning key 13 (a test hook, default 0) sends multi-round 256^2 launches through the persistent kernel: same tiles, same epilogue"""
    rng = np.random.default_rng(11)
    M, N, K = 33, 152064, 64
    a = dev(rng.standard_normal((M, K)).astype(np.float32), "bf16")
    w = dev((rng.standard_normal((N, K)) / 8).astype(np.float32), "bf16")
    labels = [IGN if r % 5 == 0 else int(rng.integers(0, N)) for r in range(M)]
    lp0, lse0 = _op(gpu_lib, "bf16", a, w, labels)
    check(gpu_lib.omchat_op_set_tuning(13, 1))
    try:
        lp1, lse1 = _op(gpu_lib, "bf16", a, w, labels)
    finally:
        check(gpu_lib.omchat_op_set_tuning(13, 0))
    assert np.array_equal(lp0.view(np.uint32), lp1.view(np.uint32)) and np.array_equal(lse0.view(np.uint32), lse1.view(np.uint32))
    assert not np.isnan(lp1).any() and np.all(lp1[[r for r in range(M) if r % 5]] < 0)


def test_refusals_leave_the_state_alone(gpu_lib, models):
    g = golden("score_tiny")
    cfg, e, m, _ = models("bf16", 320)
    prompt = torch.tensor([[3, 17, 18, 19, 20, 21, 7, 9]])
    before = m.generate(input_ids=prompt, max_new_tokens=4, do_sample=False).cpu()
    lens = e.kv_lengths(1)
    # labels on a decode call
    out = m.forward(input_ids=prompt, use_cache=True)
    lens = e.kv_lengths(1)
    with pytest.raises(ValueError):
        m.forward(input_ids=torch.tensor([[5]]), past_key_values=out.past_key_values, labels=torch.tensor([[5]]))
    assert e.kv_lengths(1) == lens
    # labels of another shape, labels outside the vocabulary: before any work
    with pytest.raises(ValueError):
        m.forward(input_ids=prompt, labels=prompt[:, :-1])
    with pytest.raises(ValueError):
        m.forward(input_ids=prompt, labels=torch.full_like(prompt, 320))
    H = cfg.text["hidden_size"]
    with pytest.raises(ValueError):      # beside inputs_embeds: the shape of its rows, ids of the vocabulary
        m.forward(inputs_embeds=torch.zeros(1, 8, H, dtype=torch.bfloat16, device="cuda"), labels=prompt[:, :-1])
    with pytest.raises(ValueError):
        m.forward(inputs_embeds=torch.zeros(1, 8, H, dtype=torch.bfloat16, device="cuda"), labels=torch.full_like(prompt, -7))
    assert e.kv_lengths(1) == lens
    # ... and none of them touched what the earlier prefill left: its decode step runs as if nothing had been asked
    state = (m._padded_batch, m._prefill_slots, m._last_lengths)
    with pytest.raises(ValueError):
        m.forward(input_ids=torch.cat([prompt, prompt], 1), labels=torch.full((1, 16), 999))
    assert (m._padded_batch, m._prefill_slots, m._last_lengths) == state
    # a label at an image-token or a masked position is never looked at (score() passes the ids themselves)
    ok = m.forward(input_ids=prompt, attention_mask=torch.tensor([[1] * 7 + [0]]), labels=torch.tensor([[3, 17, 18, 19, 20, 21, 7, 99999]]))
    assert not bool(torch.isnan(ok.loss))
    out = m.forward(input_ids=prompt, use_cache=True)
    lens = e.kv_lengths(1)
    # the C entry: b * S != rows, rows > max_prefill_rows (2 x 128 here)
    hid = torch.zeros(300, H, dtype=torch.bfloat16, device="cuda")
    lab = torch.full((300,), IGN, dtype=torch.int32, device="cuda")
    lp = torch.full((300,), 7.0, device="cuda"); o = torch.full((8,), 7.0, device="cuda")
    for rows, b, S in ((12, 2, 5), (300, 1, 300)):
        rc = e.lib.omchat_score_hidden(e.h, ptr(hid), rows, ptr(lab), b, S, ptr(lp), ptr(o), cur_stream())
        torch.cuda.synchronize()
        assert rc == 1 and bool((lp == 7.0).all()) and bool((o == 7.0).all())
    # a rank context of TP = 2: refused by the model, by the engine and by the C entry, each before any work
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    e2 = Engine(cfg, dtype="bf16", max_seq=16, max_batch=1, max_tiles=1, vision=False, tp_rank=0, tp_size=2, comm=C.c_void_p(1))
    m2 = OmChatQwen2ForCausalLM(cfg.clone(), e2)
    lens2 = e2.kv_lengths(1)
    with pytest.raises(NotImplementedError):
        m2.forward(input_ids=prompt, labels=prompt)
    with pytest.raises(NotImplementedError):
        e2.score_hidden(torch.zeros(1, 4, H, dtype=torch.bfloat16, device="cuda"), torch.zeros(1, 4, dtype=torch.long))
    rc = e2.lib.omchat_score_hidden(e2.h, ptr(hid), 4, ptr(lab), 1, 4, ptr(lp), ptr(o), cur_stream())
    torch.cuda.synchronize()
    assert rc == 1 and b"tensor parallelism" in e2.lib.omchat_last_error() and bool((lp == 7.0).all())
    assert e2.kv_lengths(1) == lens2
    e2.close()
    # missing weights; then b * S > max_prefill_rows through forward()
    e3 = Engine(cfg, dtype="bf16", max_seq=64, max_batch=2, max_tiles=1, max_prefill_rows=16, vision=False)
    rc = e3.lib.omchat_score_hidden(e3.h, ptr(hid), 4, ptr(lab), 1, 4, ptr(lp), ptr(o), cur_stream())
    torch.cuda.synchronize()
    assert rc == 1 and b"weights" in e3.lib.omchat_last_error() and bool((lp == 7.0).all())
    e3.load_state_dict(synth.state_dict(cfg, seed=int(g["seed"])), strict=False)
    m3 = OmChatQwen2ForCausalLM(cfg.clone(), e3)
    ok = m3.forward(input_ids=prompt, labels=prompt)
    assert not bool(torch.isnan(ok.loss))
    lens3 = e3.kv_lengths(1)
    long_ids = torch.arange(1, 21).view(1, 20)
    with pytest.raises(ValueError):
        m3.forward(input_ids=long_ids, labels=long_ids)
    with pytest.raises(ValueError):
        m3.forward(input_ids=long_ids[:, :18].reshape(2, 9), labels=torch.zeros(2, 9, dtype=torch.long))      # 2 x 9 rows
    assert e3.kv_lengths(1) == lens3
    again = m3.forward(input_ids=prompt, labels=prompt)
    assert torch.equal(again.token_logprobs, ok.token_logprobs)
    e3.close()
    after = m.generate(input_ids=prompt, max_new_tokens=4, do_sample=False).cpu()
    assert torch.equal(before, after)


def test_no_scored_token_gives_nan_loss(gpu_lib, models):
    cfg, e, m, _ = models("bf16", 320)
    ids = torch.tensor([[3, 17, 18, 19]])
    out = m.forward(input_ids=ids, labels=torch.full_like(ids, IGN))
    assert bool(torch.isnan(out.loss)) and bool((out.token_logprobs == 0).all())
    one = m.forward(input_ids=ids, labels=torch.tensor([[9, IGN, IGN, IGN]]))      # a label in column 0 only: nothing predicts it
    assert bool(torch.isnan(one.loss)) and bool((one.token_logprobs == 0).all())
