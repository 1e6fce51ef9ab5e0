"""GPU: prompt-lookup decoding.  The multi-query verify attention against an fp32 reference, against the prefill
kernel and against rope_kv's bytes; the verify step against T single decode steps; acceptance and trimming; generate(prompt_lookup_num_tokens)
against generate() on tiny models (text, image, decode graph, streamer / stopping criteria); TP 2 / 4 rank contexts on one device; the
configs[1] full-depth fixture; the refusals."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from gpu_util import CODE, DT, TOL, ptr, rel, sync
from omchat_amd import _lib, synth
from omchat_amd.config import tiny
from omchat_amd.engine import Engine

SCALE = 1.0 / math.sqrt(128)


# ---------------------------------------------------------------------------------------------------------------- op level
def _ref_attn(q, k, v, L):
    """fp32 causal GQA: q [T, Hq, 128], k / v [Hkv, L + T, 128]; query t sees keys 0 .. L + t"""
    T, Hq, _ = q.shape
    Hkv = k.shape[0]
    rep = Hq // Hkv
    kk = k.float().repeat_interleave(rep, dim=0)            # [Hq, Lt, 128]
    vv = v.float().repeat_interleave(rep, dim=0)
    s = torch.einsum("thd,hkd->htk", q.float(), kk) * SCALE
    keys = torch.arange(L + T)
    mask = keys[None, :] > (L + torch.arange(T))[:, None]
    s = s.masked_fill(mask[None], float("-inf"))
    return torch.einsum("htk,hkd->thd", torch.softmax(s, -1), vv)


CASES = [(2, 0), (3, 62), (8, 60), (9, 60), (16, 56), (8, 0), (16, 0), (5, 123)]      # (T, L): L = 0, a 64-key straddle, L + T = cap


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("Hq,Hkv", [(7, 1), (4, 2), (2, 2)])
def test_op_verify_attention(gpu_lib, dt, Hq, Hkv):
    cap = 128
    g = torch.Generator().manual_seed(Hq * 10 + Hkv)
    worst = 0.0
    for T, L in CASES:
        if L + T > cap:
            L = cap - T
        qkvd = (Hq + 2 * Hkv) * 128
        qkv = (torch.randn(T, qkvd, generator=g)).to("cuda", DT[dt])
        kc0 = torch.randn(Hkv, cap, 128, generator=g).to("cuda", DT[dt])
        vc0 = torch.randn(Hkv, cap, 128, generator=g).to("cuda", DT[dt])
        ws_b = gpu_lib.omchat_op_attn_decode_ws(T, Hq, L + T)
        ws = torch.empty(ws_b // 4 + 64, dtype=torch.float32, device="cuda")
        # rope_kv (the prefill's RoPE + append) on a copy: rotated q in place, rows L .. L + T - 1 of its cache
        qkv_r = qkv.clone(); kr, vr = kc0.clone(), vc0.clone()
        _lib.check(gpu_lib.omchat_op_rope_kv(CODE[dt], ptr(qkv_r), 1, T, Hq, Hkv, L, 1e6, ptr(kr), ptr(vr), cap, None))
        # fused form: the same cache bytes
        kf, vf = kc0.clone(), vc0.clone()
        out_f = torch.empty(T, Hq, 128, dtype=DT[dt], device="cuda")
        _lib.check(gpu_lib.omchat_op_attn_verify_append(CODE[dt], ptr(qkv), 1e6, ptr(kf), ptr(vf), ptr(out_f), T, Hq, Hkv, cap, L, SCALE,
                                                        ptr(ws), ws_b, None))
        sync()
        assert torch.equal(kf.view(torch.int16), kr.view(torch.int16)), (T, L)
        assert torch.equal(vf.view(torch.int16), vr.view(torch.int16)), (T, L)
        q = qkv_r[:, :Hq * 128].reshape(T, Hq, 128).contiguous()
        ref = _ref_attn(q.cpu(), kr[:, :L + T].cpu(), vr[:, :L + T].cpu(), L)
        e_f = rel(out_f.cpu(), ref)
        # unfused form over the appended cache
        out_u = torch.empty_like(out_f)
        _lib.check(gpu_lib.omchat_op_attn_verify(CODE[dt], ptr(q), ptr(kr), ptr(vr), ptr(out_u), T, Hq, Hkv, cap, L, SCALE, ptr(ws), ws_b, None))
        # the prefill kernel with q_pos0 = L over the same keys
        kp, vp = kr[:, :L + T].contiguous(), vr[:, :L + T].contiguous()
        out_p = torch.empty(1, T, Hq, 128, dtype=DT[dt], device="cuda")
        _lib.check(gpu_lib.omchat_op_attn_prefill(CODE[dt], ptr(q), ptr(kp), ptr(vp), ptr(out_p), 1, T, L + T, Hq, Hkv, None, 1, L, SCALE, None))
        sync()
        e_u = rel(out_u.cpu(), ref)
        e_p = rel(out_u.cpu(), out_p[0].cpu())
        worst = max(worst, e_f, e_u, e_p)
        assert e_f < TOL[dt] and e_u < TOL[dt] and e_p < TOL[dt], (T, L, e_f, e_u, e_p)
        assert torch.isfinite(out_f.float()).all()
    print(f"\n{dt} Hq={Hq} Hkv={Hkv}: worst rel err {worst:.2e}")


@pytest.mark.parametrize("Hq,Hkv,T,L", [(28, 4, 8, 32764), (28, 4, 16, 32956), (28, 4, 2, 33000), (7, 1, 9, 40000), (7, 1, 16, 4090)])
def test_op_verify_long_context(gpu_lib, Hq, Hkv, T, L):
    """long contexts take several 64-key tiles per split (launch_attn_block's ATTN_VERIFY plan, tpw > 1: the tile loop, the LDS hand-over between tiles, the
    rescale of the online softmax, the merge over splits of 64 tpw keys); the new rows straddle a tile inside a split (32764 + 8) and a split
    boundary (32956 + 16 at 5 tiles per split on 256 CUs), with the fused RoPE + append checked against rope_kv's bytes"""
    dt = "bf16"
    cap = L + T
    tpw = gpu_lib.omchat_op_attn_verify_tpw(L + T, Hkv)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"\nHq={Hq} Hkv={Hkv} T={T} L={L}: {tpw} tiles per split ({cus} CUs)")
    if (L + T + 63) // 64 * Hkv > 2 * cus:
        assert tpw > 1
    g = torch.Generator().manual_seed(L + T)
    qkvd = (Hq + 2 * Hkv) * 128
    qkv = torch.randn(T, qkvd, generator=g).to("cuda", DT[dt])
    kc0 = torch.randn(Hkv, cap, 128, generator=g).to("cuda", DT[dt])
    vc0 = torch.randn(Hkv, cap, 128, generator=g).to("cuda", DT[dt])
    ws_b = gpu_lib.omchat_op_attn_decode_ws(T, Hq, L + T)
    ws = torch.empty(ws_b // 4 + 64, dtype=torch.float32, device="cuda")
    qkv_r = qkv.clone(); kr, vr = kc0.clone(), vc0.clone()
    _lib.check(gpu_lib.omchat_op_rope_kv(CODE[dt], ptr(qkv_r), 1, T, Hq, Hkv, L, 1e6, ptr(kr), ptr(vr), cap, None))
    kf, vf = kc0.clone(), vc0.clone()
    out_f = torch.empty(T, Hq, 128, dtype=DT[dt], device="cuda")
    _lib.check(gpu_lib.omchat_op_attn_verify_append(CODE[dt], ptr(qkv), 1e6, ptr(kf), ptr(vf), ptr(out_f), T, Hq, Hkv, cap, L, SCALE,
                                                    ptr(ws), ws_b, None))
    sync()
    assert torch.equal(kf.view(torch.int16), kr.view(torch.int16)) and torch.equal(vf.view(torch.int16), vr.view(torch.int16))
    q = qkv_r[:, :Hq * 128].reshape(T, Hq, 128).contiguous()
    out_u = torch.empty_like(out_f)
    _lib.check(gpu_lib.omchat_op_attn_verify(CODE[dt], ptr(q), ptr(kr), ptr(vr), ptr(out_u), T, Hq, Hkv, cap, L, SCALE, ptr(ws), ws_b, None))
    sync()
    ref = _ref_attn(q.cpu(), kr.cpu(), vr.cpu(), L)
    e_f, e_u = rel(out_f.cpu(), ref), rel(out_u.cpu(), ref)
    # per query row too: a row whose merge went wrong hides in the norm over all rows
    e_rows = max(rel(out_u[t].cpu(), ref[t]) for t in range(T))
    print(f"rel err fused {e_f:.2e} unfused {e_u:.2e} worst row {e_rows:.2e}")
    assert e_f < TOL[dt] and e_u < TOL[dt] and e_rows < TOL[dt]


# ---------------------------------------------------------------------------------------------------------------- model level
def _tiny_model(q=7, kv=1, seed=21, max_seq=128, dt="bf16", vision=False):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    cfg = tiny(q_heads=q, kv_heads=kv)
    e = Engine(cfg, dtype=dt, max_seq=max_seq, max_batch=1, max_tiles=2, vision=vision)
    e.load_state_dict(synth.state_dict(cfg, seed), strict=False)
    return cfg, e, OmChatQwen2ForCausalLM(cfg.clone(), e)


PROMPT = [3, 17, 18, 19, 20, 21, 7, 9, 17, 18, 19, 30, 31]
# max |logit| difference, verify rows (MFMA-form GEMVs) against single steps (whole-row GEMVs): about 2 x the measured 3.7e-3 (bf16) / 5.8e-4 (f16)
BOUND = {"bf16": 8e-3, "f16": 1.2e-3}


def _margin(lg):
    t = torch.topk(lg.float(), 2).values
    return float(t[0] - t[1])


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("q,kv", [(7, 1), (4, 2)])
@pytest.mark.parametrize("T", [2, 5, 16])
def test_verify_equals_single_steps(gpu_lib, dt, q, kv, T):
    _, e, m = _tiny_model(q, kv, dt=dt)
    ids = torch.tensor([PROMPT])
    g = torch.Generator().manual_seed(T)
    toks = torch.randint(0, 320, (T,), generator=g)
    out = m.forward(input_ids=ids, use_cache=True)
    P = e.kv_lengths(1)[0]
    picks, n, lg_v = e.decode_verify(toks, keep_all=True, want_logits=True)
    sync()
    assert e.kv_lengths(1)[0] == P + T
    m.forward(input_ids=ids, use_cache=True)
    rows, nx = [], []
    for t in toks.tolist():
        nxt, lg = e.decode_step(torch.tensor([t]), want_logits=True)
        rows.append(lg[0]); nx.append(int(nxt[0]))
    sync()
    assert e.kv_lengths(1)[0] == P + T
    lg_s = torch.stack(rows)
    d = float((lg_v - lg_s).abs().max())
    print(f"\n{dt} {q}q/{kv}kv T={T}: max |logit diff| verify vs single steps {d:.3e} (bound {BOUND[dt]})")
    assert d < BOUND[dt]
    for j in range(T):
        if _margin(lg_s[j]) > 2 * BOUND[dt]:
            assert int(picks[j]) == nx[j], j
    e.close()


def _greedy_chain(e, m, ids, n):
    out = m.forward(input_ids=ids, use_cache=True)
    chain = [int(e.argmax(out.local_logits)[0])]
    for _ in range(n - 1):
        nxt, _ = e.decode_step(torch.tensor([chain[-1]]))
        chain.append(int(nxt[0]))
    return chain


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_acceptance_and_trimming(gpu_lib, dt):
    _, e, m = _tiny_model(dt=dt)
    ids = torch.tensor([PROMPT])
    chain = _greedy_chain(e, m, ids, 40)
    T = 8
    # draft = the recorded greedy continuation: every draft accepted
    m.forward(input_ids=ids, use_cache=True)
    P = e.kv_lengths(1)[0]
    picks, n = e.decode_verify(chain[:T])
    assert n == T - 1 and picks.tolist() == chain[1:T + 1]
    assert e.kv_lengths(1)[0] == P + T
    # a draft corrupted at index j: n = j, cache L + 1 + j
    for j in range(T - 1):
        m.forward(input_ids=ids, use_cache=True)
        bad = list(chain[:T]); bad[j + 1] = (bad[j + 1] + 1) % 320
        picks, n = e.decode_verify(bad)
        assert n == j, (j, n)
        assert e.kv_lengths(1)[0] == P + 1 + j
        assert picks.tolist()[:j + 1] == chain[1:j + 2]
    # several verify steps with corrupted drafts, then plain steps: the greedy ids
    m.forward(input_ids=ids, use_cache=True)
    got = [chain[0]]
    for j in (2, 0, 5, 3):
        L = len(got)
        draft = list(chain[L:L + 6]); draft[j] = (draft[j] + 7) % 320
        picks, n = e.decode_verify([got[-1]] + draft)
        assert n == j
        got += picks.tolist()[:n + 1]
        assert e.kv_lengths(1)[0] == P + len(got) - 1
    while len(got) < 40:
        nxt, _ = e.decode_step(torch.tensor([got[-1]]))
        got.append(int(nxt[0]))
    assert got == chain
    e.close()


def _gen_pair(m, ids, k, **kw):
    e = m.engine
    e.lookup_stats(reset=True)
    base = m.generate(ids, **kw)
    got = m.generate(ids, prompt_lookup_num_tokens=k, **kw)
    return base, got, e.lookup_stats()


def _check_equal_or_near_tie(e, m, ids, base, got, dt, images=None):
    """equal ids; otherwise the first difference must sit at a greedy top-2 margin below the verify-vs-single bound"""
    if torch.equal(base, got):
        return "equal"
    P = ids.shape[1]
    j = next(i for i in range(min(base.shape[1], got.shape[1])) if base[0, i] != got[0, i])
    out = m.forward(input_ids=ids, images=images, use_cache=True)
    lg = out.local_logits[0]
    for t in base[0, P:j].tolist():
        _, l2 = e.decode_step(torch.tensor([t]), want_logits=True)
        lg = l2[0]
    mg = _margin(lg)
    assert mg < 2 * BOUND[dt], (j, mg)
    return f"near tie at {j} (margin {mg:.3e})"


@pytest.mark.parametrize("k", [1, 4, 10])
def test_generate_lookup_equals_generate(gpu_lib, k):
    _, e, m = _tiny_model(seed=5)
    ids = torch.tensor([PROMPT])
    base, got, st = _gen_pair(m, ids, k, max_new_tokens=60)
    case = _check_equal_or_near_tie(e, m, ids, base, got, "bf16")
    print(f"\nk={k}: {case}; {st}")
    assert st["verify_steps"] > 0 and st["accepted"] > 0
    assert got.shape == base.shape
    e.close()


def test_generate_lookup_with_image(gpu_lib):
    cfg, e, m = _tiny_model(seed=9, vision=True)
    ids = torch.tensor([[3, -200, 17, 18, 19, 17, 18, 19, 20]])
    img = torch.from_numpy(synth.pixels(1, 56, 3)).cuda()
    base, got, st = _gen_pair(m, ids, 4, images=img, max_new_tokens=48)
    case = _check_equal_or_near_tie(e, m, ids, base, got, "bf16", images=img)
    print(f"\nimage: {case}; {st}")
    assert st["accepted"] > 0
    e.close()


def test_generate_lookup_graph_streamer_stopping(gpu_lib):
    _, e, m = _tiny_model(seed=5)
    ids = torch.tensor([PROMPT])
    base = m.generate(ids, max_new_tokens=60)
    e.enable_decode_graph(True)
    e.lookup_stats(reset=True)
    g = m.generate(ids, max_new_tokens=60, prompt_lookup_num_tokens=4)
    assert e.decode_graph_stats()["replays"] > 0 and e.lookup_stats()["accepted"] > 0
    e.enable_decode_graph(False)
    assert torch.equal(g, base)

    class S:
        def __init__(self):
            self.got = []
        def put(self, t):
            self.got.extend(int(x) for x in t.view(-1))
        def end(self):
            self.got.append("end")

    P = ids.shape[1]
    stop_id = int(base[0, P + 25])
    crit = lambda ids_, s: int(ids_[0, -1]) == stop_id
    s1, s2 = S(), S()
    a = m.generate(ids, max_new_tokens=60, streamer=s1, stopping_criteria=[crit])
    b = m.generate(ids, max_new_tokens=60, streamer=s2, stopping_criteria=[crit], prompt_lookup_num_tokens=10)
    assert torch.equal(a, b) and s1.got == s2.got
    assert int(b[0, -1]) == stop_id and b.shape[1] <= P + 26
    # EOS inside an accepted run, kept in the output
    eos = int(base[0, P + 30])
    a = m.generate(ids, max_new_tokens=60, eos_token_id=eos)
    b = m.generate(ids, max_new_tokens=60, eos_token_id=eos, prompt_lookup_num_tokens=10)
    assert torch.equal(a, b) and int(b[0, -1]) == eos
    # the cache is left as the greedy loop leaves it: every id but the last one cached
    assert e.kv_lengths(1)[0] == b.shape[1] - 1
    e.close()


def test_refusals(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor([PROMPT])
    m.forward(input_ids=ids, use_cache=True)
    before = e.kv_lengths(1)
    with pytest.raises(ValueError, match="batch_size = 1"):
        m.generate(torch.tensor([PROMPT, PROMPT]), prompt_lookup_num_tokens=4)
    with pytest.raises(NotImplementedError):
        m.generate(ids, prompt_lookup_num_tokens=4, do_sample=True, seed=1)
    with pytest.raises(NotImplementedError):
        m.generate(ids, prompt_lookup_num_tokens=4, num_beams=2)
    with pytest.raises(ValueError):
        m.generate(ids, prompt_lookup_num_tokens=0)
    with pytest.raises(ValueError):
        m.generate(ids, prompt_lookup_num_tokens=4, max_matching_ngram_size=0)
    with pytest.raises(ValueError, match="15"):
        m.generate(ids, prompt_lookup_num_tokens=16)
    e.enable_fp8_kv(True)
    with pytest.raises(NotImplementedError):
        m.generate(ids, prompt_lookup_num_tokens=4)
    e.enable_fp8_kv(False)
    assert e.kv_lengths(1) == before
    # the C ABI refuses a verify step past the cache and T outside 2 .. 16
    with pytest.raises(ValueError, match="T <= 16"):
        e.decode_verify([1])
    with pytest.raises(ValueError, match="T <= 16"):
        e.decode_verify([1] * 17)
    long_ids = torch.tensor([PROMPT * 9])                     # 117 slots: 117 + 16 > max_seq = 128
    m.forward(input_ids=long_ids, use_cache=True)
    with pytest.raises(ValueError, match="KV cache full"):
        e.decode_verify([1] * 16)
    assert e.kv_lengths(1) == [117]
    m.forward(input_ids=ids, use_cache=True)
    assert e.kv_lengths(1) == before
    # generation_config carries the setting too
    m.generation_config.prompt_lookup_num_tokens = 3
    e.lookup_stats(reset=True)
    m.generate(ids, max_new_tokens=40)
    assert e.lookup_stats()["verify_steps"] > 0
    m.generation_config.prompt_lookup_num_tokens = None
    e.close()


# ---------------------------------------------------------------------------------------------------------------- tensor parallelism
TP_BOUND = 0.012     # max |logit| difference of a bf16 verify step at TP = 2 / 4 against TP = 1 (tiny model): ~2 x the measured 5.7e-3


@pytest.mark.parametrize("tp", [2, 4])
def test_tp_verify_equals_tp1(gpu_lib, tp):
    from test_gpu_tp_single import Group, _run_ranks
    cfg = tiny(q_heads=4, kv_heads=2)
    sd = synth.state_dict(cfg, 13)
    ids = torch.tensor([PROMPT])
    # drafts from the TP = 1 greedy chain, each corrupted at a known index (length, index): n > 0 is compared, not only rejections
    plan = [(3, None), (7, 4), (15, 9), (7, 0), (5, 2)]

    def prefill(e):
        embeds, lengths, _ = e.splice(ids, None, None)
        logits, _ = e.prefill(embeds, lengths)
        return int(e.argmax(logits)[0])

    def drive(e, chain):
        got = [prefill(e)]
        res = []
        for ln, j in plan:
            d = list(chain[len(got):len(got) + ln])
            if j is not None:
                d[j] = (d[j] + 1) % 320
            picks, n, lg = e.decode_verify([got[-1]] + d, want_logits=True)
            res.append((picks.tolist(), n, e.kv_lengths(1)[0], lg.float().cpu()))
            got += picks.tolist()[:n + 1]
        return res

    e1 = Engine(cfg, dtype="bf16", max_seq=128, max_batch=1, max_tiles=1, vision=False)
    e1.load_state_dict(sd, strict=False)
    chain = [prefill(e1)]
    for _ in range(60):
        nxt, _ = e1.decode_step(torch.tensor([chain[-1]]))
        chain.append(int(nxt[0]))
    want = drive(e1, chain)
    e1.close()
    print(f"\nTP = 1 accepted per step: {[w[1] for w in want]}")
    assert sum(w[1] for w in want) > 0
    grp = Group(tp)
    engines, hooks = [], []
    for r in range(tp):
        e = Engine(cfg, dtype="bf16", max_seq=128, max_batch=1, max_tiles=1, tp_rank=r, tp_size=tp, comm=C.c_void_p(1), vision=False)
        h = grp.hook_for(r)
        _lib.check(gpu_lib.omchat_set_allreduce_hook(e.h, C.cast(h, C.c_void_p), None))
        e.load_state_dict(sd, strict=False)
        engines.append(e); hooks.append(h)
    res = _run_ranks(lambda r: drive(engines[r], chain), tp)
    # every rank holds the same picks, n and cache length
    for r in range(1, tp):
        assert [x[:3] for x in res[r]] == [x[:3] for x in res[0]]
    # against TP = 1: the same picks and n, up to the first pick that differs; that one must sit at a near-tie of the TP = 1 logits (the
    # ranks' partial sums are added in another order than one GPU adds them, so the logits differ in the last bits)
    diffs, first = [], None
    for k, ((p, n, L, _), (pw, nw, Lw, lw)) in enumerate(zip(res[0], want)):
        full = torch.cat([res[r][k][3] for r in range(tp)], dim=-1)
        m = min(n, nw) + 1
        diffs.append(float((full[:m] - lw[:m]).abs().max()))
        j = next((i for i in range(m) if p[i] != pw[i]), None)
        if j is not None:
            first = (k, j, _margin(lw[j]))
            break
        assert n == nw and L == Lw and p[:n + 1] == pw[:nw + 1]
    print(f"TP = {tp}: max |logit diff| against TP = 1 per step {['%.2e' % d for d in diffs]}; first differing pick {first}")
    assert max(diffs) < TP_BOUND
    if first is not None:
        assert first[2] < 2 * diffs[-1], (first, diffs[-1])      # the measured difference of that step could flip it
        assert first[0] > 0 or first[1] > 0          # not at the very first pick
    for e in engines:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- full depth (configs[1])
def test_full_depth_verify_and_lookup_generate_vs_oracle_fixture(gpu_lib):
    import fulldepth_sample as fs
    from omchat_amd.config import omchat13b
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", fs.FIXTURE)
    fx = np.load(path)
    forced = [int(t) for t in fx["forced"]]
    VOCAB, tol = 152064, 8e-3                 # f16 logits bound of the full-depth decode comparison (test_gpu_fulldepth.py)
    cfg = omchat13b()
    S = fs.N_TILES * 1024 + fs.N_TEXT
    e = Engine(cfg, dtype="f16", max_seq=S + len(forced) + 8, max_batch=1, max_tiles=fs.N_TILES, max_prefill_rows=S + 8)
    e.fill_synthetic(0)
    px, ids = fs.sample()
    feats = e.encode_images(px)
    embeds, lengths, _ = e.splice(ids, None, feats)
    logits, _ = e.prefill(embeds, [S])
    first = int(e.argmax(logits)[0])
    rows = []
    for c0 in range(0, len(forced), 8):
        _, _, lg = e.decode_verify(forced[c0:c0 + 8], keep_all=True, want_logits=True)
        rows += [lg[j].cpu() for j in range(lg.shape[0])]
    sync()
    assert e.kv_lengths(1)[0] == S + len(forced)
    errs = [fs.logit_rel(rows[k], fx["logit_samples"][k + 1]) for k in range(len(forced))]
    print(f"\nfull depth f16, teacher-forced verify steps (1 + 7): logits rel err {min(errs):.3e} .. {max(errs):.3e} (bound {tol})")
    assert max(errs) < tol
    # free-running generate(prompt_lookup_num_tokens=10) against the oracle's chain (margin rule of the free-running test)
    m = OmChatQwen2ForCausalLM(cfg.clone(), e)
    e.lookup_stats(reset=True)
    gen = m.generate(ids, images=px, max_new_tokens=len(forced), eos_token_id=[], prompt_lookup_num_tokens=10)[0, ids.shape[1]:].tolist()
    assert gen[0] == first and len(gen) == len(forced)
    errs0 = [fs.logit_rel(logits[0].cpu(), fx["logit_samples"][0])] + errs
    n_equal = 0
    for k in range(len(forced)):
        margin = float(fx["top_vals"][k][0] - fx["top_vals"][k][1])
        sigma = errs0[k] * math.sqrt(float(fx["logit_norm2"][k]) / VOCAB)
        if gen[k] != int(fx["top_ids"][k][0]):
            assert margin <= 6.0 * sigma, (k, margin, sigma)
            break
        n_equal += 1
    st = e.lookup_stats()
    print(f"full depth f16 prompt-lookup generation: the first {n_equal} of {len(forced)} ids are the oracle's; {st}")
    assert n_equal >= 1
    assert st["verify_steps"] > 0 and st["accepted"] > 0
    e.close()
