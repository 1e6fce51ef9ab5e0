"""GPU: generate(do_sample=True, num_return_sequences=N) with num_beams == 1.  The shared-prompt decode attention
(omchat_op_attn_shared) against an fp64 restatement and against poisoned cache slots; omchat_group_begin with the forked and the shared
form on the tiny decoder -- every pick against tests/sampling_ref.py on the step's own logits, eager and as a decode graph, the logits
against the fp32 oracle -- and generate() itself: shape, row order, reproducibility, EOS, the e4m3 cache and MXFP4 weights, an image prompt."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from gpu_util import CODE, DT, TOL, TOL_DEEP, ptr, rel, sync
import group_ref as gr
import oracle
import sampling_ref as sr
from omchat_amd import _lib, synth
from omchat_amd.config import tiny
from omchat_amd.engine import Engine

SCALE = 1.0 / np.sqrt(128.0)


# ---------------------------------------------------------------------------------------------------------------- op level
def _run_shared(lib, dt, q, k, v, G, N, P, L):
    rows, Hq, _ = q.shape
    Hkv, cap = k.shape[1], k.shape[2]
    ws_b = lib.omchat_op_attn_shared_ws(G, N, Hq, Hkv, P, L)
    assert ws_b > 0
    ws = torch.empty(ws_b // 4 + 64, dtype=torch.float32, device="cuda")
    out = torch.empty(rows, Hq, 128, dtype=DT[dt], device="cuda")
    _lib.check(lib.omchat_op_attn_shared(CODE[dt], ptr(q), ptr(k), ptr(v), ptr(out), G, N, Hq, Hkv, cap, P, L, float(SCALE), ptr(ws), ws_b, None))
    sync()
    return out


GS, NS, PS, DS = [1, 2], [2, 3, 16], [1, 63, 64, 65, 200], [1, 2, 64, 65, 130]
CAP = max(PS) + max(DS) + 6


def _kv(dt, Hkv, seed):
    g = torch.Generator().manual_seed(seed)
    rows = max(GS) * max(NS)
    k = torch.randn(rows, Hkv, CAP, 128, generator=g).to("cuda", DT[dt])
    v = torch.randn(rows, Hkv, CAP, 128, generator=g).to("cuda", DT[dt])
    return g, k, v


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("Hq,Hkv", [(28, 4), (7, 1), (4, 2)])
def test_op_attn_shared_vs_fp64_reference(gpu_lib, dt, Hq, Hkv):
    g, k, v = _kv(dt, Hkv, Hq * 100 + Hkv)
    worst = 0.0
    for G in GS:
        for N in NS:
            q = torch.randn(G * N, Hq, 128, generator=g).to("cuda", DT[dt])
            for P in PS:
                for d in DS:
                    L = P + d
                    out = _run_shared(gpu_lib, dt, q, k, v, G, N, P, L)
                    ref = gr.attn_shared_ref(q, k, v, G, N, P, L)
                    e = rel(out, ref)
                    e_rows = float(((out.double() - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)).max())
                    print(f"{dt} Hq={Hq} Hkv={Hkv} G={G} N={N} P={P} L={L}: rel err {e:.3e} worst row {e_rows:.3e}")
                    worst = max(worst, e, e_rows)
                    assert torch.isfinite(out.float()).all(), (G, N, P, L)
                    assert e < TOL[dt] and e_rows < TOL[dt], (G, N, P, L, e, e_rows)
    print(f"\n{dt} Hq={Hq} Hkv={Hkv}: worst rel err {worst:.2e}")


@pytest.mark.parametrize("Hq,Hkv", [(28, 4), (7, 1), (4, 2)])
def test_op_attn_shared_reads_the_leader_below_P_only(gpu_lib, Hq, Hkv):
    """the prefix pass must stop at exactly P in the leader's row (its slots >= P are its own suffix) and a sibling's slots < P must never be
    read: large finite values there leave the siblings' bits alone; slots >= L of every row are nobody's"""
    dt = "bf16"
    g, k, v = _kv(dt, Hkv, 7 * Hq + Hkv)
    for G, N in ((2, 3), (1, 16), (2, 2)):
        q = torch.randn(G * N, Hq, 128, generator=g).to("cuda", DT[dt])
        lead = torch.arange(G * N) % N == 0
        for P in (1, 63, 64, 65, 200):
            for d in (1, 2, 65):
                L = P + d
                base = _run_shared(gpu_lib, dt, q, k, v, G, N, P, L)
                assert rel(base, gr.attn_shared_ref(q, k, v, G, N, P, L)) < TOL[dt]
                # 1. nobody's slots: siblings below P, every row from L on -- every row keeps its bits
                kp, vp = k.clone(), v.clone()
                kp[:, :, L:] = 3e4; vp[:, :, L:] = -3e4
                for r in range(G * N):
                    if r % N:
                        kp[r, :, :P] = 3e4; vp[r, :, :P] = -3e4
                got = _run_shared(gpu_lib, dt, q, kp, vp, G, N, P, L)
                assert torch.equal(got.view(torch.int16), base.view(torch.int16)), (G, N, P, L)
                # 2. the leader's private suffix as well: the siblings keep their bits, the leader (which reads it) does not
                for r in range(G * N):
                    if r % N == 0:
                        kp[r, :, P:] = 3e4; vp[r, :, P:] = -3e4
                got = _run_shared(gpu_lib, dt, q, kp, vp, G, N, P, L)
                assert torch.equal(got[~lead].view(torch.int16), base[~lead].view(torch.int16)), (G, N, P, L)
                assert not torch.equal(got[lead].view(torch.int16), base[lead].view(torch.int16))


def test_op_attn_shared_refuses_bad_geometry(gpu_lib):
    q = torch.zeros(34, 28, 128, dtype=torch.bfloat16, device="cuda")
    k = torch.zeros(34, 4, 16, 128, dtype=torch.bfloat16, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    call = lambda G, N, P, L, Hq=28: gpu_lib.omchat_op_attn_shared(CODE["bf16"], ptr(q), ptr(k), ptr(k), ptr(q), G, N, Hq, 4, 16, P, L, 0.1, ptr(ws), 1 << 22, None)
    assert call(2, 17, 4, 8) != 0            # N > 16
    assert call(1, 2, 4, 4) != 0             # no own key
    assert call(1, 2, 0, 4) != 0             # no prompt
    assert call(1, 2, 4, 17) != 0            # beyond the capacity
    assert gpu_lib.omchat_op_attn_shared(CODE["bf16"], ptr(q), ptr(k), ptr(k), ptr(q), 1, 2, 28, 4, 16, 4, 8, 0.1, ptr(ws), 64, None) != 0      # workspace
    assert call(1, 2, 4, 8) == 0
    sync()


# ---------------------------------------------------------------------------------------------------------------- model level
PROMPT = [[3, 17, 18, 19, 20, 21, 7, 9], [5, 6, 11, 12, 13, 40, 41, 42]]
SP = dict(temperature=0.9, top_k=50, top_p=0.9, repetition_penalty=1.3)


def _tiny_model(max_batch=8, seed=21, dt="bf16", max_seq=128, **cfg_kw):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    cfg = tiny(**cfg_kw)
    sd = synth.state_dict(cfg, seed)
    e = Engine(cfg, dtype=dt, max_seq=max_seq, max_batch=max_batch, max_tiles=1, vision=False)
    e.load_state_dict(sd, strict=False)
    return cfg, e, OmChatQwen2ForCausalLM(cfg.clone(), e), sd


def _group_loop(e, m, ids, N, n, seed, share, graph=False, **p):
    """what generate(num_return_sequences=N) does, one step at a time: every pick checked against sampling_ref on the step's own logits with
    row index i*N + j.  -> (ids [b*N, n], the logits of every step)"""
    e.enable_decode_graph(graph)
    out = m.forward(input_ids=ids, use_cache=True)
    b = ids.shape[0]
    e.group_begin(b, N, share=share)
    assert e.kv_lengths(b * N) == [ids.shape[1]] * (b * N)
    seen = gr.seen_sets(ids.tolist(), N)
    kw = dict(temperature=p["temperature"], top_k=p["top_k"], top_p=p["top_p"], penalty=p["repetition_penalty"])
    e.set_sampling(b * N, seed=seed, seen=seen, **p)
    lg = out.local_logits.repeat_interleave(N, dim=0)
    tok = e.sample(lg)
    got, lgs = [], []
    for step in range(n):
        ref = sr.sample(lg.cpu().numpy(), seed, step, seen=seen, **kw)
        assert np.array_equal(tok.cpu().numpy(), ref), (step, tok.tolist(), ref)
        got.append(tok.cpu().numpy().astype(np.int64)); lgs.append(lg.cpu().numpy())
        for r in range(b * N):
            seen[r].append(int(ref[r]))
        tok, lg = e.decode_step(tok, want_logits=True)
    e.enable_decode_graph(False)
    return np.stack(got, 1), np.stack(lgs)


@pytest.mark.parametrize("share", [0, 1])
@pytest.mark.parametrize("b,N", [(1, 2), (1, 4), (2, 2), (2, 4)])
def test_group_steps_pick_what_the_ref_picks_eager_and_graph(gpu_lib, b, N, share):
    _, e, m, _ = _tiny_model()
    ids = torch.tensor(PROMPT[:b])
    eager, lg_e = _group_loop(e, m, ids, N, 10, 77, share, **SP)
    r0 = e.decode_graph_stats()["replays"]
    g, lg_g = _group_loop(e, m, ids, N, 10, 77, share, graph=True, **SP)
    assert e.decode_graph_stats()["replays"] > r0
    assert np.array_equal(g, eager)
    assert np.array_equal(lg_g.view(np.int32), lg_e.view(np.int32))      # eager and captured steps agree bit for bit
    # another (N, P) on the same context: the graph must not replay the old group's arguments
    ids2 = torch.tensor([p + [8, 9] for p in PROMPT[:1]])                    # (the same row count: b * N rows of one prompt)
    e2, _ = _group_loop(e, m, ids2, b * N, 6, 78, share, **SP)
    g2, _ = _group_loop(e, m, ids2, b * N, 6, 78, share, graph=True, **SP)
    assert np.array_equal(g2, e2)
    e.close()


def test_group_shared_wide_form_and_rewind(gpu_lib):
    """N = 16 x 7 query heads per kv head = 112 query rows (the eight-wave form); a rewound step is taken again with the same result"""
    _, e, m, _ = _tiny_model(max_batch=16)
    ids = torch.tensor(PROMPT[:1])
    a, _ = _group_loop(e, m, ids, 16, 5, 5, 1, **SP)
    f, _ = _group_loop(e, m, ids, 16, 5, 5, 0, **SP)
    print("wide: shared", a[:3].tolist(), "forked", f[:3].tolist())
    m.forward(input_ids=ids, use_cache=True)
    e.group_begin(1, 16, share=True)
    e.sampling_off()
    t0 = torch.arange(16, dtype=torch.int32) + 30
    _, lg1 = e.decode_step(t0, want_logits=True)
    _, lg2 = e.decode_step(t0 + 1, want_logits=True)
    e.kv_rewind(16, 1)
    _, lg2b = e.decode_step(t0 + 1, want_logits=True); sync()
    assert torch.equal(lg2, lg2b)
    e.close()


def _oracle_last(cfg, sdt, seq):
    cache = oracle.decoder.KVCache(cfg.text["num_hidden_layers"])
    emb = sdt["model.embed_tokens.weight"][torch.as_tensor(seq)]
    h = oracle.qwen2_model(emb.float()[None], sdt, cfg.text, cache)
    return oracle.lm_head(h, sdt)[0, -1]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_group_logits_vs_oracle_three_ways(gpu_lib, dt):
    """the same teacher-forced tokens through the shared form, the forked form and the plain step on the repeat_interleave'd batch: the last
    position's logits of every sibling against the fp32 oracle's forward of its whole sequence"""
    cfg, e, m, sd = _tiny_model(dt=dt)
    sdt = {k_: torch.from_numpy(v_).to(DT[dt]).float() for k_, v_ in sd.items()}
    b, N, steps = 2, 3, 70                               # 70 own keys: the suffix crosses a 64-key split
    ids = torch.tensor(PROMPT)
    g = torch.Generator().manual_seed(9)
    forced = torch.randint(1, 320, (steps, b * N), generator=g, dtype=torch.int32)
    ref = [_oracle_last(cfg, sdt, PROMPT[r // N] + forced[:, r].tolist()) for r in range(b * N)]
    e.sampling_off()
    for name in ("shared", "forked", "expanded"):
        if name == "expanded":
            m.forward(input_ids=ids.repeat_interleave(N, dim=0), use_cache=True)
        else:
            m.forward(input_ids=ids, use_cache=True)
            e.group_begin(b, N, share=name == "shared")
        for t in range(steps):
            _, lg = e.decode_step(forced[t], want_logits=True)
        sync()
        errs = [rel(lg[r], ref[r]) for r in range(b * N)]
        print(f"{dt} {name}: last-position logits vs the oracle, worst row rel err {max(errs):.3e} (tol {TOL_DEEP[dt]:g})")
        assert max(errs) < TOL_DEEP[dt], (name, errs)
    e.close()


def test_generate_num_return_sequences(gpu_lib):
    _, e, m, _ = _tiny_model()
    ids = torch.tensor(PROMPT)
    T = ids.shape[1]
    greedy = m.generate(ids, max_new_tokens=10)
    for share in (False, True, None):
        out = m.generate(ids, do_sample=True, seed=77, max_new_tokens=10, num_return_sequences=3, share_prompt=share, **SP)
        assert tuple(out.shape) == (6, T + 10)                                  # b * N rows (the parent returned b)
        assert torch.equal(out[:, :T], ids.repeat_interleave(3, dim=0))         # prompt-major
        loop, _ = _group_loop(e, m, ids, 3, 10, 77, bool(share), **SP)
        assert np.array_equal(out[:, T:].numpy(), loop), share
        assert torch.equal(out, m.generate(ids, do_sample=True, seed=77, max_new_tokens=10, num_return_sequences=3, share_prompt=share, **SP))
        # from generation_config too
        m.generation_config.num_return_sequences = 3
        assert torch.equal(out, m.generate(ids, do_sample=True, seed=77, max_new_tokens=10, share_prompt=share, **SP))
        m.generation_config.num_return_sequences = 1
        free = m.generate(ids, do_sample=True, seed=5, max_new_tokens=10, num_return_sequences=3, share_prompt=share, temperature=1.0, top_k=0)
        for i in range(2):
            assert len({tuple(r) for r in free[3 * i:3 * i + 3].tolist()}) > 1      # siblings draw with their own row keys
        one = m.generate(ids, do_sample=True, seed=5, max_new_tokens=10, num_return_sequences=3, share_prompt=share, top_k=1)
        assert torch.equal(one, greedy.repeat_interleave(3, dim=0))
        # the mode ended: a plain call is what it was on the fresh model
        assert torch.equal(m.generate(ids, max_new_tokens=10), greedy)
    e.close()


@pytest.mark.parametrize("share", [False, True])
def test_generate_group_eos_pads_only_its_row_and_logprobs_shape(gpu_lib, share):
    _, e, m, _ = _tiny_model()
    ids = torch.tensor(PROMPT[:1])
    T, N, new = ids.shape[1], 4, 10
    kw = dict(do_sample=True, seed=31, max_new_tokens=new, num_return_sequences=N, share_prompt=share, temperature=1.0, top_k=0)
    free = m.generate(ids, **kw)[:, T:].tolist()
    eos = next(t for t in free[0] if any(t not in r for r in free[1:]))
    pad = 0
    out = m.generate(ids, eos_token_id=eos, pad_token_id=pad, **kw)[:, T:].tolist()
    first = [r.index(eos) if eos in r else None for r in free]
    width = max(new if f is None else f + 1 for f in first)
    want = [(r if f is None else r[:f + 1] + [pad] * new)[:width] for r, f in zip(free, first)]
    assert out == want, (eos, out, want)
    assert any(f is None for f in first) and first[0] is not None
    res = m.generate(ids, return_dict_in_generate=True, output_logprobs=True, **kw)
    assert tuple(res.sequences.shape) == (N, T + new) and tuple(res.logprobs.shape) == (N, new) == tuple(res.processed_logprobs.shape)
    assert res.sequences[:, T:].tolist() == free and bool((res.logprobs <= 0).all())
    e.close()


def test_generate_group_forked_with_e4m3_cache_and_mxfp4_weights(gpu_lib):
    _, e, m, _ = _tiny_model(q_heads=4, kv_heads=2)
    ids = torch.tensor(PROMPT)
    e.enable_fp8_kv(True)
    a, _ = _group_loop(e, m, ids, 3, 8, 11, 0, **SP)                         # every pick is the ref's on the step's own logits
    out = m.generate(ids, do_sample=True, seed=11, max_new_tokens=8, num_return_sequences=3, share_prompt=False, **SP)
    assert np.array_equal(out[:, ids.shape[1]:].numpy(), a)
    out = m.generate(ids, do_sample=True, seed=11, max_new_tokens=8, num_return_sequences=3, **SP)      # the engine's rule: forked here
    assert np.array_equal(out[:, ids.shape[1]:].numpy(), a)
    with pytest.raises(NotImplementedError):
        m.generate(ids, do_sample=True, seed=11, max_new_tokens=8, num_return_sequences=3, share_prompt=True, **SP)
    m.forward(input_ids=ids, use_cache=True)
    with pytest.raises((ValueError, _lib.OmchatError)):
        e.group_begin(2, 3, share=True)                                      # the library refuses too, and leaves the rows alone
    assert e.kv_lengths(2) == [ids.shape[1]] * 2
    e.enable_fp8_kv(False)
    m.enable_mxfp4_decode(True, batched=True)
    for share in (0, 1):                                                     # attention does not see the weights
        x, _ = _group_loop(e, m, ids, 3, 8, 12, share, **SP)
        out = m.generate(ids, do_sample=True, seed=12, max_new_tokens=8, num_return_sequences=3, share_prompt=bool(share), **SP)
        assert np.array_equal(out[:, ids.shape[1]:].numpy(), x)
    e.close()


def test_group_mode_refusals_and_end(gpu_lib):
    from omchat_amd.engine import GROUP_SHARE_P_MIN
    _, e, m, _ = _tiny_model()
    # share_prompt=None: shared from the measured prompt length on, where the form is available
    assert not e.group_share_default(4, 8) and e.group_share_default(4, GROUP_SHARE_P_MIN) and not e.group_share_default(17, GROUP_SHARE_P_MIN)
    ids = torch.tensor(PROMPT[:1])
    m.forward(input_ids=ids, use_cache=True)
    e.group_begin(1, 4, share=True)
    e.sampling_off()
    tok = torch.tensor([4, 5, 6, 7], dtype=torch.int32)
    e.decode_step(tok)
    with pytest.raises((ValueError, _lib.OmchatError)):
        e.decode_step(tok[:2])                                               # all the group's rows or none
    with pytest.raises((ValueError, _lib.OmchatError)):
        e.decode_verify([4, 5, 6])
    with pytest.raises((ValueError, _lib.OmchatError)):
        e.beam_begin(1, 2, eos=[1], max_new=4)
    with pytest.raises((ValueError, _lib.OmchatError)):
        e.prefill_extend(torch.zeros(2, 256, dtype=torch.bfloat16, device="cuda"), 4)
    with pytest.raises((ValueError, _lib.OmchatError)):
        e.decode_step_masked(tok, torch.full((4,), 9), torch.ones(4, 10))
    assert e.kv_lengths(4) == [9] * 4
    e.group_end()
    e.decode_step(tok[:1])                                                   # an ordinary batch again (row 0 holds its whole sequence)
    m.forward(input_ids=ids, use_cache=True)
    with pytest.raises((ValueError, _lib.OmchatError)):
        e.group_begin(1, 9, share=False)                                     # b * N > max_batch
    with pytest.raises((ValueError, _lib.OmchatError)):
        e.group_begin(1, 4, prompt_len=5, share=False)                       # not the rows' length
    e.close()


def test_generate_group_image_prompt_runs_the_tower_once(gpu_lib):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    cfg = tiny()
    e = Engine(cfg, dtype="bf16", max_seq=256, max_batch=2, max_tiles=1)
    e.load_state_dict(synth.state_dict(cfg, 5))
    m = OmChatQwen2ForCausalLM(cfg.clone(), e)
    img = torch.from_numpy(synth.pixels(1, 56, 3)).to(torch.bfloat16).cuda()
    ids = torch.tensor([[3, -200, 17, 18, 19]])
    for share in (False, True):
        e.encode_stats(reset=True)
        out = m.generate(ids, images=img, do_sample=True, seed=3, max_new_tokens=6, num_return_sequences=2, share_prompt=share, **SP)
        assert tuple(out.shape) == (2, ids.shape[1] + 6) and torch.equal(out[:, :5], ids.repeat_interleave(2, dim=0))
        assert e.encode_stats() == dict(calls=1, tiles=1)                    # one prefill: the tile went through the tower once
        assert e.kv_lengths(2) == [4 + e.ntok + 6 - 1] * 2
    e.close()
