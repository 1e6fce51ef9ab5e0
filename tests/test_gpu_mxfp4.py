"""Weight-only MXFP4 decode path (omchat_enable_mxfp4_decode).  The reference has no quantised path, so parity is
stated as tests/test_gpu_fp8.py states it: (1) the quantiser against the CPU reference (tests/mxfp4_ref.py), bit-exact; (2) the MXFP4 GEMV
forms and the whole decode step against the oracle run on the DE-QUANTISED weights, at the usual 16-bit tolerances.  The drift against the
16-bit step is printed, not bounded."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from gpu_util import DT, CODE, TOL, TOL_DEEP, dev, rnd, rel, sync, ptr, randn, synth_state_dict
from mxfp4_ref import quant_ref, dequant_ref, pack
from omchat_amd import synth, _lib
from omchat_amd.config import tiny, omchat13b
from omchat_amd.engine import Engine
import oracle

DTS = ["bf16", "f16"]
T32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
EPI_NONE, EPI_RESID, EPI_SWIGLU, EPI_PARTIAL = _lib.EPI_NONE, _lib.EPI_RESID, _lib.EPI_SWIGLU, 5


def dev_quant(w_dev, dt):
    lib = _lib.lib()
    N, K = w_dev.shape
    w4 = torch.empty(N, K // 2, dtype=torch.uint8, device="cuda")
    sc = torch.empty(N, K // 32, dtype=torch.uint8, device="cuda")
    _lib.check(lib.omchat_op_quant_mxfp4(CODE[dt], ptr(w_dev), N, K, ptr(w4), ptr(sc), None))
    sync()
    return w4, sc


def _quant_matrix(dt):
    w = rnd(randn((96, 1024), 0, 0.05), dt)
    w[3] = 0                                             # a zero row
    w[4, 64:96] = 0                                      # a zero block inside a non-zero row
    w[6] = rnd(torch.linspace(-1, 1, 1024), dt)          # dense grid coverage and ties
    w[7] = rnd(randn((1024,), 1, 0.01), dt)
    w[7, 5::32] = 3.0                                    # one dominant element per block
    w[8] = rnd(randn((1024,), 2, 1e-6), dt)              # the two ends of the exponent range
    w[9] = rnd(randn((1024,), 3, 1e3), dt)
    return w


@pytest.mark.parametrize("dt", DTS)
def test_quantiser_bit_exact(gpu_lib, dt):
    w = _quant_matrix(dt)
    w4, sc = dev_quant(dev(w, dt), dt)
    codes, s, _ = quant_ref(w)
    assert torch.equal(sc.cpu(), s)
    assert torch.equal(w4.cpu(), pack(codes))
    assert int(w4[3].max()) == 0 and bool((sc[3] == 127).all()) and int(sc[4, 2]) == 127 and int(w4[4, 32:48].max()) == 0
    assert int(sc[8].max()) < 127 - 15 and int(sc[9].min()) > 127


def _gemv(dt, xd, w4, sc, y, N, K, bias, resid, epi, out_f32, ks):
    _lib.check(_lib.lib().omchat_op_gemv_mxfp4(CODE[dt], ptr(xd), ptr(w4), ptr(sc), ptr(y), N, K, ptr(bias), ptr(resid), epi, out_f32, ks, None))
    sync()


def _case(dt, N, K, wscale=0.02, seed=1):
    w = rnd(randn((N, K), seed, wscale), dt)
    x = rnd(randn((K,), seed + 1, 0.5), dt)
    w4, sc = dev_quant(dev(w, dt), dt)
    acc = dequant_ref(w) @ x.double()
    return w, x, dev(x, dt), w4, sc, acc


def _check(dt, N, K, epi, ks=1, wscale=0.02):
    """one GEMV against dequant @ x in fp64; 16-bit outputs within TOL[dt], fp32 and partial outputs within 2e-5"""
    w, x, xd, w4, sc, acc = _case(dt, N, K, wscale)
    if epi == "partial":
        y = torch.empty(ks, N, dtype=torch.float32, device="cuda")
        _gemv(dt, xd, w4, sc, y, N, K, None, None, EPI_PARTIAL, 0, ks)
        err, tol = rel(y.sum(0), acc), 2e-5
    elif epi == "f32":
        bias = rnd(randn((N,), 3, 0.1 * wscale / 0.02), dt)
        y = torch.empty(N, dtype=torch.float32, device="cuda")
        _gemv(dt, xd, w4, sc, y, N, K, dev(bias, dt), None, EPI_NONE, 1, 1)
        err, tol = rel(y, acc + bias.double()), 2e-5
    elif epi == "none":
        bias = rnd(randn((N,), 3, 0.1 * wscale / 0.02), dt)
        y = torch.empty(N, dtype=DT[dt], device="cuda")
        _gemv(dt, xd, w4, sc, y, N, K, dev(bias, dt), None, EPI_NONE, 0, 1)
        err, tol = rel(y, acc + bias.double()), TOL[dt]
    elif epi == "resid":
        r = rnd(randn((N,), 4, 1.0), dt)
        y = torch.empty(N, dtype=DT[dt], device="cuda")
        _gemv(dt, xd, w4, sc, y, N, K, None, dev(r, dt), EPI_RESID, 0, 1)
        err, tol = rel(y, r.double() + rnd(acc.float(), dt).double()), TOL[dt]
    else:   # swiglu: rows interleaved in 16-row blocks [gate 16 | up 16]
        y = torch.empty(N // 2, dtype=DT[dt], device="cuda")
        _gemv(dt, xd, w4, sc, y, N, K, None, None, EPI_SWIGLU, 0, 1)
        a = acc.view(N // 32, 2, 16)
        g, u = rnd(a[:, 0].reshape(-1).float(), dt), rnd(a[:, 1].reshape(-1).float(), dt)
        err, tol = rel(y, rnd(torch.nn.functional.silu(g), dt) * u), TOL[dt]
    print(f"MX4 gemv {dt} N={N} K={K} {epi} ks={ks} wscale={wscale:g}: rel {err:.3e} (tol {tol:g})")
    assert err < tol, err


# shapes: N not a multiple of the rows per wave, one chunk | ragged last chunk (K % 32 == 0, K % 512 != 0) | eight chunks | the long-K forms
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N,K,epi,ks", [(70, 512, "none", 1), (64, 544, "none", 1), (64, 4096, "none", 1), (64, 18944, "resid", 1),
                                         (64, 18944, "partial", 8), (70, 544, "f32", 1), (70, 4096, "partial", 3), (70, 544, "resid", 1),
                                         (96, 544, "swiglu", 1), (64, 4096, "swiglu", 1)])
def test_gemv_vs_dequantised_reference(gpu_lib, dt, N, K, epi, ks):
    _check(dt, N, K, epi, ks)


@pytest.mark.parametrize("epi", ["none", "f32", "resid"])
def test_gemv_tiny_magnitude_weights_f16(gpu_lib, epi):
    """weights of magnitude 1e-6 (f16 subnormals; block scales near 2^-22): a block scale folded into the f16 convert underflows and fails this;
    applied to the fp32 partial sum it meets the ordinary tolerance.  The long-K form too."""
    _check("f16", 70, 544, epi, 1, wscale=1e-6)
    if epi == "resid":
        w, x, xd, w4, sc, acc = _case("f16", 64, 18944, 1e-6)
        r = rnd(randn((64,), 4, 1e-4), "f16")
        y = torch.empty(64, dtype=torch.float16, device="cuda")
        _gemv("f16", xd, w4, sc, y, 64, 18944, None, dev(r, "f16"), EPI_RESID, 0, 1)
        assert rel(y, r.double() + rnd(acc.float(), "f16").double()) < TOL["f16"]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N,K,epi", [(70, 544, "none"), (4608, 3584, "none"), (64, 4096, "f32"), (96, 544, "swiglu"), (2048, 3584, "swiglu")])
def test_gemv_norm_vs_rmsnorm_then_dequantised_matmul(gpu_lib, dt, N, K, epi):
    """the RMSNorm in the GEMV's registers (qkv, gate|up, lm_head of a batch-1 step): y = epi(dequant @ T(w * T(x * rsqrt(mean x^2 + eps))))"""
    lib = _lib.lib()
    w = rnd(randn((N, K), 1, 0.02), dt)
    x = rnd(randn((K,), 2, 1.5), dt)
    nw = rnd(randn((K,), 5, 0.05) + 1, dt)
    w4, sc = dev_quant(dev(w, dt), dt)
    xn = rnd(nw * rnd(x * torch.rsqrt(x.pow(2).mean() + 1e-6), dt), dt)
    acc = dequant_ref(w) @ xn.double()
    xd, nd = dev(x, dt), dev(nw, dt)
    if epi == "swiglu":
        y = torch.empty(N // 2, dtype=DT[dt], device="cuda")
        _lib.check(lib.omchat_op_gemv_mxfp4_norm(CODE[dt], ptr(xd), ptr(w4), ptr(sc), ptr(y), N, K, ptr(nd), 1e-6, None, EPI_SWIGLU, 0, None)); sync()
        a = acc.view(N // 32, 2, 16)
        g, u = rnd(a[:, 0].reshape(-1).float(), dt), rnd(a[:, 1].reshape(-1).float(), dt)
        err, tol = rel(y, rnd(torch.nn.functional.silu(g), dt) * u), TOL[dt]
    else:
        f32 = epi == "f32"
        bias = rnd(randn((N,), 3, 0.1), dt)
        y = torch.empty(N, dtype=torch.float32 if f32 else DT[dt], device="cuda")
        _lib.check(lib.omchat_op_gemv_mxfp4_norm(CODE[dt], ptr(xd), ptr(w4), ptr(sc), ptr(y), N, K, ptr(nd), 1e-6, ptr(dev(bias, dt)), EPI_NONE,
                                                 int(f32), None)); sync()
        # fp32 out keeps TOL[dt] here, as the 16-bit norm-in-GEMV tests do: the device's rsqrt may differ from torch's in the last bit, which
        # moves single elements of the 16-bit xn by one 16-bit step -- an error of the reference's own rounding points, above 2e-5
        err, tol = rel(y, acc + bias.double()), TOL[dt]
    print(f"MX4 gemv_norm {dt} N={N} K={K} {epi}: rel {err:.3e}")
    assert err < tol, err


@pytest.mark.parametrize("N,K,epi", [(4608, 3584, "none"), (8192 + 64, 2048, "swiglu"), (4100, 3000 + 8, "none")])
def test_gemv_norm_loop_form_is_bit_identical(gpu_lib, N, K, epi):
    """the loop form of the norm-in-GEMV launches (tuning key 16) on MXFP4 weights against the one-shot form: the same bits; ragged K, output
    counts that do not divide by the grid"""
    lib, dt = _lib.lib(), "bf16"
    w = rnd(randn((N, K), 1, 0.02), dt); x = rnd(randn((K,), 2, 1.5), dt); nw = rnd(randn((K,), 5, 0.05) + 1, dt); bias = rnd(randn((N,), 4), dt)
    w4, sc = dev_quant(dev(w, dt), dt)
    xd, nd, bd = dev(x, dt), dev(nw, dt), dev(bias, dt)
    code = EPI_SWIGLU if epi == "swiglu" else EPI_NONE
    outs = []
    try:
        for key in (0, 15):
            lib.omchat_op_set_tuning(16, key)
            y = torch.full((N // 2 if epi == "swiglu" else N,), float("nan"), dtype=DT[dt], device="cuda")
            _lib.check(lib.omchat_op_gemv_mxfp4_norm(CODE[dt], ptr(xd), ptr(w4), ptr(sc), ptr(y), N, K, ptr(nd), 1e-6,
                                                     None if epi == "swiglu" else ptr(bd), code, 0, None))
            sync()
            outs.append(y)
    finally:
        lib.omchat_op_set_tuning(16, 0)
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1])


def _decoder_sd(cfg, seed):
    return {k: T32(v) for k, v in synth.state_dict(cfg, seed).items() if not k.startswith(synth.TOWER) and "mm_projector" not in k}


def _dequant_decoder_weights(sd, dt):
    out = dict(sd)
    for k, v in sd.items():
        if (".self_attn." in k or ".mlp." in k or k == "lm_head.weight") and k.endswith("weight") and "layernorm" not in k:
            out[k] = dequant_ref(rnd(v, dt)).float()
    return out


def test_refusals(gpu_lib):
    lib = _lib.lib()
    cfg = tiny()
    e = Engine(cfg, dtype="bf16", max_seq=32, max_batch=1, vision=False)
    with pytest.raises(ValueError, match="load the weights"):      # before the weights are loaded
        e.enable_mxfp4_decode()
    assert not getattr(e, "_mxfp4_decode", False)
    e.load_state_dict(_decoder_sd(cfg, 7))
    e.enable_fp8_decode(True)
    with pytest.raises(ValueError, match="one weight format"):
        e.enable_mxfp4_decode()
    e.enable_fp8_decode(False)
    e.enable_mxfp4_decode(True)
    with pytest.raises(ValueError, match="one weight format"):
        e.enable_fp8_decode(True)
    e.enable_fp8_kv(True); e.enable_fp8_kv(False)                   # orthogonal modes stay allowed
    e.enable_mxfp4_decode(False)
    e.enable_fp8_decode(True); e.enable_fp8_decode(False)
    e.close()
    # K % 32 != 0 at the op level: refused by the quantiser and by the GEMV, nothing enqueued
    w = torch.zeros(8, 80, dtype=torch.bfloat16, device="cuda")
    w4 = torch.full((8, 40), 0x55, dtype=torch.uint8, device="cuda"); sc = torch.full((8, 3), 0x55, dtype=torch.uint8, device="cuda")
    y = torch.full((8,), 7.0, dtype=torch.bfloat16, device="cuda")
    assert lib.omchat_op_quant_mxfp4(CODE["bf16"], ptr(w), 8, 80, ptr(w4), ptr(sc), None) != 0
    assert b"32" in lib.omchat_last_error()
    assert lib.omchat_op_gemv_mxfp4(CODE["bf16"], ptr(w), ptr(w4), ptr(sc), ptr(y), 8, 80, None, None, EPI_NONE, 0, 1, None) != 0
    assert b"32" in lib.omchat_last_error()
    sync()
    assert bool((w4 == 0x55).all()) and bool((sc == 0x55).all()) and bool((y == 7.0).all())


def test_generate_refuses_prompt_lookup(gpu_lib):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    cfg = tiny()
    e = Engine(cfg, dtype="bf16", max_seq=128, max_batch=1, max_tiles=1, vision=False)
    e.load_state_dict(synth.state_dict(cfg, 3), strict=False)
    m = OmChatQwen2ForCausalLM(cfg.clone(), e)
    m.enable_mxfp4_decode(True)
    assert e._mxfp4_decode
    ids = torch.tensor([[3, 17, 18, 19, 20, 21, 7, 9]])
    with pytest.raises(NotImplementedError, match="MXFP4"):
        m.generate(ids, max_new_tokens=4, prompt_lookup_num_tokens=3)
    assert e.kv_lengths(1) == [0]                                    # no prefill was enqueued
    m.enable_mxfp4_decode(False)
    assert m.generate(ids, max_new_tokens=4, prompt_lookup_num_tokens=3).shape[1] > ids.shape[1]      # off again: accepted
    e.close()


@pytest.mark.parametrize("dt", DTS)
def test_decode_vs_oracle_on_dequantised_weights(gpu_lib, dt):
    cfg = tiny()
    e = Engine(cfg, dtype=dt, max_seq=64, max_batch=1, vision=False)
    sd = _decoder_sd(cfg, 7)
    e.load_state_dict(sd)
    x = rnd(randn((1, 24, 256), 5, 0.5), dt)
    logits, _ = e.prefill(x); sync()
    cache = oracle.KVCache(cfg.text["num_hidden_layers"])
    h = oracle.qwen2_model(x, sd, cfg.text, cache)                         # prefill: 16-bit weights on both sides
    assert rel(logits[0], oracle.lm_head(h, sd)[0, -1]) < TOL_DEEP[dt]
    sdq = _dequant_decoder_weights(sd, dt)
    e.enable_mxfp4_decode(True)
    for tok in (3, 11, 200):
        nxt, lg = e.decode_step(torch.tensor([tok]), want_logits=True); sync()
        ref = oracle.decode_step(torch.tensor([[tok]]), sdq, cfg.text, cache)[0, 0]
        assert rel(lg[0], ref) < TOL_DEEP[dt], rel(lg[0], ref)
        assert int(nxt[0]) == int(torch.argmax(lg[0]))
    # the replica is really read: off and on again across a prefill, the step differs from the 16-bit one (the floor of the fp8 test)
    e.enable_mxfp4_decode(False)
    e.prefill(x)
    _, lg16 = e.decode_step(torch.tensor([3]), want_logits=True)
    e.enable_mxfp4_decode(True)
    e.prefill(x)
    _, lg4 = e.decode_step(torch.tensor([3]), want_logits=True); sync()
    d = rel(lg4[0], lg16[0])
    print(f"MX4 tiny decoder {dt}: relative logits difference against the 16-bit step d = {d:.4f}")
    assert d > 1e-3, d
    # ---- reload: one projection replaced, the next step streams the re-quantised replica (the stale flag)
    sd2 = dict(sd)
    key = "model.layers.1.mlp.down_proj.weight"
    sd2[key] = rnd(randn(tuple(sd[key].shape), 9, 0.05), dt)
    cache2 = oracle.KVCache(cfg.text["num_hidden_layers"])
    oracle.qwen2_model(x, sd, cfg.text, cache2)
    e.prefill(x)                                                           # the cache of the ORIGINAL weights, as the oracle's
    e.load_tensor(key, sd2[key])
    sdq2 = _dequant_decoder_weights(sd2, dt)
    _, lg = e.decode_step(torch.tensor([3]), want_logits=True); sync()
    ref = oracle.decode_step(torch.tensor([[3]]), sdq2, cfg.text, cache2)[0, 0]
    assert rel(lg[0], ref) < TOL_DEEP[dt], rel(lg[0], ref)
    assert rel(lg[0], lg4[0]) > 1e-3                                       # and it is not the old replica
    e.close()


@pytest.mark.parametrize("dt", ["bf16"])
def test_full_width_layer_mxfp4_decode(gpu_lib, dt):
    """one Qwen2-7B-width layer: the production launch shapes (norm-in-GEMV qkv / gate|up / lm_head, seven-wave o_proj, long-K down_proj)"""
    cfg = omchat13b()
    cfg.text["num_hidden_layers"] = 1
    cfg.text["vocab_size"] = 2048
    e = Engine(cfg, dtype=dt, max_seq=512, max_batch=1, vision=False)
    sd = {k: T32(v) for k, v in synth_state_dict(cfg, 0, lambda k: not k.startswith(synth.TOWER) and "mm_projector" not in k).items()}
    e.load_state_dict(sd)
    x = rnd(randn((1, 100, 3584), 1, 0.5), dt)
    e.prefill(x); sync()
    cache = oracle.KVCache(1)
    oracle.qwen2_model(x, sd, cfg.text, cache)
    sdq = _dequant_decoder_weights(sd, dt)
    e.enable_mxfp4_decode(True)
    for tok in (5, 9):
        nxt, lg = e.decode_step(torch.tensor([tok]), want_logits=True); sync()
        ref = oracle.decode_step(torch.tensor([[tok]]), sdq, cfg.text, cache)[0, 0]
        assert rel(lg[0], ref) < TOL_DEEP[dt], rel(lg[0], ref)
    e.close()


def test_graph_replay_equals_eager_with_the_mxfp4_replica(gpu_lib):
    from test_gpu_graph import _run
    cfg = tiny()
    e = Engine(cfg, dtype="bf16", max_seq=256, max_batch=1, vision=False)
    e.load_state_dict(_decoder_sd(cfg, 3))
    x = rnd(randn((1, 10, 256), 1, 0.5), "bf16")
    first = torch.tensor([5], dtype=torch.int32)
    t16, _ = _run(e, x, [10], first, 6, False)
    e.enable_mxfp4_decode(True)
    t0, l0 = _run(e, x, [10], first, 6, True)
    e.enable_decode_graph(True)
    t1, l1 = _run(e, x, [10], first, 6, True)
    st = e.decode_graph_stats()
    assert st["replays"] == 6 and st["captures"] == 1
    assert torch.equal(t0, t1) and torch.equal(l0, l1)
    # the mode is part of the graph key: off -> a second capture (16-bit), on again -> the first graph is replayed
    e.enable_mxfp4_decode(False)
    t2, _ = _run(e, x, [10], first, 6, False)
    assert torch.equal(t2, t16) and e.decode_graph_stats()["captures"] == 2
    e.enable_mxfp4_decode(True)
    t3, l3 = _run(e, x, [10], first, 6, True)
    assert torch.equal(t3, t0) and torch.equal(l3, l0) and e.decode_graph_stats()["captures"] == 2
    e.close()


def test_generate_with_the_mxfp4_replica(gpu_lib):
    """greedy ids equal those of engine-level steps on a second engine whose decoder weights were replaced, after the prefill, by the de-quantised
    ones (exactly representable in f16, so the two differ in fp32 summation order only); a sampled run with logprobs repeats under its seed"""
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    dt, n = "f16", 8
    cfg = tiny()
    sd = synth.state_dict(cfg, 3)
    e = Engine(cfg, dtype=dt, max_seq=128, max_batch=1, max_tiles=1, vision=False)
    e.load_state_dict(sd, strict=False)
    m = OmChatQwen2ForCausalLM(cfg.clone(), e)
    m.enable_mxfp4_decode(True)
    ids = torch.tensor([[3, 17, 18, 19, 20, 21, 7, 9]])
    T = ids.shape[1]
    out = m.generate(ids, max_new_tokens=n)
    assert out.shape == (1, T + n)
    # second engine: prefill on the original weights, then the de-quantised decoder weights for the steps
    e2 = Engine(cfg, dtype=dt, max_seq=128, max_batch=1, max_tiles=1, vision=False)
    e2.load_state_dict(sd, strict=False)
    m2 = OmChatQwen2ForCausalLM(cfg.clone(), e2)
    tok = torch.argmax(m2.forward(input_ids=ids, use_cache=True).local_logits, dim=-1).to(torch.int32)
    assert int(tok[0]) == int(out[0, T])
    sdq = _dequant_decoder_weights({k: T32(v) for k, v in sd.items()}, dt)
    e2.load_state_dict(sdq, strict=False)
    got = [int(tok[0])]
    for _ in range(n - 1):
        tok, _ = e2.decode_step(tok)
        got.append(int(tok[0]))
    sync()
    assert got == out[0, T:].tolist(), (got, out[0, T:].tolist())
    e2.close()
    # sampled, with log-probabilities: finite, and the same ids under the same seed
    kw = dict(max_new_tokens=n, do_sample=True, seed=5, temperature=0.9, top_k=50, top_p=0.9, output_logprobs=True, return_dict_in_generate=True)
    a = m.generate(ids, **kw)
    b = m.generate(ids, **kw)
    assert torch.equal(a.sequences, b.sequences)
    assert bool(torch.isfinite(a.logprobs).all()) and bool(torch.isfinite(a.processed_logprobs).all())
    e.close()
