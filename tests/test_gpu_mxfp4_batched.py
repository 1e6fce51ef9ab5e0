"""MXFP4 weights on the packed batched decode path (omchat_enable_mxfp4_decode mode 2): steps of 2 <= b <= 32 rows --
batched, padded-batch, beam and prompt-lookup verify steps -- stream a packed copy of the MXFP4 replica through the MFMA-form GEMVs
(gemv_pk_mx4_kernel, gemv_xs_mx4_kernel, gemv_xs_split_mx4_kernel).  Parity is stated as tests/test_gpu_mxfp4.py states it: against fp64 /
the oracle on the DE-QUANTISED weights (tests/mxfp4_ref.py) at the tolerances of gpu_util: TOL for 16-bit outputs, TOL_DEEP for decoder
steps, 1e-4 relative for fp32 and split-K-sum outputs (the bound test_gemv_packed_operands uses for the same MFMA accumulation)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from gpu_util import DT, CODE, TOL, TOL_DEEP, dev, rnd, rel, sync, ptr, randn, synth_state_dict
from mxfp4_ref import dequant_ref
from omchat_amd import synth, _lib
from omchat_amd.config import tiny, omchat13b
from omchat_amd.engine import Engine
import oracle

DTS = ["bf16", "f16"]
T32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
EPI_NONE, EPI_SWIGLU, EPI_PARTIAL = _lib.EPI_NONE, _lib.EPI_SWIGLU, 5
F32_TOL = 1e-4
BASE_ROWS = 2048


def _dev_quant(w_dev, dt):
    N, K = w_dev.shape
    w4 = torch.empty(N, K // 2, dtype=torch.uint8, device="cuda")
    sc = torch.empty(N, K // 32, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().omchat_op_quant_mxfp4(CODE[dt], ptr(w_dev), N, K, ptr(w4), ptr(sc), None))
    sync()
    return w4, sc


@functools.lru_cache(maxsize=2)
def _case(dt, b, N, K, wscale):
    """-> (x on the device, row-major MXFP4 replica of w on the device, dequant_ref(w) @ x^T in fp64 as [b, N], bias).

    w = randn * wscale with a zero row, a zero block inside a non-zero row and a row with one dominant element per block.  dequant_ref costs
    about 0.1 s per million weights on the host, so a matrix of more than 2^24 weights is built from BASE_ROWS distinct rows: row r is row
    r % BASE_ROWS times 2^s(r), s in 0..3 changing from one 16-row tile to the next.  Scaling a row up by a power of two is exact in the 16-bit
    type and commutes with the quantiser (the block exponent moves by s, the codes stay), so dequant_ref(w)[r] = 2^s(r) dequant_ref(base)[r %
    BASE_ROWS] exactly, and its fp64 product with x likewise; the identity is asserted on a sample of rows below."""
    R = N if N * K <= (1 << 24) else BASE_ROWS
    base = rnd(randn((R, K), 1, wscale), dt)
    base[3] = 0
    base[4, 32:64] = 0
    base[7] = rnd(randn((K,), 7, wscale / 2), dt)
    base[7, 5::32] = rnd(torch.tensor(150.0 * wscale), dt)
    x = rnd(randn((b, K), 2, 0.5), dt)
    bias = rnd(randn((N,), 3, 5 * wscale), dt)
    deq = dequant_ref(base)
    acc = (deq @ x.double().t()).t().contiguous()                      # [b, R]
    if R == N:
        wd = dev(base, dt)
    else:
        r = torch.arange(N)
        idx, f = r % R, 2.0 ** ((r // R * 3 + r // 16) % 4).double()
        wd = dev(base, dt)[idx.cuda()] * f.to("cuda", DT[dt])[:, None]
        s = torch.randperm(N, generator=torch.Generator().manual_seed(5))[:48]
        ws = wd[s.cuda()].float().cpu()
        assert torch.equal(ws, base[idx[s]] * f[s, None].float())
        assert torch.equal(dequant_ref(ws), deq[idx[s]] * f[s, None])
        acc = acc[:, idx] * f[None, :]
    w4, sc = _dev_quant(wd.contiguous(), dt)
    return dev(x, dt), w4, sc, acc, bias


def _call(dt, xd, w4, sc, y, ldy, b, N, K, bias, epi, out_f32, ks, ypk):
    rc = _lib.lib().omchat_op_gemv_mxfp4_packed(CODE[dt], ptr(xd), K, ptr(w4), ptr(sc), ptr(y), ldy, b, N, K, ptr(bias), epi, out_f32, ks, ypk, None)
    sync()
    return rc


def _unpack_x(packed, b, K, NB):
    from test_gpu_round2 import _unpack_x as u
    return u(packed, b, K, NB)


def _check_all(dt, b, N, K, ks, wscale=0.02, swiglu=True):
    xd, w4, sc, acc, bias = _case(dt, b, N, K, wscale)
    NB = 2 if b > 16 else 1
    tag = f"MX4 packed gemv {dt} b={b} N={N} K={K} ks={ks} wscale={wscale:g}"
    out = torch.full((b, N), float("nan"), dtype=DT[dt], device="cuda")
    _lib.check(_call(dt, xd, w4, sc, out, N, b, N, K, dev(bias, dt), EPI_NONE, 0, 1, 0))
    e1 = rel(out, acc + bias.double()[None])
    outf = torch.full((b, N), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(_call(dt, xd, w4, sc, outf, N, b, N, K, None, EPI_NONE, 1, 1, 0))
    e2 = rel(outf, acc)
    part = torch.full((ks, b, N), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(_call(dt, xd, w4, sc, part, N, b, N, K, None, EPI_PARTIAL, 0, ks, 0))
    e3 = rel(part.sum(0), acc)
    print(f"{tag}: 16-bit + bias {e1:.3e} (tol {TOL[dt]:g}), fp32 {e2:.3e}, split-K sum {e3:.3e} (tol {F32_TOL:g})")
    assert e1 < TOL[dt], e1
    assert e2 < F32_TOL, e2
    assert bool(torch.isfinite(part).all()) and e3 < F32_TOL, e3
    # the all-zero row and the zero block: exact zeros come out of zero codes whatever the scale byte
    assert bool((outf[:, 3] == 0).all())
    if swiglu and N % 32 == 0 and (N // 2) % 64 == 0:
        a = acc.view(b, N // 32, 2, 16)
        g, u = rnd(a[:, :, 0].reshape(b, -1).float(), dt), rnd(a[:, :, 1].reshape(b, -1).float(), dt)
        ref = rnd(torch.nn.functional.silu(g), dt) * u
        o3 = torch.full((b, N // 2), float("nan"), dtype=DT[dt], device="cuda")
        _lib.check(_call(dt, xd, w4, sc, o3, N // 2, b, N, K, None, EPI_SWIGLU, 0, 1, 0))
        e4 = rel(o3, ref)
        print(f"{tag}: SwiGLU {e4:.3e} (tol {TOL[dt]:g})")
        assert e4 < TOL[dt], e4
        o4 = torch.zeros(NB * 16 * (N // 2), dtype=DT[dt], device="cuda")
        _lib.check(_call(dt, xd, w4, sc, o4, 0, b, N, K, None, EPI_SWIGLU, 0, 1, 1))
        assert torch.equal(_unpack_x(o4, b, N // 2, NB), o3.cpu())            # the same values, packed for the next GEMV


# (b, N, K, ks): the smallest shapes that reach each form and its ragged edges
SHAPES = [(2, 320, 512, 1),              # pk, NB = 1
          (17, 320, 576, 2),             # NB = 2, ragged batch, 9 chunks in two uneven slices
          (24, 160, 64, 1),              # one chunk: seven waves idle
          (5, 3584, 3584, 3),            # split-K that does not divide
          (32, 32768 + 64, 256, 1),      # the wide-output launch shape
          (16, 4608, 3584, 1),           # x-stationary, two tiles per workgroup (qkv)
          (3, 16384, 3584, 1),           # x-stationary, persistent
          (17, 32768, 3584, 1),          # x-stationary SwiGLU pairs, NB = 2
          (20, 3584, 18944, 8),          # x-stationary split, 7 x 40 + 16 chunks
          (8, 3584, 3584, 2)]            # x-stationary split at NB = 1: 40 + 16 chunks, two tiles per workgroup (o_proj)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("b,N,K,ks", SHAPES)
def test_packed_gemv_vs_dequantised_reference(gpu_lib, dt, b, N, K, ks):
    _check_all(dt, b, N, K, ks)


@pytest.mark.parametrize("b,N,K", [(17, 320, 576), (3, 16384, 3584)])
def test_packed_gemv_tiny_magnitude_weights_f16(gpu_lib, b, N, K):
    """weights of magnitude 1e-6 (f16 subnormals, block scales near 2^-22): a block scale folded into the f16 convert underflows and fails
    this; folded into the fp32 accumulator behind the MFMA it meets the ordinary tolerances.  The pk form and the x-stationary form.
    (Without the SwiGLU epilogue, as the batch-1 test: silu(g) u of two values near 3e-5 is 5e-10, below f16's smallest subnormal 6e-8 -- the
    reference's own output type holds nothing there.)"""
    _check_all("f16", b, N, K, 1, wscale=1e-6, swiglu=False)


@pytest.mark.parametrize("b,N,K", [(17, 320, 576), (16, 4608, 3584)])
def test_packed_gemv_is_deterministic(gpu_lib, b, N, K):
    dt = "bf16"
    xd, w4, sc, acc, bias = _case(dt, b, N, K, 0.02)
    outs = []
    for _ in range(2):
        y = torch.full((b, N), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(_call(dt, xd, w4, sc, y, N, b, N, K, None, EPI_NONE, 1, 1, 0))
        outs.append(y)
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])


def _np_packed_layout(w4, sc):
    """the packed image of a row-major replica (numpy, on the host), by the index formulas of test_mxfp4_batched_cpu (common.h restated)"""
    from test_mxfp4_batched_cpu import packed_w4_index, packed_s4_index
    N, K = w4.shape[0], w4.shape[1] * 2
    dw = w4.reshape(N, K // 8, 4).copy().view(np.uint32).reshape(N, K // 8)          # one little-endian dword per 8 codes
    rows, k8 = np.meshgrid(np.arange(N), np.arange(K // 8), indexing="ij")
    w4p = np.empty(N * K // 8, dtype=np.uint32)
    w4p[packed_w4_index(rows, k8 * 8, K)] = dw
    rows, blk = np.meshgrid(np.arange(N), np.arange(K // 32), indexing="ij")
    sp = np.empty(N * K // 32, dtype=np.uint8)
    sp[packed_s4_index(rows, blk, K)] = sc
    return w4p, sp


@pytest.mark.parametrize("b,N,K,ks", [(17, 320, 576, 2), (16, 4608, 3584, 1)])
def test_pack_entries_and_prepacked_launch(gpu_lib, b, N, K, ks):
    """omchat_op_pack_w4 writes the layout common.h documents (against the host restatement, every byte), and omchat_op_gemv_prepacked on
    operands packed once gives the bits of omchat_op_gemv_mxfp4_packed, which packs for the caller: a pk shape and an x-stationary shape,
    16-bit out + bias, fp32 out, split-K slices; the 16-bit twin (omchat_op_pack_w, SP = NULL) against omchat_op_gemv_packed"""
    lib, dt = _lib.lib(), "bf16"
    xd, w4, sc, acc, bias = _case(dt, b, N, K, 0.02)
    w4p = torch.empty(N * K // 8, dtype=torch.int32, device="cuda")
    sp = torch.empty(N * K // 32, dtype=torch.uint8, device="cuda")
    _lib.check(lib.omchat_op_pack_w4(ptr(w4), ptr(sc), N, K, ptr(w4p), ptr(sp), None)); sync()
    ref_w, ref_s = _np_packed_layout(w4.cpu().numpy(), sc.cpu().numpy())
    assert np.array_equal(w4p.cpu().numpy().view(np.uint32), ref_w) and np.array_equal(sp.cpu().numpy(), ref_s)
    NB = 2 if b > 16 else 1
    xp = torch.empty(NB * 16 * K, dtype=DT[dt], device="cuda")
    _lib.check(lib.omchat_op_pack_x(CODE[dt], ptr(xd), K, b, K, ptr(xp), None)); sync()
    bd = dev(bias, dt)
    for epi, f32, k_s, bi, shape, ty in ((EPI_NONE, 0, 1, bd, (b, N), DT[dt]), (EPI_NONE, 1, 1, None, (b, N), torch.float32),
                                         (EPI_PARTIAL, 0, ks, None, (ks, b, N), torch.float32)):
        y0 = torch.full(shape, float("nan"), dtype=ty, device="cuda")
        y1 = torch.full(shape, float("nan"), dtype=ty, device="cuda")
        _lib.check(_call(dt, xd, w4, sc, y0, N, b, N, K, bi, epi, f32, k_s, 0))
        _lib.check(lib.omchat_op_gemv_prepacked(CODE[dt], ptr(xp), ptr(w4p), ptr(sp), ptr(y1), N, b, N, K, ptr(bi), epi, f32, k_s, 0, None)); sync()
        assert bool(torch.isfinite(y0.float()).all()) and torch.equal(y0, y1), (epi, f32)
    # 16-bit weights through the same two entries
    W = dev(rnd(randn((N, K), 4, 0.03), dt), dt)
    wp = torch.empty_like(W)
    _lib.check(lib.omchat_op_pack_w(CODE[dt], ptr(W), K, N, K, ptr(wp), None)); sync()
    y0 = torch.full((b, N), float("nan"), dtype=torch.float32, device="cuda")
    y1 = torch.full((b, N), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib.omchat_op_gemv_packed(CODE[dt], ptr(xd), K, ptr(W), K, ptr(y0), N, b, N, K, None, EPI_NONE, 1, 1, 1, 0, None))
    _lib.check(lib.omchat_op_gemv_prepacked(CODE[dt], ptr(xp), ptr(wp), None, ptr(y1), N, b, N, K, None, EPI_NONE, 1, 1, 0, None)); sync()
    assert bool(torch.isfinite(y0).all()) and torch.equal(y0, y1)


def test_op_refusals(gpu_lib):
    lib = _lib.lib()
    dt = "bf16"

    def refused(b, N, K, what):
        x = torch.zeros(b, K, dtype=DT[dt], device="cuda")
        w4 = torch.full((N, K // 2), 0x22, dtype=torch.uint8, device="cuda")
        sc = torch.full((N, K // 32), 127, dtype=torch.uint8, device="cuda")
        y = torch.full((b, N), 7.0, dtype=DT[dt], device="cuda")
        assert _call(dt, x, w4, sc, y, N, b, N, K, None, EPI_NONE, 0, 1, 0) != 0
        assert what in lib.omchat_last_error(), lib.omchat_last_error()
        assert bool((y == 7.0).all())

    refused(4, 32, 96, b"K % 64")
    refused(4, 40, 64, b"N % 16")
    refused(33, 32, 64, b"b <= 32")
    # row-major operands: MXFP4 at b > 1 stays refused; b = 1 is the whole-row form
    N, K = 32, 64
    w = rnd(randn((N, K), 1, 0.02), dt)
    x = rnd(randn((3, K), 2, 0.5), dt)
    w4, sc = _dev_quant(dev(w, dt), dt)
    xd = dev(x, dt)
    y = torch.full((3, N), 7.0, dtype=torch.float32, device="cuda")
    assert lib.omchat_op_gemv_mxfp4_rows(CODE[dt], ptr(xd), K, ptr(w4), ptr(sc), ptr(y), N, 3, N, K, None, EPI_NONE, 1, 1, None) != 0
    assert b"batch 1 only" in lib.omchat_last_error()
    sync()
    assert bool((y == 7.0).all())
    assert lib.omchat_op_gemv_mxfp4_rows(CODE[dt], ptr(xd), K, ptr(w4), ptr(sc), ptr(y), N, 1, N, K, None, EPI_NONE, 1, 1, None) == 0
    sync()
    assert rel(y[0], dequant_ref(w) @ x[0].double()) < F32_TOL and bool((y[1:] == 7.0).all())


def test_mode_2_refusals(gpu_lib):
    """a geometry outside the packed path (vocabulary not a multiple of 16) is refused with the mode left as it was; a step of more than 32
    rows while mode 2 is on is refused before it touches any state"""
    cfg = tiny(vocab=328)
    e = Engine(cfg, dtype="bf16", max_seq=32, max_batch=1, vision=False)
    e.load_state_dict(_decoder_sd(cfg, 7))
    with pytest.raises(ValueError, match="multiple of 16"):
        e.enable_mxfp4_decode(True, batched=True)
    assert not getattr(e, "_mxfp4_decode", False) and not getattr(e, "_mxfp4_batched", False)
    e.enable_mxfp4_decode(True)                                            # mode 1 takes this geometry
    with pytest.raises(ValueError, match="multiple of 16"):
        e.enable_mxfp4_decode(True, batched=True)
    assert e._mxfp4_decode and not e._mxfp4_batched                        # and stays on
    e.close()
    cfg = tiny()
    b = 33
    e = Engine(cfg, dtype="bf16", max_seq=32, max_batch=b, vision=False)
    e.load_state_dict(_decoder_sd(cfg, 7))
    x = rnd(randn((b, 6, 256), 1, 0.5), "bf16")
    e.prefill(x, [6] * b)
    toks = torch.arange(5, 5 + b, dtype=torch.int32)
    n0, l0 = e.decode_step(toks, want_logits=True); sync()                 # 16 bits: b = 33 is an ordinary step
    e.prefill(x, [6] * b)
    e.enable_mxfp4_decode(True, batched=True)
    steps = e.decode_graph_stats()["steps"]
    with pytest.raises(ValueError, match="at most 32 rows"):
        e.decode_step(toks)
    assert e.kv_lengths(b) == [6] * b and e.decode_graph_stats()["steps"] == steps
    e.enable_mxfp4_decode(False)
    n1, l1 = e.decode_step(toks, want_logits=True); sync()                 # nothing was disturbed: the 16-bit step, bit for bit
    assert torch.equal(n0, n1) and torch.equal(l0, l1)
    e.close()


# ---------------------------------------------------------------------------------------------------------------- decoder level
def _decoder_sd(cfg, seed):
    return {k: T32(v) for k, v in synth.state_dict(cfg, seed).items() if not k.startswith(synth.TOWER) and "mm_projector" not in k}


def _dequant_decoder_weights(sd, dt):
    from test_gpu_mxfp4 import _dequant_decoder_weights as d
    return d(sd, dt)


def _oracle_rows(cfg, sd16, sdq, x, lens, rows, steps):
    """per checked row: prefill on the 16-bit weights, then the given tokens one by one on the de-quantised ones -> logits [row][step]"""
    out = {}
    for i in rows:
        cache = oracle.KVCache(cfg.text["num_hidden_layers"])
        oracle.qwen2_model(x[i:i + 1, :lens[i]], sd16, cfg.text, cache)
        out[i] = [oracle.decode_step(torch.tensor([[int(t[i])]]), sdq, cfg.text, cache)[0, 0] for t in steps]
    return out


@pytest.mark.parametrize("dt", DTS)
def test_batched_decode_vs_oracle_on_dequantised_weights(gpu_lib, dt):
    cfg = tiny(q_heads=4, kv_heads=2)
    sd = _decoder_sd(cfg, 3)
    sd16 = {k: rnd(v, dt) for k, v in sd.items()}
    sdq = _dequant_decoder_weights(sd16, dt)
    for b in (3, 20):
        e = Engine(cfg, dtype=dt, max_seq=64, max_batch=b, max_tiles=1, vision=False)
        e.load_state_dict(sd)
        S = 9
        x = rnd(randn((b, S, 256), b, 0.5), dt)
        lens = [S - (i % 4) for i in range(b)]
        e.prefill(x, lens)                                                   # the original weights, on both sides
        e.enable_mxfp4_decode(True, batched=True)
        toks = (torch.arange(b) % 300 + 5).to(torch.int32)
        nxt, lg = e.decode_step(toks, want_logits=True)
        nxt2, lg2 = e.decode_step(nxt, want_logits=True); sync()
        assert torch.equal(nxt.cpu().long(), torch.argmax(lg, dim=-1).cpu()) and torch.equal(nxt2.cpu().long(), torch.argmax(lg2, dim=-1).cpu())
        rows = range(b)                                                      # every row: both batch tiles and the ragged tail
        ref = _oracle_rows(cfg, sd16, sdq, x, lens, rows, [toks, nxt.cpu()])
        errs = [(rel(lg[i], ref[i][0]), rel(lg2[i], ref[i][1])) for i in rows]
        print(f"MX4 batched decode {dt} b={b}: worst row rel {max(r for r, _ in errs):.3e} {max(r for _, r in errs):.3e} (tol {TOL_DEEP[dt]:g})")
        for i, (r1, r2) in enumerate(errs):
            assert r1 < TOL_DEEP[dt] and r2 < TOL_DEEP[dt], (b, i, r1, r2)
        # the replica is really read: the same step on the 16-bit weights differs
        e.enable_mxfp4_decode(False)
        e.prefill(x, lens)
        _, lg16 = e.decode_step(toks, want_logits=True); sync()
        d = rel(lg, lg16)
        print(f"MX4 batched decode {dt} b={b}: relative logits difference against the 16-bit step {d:.4f}")
        assert d > 1e-3, d
        e.close()


def test_mode_1_leaves_batched_steps_on_16_bit_weights(gpu_lib):
    cfg = tiny()
    e = Engine(cfg, dtype="bf16", max_seq=64, max_batch=3, vision=False)
    e.load_state_dict(_decoder_sd(cfg, 7))
    x = rnd(randn((3, 8, 256), 1, 0.5), "bf16")
    toks = torch.tensor([5, 6, 7], dtype=torch.int32)
    e.prefill(x, [8, 8, 8])
    n0, l0 = e.decode_step(toks, want_logits=True)
    e.enable_mxfp4_decode(True)
    e.prefill(x, [8, 8, 8])
    n1, l1 = e.decode_step(toks, want_logits=True); sync()
    assert torch.equal(n0, n1) and torch.equal(l0, l1)
    e.close()


def test_full_width_layer_batch_32(gpu_lib):
    """one Qwen2-7B-width layer at b = 32: the production launch shapes (x-stationary qkv / gate|up, split o_proj and down_proj with 2 and 8 slices)"""
    dt = "bf16"
    cfg = omchat13b()
    cfg.text["num_hidden_layers"] = 1
    cfg.text["vocab_size"] = 2048
    b, S = 32, 12
    e = Engine(cfg, dtype=dt, max_seq=64, max_batch=b, vision=False)
    sd = {k: T32(v) for k, v in synth_state_dict(cfg, 0, lambda k: not k.startswith(synth.TOWER) and "mm_projector" not in k).items()}
    e.load_state_dict(sd)
    x = rnd(randn((b, S, 3584), 1, 0.5), dt)
    lens = [S - (i % 3) for i in range(b)]
    e.prefill(x, lens); sync()
    sdq = _dequant_decoder_weights(sd, dt)
    e.enable_mxfp4_decode(True, batched=True)
    toks = (torch.arange(b) % 500 + 5).to(torch.int32)
    nxt, lg = e.decode_step(toks, want_logits=True)
    _, lg2 = e.decode_step(nxt, want_logits=True); sync()
    rows = (0, 17, 31)
    ref = _oracle_rows(cfg, sd, sdq, x, lens, rows, [toks, nxt.cpu()])
    for i in rows:
        r1, r2 = rel(lg[i], ref[i][0]), rel(lg2[i], ref[i][1])
        print(f"MX4 full-width layer b=32 row {i}: rel {r1:.3e} {r2:.3e} (tol {TOL_DEEP[dt]:g})")
        assert r1 < TOL_DEEP[dt] and r2 < TOL_DEEP[dt], (i, r1, r2)
    e.close()


def test_reload_repacks_the_replica(gpu_lib):
    dt = "bf16"
    cfg = tiny(q_heads=4, kv_heads=2)
    sd = _decoder_sd(cfg, 7)
    e = Engine(cfg, dtype=dt, max_seq=64, max_batch=3, vision=False)
    e.load_state_dict(sd)
    x = rnd(randn((3, 10, 256), 5, 0.5), dt)
    lens = [10, 9, 8]
    toks = torch.tensor([3, 11, 200], dtype=torch.int32)
    e.enable_mxfp4_decode(True, batched=True)
    e.prefill(x, lens)
    _, lg_old = e.decode_step(toks, want_logits=True); sync()
    key = "model.layers.1.mlp.down_proj.weight"
    sd2 = dict(sd)
    sd2[key] = rnd(randn(tuple(sd[key].shape), 9, 0.05), dt)
    e.prefill(x, lens)                                                       # the cache of the ORIGINAL weights, as the oracle's
    e.load_tensor(key, sd2[key])
    _, lg = e.decode_step(toks, want_logits=True); sync()
    sd16 = {k: rnd(v, dt) for k, v in sd.items()}
    sdq2 = _dequant_decoder_weights({k: rnd(v, dt) for k, v in sd2.items()}, dt)
    ref = _oracle_rows(cfg, sd16, sdq2, x, lens, range(3), [toks])
    for i in range(3):
        assert rel(lg[i], ref[i][0]) < TOL_DEEP[dt], (i, rel(lg[i], ref[i][0]))
    assert rel(lg, lg_old) > 1e-3                                            # and it is not the old replica
    e.close()


def test_graph_replay_equals_eager_in_mode_2(gpu_lib):
    from test_gpu_graph import _run
    cfg = tiny()
    b = 3
    e = Engine(cfg, dtype="bf16", max_seq=256, max_batch=b, vision=False)
    e.load_state_dict(_decoder_sd(cfg, 3))
    x = rnd(randn((b, 10, 256), 1, 0.5), "bf16")
    lens = [10, 9, 8]
    first = torch.tensor([5, 6, 7], dtype=torch.int32)
    t16, _ = _run(e, x, lens, first, 6, False)
    e.enable_mxfp4_decode(True, batched=True)
    t0, l0 = _run(e, x, lens, first, 6, True)
    e.enable_decode_graph(True)
    t1, l1 = _run(e, x, lens, first, 6, True)
    st = e.decode_graph_stats()
    assert st["replays"] == 6 and st["captures"] == 1
    assert torch.equal(t0, t1) and torch.equal(l0, l1)
    # the format is part of the graph key: 2 -> 0 captures the 16-bit step, 0 -> 2 replays the first graph
    e.enable_mxfp4_decode(False)
    t2, _ = _run(e, x, lens, first, 6, False)
    assert torch.equal(t2, t16) and e.decode_graph_stats()["captures"] == 2
    e.enable_mxfp4_decode(True, batched=True)
    t3, l3 = _run(e, x, lens, first, 6, True)
    assert torch.equal(t3, t0) and torch.equal(l3, l0) and e.decode_graph_stats()["captures"] == 2
    e.close()


def test_prompt_lookup_in_mode_2(gpu_lib):
    from test_gpu_lookup import _tiny_model, _check_equal_or_near_tie, PROMPT
    dt = "bf16"
    _, e, m = _tiny_model(seed=5, dt=dt)
    m.enable_mxfp4_decode(True, batched=True)
    assert e._mxfp4_decode and e._mxfp4_batched
    ids = torch.tensor([PROMPT])
    base = m.generate(ids, max_new_tokens=40)
    e.lookup_stats(reset=True)
    got = m.generate(ids, max_new_tokens=40, prompt_lookup_num_tokens=3)
    st = e.lookup_stats()
    case = _check_equal_or_near_tie(e, m, ids, base, got, dt)
    print(f"MX4 lookup: {case}; {st}")
    assert st["verify_steps"] > 0 and got.shape == base.shape
    # verify rows (packed MXFP4, MFMA form) against single steps (row-major MXFP4, whole-row form) of the same engine
    T = 8
    toks = torch.randint(0, 320, (T,), generator=torch.Generator().manual_seed(T))
    m.forward(input_ids=ids, use_cache=True)
    _, _, lg_v = e.decode_verify(toks, keep_all=True, want_logits=True); sync()
    m.forward(input_ids=ids, use_cache=True)
    rows = [e.decode_step(torch.tensor([t]), want_logits=True)[1][0] for t in toks.tolist()]
    sync()
    for j in range(T):
        assert rel(lg_v[j], rows[j]) < TOL_DEEP[dt], (j, rel(lg_v[j], rows[j]))
    e.close()
    # batched=False: the refusal stands, before any work
    _, e, m = _tiny_model(seed=5, dt=dt)
    m.enable_mxfp4_decode(True)
    assert e._mxfp4_decode and not e._mxfp4_batched
    with pytest.raises(NotImplementedError, match="MXFP4"):
        m.generate(ids, max_new_tokens=4, prompt_lookup_num_tokens=3)
    assert e.kv_lengths(1) == [0]
    e.close()


def test_generate_batched_in_mode_2(gpu_lib):
    from test_gpu_beam import _tiny_model
    _, e, m = _tiny_model(b=4, seed=3)
    m.enable_mxfp4_decode(True, batched=True)
    ids = torch.tensor([[3, 17, 18, 19, 20, 21, 7, 9], [5, 6, 11, 12, 13, 40, 41, 42], [9, 8, 7, 6, 5, 4, 3, 2]])
    n, T = 8, 8
    out = m.generate(ids, max_new_tokens=n)
    assert out.shape == (3, T + n)
    # the same kernels from the same prefill, one engine-level step at a time: bit-equal ids
    tok = e.argmax(m.forward(input_ids=ids, use_cache=True).local_logits)
    got = [tok.cpu().tolist()]
    for _ in range(n - 1):
        tok, _ = e.decode_step(tok)
        got.append(tok.cpu().tolist())
    sync()
    assert torch.tensor(got).t().tolist() == out[:, T:].tolist()
    # sampled with log-probabilities: repeats under its seed, finite
    kw = dict(max_new_tokens=n, do_sample=True, seed=5, temperature=0.9, top_k=50, top_p=0.9, output_logprobs=True, return_dict_in_generate=True)
    a = m.generate(ids, **kw)
    b2 = m.generate(ids, **kw)
    assert torch.equal(a.sequences, b2.sequences)
    assert bool(torch.isfinite(a.logprobs).all()) and bool(torch.isfinite(a.processed_logprobs).all())
    # a right-padded batch of two takes the masked step
    pids = torch.tensor([[3, 17, 18, 19, 20, 21, 7, 9], [5, 6, 11, 12, 0, 0, 0, 0]])
    mask = torch.tensor([[1] * 8, [1] * 4 + [0] * 4])
    p1 = m.generate(pids, attention_mask=mask, max_new_tokens=n, pad_token_id=0)
    assert m._padded_batch
    p2 = m.generate(pids, attention_mask=mask, max_new_tokens=n, pad_token_id=0)
    assert torch.equal(p1, p2) and p1.shape == (2, T + n) and int(p1.max()) < 320 and int(p1.min()) >= 0
    e.close()


def test_beam_search_in_mode_2_smoke(gpu_lib):
    """smoke level only: beam search under quantised weights returns, repeats and replays; no score-level oracle"""
    from test_gpu_beam import _tiny_model, PROMPT
    _, e, m = _tiny_model()
    m.enable_mxfp4_decode(True, batched=True)
    ids = torch.tensor(PROMPT)
    kw = dict(num_beams=2, num_return_sequences=2, max_new_tokens=10, return_dict_in_generate=True)
    a = m.generate(ids, **kw)
    b2 = m.generate(ids, **kw)
    assert bool(torch.isfinite(a.sequences_scores).all())
    assert torch.equal(a.sequences, b2.sequences) and torch.equal(a.sequences_scores, b2.sequences_scores)
    e.enable_decode_graph(True)
    g = m.generate(ids, **kw)
    assert e.decode_graph_stats()["replays"] > 0
    e.enable_decode_graph(False)
    assert torch.equal(g.sequences, a.sequences) and torch.equal(g.sequences_scores, a.sequences_scores)
    e.close()
