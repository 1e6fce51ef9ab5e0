"""GPU: direct tests of the kernels every forward pass goes through but only whole-model runs reached: left-padded prefill attention
(AttnArgs.kv_start, launch_attn_uniform_rows), rope_kv_kernel's pos[] / slot0 paths, argmax with a row stride, the copy / gather kernels,
tp_finish and the norm family at the widths where a thread's chunk count changes.  References: tests/glue_ref.py (checked on the CPU by
tests/test_glue_ref_cpu.py) and the oracle.  Every output buffer starts as NaN, every row padding holds a sentinel that must survive."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
from gpu_util import DT, CODE, TOL, dev, rnd, rel, ptr, sync, randn
from omchat_amd import _lib
import glue_ref as gr
import oracle

DTS = ["bf16", "f16"]
NAN = float("nan")
SENT = 777.0            # row-padding sentinel, exact in both 16-bit types


def nan_like(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def strided(t, ld, dtype):
    """device buffer [rows, ld] holding t [rows, H] (cast to dtype) in its first H columns and the sentinel in the padding"""
    buf = torch.full((t.shape[0], ld), SENT, dtype=dtype, device="cuda")
    buf[:, :t.shape[1]] = t.to("cuda", dtype)
    return buf


def pad_ok(buf, H):
    return bool((buf[:, H:] == SENT).all())


# ------------------------------------------------------------------------------------------------ left-padded prefill attention
S_ATT = 330
STARTS = [0, 63, 64, 65, 129, 200]            # none; just before, on and just after a 64-key tile edge; inside tile 2; tile 3 (query blocks wholly in the padding)
LENS_SHORT = [330, 330, 300, 330, 257, 330]   # two rows end before Skv (257 = four tiles + one key): both masks in one tile walk
PAD_K, PAD_V = 24.0, 1000.0                   # masked K / V rows: finite, and a leaked key takes the softmax over (score ~ 24 * sum(q) * scale) and drags the output towards 1000


def _left_inputs(dt, Hq, Hkv, lens):
    b = len(STARTS)
    q = rnd(randn((b, S_ATT, Hq, 128), 1), dt); k = rnd(randn((b, Hkv, S_ATT, 128), 2), dt); v = rnd(randn((b, Hkv, S_ATT, 128), 3), dt)
    for i, s in enumerate(STARTS):
        k[i, :, :s] = PAD_K; v[i, :, :s] = PAD_V
        k[i, :, lens[i]:] = PAD_K; v[i, :, lens[i]:] = PAD_V
    return q, k, v


def _left_case(lib, dt, Hq, Hkv, causal, lens_arg, gen):
    b, S, T = len(STARTS), S_ATT, DT[dt]
    lens = lens_arg or [S] * b
    q, k, v = _left_inputs(dt, Hq, Hkv, lens)
    dq, dk, dv = dev(q, dt), dev(k, dt), dev(v, dt)
    dstart = i32(STARTS); dlen = None if lens_arg is None else i32(lens)
    scale = 128 ** -0.5
    tag = (dt, Hq, Hkv, causal, lens_arg is not None, gen)

    def run(fill):
        out = nan_like((b, S, Hq, 128), T)
        _lib.check(lib.omchat_op_attn_prefill_left(CODE[dt], ptr(dq), ptr(dk), ptr(dv), ptr(out), b, S, S, Hq, Hkv, ptr(dlen), ptr(dstart), causal, 0,
                                                   scale, fill, None))
        sync()
        return out

    plain = run(0)
    ref = gr.attn_left(q, k, v, scale, causal, 0, lens, STARTS)
    assert torch.isfinite(plain.float()).all(), (tag, "unwritten or non-finite rows")
    for i, s in enumerate(STARTS):
        r = rel(plain[i, s:], ref[i, s:])
        print("left-padded attention", tag, "seq", i, "start", s, "rel", r)
        assert r < TOL[dt], (tag, i, r)
        # the same rows with the padding physically removed: queries and keys shifted by `start`, so q_pos0 stays 0
        n = S - s
        q1, k1, v1 = dq[i:i + 1, s:].contiguous(), dk[i:i + 1, :, s:].contiguous(), dv[i:i + 1, :, s:].contiguous()
        l1 = i32([lens[i] - s])
        cut = nan_like((1, n, Hq, 128), T)
        _lib.check(lib.omchat_op_attn_prefill(CODE[dt], ptr(q1), ptr(k1), ptr(v1), ptr(cut), 1, n, n, Hq, Hkv, ptr(l1), causal, 0, scale, None))
        sync()
        r2 = rel(plain[i, s:], cut[0])
        print("   against the unpadded call: rel", r2)
        assert r2 < TOL[dt], (tag, i, r2)
        if s == 0:
            continue
        if causal:
            # model.hip: "the flash kernel leaves exactly 0" in the query rows that see no key (with tensor parallelism nothing overwrites them)
            assert bool((plain[i, :s] == 0).all()), (tag, i, "padded query rows are not exactly 0")
        else:
            # without the causal mask a padded QUERY row still sees every valid key (kernels.h AttnArgs): an ordinary row
            rp = rel(plain[i, :s], ref[i, :s])
            assert rp < TOL[dt], (tag, i, rp)
    filled = run(1)
    uni = gr.uniform_rows(v, T)                                   # [b, Hkv, 128] fp64, all Skv rows, the padding rows included
    rep = Hq // Hkv
    for i, s in enumerate(STARTS):
        assert torch.equal(filled[i, s:], plain[i, s:]), (tag, i, "the fill touched a valid row")
        if s == 0:
            continue
        want = uni[i].repeat_interleave(rep, dim=0)[None].expand(s, Hq, 128)
        ru = rel(filled[i, :s], want)
        print("   uniform rows: rel", ru)
        assert ru < TOL[dt], (tag, i, ru)
        assert bool((filled[i, :s] == filled[i, 0:1]).all())      # one value per (head, column) in every padded row


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Hq,Hkv", [(7, 1), (4, 2), (3, 3)])
@pytest.mark.parametrize("gen", [1, 0])
def test_attn_prefill_left_padded(gpu_lib, dt, Hq, Hkv, gen):
    """kv_start in both prefill kernels (gen 0: tuning key 8 = 0, the first-generation kernel): skipped key tiles (t_begin), the partial tile
    masked from below (rel_lo), query blocks wholly inside the padding, alone and combined with kv_len, with and without the causal mask"""
    gpu_lib.omchat_op_set_tuning(8, gen)
    try:
        for causal in (1, 0):
            for lens in (None, LENS_SHORT):
                _left_case(gpu_lib, dt, Hq, Hkv, causal, lens, gen)
    finally:
        gpu_lib.omchat_op_set_tuning(8, 1)


# ------------------------------------------------------------------------------------------------ RoPE + KV append
ROPE_MAX_POS, ROPE_CAP, THETA = 90, 96, 1e6


def _rope_case(lib, dt, b, S, pos, pos0, slot0):
    """pos: [b][S] list or None"""
    Hq, Hkv, cap, T = 4, 2, ROPE_CAP, DT[dt]
    nh = Hq + 2 * Hkv
    qkv = rnd(randn((b * S, nh * 128), 7), dt)
    d = dev(qkv, dt)
    kc = torch.zeros(b, Hkv, cap, 128, dtype=T, device="cuda"); vc = torch.zeros_like(kc)
    dpos = None if pos is None else i32(pos).reshape(-1)
    _lib.check(lib.omchat_op_rope_kv_pos(CODE[dt], ptr(d), b, S, Hq, Hkv, ptr(dpos), pos0, slot0, ROPE_MAX_POS, THETA, ptr(kc), ptr(vc), cap, None))
    sync()
    pr, pp = gr.rope_slots(b, S, None if pos is None else torch.tensor(pos).reshape(-1), pos0, slot0)
    pr, pp = pr.view(b, S), pp.view(b, S)
    x = qkv.to(T).view(b, S, nh, 128)
    q = x[:, :, :Hq].transpose(1, 2); k = x[:, :, Hq:Hq + Hkv].transpose(1, 2); v = x[:, :, Hq + Hkv:].transpose(1, 2)
    cos, sin = oracle.rope_cos_sin(pr, 128, THETA, T)
    qr, kr = oracle.apply_rope(q, k, cos, sin)
    got_q = d.view(b, S, nh, 128)[:, :, :Hq].transpose(1, 2)
    assert rel(got_q, qr.float()) < 3e-3
    kcc, vcc = kc.cpu(), vc.cpu()
    touched = torch.zeros(b, cap, dtype=torch.bool)
    for i in range(b):
        got_k = kcc[i][:, pp[i]]                       # [Hkv, S, 128] at the slots, in row order
        assert rel(got_k, kr[i].float()) < 3e-3, (i, rel(got_k, kr[i].float()))
        # a row rotated to the wrong position (the slot instead of pos[], a neighbour's) is far outside 3e-3 unless the two positions agree
        assert torch.equal(vcc[i][:, pp[i]], v[i]), i
        touched[i, pp[i]] = True
    free = ~touched[:, None, :, None].expand(b, Hkv, cap, 128)
    assert float(kcc[free].float().abs().max()) == 0.0 and float(vcc[free].float().abs().max()) == 0.0
    # the raw k / v columns of qkv are read-only
    assert torch.equal(d.view(b, S, nh, 128)[:, :, Hq:].cpu(), x[:, :, Hq:])


@pytest.mark.parametrize("dt", DTS)
def test_rope_kv_positions_and_slots(gpu_lib, dt):
    """rope_kv_kernel beyond pos0: per-row positions (the padded batches), the cache slot apart from the position (masked decode)"""
    pos = [[0, 89, 17, 3, 40], [17, 0, 88, 89, 5], [62, 2, 1, 0, 89]]       # unordered, repeated across sequences, both ends of the table
    _rope_case(gpu_lib, dt, 3, 5, pos, 0, -1)
    rep = [[5, 5, 89, 0, 33], [89, 89, 89, 1, 0], [44, 3, 44, 3, 44]]        # with slot0 a sequence may repeat a position: the slots differ
    _rope_case(gpu_lib, dt, 3, 5, rep, 0, 70)
    _rope_case(gpu_lib, dt, 3, 5, rep, 0, 91)                                # the last slots of the cache
    _rope_case(gpu_lib, dt, 3, 5, None, 7, 20)                               # pos0 for the rotation, slot0 for the slot
    _rope_case(gpu_lib, dt, 3, 5, None, 85, -1)                              # pos0 alone, up to the table's end
    dec = [[0], [89], [44], [44], [7]]                                       # S = 1, b = 5: the decode shape
    _rope_case(gpu_lib, dt, 5, 1, dec, 0, -1)
    _rope_case(gpu_lib, dt, 5, 1, dec, 0, 50)
    _rope_case(gpu_lib, dt, 5, 1, dec, 0, 95)


@pytest.mark.parametrize("dt", DTS)
def test_rope_kv_refuses_positions_and_slots_out_of_range(gpu_lib, dt):
    b, S, Hq, Hkv, cap, T = 3, 5, 4, 2, ROPE_CAP, DT[dt]
    qkv = rnd(randn((b * S, (Hq + 2 * Hkv) * 128), 7), dt)
    d = dev(qkv, dt)
    kc = torch.zeros(b, Hkv, cap, 128, dtype=T, device="cuda"); vc = torch.zeros_like(kc)
    good = [[0, 89, 17, 3, 40], [17, 0, 88, 89, 5], [62, 2, 1, 0, 89]]

    def call(pos, pos0, slot0, max_pos):
        dpos = None if pos is None else i32(pos).reshape(-1)
        return gpu_lib.omchat_op_rope_kv_pos(CODE[dt], ptr(d), b, S, Hq, Hkv, ptr(dpos), pos0, slot0, max_pos, THETA, ptr(kc), ptr(vc), cap, None)

    bad = [row[:] for row in good]; bad[1][2] = ROPE_MAX_POS                 # one position == max_pos
    over = [row[:] for row in good]; over[2][4] = cap                        # inside a longer table, but the slot == cap
    neg = [row[:] for row in good]; neg[0][0] = -1
    for args in [(bad, 0, -1, ROPE_MAX_POS), (bad, 0, 20, ROPE_MAX_POS), (over, 0, -1, 200), (neg, 0, -1, ROPE_MAX_POS), (good, 0, 92, ROPE_MAX_POS),
                 (None, 86, -1, ROPE_MAX_POS), (None, 86, 10, ROPE_MAX_POS), (None, 92, -1, 200), (None, 3, 92, ROPE_MAX_POS)]:
        with pytest.raises(ValueError):
            _lib.check(call(*args))
    sync()
    # nothing was launched: q is not rotated, the caches are still empty
    assert torch.equal(d.cpu(), qkv.to(T))
    assert float(kc.float().abs().max()) == 0.0 and float(vc.float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ argmax
def _argmax_rows(V, b, seed):
    """[(name, logits [b, V])]: the places a two-stage argmax goes wrong"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(b, V, generator=g)
    per = (V + 63) // 64                       # ids per first-stage workgroup
    out = [("random", base.clone())]
    x = base.clone(); x[:, 0] = 9.0; out.append(("max at id 0", x))
    x = base.clone(); x[:, V - 1] = 9.0; out.append(("max at the last id", x))
    if V >= 2:
        for c in sorted({1, min(63, (V - 1) // per)}):      # the first chunk edge and the last one the vocabulary has
            if c * per < V:
                x = base.clone(); x[:, c * per - 1] = 9.0; x[:, c * per] = 9.0
                out.append((f"tie across the edge of chunks {c - 1} / {c}", x))
        x = base.clone(); x[:, V - 1] = 9.0; x[:, V // 2] = 9.0; out.append(("tie far apart", x))
    out.append(("all -inf", torch.full((b, V), -float("inf"))))
    x = base.clone(); x[:, V // 3] = float("inf"); out.append(("+inf", x))
    if V >= 3:
        x = base.clone(); x[:, V - 1] = float("inf"); x[:, V // 3] = float("inf"); x[:, 0] = -float("inf"); out.append(("two +inf, -inf at id 0", x))
    return out


@pytest.mark.parametrize("b", [1, 5])
@pytest.mark.parametrize("V", [1, 37, 63, 64, 65, 1000, 152064])
def test_argmax_strided_rows(gpu_lib, V, b):
    for ld in (V, V + 24):
        for name, x in _argmax_rows(V, b, 100 + V):
            buf = torch.full((b, ld), 3.0e38)                  # the padding columns beat every logit but +inf: they must never be read
            buf[:, :V] = x
            if "inf" in name and ld > V:
                buf[:, V:] = float("inf")
            d = buf.cuda()
            out = torch.full((b,), -7, dtype=torch.int32, device="cuda")
            _lib.check(gpu_lib.omchat_op_argmax_ld(ptr(d), ld, b, V, ptr(out), None, None, None))
            sync()
            want = torch.argmax(x, dim=1)
            assert out.cpu().tolist() == want.tolist(), (name, V, b, ld)


def test_argmax_advances_the_position_words(gpu_lib):
    b, V = 5, 1000
    x = torch.randn(b, V, generator=torch.Generator().manual_seed(5))
    d = x.cuda()
    pos0, len0 = [3, 0, 99, 7, 41], [4, 1, 100, 8, 42]
    for use_pos, use_len in [(1, 1), (1, 0), (0, 1), (0, 0)]:
        pos, ln = i32(pos0), i32(len0)
        out = torch.full((b,), -7, dtype=torch.int32, device="cuda")
        _lib.check(gpu_lib.omchat_op_argmax_ld(ptr(d), V, b, V, ptr(out), ptr(pos) if use_pos else None, ptr(ln) if use_len else None, None))
        sync()
        assert out.cpu().tolist() == torch.argmax(x, dim=1).tolist()
        assert pos.cpu().tolist() == [p + use_pos for p in pos0], (use_pos, use_len)
        assert ln.cpu().tolist() == [p + use_len for p in len0], (use_pos, use_len)
    with pytest.raises(ValueError):
        _lib.check(gpu_lib.omchat_op_argmax_ld(ptr(d), V - 1, b, V, ptr(out), None, None, None))


# ------------------------------------------------------------------------------------------------ copies and gathers (bit-exact)
GRID_CAP = 8192 * 256            # elementwise.hip grid_for: beyond this many work items a thread takes more than one


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,HW,patch,Kpad", [(2, 28, 14, 640), (2, 12, 4, 64)])
def test_im2col(gpu_lib, dt, B, HW, patch, Kpad):
    T = DT[dt]
    px = randn((B, 3, HW, HW), 1).to(T)
    g = HW // patch
    dpx = px.cuda()
    cols = nan_like((B * g * g, Kpad), T)
    _lib.check(gpu_lib.omchat_op_im2col(CODE[dt], ptr(dpx), ptr(cols), B, HW, patch, Kpad, None)); sync()
    assert torch.equal(cols.cpu(), gr.im2col(px, patch, Kpad))
    with pytest.raises(ValueError):                                    # Kpad < 3 * patch * patch
        _lib.check(gpu_lib.omchat_op_im2col(CODE[dt], ptr(dpx), ptr(cols), B, HW, patch, 3 * patch * patch - 8, None))
    with pytest.raises(ValueError):                                    # the image is not a whole number of patches
        _lib.check(gpu_lib.omchat_op_im2col(CODE[dt], ptr(dpx), ptr(cols), B, HW, patch + 1, Kpad, None))


@pytest.mark.parametrize("dt", DTS)
def test_vit_assemble(gpu_lib, dt):
    B, np_, C, T = 3, 4, 72, DT[dt]
    pe = randn((B * np_, C), 1).to(T); cls = randn((C,), 2).to(T); pos = randn((np_ + 1, C), 3).to(T)
    dpe, dcls, dpos = pe.cuda(), cls.cuda(), pos.cuda()
    x = nan_like((B, np_ + 1, C), T)
    _lib.check(gpu_lib.omchat_op_vit_assemble(CODE[dt], ptr(dpe), ptr(dcls), ptr(dpos), ptr(x), B, np_, C, None)); sync()
    assert torch.equal(x.cpu(), gr.vit_assemble(pe, cls, pos, B, np_, T))
    with pytest.raises(ValueError):
        _lib.check(gpu_lib.omchat_op_vit_assemble(CODE[dt], ptr(dpe), ptr(dcls), ptr(dpos), ptr(x), B, np_, 68, None))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H,rows", [(8, 9), (72, 9), (3584, 9), (8, GRID_CAP + 2915)])
def test_gather_rows(gpu_lib, dt, H, rows):
    T = DT[dt]
    table = randn((11, H), 1).to(T); feats = randn((5, H), 2).to(T)
    pat = torch.tensor([10, -1, gr.INT_MIN, 0, -5, 3, 3, gr.INT_MIN, -2], dtype=torch.int32)      # table rows, feature rows (-1 - i), zero rows
    idx = pat.repeat((rows + 8) // 9)[:rows].contiguous()
    dt_, df, di = table.cuda(), feats.cuda(), idx.cuda()
    out = nan_like((rows, H), T)
    _lib.check(gpu_lib.omchat_op_gather_rows(CODE[dt], ptr(di), ptr(dt_), ptr(df), ptr(out), rows, H, None)); sync()
    assert torch.equal(out.cpu(), gr.gather_rows(idx, table, feats))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows,H,group,skip", [(13, 72, 4, 1), (13, 72, 5, 0), (13, 72, 1, 2), (GRID_CAP + 2915, 8, 4, 1)])
def test_copy_rows(gpu_lib, dt, rows, H, group, skip):
    T = DT[dt]
    src_ld, dst_ld = H + 8, H + 16
    smap = gr.copy_rows_map(rows, group, skip)
    nsrc = int(smap.max()) + 1 + skip
    # a counter through the (finite, positive) 16-bit patterns: neighbouring rows and chunks all differ
    src = (torch.arange(nsrc * src_ld, dtype=torch.int32) % 30011).to(torch.int16).view(T).view(nsrc, src_ld)
    dsrc = src.cuda()
    dst = torch.full((rows, dst_ld), SENT, dtype=T, device="cuda"); dst[:, :H] = NAN
    _lib.check(gpu_lib.omchat_op_copy_rows(CODE[dt], ptr(dsrc), src_ld, ptr(dst), dst_ld, rows, H, group, skip, None)); sync()
    got = dst.cpu()
    assert torch.equal(got[:, :H].view(torch.int16), src[smap][:, :H].view(torch.int16))
    assert pad_ok(got, H)
    with pytest.raises(ValueError):
        _lib.check(gpu_lib.omchat_op_copy_rows(CODE[dt], ptr(dsrc), src_ld, ptr(dst), dst_ld, rows, H, 0, skip, None))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [1, 255, 256, 257, GRID_CAP + 777])
def test_cast_f32(gpu_lib, dt, n):
    T = DT[dt]
    src = (randn((n,), 4) * 3).to(T)
    d = src.cuda()
    out = torch.full((n + 8,), NAN, dtype=torch.float32, device="cuda")
    _lib.check(gpu_lib.omchat_op_cast_f32(CODE[dt], ptr(d), ptr(out), n, None)); sync()
    assert torch.equal(out[:n].cpu(), src.float())
    assert bool(torch.isnan(out[n:]).all())              # nothing past n


# ------------------------------------------------------------------------------------------------ tp_finish
EPIS = [_lib.EPI_NONE, _lib.EPI_RESID, _lib.EPI_LS_RESID]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N", [(3, 8), (130, 3200), (1, 4)])
def test_tp_finish_rounding_sequence(gpu_lib, dt, M, N):
    T = DT[dt]
    acc = randn((M, N), 1, 3.0)
    bias = randn((N,), 2, 0.5).to(T); ls = (randn((N,), 3, 0.1) + 0.1).to(T); resid = randn((M, N), 4).to(T)
    dacc, dbias, dls = acc.cuda(), bias.cuda(), ls.cuda()
    for epi in EPIS:
        for bb in (None, bias):
            for alias in ((False, True) if epi != _lib.EPI_NONE else (False,)):
                dres = resid.cuda()
                out = dres if alias else nan_like((M, N), T)
                _lib.check(gpu_lib.omchat_op_tp_finish(CODE[dt], ptr(dacc), None if bb is None else ptr(dbias), ptr(dls), ptr(dres), ptr(out), M, N, epi, None))
                sync()
                want = gr.tp_finish(acc, bb, ls, resid, epi, T)
                assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16)), (epi, bb is not None, alias)
    with pytest.raises(ValueError):
        _lib.check(gpu_lib.omchat_op_tp_finish(CODE[dt], ptr(dacc), None, None, None, ptr(nan_like((M, N), T)), 1, 6, _lib.EPI_NONE, None))
    with pytest.raises(ValueError):      # an epilogue without its operands
        _lib.check(gpu_lib.omchat_op_tp_finish(CODE[dt], ptr(dacc), None, None, None, ptr(nan_like((M, N), T)), M, N, _lib.EPI_RESID, None))


@pytest.mark.parametrize("dt", DTS)
def test_tp_finish_is_the_one_gpu_gemm_epilogue(gpu_lib, dt):
    """tp_finish's header: the epilogue applied once to the fp32 sum has the rounding points of the one-GPU epilogue -- so on the SAME fp32
    accumulators (EPI_F32OUT of the same tile kernel) it gives the GEMM's bits"""
    M, N, K, T = 130, 3200, 128, DT[dt]
    A = rnd(randn((M, K), 1), dt); W = rnd(randn((N, K), 2, 0.05), dt)
    bias = rnd(randn((N,), 3, 0.1), dt); ls = rnd(randn((N,), 4, 0.1) + 0.1, dt); resid = rnd(randn((M, N), 5), dt)
    dA, dW, db, dl, dr = dev(A, dt), dev(W, dt), dev(bias, dt), dev(ls, dt), dev(resid, dt)
    acc = torch.full((M, N), NAN, dtype=torch.float32, device="cuda")
    _lib.check(gpu_lib.omchat_op_gemm(CODE[dt], ptr(dA), K, ptr(dW), K, ptr(acc), N, M, N, K, None, None, None, 0, _lib.EPI_F32OUT, 1, None)); sync()
    assert rel(acc, A @ W.t()) < 1e-5
    for epi in EPIS:
        for bb in (None, db):
            fused = nan_like((M, N), T)      # force_tile 1: the 128 x 128 kernel the fp32-output GEMM of this size takes
            _lib.check(gpu_lib.omchat_op_gemm(CODE[dt], ptr(dA), K, ptr(dW), K, ptr(fused), N, M, N, K, ptr(bb), ptr(dl), ptr(dr), N, epi, 1, None))
            two = nan_like((M, N), T)
            _lib.check(gpu_lib.omchat_op_tp_finish(CODE[dt], ptr(acc), ptr(bb), ptr(dl), ptr(dr), ptr(two), M, N, epi, None))
            sync()
            assert torch.equal(fused.view(torch.int16), two.view(torch.int16)), (epi, bb is not None)


# ------------------------------------------------------------------------------------------------ norm family
WIDTHS = [8, 2048, 2056, 16384]      # one chunk in all; exactly one chunk per thread, and one thread with a second; the limit (eight per thread)
ROWS = 3


def _rms_inputs(dt, H, rows=ROWS):
    return rnd(randn((rows, H), 1, 2.0), dt), rnd(randn((H,), 2, 0.1) + 1.0, dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", WIDTHS)
def test_rmsnorm_strided(gpu_lib, dt, H):
    T, ld = DT[dt], H + 8
    x, w = _rms_inputs(dt, H)
    dx, dw = strided(x, ld, T), dev(w, dt)
    y = torch.full((ROWS, ld), SENT, dtype=T, device="cuda"); y[:, :H] = NAN
    _lib.check(gpu_lib.omchat_op_rmsnorm_ld(CODE[dt], ptr(dx), ld, ptr(dw), ptr(y), ld, ROWS, H, 1e-6, 0, None)); sync()
    ref = oracle.rms_norm(x.to(T), w.to(T), 1e-6).float()
    got = y[:, :H].float().cpu()
    assert rel(got, ref) < 2e-3
    assert (got == ref).float().mean() > 0.98
    assert pad_ok(y, H) and pad_ok(dx, H)
    # the dense entry point on the same rows: the stride changes no bit
    dense = nan_like((ROWS, H), T); dxc = dev(x, dt)
    _lib.check(gpu_lib.omchat_op_rmsnorm(CODE[dt], ptr(dxc), ptr(dw), ptr(dense), ROWS, H, 1e-6, None)); sync()
    assert torch.equal(dense, y[:, :H])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nb,rows", [(1, 3), (2, 19)])
def test_rmsnorm_packed_output(gpu_lib, dt, nb, rows):
    T, H = DT[dt], 2048
    ld = H + 8
    x, w = _rms_inputs(dt, H, rows)
    dx, dw = strided(x, ld, T), dev(w, dt)
    plain = nan_like((rows, H), T)
    _lib.check(gpu_lib.omchat_op_rmsnorm_ld(CODE[dt], ptr(dx), ld, ptr(dw), ptr(plain), H, rows, H, 1e-6, 0, None))
    packed = nan_like((nb * 16 * H,), T)
    _lib.check(gpu_lib.omchat_op_rmsnorm_ld(CODE[dt], ptr(dx), ld, ptr(dw), ptr(packed), H, rows, H, 1e-6, nb, None)); sync()
    assert torch.equal(gr.unpack_x(packed.cpu(), rows, H, nb).view(torch.int16), plain.cpu().view(torch.int16))
    with pytest.raises(ValueError):      # more rows than the layout holds
        _lib.check(gpu_lib.omchat_op_rmsnorm_ld(CODE[dt], ptr(dx), ld, ptr(dw), ptr(packed), H, 16 * nb + 1, H, 1e-6, nb, None))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", WIDTHS)
def test_layernorm_strided(gpu_lib, dt, H):
    T, ld = DT[dt], H + 8
    x = rnd(randn((ROWS, H), 1, 2.0) + 0.3, dt); w = rnd(randn((H,), 2, 0.05) + 1, dt); b = rnd(randn((H,), 3, 0.02), dt)
    dx, dw, db = strided(x, ld, T), dev(w, dt), dev(b, dt)
    y = torch.full((ROWS, ld), SENT, dtype=T, device="cuda"); y[:, :H] = NAN
    _lib.check(gpu_lib.omchat_op_layernorm_ld(CODE[dt], ptr(dx), ld, ptr(dw), ptr(db), ptr(y), ld, ROWS, H, 1e-6, None)); sync()
    ref = F.layer_norm(x, (H,), w, b, 1e-6)
    got = y[:, :H]
    assert rel(got, ref) < TOL[dt]
    half = F.layer_norm(x.to(T), (H,), w.to(T), b.to(T), 1e-6)      # ATen on the 16-bit tensors
    assert (got.cpu().float() - half.float()).abs().max() <= 2 * torch.finfo(T).eps * ref.abs().max()
    assert pad_ok(y, H) and pad_ok(dx, H)


@pytest.mark.parametrize("dt", DTS)
def test_norm_widths_refused(gpu_lib, dt):
    T = DT[dt]
    buf = torch.zeros(ROWS, 16400, dtype=T, device="cuda"); w = torch.ones(16400, dtype=T, device="cuda"); part = torch.zeros(9 * ROWS * 16400, device="cuda")
    for H in (16392, 12):
        with pytest.raises(ValueError):
            _lib.check(gpu_lib.omchat_op_rmsnorm_ld(CODE[dt], ptr(buf), 16400, ptr(w), ptr(buf), 16400, ROWS, H, 1e-6, 0, None))
        with pytest.raises(ValueError):
            _lib.check(gpu_lib.omchat_op_layernorm_ld(CODE[dt], ptr(buf), 16400, ptr(w), ptr(w), ptr(buf), 16400, ROWS, H, 1e-6, None))
        with pytest.raises(ValueError):
            _lib.check(gpu_lib.omchat_op_resid_rmsnorm(CODE[dt], ptr(buf), 16400, ptr(part), 1, ptr(w), ptr(buf), 16400, ROWS, H, 1e-6, 0, None))
        with pytest.raises(ValueError):
            _lib.check(gpu_lib.omchat_op_resid16_norm(CODE[dt], ptr(buf), 16400, ptr(buf), 16400, ptr(w), None, ptr(buf), 16400, ROWS, H, 1e-6, None))
    with pytest.raises(ValueError):      # at most 8 split-K slices
        _lib.check(gpu_lib.omchat_op_resid_rmsnorm(CODE[dt], ptr(buf), 16400, ptr(part), 9, ptr(w), ptr(buf), 16400, ROWS, 2048, 1e-6, 0, None))
    with pytest.raises(ValueError):      # a row stride below the width
        _lib.check(gpu_lib.omchat_op_rmsnorm_ld(CODE[dt], ptr(buf), 2040, ptr(w), ptr(buf), 2048, ROWS, 2048, 1e-6, 0, None))
    sync()
    assert float(buf.float().abs().max()) == 0.0


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", WIDTHS)
def test_resid_rmsnorm(gpu_lib, dt, H):
    T, ld = DT[dt], H + 8
    x, w = _rms_inputs(dt, H)
    dw = dev(w, dt)
    for ks in (1, 3, 8):
        part = randn((ks, ROWS, H), 10 + ks, 0.7)
        dpart = part.cuda()
        want_x = gr.resid_sum(x.to(T), part, T)
        dwx = want_x.cuda()
        want_n = nan_like((ROWS, H), T)
        _lib.check(gpu_lib.omchat_op_rmsnorm(CODE[dt], ptr(dwx), ptr(dw), ptr(want_n), ROWS, H, 1e-6, None))
        for with_w in (True, False):
            dx = strided(x, ld, T)
            xn = torch.full((ROWS, ld), SENT, dtype=T, device="cuda"); xn[:, :H] = NAN
            _lib.check(gpu_lib.omchat_op_resid_rmsnorm(CODE[dt], ptr(dx), ld, ptr(dpart), ks, ptr(dw) if with_w else None, ptr(xn), ld, ROWS, H, 1e-6, 0, None))
            sync()
            assert torch.equal(dx[:, :H].cpu().view(torch.int16), want_x.view(torch.int16)), (ks, with_w)
            assert pad_ok(dx, H) and pad_ok(xn, H)
            if with_w:
                assert torch.equal(xn[:, :H].view(torch.int16), want_n.view(torch.int16)), ks
            else:
                assert bool(torch.isnan(xn[:, :H]).all())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", WIDTHS)
def test_resid16_norm(gpu_lib, dt, H):
    T, ld = DT[dt], H + 8
    x, w = _rms_inputs(dt, H)
    y = rnd(randn((ROWS, H), 5, 0.7), dt); b = rnd(randn((H,), 6, 0.02), dt)
    dw, db, dy = dev(w, dt), dev(b, dt), strided(y, ld + 8, T)
    want_x = gr.resid16(x.to(T), y.to(T), T)
    dwx = want_x.cuda()
    want_rms = nan_like((ROWS, H), T); want_ln = nan_like((ROWS, H), T)
    _lib.check(gpu_lib.omchat_op_rmsnorm(CODE[dt], ptr(dwx), ptr(dw), ptr(want_rms), ROWS, H, 1e-6, None))
    _lib.check(gpu_lib.omchat_op_layernorm(CODE[dt], ptr(dwx), ptr(dw), ptr(db), ptr(want_ln), ROWS, H, 1e-6, None))
    for mode in ("rms", "ln", "none"):
        dx = strided(x, ld, T)
        xn = torch.full((ROWS, ld), SENT, dtype=T, device="cuda"); xn[:, :H] = NAN
        _lib.check(gpu_lib.omchat_op_resid16_norm(CODE[dt], ptr(dx), ld, ptr(dy), ld + 8, None if mode == "none" else ptr(dw), ptr(db) if mode == "ln" else None,
                                                  ptr(xn), ld, ROWS, H, 1e-6, None))
        sync()
        assert torch.equal(dx[:, :H].cpu().view(torch.int16), want_x.view(torch.int16)), mode
        assert pad_ok(dx, H) and pad_ok(xn, H) and pad_ok(dy, H)
        if mode == "none":
            assert bool(torch.isnan(xn[:, :H]).all())
        else:
            assert torch.equal(xn[:, :H].view(torch.int16), (want_rms if mode == "rms" else want_ln).view(torch.int16)), mode
    # rows = 0: nothing happens
    dx = strided(x, ld, T); before = dx.clone()
    xn = nan_like((ROWS, ld), T)
    _lib.check(gpu_lib.omchat_op_resid16_norm(CODE[dt], ptr(dx), ld, ptr(dy), ld + 8, ptr(dw), None, ptr(xn), ld, 0, H, 1e-6, None)); sync()
    assert torch.equal(dx.view(torch.int16), before.view(torch.int16)) and bool(torch.isnan(xn).all())
