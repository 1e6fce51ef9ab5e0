"""Exact per-row tests of the statistics chain of the fused ViT layer (csrc/model.hip vit_layer_fused, tuning key 44 = 1):

    row_sumsq -> qkv GEMM (row scale finished in the launch from x's slots; EPI_NONE_STATS leaves the q / k slots) -> vit_knorm_slots
              -> attention with the Q norm on load -> proj GEMM (EPI_LS_RESID_STATS) -> fc1 GEMM (row scale) -> fc2 GEMM (EPI_LS_RESID_STATS)

on the operands of tests/vit_stats_ref.py, for which the expected BITS of every link are determined: rows whose statistics differ by factors of
at least 2 from every neighbour, hand-made slots that sum exactly in any order with NaN behind the last slot and the last row, and GEMM
operands with integer outputs.  The links are asserted with torch.equal per (slot, row) / per element, the attention additionally per
(sequence, row, head) against the fp64 restatement, the whole tower per token row against the oracle.  tests/test_vit_stats_cpu.py proves the
preconditions and that each named mistake changes an expected bit (or moves a row by more than ten bounds)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
from gpu_util import DT, CODE, TOL, TOL_DEEP, ptr, sync, rnd, rel, synth_state_dict
from omchat_amd import _lib
import gemm_exact_ref as X
import vit_stats_ref as V
from attn_prefill_ref import attend, row_rel, pack_qkv
from gemm_exact_gpu import Problem, _run, _check, _sentinel, _padded, _cus

DTS = ["bf16", "f16"]
NAN = float("nan")


def _sentinel_f32(*shape):
    return torch.full(shape, X.SENTINEL32, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _untouched(t):
    return bool((_bits(t) == (X.SENTINEL32 if t.dtype == torch.float32 else X.SENTINEL16)).all())


def _poisoned(rows, ld, T):
    """[rows, ld] of T holding the recognisable finite pattern 0x5A5A"""
    return torch.full((rows, ld), V.POISON16, dtype=torch.int16).view(T)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the statistics epilogues, per slot
# ---------------------------------------------------------------------------------------------------------------------------------------
def _stats_case(lib, dt, epi, tile, M, N, K, alias=False):
    """EPI_*_STATS on the poisoned strided layout: C has the plain epilogue's bits, *nslots = the slots of the tile table, every (slot, row < M)
    is the fp32 sum of squares of the stored values of exactly that slot's columns, every other word keeps its sentinel"""
    base = "bias" if epi == V.EPI_NONE_STATS else "ls_resid"
    ops = V.cached_stats_operands(1, M, N, K, dt)
    P = Problem(ops, dt, True)
    what = ("stats", base, "tile", tile, M, N, K, "alias" if alias else "")
    plain = _run(lib, P, base, tile)
    want = X.reference(ops, X.EPI_NONE if base == "bias" else X.EPI_LS_RESID, dt, bias=True)
    edges = V.slot_edges(tile, epi, M, N, _cus())
    assert V.stats_precondition(want, edges), what
    Cs, ldc = P.out(N, DT[dt])
    resid, ldr = (P.R, P.ldr) if base == "ls_resid" else (None, 0)
    if alias:                     # the model's in-place form: x = x + ls * branch, resid == C
        Cs[:M, :N] = ops["resid"].to(torch.float32).to(DT[dt]).cuda()
        resid, ldr = Cs, ldc
    cap, ld = len(edges) + 2, M + 5
    stats = _sentinel_f32(cap, ld)
    ns = C.c_int(-1)
    _lib.check(lib.omchat_op_gemm_fused(CODE[dt], ptr(P.A), P.lda, ptr(P.W), P.ldw, ptr(Cs), ldc, M, N, K, ptr(P.bias), ptr(P.ls), ptr(resid), ldr,
                                        epi, tile, None, None, 0, 0, 0, 0.0, ptr(stats), ld, C.byref(ns), None))
    sync()
    _check(Cs, M, N, want, 0, what)
    assert torch.equal(_bits(Cs), _bits(plain)), (what, "C differs from the plain epilogue's bits")
    assert ns.value == len(edges), (what, "nslots", ns.value, "want", len(edges))
    host = stats.cpu()
    exp = V.expected_stats(want, edges).float()
    got = host[:len(edges), :M]
    if not torch.equal(got, exp):
        s, r = (int(v) for v in (got != exp).nonzero()[0])
        raise AssertionError((what, f"slot {s} (columns {edges[s]}), row {r}: got {float(got[s, r])!r}, want {float(exp[s, r])!r}",
                              int((got != exp).sum()), "of", exp.numel()))
    assert _untouched(host[:, M:]), (what, "a word at row >= M was written")
    assert _untouched(host[len(edges):]), (what, "a slot >= nslots was written")


STATS_PARAMS = [(V.EPI_LS_RESID_STATS, t) for t in sorted(X.TILES)] + [(V.EPI_NONE_STATS, t) for t in V.NONE_STATS_TILES + (10,)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("epi,tile", STATS_PARAMS)
def test_statistics_epilogue_per_slot(gpu_lib, dt, epi, tile):
    """every tile id under EPI_LS_RESID_STATS; under EPI_NONE_STATS the ids that keep 64-column slots and one id (10) that launch_t remaps to
    tile 2.  M in {1, BM + 1}, N = two whole slots and 4 / 24 columns, K = 64 / 192"""
    for M, N, K in V.stats_shapes(tile, epi):
        _stats_case(gpu_lib, dt, epi, tile, M, N, K)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("tile", [12, 13])
def test_statistics_epilogue_two_launch_split(gpu_lib, dt, tile):
    """tiles 12 / 13 where launch_epi's split applies: the 64-column slots of the 256^2 launch, the 112-column slots of the tail behind them"""
    M, N, K = X.split_shape(_cus())
    _stats_case(gpu_lib, dt, V.EPI_LS_RESID_STATS, tile, M, N, K)


@pytest.mark.parametrize("dt", DTS)
def test_statistics_epilogue_in_place_and_dead_row_blocks(gpu_lib, dt):
    """resid aliasing C (the model's in-place proj / fc2), and tuning key 43 (row blocks beyond M issue nothing) in both states"""
    bm = X.TILES[2][0]
    _stats_case(gpu_lib, dt, V.EPI_LS_RESID_STATS, 2, bm + 1, 152, 192, alias=True)
    _stats_case(gpu_lib, dt, V.EPI_LS_RESID_STATS, 10, X.TILES[10][0] + 1, 248, 64, alias=True)
    try:
        for key in (0, 1):
            gpu_lib.omchat_op_set_tuning(43, key)
            for epi, tile in ((V.EPI_LS_RESID_STATS, 2), (V.EPI_NONE_STATS, 8), (V.EPI_LS_RESID_STATS, 9)):
                M, N, K = V.stats_shapes(tile, epi)[1]
                _stats_case(gpu_lib, dt, epi, tile, M, N, K)
    finally:
        gpu_lib.omchat_op_set_tuning(43, 1)


@pytest.mark.parametrize("dt", DTS)
def test_statistics_epilogue_persistent_form(gpu_lib, dt):
    """tuning key 13: launch_cfg8 gives a statistics epilogue (no in-launch row scale) to the persistent kernel when there are more tiles than CUs"""
    M, N, K = X.persistent_shape(_cus())
    assert -(-M // 256) * -(-N // 256) > _cus()
    gpu_lib.omchat_op_set_tuning(13, 1)
    try:
        _stats_case(gpu_lib, dt, V.EPI_LS_RESID_STATS, 2, M, N, K)
    finally:
        gpu_lib.omchat_op_set_tuning(13, 0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the row scale finished in the launch
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("tile", V.RS_TILES)
def test_row_scale_from_slots_exact(gpu_lib, dt, tile):
    """rs_stats with 1 .. 67 slots per row (NaN behind the last slot and behind row M, rs_ld > M), factors 4, 2, 1, 1/2 by row, M = BM + 1 (the
    clamp of rows >= M): the bits of X.reference(scale=) under bias, layer scale + residual and GELU (<= 1 ulp, as the exact suite holds it).
    The slot counts reach the LDS-DMA source and the global one on every tile (vit_stats_ref.rs_source; printed)"""
    M, N, K = X.row_scale_shape(tile)
    assert M == X.TILES[tile][0] + 1
    ops = X.cached_operands(1, M, N, K, dt)
    P = Problem(ops, dt, True)
    sources = {}
    for n in V.RS_NSLOTS:
        s, sl = V.rs_slots(M, n)
        rs_ld = M + 3
        buf = V.slot_buffer(sl, rs_ld).cuda()
        sources[n] = V.rs_source(tile, n)
        for name in V.RS_EPIS:
            _run(gpu_lib, P, name, tile, scale=s, rs=(buf, rs_ld, n, V.RS_DIM))
    print("row scale source, tile", tile, sources)
    assert set(sources.values()) == {"dma", "global"}


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. row_sumsq, vit_qk_sumsq, stats_finish
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows,H", V.SUMSQ_CASES)
def test_row_sumsq_and_qk_sumsq_exact(gpu_lib, dt, rows, H):
    T = DT[dt]
    e = V.row_exponents(1, rows)
    eq = V.q_exponents(e)
    xk, xq = V.scaled_rows(V.groups(21, rows, H), e), V.scaled_rows(V.groups(22, rows, H), eq)
    # row_sumsq: rows of stride ldx > H, NaN in the padding; slot 0 of a slot-major buffer, nothing else written
    ldx = H + 8
    dx = _padded(xk, ldx, 0, T)
    stats = _sentinel_f32(3, rows + 7)
    _lib.check(gpu_lib.omchat_op_row_sumsq(CODE[dt], ptr(dx), ldx, rows, H, ptr(stats), None))
    sync()
    host = stats.cpu()
    assert torch.equal(host[0, :rows], V.sumsq_of(e, H).float()), ("row_sumsq", rows, H)
    assert _untouched(host[0, rows:]) and _untouched(host[1:])
    # vit_qk_sumsq: q | k | v of stride 3 H + 8, NaN in v and the padding; out [rows, 2]
    ld = 3 * H + 8
    qkv = torch.full((rows, ld), NAN, dtype=T)
    qkv[:, :H], qkv[:, H:2 * H] = xq.float().to(T), xk.float().to(T)
    dq = qkv.cuda()
    out = _sentinel_f32(rows * 2 + 8)
    _lib.check(gpu_lib.omchat_op_vit_qk_sumsq(CODE[dt], ptr(dq), ld, rows, H, ptr(out), None))
    sync()
    host = out.cpu()
    want = torch.stack((V.sumsq_of(eq, H), V.sumsq_of(e, H)), 1).float()
    assert torch.equal(host[:rows * 2].reshape(rows, 2), want), ("vit_qk_sumsq", rows, H)
    assert _untouched(host[rows * 2:])
    assert torch.equal(_bits(dq.cpu()), _bits(qkv))


@pytest.mark.parametrize("nslots", V.FINISH_NSLOTS)
def test_stats_finish_exact(gpu_lib, nslots):
    """slot0 = 3, two groups of nslots slots, 257 rows (two workgroups): raw sums (dim = 0) and rstd of power-of-four means (dim = 64, eps = 0)"""
    rows, slot0, dim = 257, 3, 64
    ld = rows + 9
    e = V.row_exponents(1, rows)
    eq = V.q_exponents(e)
    tq, tk = V.sumsq_of(eq, dim // 4), V.sumsq_of(e, dim // 4)          # dim * 4^e
    buf = torch.full((slot0 + 2 * nslots + 2, ld), NAN, dtype=torch.float32)
    buf[slot0:slot0 + nslots, :rows] = V.split_slots(tq, nslots, 1).float()
    buf[slot0 + nslots:slot0 + 2 * nslots, :rows] = V.split_slots(tk, nslots, 2).float()
    dbuf = buf.cuda()
    for d, want in ((0, torch.stack((tq, tk), 1)), (dim, torch.stack((2.0 ** -eq.reshape(-1).double(), 2.0 ** -e.reshape(-1).double()), 1))):
        out = _sentinel_f32(rows * 2 + 8)
        _lib.check(gpu_lib.omchat_op_stats_finish(ptr(dbuf), ld, slot0, nslots, 2, rows, d, 0.0, ptr(out), None))
        sync()
        host = out.cpu()
        got = host[:rows * 2].reshape(rows, 2)
        assert torch.equal(got, want.float()), ("stats_finish", nslots, d, (got != want.float()).nonzero()[:4].tolist())
        assert _untouched(host[rows * 2:])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. vit_knorm_slots
# ---------------------------------------------------------------------------------------------------------------------------------------
def _knorm_operands(rows, Cc, n, mult, dt):
    T = DT[dt]
    e = V.row_exponents(1, rows)
    grp = V.groups(31, rows, Cc)
    w = V.norm_weights(32, Cc)
    Ct = mult * Cc
    tq, tk = V.sumsq_of(V.q_exponents(e), Ct), V.sumsq_of(e, Ct)
    slots = torch.cat((V.split_slots(tq, n, 1), V.split_slots(tk, n, 2)), 0)
    qkv = _poisoned(rows, 3 * Cc, T).clone()
    qkv[:, Cc:2 * Cc] = V.scaled_rows(grp, e).float().to(T)
    return qkv, w.float().to(T), slots, tq, V.exact_knorm(grp, w, dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows,Cc,n,mult", V.KNORM_CASES)
def test_vit_knorm_slots_exact(gpu_lib, dt, rows, Cc, n, mult):
    """K == T(w_k * group / 2) from the k slots [n, 2 n), sumsq_q[row] == the q group's total, Q / V (a finite pattern) and every other word untouched"""
    qkv, w, slots, tq, want = _knorm_operands(rows, Cc, n, mult, dt)
    stats_ld = rows + 3
    dq, dw, dst = qkv.cuda(), w.cuda(), V.slot_buffer(slots, stats_ld).cuda()
    sums = _sentinel_f32(rows + 4)
    _lib.check(gpu_lib.omchat_op_vit_knorm_slots(CODE[dt], ptr(dq.view(-1)[Cc:]), 3 * Cc, ptr(dw), rows, Cc, mult * Cc, V.EPS, ptr(dst), stats_ld, n,
                                                 ptr(sums), None))
    sync()
    host = dq.cpu()
    got = host[:, Cc:2 * Cc]
    assert torch.equal(_bits(got), _bits(want)), ("K", rows, Cc, n, mult, (got != want).nonzero()[:4].tolist())
    assert torch.equal(_bits(host[:, :Cc]), _bits(qkv[:, :Cc])) and torch.equal(_bits(host[:, 2 * Cc:]), _bits(qkv[:, 2 * Cc:]))
    hs = sums.cpu()
    assert torch.equal(hs[:rows], tq.float()), ("sumsq_q", rows, Cc, n, mult)
    assert _untouched(hs[rows:])


@pytest.mark.parametrize("dt", DTS)
def test_vit_knorm_slots_refuses_65_slots(gpu_lib, dt):
    """one lane per slot: 65 q slots are refused before anything is launched"""
    rows, Cc = 19, 384
    qkv, w, slots, _, _ = _knorm_operands(rows, Cc, 65, 1, dt)
    dq, dw, dst = qkv.cuda(), w.cuda(), V.slot_buffer(slots, rows + 3).cuda()
    sums = _sentinel_f32(rows + 4)
    rc = gpu_lib.omchat_op_vit_knorm_slots(CODE[dt], ptr(dq.view(-1)[Cc:]), 3 * Cc, ptr(dw), rows, Cc, Cc, V.EPS, ptr(dst), rows + 3, 65, ptr(sums), None)
    sync()
    assert rc != 0
    assert torch.equal(_bits(dq.cpu()), _bits(qkv)) and _untouched(sums.cpu())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. vit_qknorm: own statistics, given statistics, the K half alone
# ---------------------------------------------------------------------------------------------------------------------------------------
def _qknorm_equal(got, want, dt):
    """bf16: the same bits.  f16: the same bits, except that +0 is accepted where the expectation is -0 (and nothing else: not -0 for +0, not in
    bf16).  Measured on MI355X: the f16 instance of vit_qknorm_kernel returns +0 where the CPU's T(w * T(x * rstd)) (and its product with
    q_scale) is -0; bf16, and vit_knorm_slots_kernel in both types, keep -0.  The ISA shows why: in the f16 instance the last product and its
    conversion are one v_fma_mixlo_f16 with a +0 addend, and -0 + +0 = +0 (the slots kernel's are v_mul_f32 + v_cvt_pk_f16_f32).  A zero of
    either sign contributes nothing to q . k, so the kernel is left as it is; the operands keep their -0 entries"""
    g, w = _bits(got), _bits(want)
    if dt == "bf16":
        return torch.equal(g, w)
    return bool(((g == w) | ((g == 0) & (w == -32768))).all())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows,Cc", V.QKNORM_CASES)
def test_vit_qknorm_exact(gpu_lib, dt, rows, Cc):
    """own statistics; given statistics [rows, 2] of 2 C channels (they differ from the row's own, so a kernel that recomputes them fails); the
    K half alone; the K half alone without statistics is refused.  Q == T(T(w_q * group / 2) * 128^-0.5) as torch forms it on the CPU and
    K == w_k * group / 2, both to the bit (f16: +0 accepted for -0, see above); V and the padding untouched"""
    T = DT[dt]
    e = V.row_exponents(1, rows)
    eq = V.q_exponents(e)
    gq, gk = V.groups(41, rows, Cc), V.groups(42, rows, Cc)
    wq, wk = V.norm_weights(43, Cc), V.norm_weights(44, Cc)
    ld = 3 * Cc + 8
    qkv = _poisoned(rows, ld, T).clone()
    qkv[:, :Cc], qkv[:, Cc:2 * Cc] = V.scaled_rows(gq, eq).float().to(T), V.scaled_rows(gk, e).float().to(T)
    want_k = V.exact_knorm(gk, wk, dt)
    want_q = (V.exact_knorm(gq, wq, dt).float() * torch.tensor(V.Q_SCALE, dtype=torch.float32)).to(T)
    dwq, dwk = wq.float().to(T).cuda(), wk.float().to(T).cuda()
    # the given sums are those of 2 C channels (the tensor-parallel form): a kernel that recomputes them from the row, or divides by C, is off by sqrt(2)
    given = torch.full((rows * 2 + 8,), NAN, dtype=torch.float32)
    given[:rows * 2] = torch.stack((V.sumsq_of(eq, 2 * Cc), V.sumsq_of(e, 2 * Cc)), 1).float().reshape(-1)
    dgiven = given.cuda()

    def run(C_total, sums, only_k):
        d = qkv.cuda()
        rc = gpu_lib.omchat_op_vit_qknorm_ex(CODE[dt], ptr(d), ld, ptr(dwq), ptr(dwk), rows, Cc, C_total, V.EPS, V.Q_SCALE, ptr(sums), only_k, None)
        sync()
        return rc, d.cpu()

    for what, C_total, sums, only_k in (("own", Cc, None, 0), ("given", 2 * Cc, dgiven, 0), ("only_k", 2 * Cc, dgiven, 1)):
        rc, host = run(C_total, sums, only_k)
        assert rc == 0, (what, _lib.lib().omchat_last_error())
        if only_k:
            assert torch.equal(_bits(host[:, :Cc]), _bits(qkv[:, :Cc])), (what, "Q was written", rows, Cc)
        else:
            assert _qknorm_equal(host[:, :Cc], want_q, dt), (what, "Q", rows, Cc)
        assert _qknorm_equal(host[:, Cc:2 * Cc], want_k, dt), (what, "K", rows, Cc)
        assert torch.equal(_bits(host[:, 2 * Cc:]), _bits(qkv[:, 2 * Cc:])), (what, "V or the padding was written")
    rc, host = run(Cc, None, 1)
    assert rc != 0 and torch.equal(_bits(host), _bits(qkv)), "the K half alone without given statistics must be refused"
    # the entry the round-5 layer calls
    d = qkv.cuda()
    _lib.check(gpu_lib.omchat_op_vit_qknorm(CODE[dt], ptr(d), ld, ptr(dwq), ptr(dwk), rows, Cc, Cc, V.EPS, V.Q_SCALE, None))
    sync()
    assert _qknorm_equal(d.cpu()[:, :Cc], want_q, dt) and _qknorm_equal(d.cpu()[:, Cc:2 * Cc], want_k, dt)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. the Q norm on load, per (sequence, row, head)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,S,H,stride,mult", V.MHA_CASES)
def test_q_norm_on_load_per_row(gpu_lib, dt, B, S, H, stride, mult):
    """(a) omchat_op_mha_qnorm on the raw Q == omchat_mha_fwd on the buffer whose Q third holds the exactly known normed Q, bit for bit (the same
    kernel on the same MFMA inputs); (b) every (sequence, row, head) within gpu_util.TOL of the fp64 attention on that Q"""
    T = DT[dt]
    inp = V.mha_inputs(B, S, H, mult, dt)
    raw = pack_qkv(inp["q"].float(), inp["k"], inp["v"]).to(T).cuda()
    normed = pack_qkv(inp["qn"].float(), inp["k"], inp["v"]).to(T).cuda()
    sums = torch.full((B * S * stride + 8,), NAN, dtype=torch.float32)
    sums[:B * S * stride:stride] = inp["sums"].float()
    dsums, dwq = sums.cuda(), inp["wq"].float().to(T).cuda()
    out = _sentinel(B * S + 1, H * 128, T)
    _lib.check(gpu_lib.omchat_op_mha_qnorm(CODE[dt], ptr(raw), B, S, H, ptr(dsums), stride, inp["dim"], ptr(dwq), V.EPS, V.Q_SCALE, ptr(out), None))
    want = _sentinel(B * S + 1, H * 128, T)
    _lib.check(gpu_lib.omchat_mha_fwd(ptr(normed), B, S, H, 1.0, 0, ptr(want), CODE[dt], None))
    sync()
    got, exp = out.cpu(), want.cpu()
    assert _untouched(got[B * S:]) and not torch.isnan(got[:B * S].float()).any()
    assert torch.equal(_bits(raw.cpu()), _bits(pack_qkv(inp["q"].float(), inp["k"], inp["v"]).to(T))), "the raw qkv buffer was written"
    if not torch.equal(_bits(got), _bits(exp)):
        bad = (got[:B * S] != exp[:B * S]).reshape(B, S, H, 128).any(-1).nonzero()
        raise AssertionError(("differs from the attention on the exact normed Q", len(bad), "of", B * S * H, "(sequence, row, head); first", bad[:4].tolist()))
    ref = attend(inp["qn"].float(), inp["k"], inp["v"], 1.0, 0, 0, None, None)
    r = row_rel(got[:B * S].float().reshape(B, S, H, 128), ref)
    worst = int(r.argmax())
    print(f"q norm on load {dt} B{B} S{S} H{H} stride{stride} dim x{mult}: worst (sequence, row, head) {float(r.max()):.5f} of {TOL[dt]}")
    assert float(r.max()) <= TOL[dt], (float(r.max()), "at (sequence, row, head)", (worst // (S * H), worst // H % S, worst % H))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. the tower, per token row
# ---------------------------------------------------------------------------------------------------------------------------------------
def _tower_rows(lib, dt, cfg, n_tiles=3):
    """(vit_forward, encode_images) under tuning key 44 = 1 and 0 on a synthetic tower whose position rows are scaled by 2^(r % 5 - 2) and whose
    tiles by 4^(b - 1), and the oracle's output: per token row relative errors of both paths"""
    import oracle
    from omchat_amd import synth
    from omchat_amd.engine import Engine
    sd = synth_state_dict(cfg, 3)
    key = synth.TOWER + V.POS_KEY
    sd[key] = V.scale_pos_rows(torch.from_numpy(sd[key])).numpy()
    px = V.scale_tiles(torch.from_numpy(synth.pixels(n_tiles, 56, 1)))
    outs = {}
    try:
        for k44 in (1, 0):
            lib.omchat_op_set_tuning(44, k44)
            e = Engine(cfg, dtype=dt, max_seq=64, max_batch=1, max_tiles=n_tiles)
            e.load_state_dict(sd)
            outs[k44] = (e.vit_forward(px).float().cpu(), e.encode_images(px).float().cpu())
            sync()
            e.close()
    finally:
        lib.omchat_op_set_tuning(44, 1)
    tower = {k[len(synth.TOWER):]: rnd(torch.from_numpy(v), dt) for k, v in sd.items() if k.startswith(synth.TOWER)}
    ref = oracle.vision_tower_forward(px, tower, cfg.vision)
    return outs, ref


def _hold_tower(dt, name, outs, ref, same_layer=False):
    """the round-5 path's worst token row against the oracle is MEASURED here; the fused path is held to twice that (it has one rounding fewer
    but rounds the norm weight into W': not expected to be closer).  The round-5 path itself is held, per token row, to gpu_util.TOL_DEEP --
    the bound the suite holds the whole tensor to (test_gpu_round6.py) -- and so are the projected features of the two paths against each other.
    same_layer: both keys run the round-5 layer, so the tower's and the projector's outputs agree bit for bit, and the per-row TOL_DEEP bound is
    that tower's comparison with the oracle."""
    r5, r6 = row_rel(outs[0][0], ref), row_rel(outs[1][0], ref)
    enc = row_rel(outs[1][1], outs[0][1])
    print(f"tower {name} {dt}: worst token row against the oracle: round-5 path {float(r5.max()):.5f}, fused path {float(r6.max()):.5f} "
          f"(bound {2 * float(r5.max()):.5f}); encode_images fused against round-5, worst row {float(enc.max()):.5f}")
    assert not torch.isnan(outs[1][0]).any() and not torch.isnan(outs[1][1]).any()
    assert rel(outs[0][0], ref) < TOL_DEEP[dt]
    assert float(r5.max()) <= TOL_DEEP[dt], (float(r5.max()), "token (tile, row)", divmod(int(r5.argmax()), r5.shape[1]))
    assert float(enc.max()) <= TOL_DEEP[dt], (float(enc.max()), "token (tile, row)", divmod(int(enc.argmax()), enc.shape[1]))
    assert float(r6.max()) <= 2 * float(r5.max()), (float(r6.max()), float(r5.max()), "token (tile, row)", divmod(int(r6.argmax()), r6.shape[1]))
    if same_layer:
        assert torch.equal(outs[1][0], outs[0][0]) and torch.equal(outs[1][1], outs[0][1])


@pytest.mark.parametrize("dt", DTS)
def test_tower_per_token_row_against_the_oracle(gpu_lib, dt):
    from omchat_amd.config import tiny
    outs, ref = _tower_rows(gpu_lib, dt, tiny(layers_v=2, heads_v=3))
    _hold_tower(dt, "3 heads x 2 layers", outs, ref)


@pytest.mark.parametrize("dt", DTS)
def test_tower_of_33_heads_runs_under_the_default_key(gpu_lib, dt):
    """33 heads of 128 = 66 q slots, more than vit_knorm_slots' one lane per slot: vit_run must not pick the fused layer for it (it did:
    Cq / 64 <= 256, and encode_images failed in the default mode).  Such a tower takes the round-5 layer under either key"""
    from omchat_amd.config import tiny
    outs, ref = _tower_rows(gpu_lib, dt, tiny(layers_v=1, heads_v=33))
    _hold_tower(dt, "33 heads x 1 layer", outs, ref, same_layer=True)
