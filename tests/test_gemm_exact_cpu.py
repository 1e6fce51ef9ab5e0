"""The exact GEMM / GEMV reference (tests/gemm_exact_ref.py) checks itself here, without a GPU: the exactness preconditions, the agreement of
the float64 restatement with a plain fp32 evaluation, the share of outputs whose final rounding is a real rounding, and that the case
lists the GPU tests import reach every edge of every tile."""
import ctypes as C
import pytest
import torch

import gemm_exact_ref as X

DTS = ["bf16", "f16"]
N_CU = 256          # the case lists that depend on the device are checked for the MI355X's 256 compute units


def _all_gemm_shapes():
    """every (M, N, K) that tests/test_gpu_gemm_exact.py builds operands for (16-bit operands)"""
    shapes = set()
    for tile in X.TILES:
        shapes |= {(m, n, k) for m, n, k, _, _ in X.gemm_cases(tile)}
    shapes |= {(m, n, k) for m, n, k, _ in X.f32out_cases()}
    shapes |= {X.persistent_shape(N_CU), X.stream_k_shape(N_CU), X.split_shape(N_CU), X.TILE3_SWIGLU_SHAPE}
    shapes |= {X.row_scale_shape(t) for t in X.ROW_SCALE_TILES}
    return sorted(shapes)


SMALL = [s for s in _all_gemm_shapes() if s[0] * s[1] <= 1 << 20]
LARGE = [s for s in _all_gemm_shapes() if s[0] * s[1] > 1 << 20]


@pytest.mark.parametrize("dt", DTS)
def test_preconditions_hold_for_every_gemm_shape(dt):
    """make_operands asserts them: every operand survives a round trip through T, K max|A| max|W| < 2^24, acc * row_scale and acc + bias are
    exact in fp32; and the fp32 matmul of the integer operands IS the float64 one, element by element"""
    for M, N, K in SMALL + LARGE:
        ops = X.make_operands(1, M, N, K, dt)
        if (M, N, K) in SMALL:
            assert torch.equal((ops["A"].float() @ ops["W"].float().t()).double(), ops["acc"]), (M, N, K)
        assert len(ops["row_scale"].unique()) == min(M, 16)


@pytest.mark.parametrize("dt", DTS)
def test_preconditions_hold_for_the_fp8_and_gemv_cases(dt):
    for M, N, K, _ in X.fp8_cases():
        ops = X.make_operands(2, M, N, K, dt, 4, 4)
        sa, sw = X.fp8_scales(M, N, 2)
        s2 = sa[:, None] * sw[None, :]
        assert torch.equal(X.f32(s2), s2) and torch.equal(X.f32(ops["acc"] * s2), ops["acc"] * s2)
        v = ops["acc"] * s2 + ops["bias"]
        assert torch.equal(X.f32(v), v)
        assert set(X.e4m3_bytes(ops["A"]).unique().tolist()) <= {0x00, 0x38, 0x40, 0x44, 0x48, 0xB8, 0xC0, 0xC4, 0xC8}
    for b, N, K, *_ in X.GEMV_CASES:
        X.make_operands(3, b, N, K, dt)


def test_e4m3_codes_decode_to_the_integers():
    x = torch.arange(-4, 5).double()
    assert torch.equal(X.e4m3_bytes(x).view(torch.float8_e4m3fn).double(), x)


@pytest.mark.parametrize("dt", DTS)
def test_float64_reference_equals_plain_fp32_evaluation(dt):
    """bit for bit on the exact epilogues, with and without bias and row scale"""
    for M, N, K in SMALL:
        ops = X.cached_operands(1, M, N, K, dt)
        for epi in (X.EPI_NONE, X.EPI_RESID, X.EPI_LS_RESID, X.EPI_F32OUT):
            for bias in (False, True):
                for scale in (None, ops["row_scale"]):
                    want = X.reference_fp32(ops, epi, dt, bias, scale)
                    got = X.reference(ops, epi, dt, bias, scale)
                    assert torch.equal(got.float(), want) and torch.equal(got.float().double(), got), (M, N, K, epi, bias, scale is not None)


@pytest.mark.parametrize("dt", DTS)
def test_final_rounding_is_exercised(dt):
    """at least a quarter of the EPI_NONE + bias outputs of every case are not representable in T before the final rounding, so a kernel that
    rounds at another point (or carries fp32 further) cannot produce the expected bits"""
    low = []
    for M, N, K in SMALL + LARGE:
        ops = X.cached_operands(1, M, N, K, dt)
        share = X.unrepresentable_share(ops["acc"] + ops["bias"], dt)
        if share < 0.25:
            low.append((M, N, K, share))
    assert not low, low
    for M, N, K, _ in X.fp8_cases():
        ops = X.make_operands(2, M, N, K, dt, 4, 4)
        sa, sw = X.fp8_scales(M, N, 2)
        assert X.unrepresentable_share(ops["acc"] * sa[:, None] * sw[None, :] + ops["bias"], dt) >= 0.25, (M, N, K)
    for b, N, K, *_ in X.GEMV_CASES:
        ops = X.make_operands(3, b, N, K, dt)
        assert X.unrepresentable_share(ops["acc"] + ops["bias"], dt) >= 0.25, (b, N, K)


def test_ulp_distance():
    for T in (torch.bfloat16, torch.float16):
        a = torch.tensor([1.0, -1.0, 0.0, -0.0, 2.0, float("nan")], dtype=T)
        b = a.clone().view(torch.int16)
        b[0] += 1; b[1] += 2                    # one ulp up, two ulps further from zero
        b = b.view(T)
        d = X.ulp_distance(a, b).tolist()
        assert d[:5] == [1, 2, 0, 0, 0] and d[5] > 1 << 30
        tiny = torch.tensor([0.0], dtype=T).view(torch.int16) + 1
        assert X.ulp_distance(tiny.view(T), -tiny.view(T)).item() == 2      # across zero: the smallest subnormals are two steps apart
    assert X.first_mismatch(torch.zeros(2, 3), torch.zeros(2, 3)) is None
    w = torch.zeros(2, 3); w[1, 2] = 1
    assert "(row 1, column 2)" in X.first_mismatch(torch.zeros(2, 3), w)


@pytest.mark.parametrize("tile", sorted(X.TILES))
def test_case_lists_cover_the_edges_of_every_tile(tile):
    cases = X.gemm_cases(tile)
    bm, bn = X.tile_block(tile)
    plain = [c for c in cases if not c[4]]
    assert {c[0] for c in plain} == {1, bm - 1, bm + 1, 2 * bm + 3}
    ns = {c[1] for c in plain}
    assert {4, bn - 4, bn + 4} <= ns
    assert any(n % 16 == 8 and n > bn for n in ns), "wide stores: a block pair that ends inside a block, beyond one tile"
    assert any(n % 8 == 4 for n in ns), "narrow-store fall-back"
    assert {c[2] for c in plain} == set(X.K_AXIS)
    assert any(c[3] for c in plain) and any(not c[3] for c in plain), "strided and dense layouts"
    wide = [c for c in plain if c[1] % 8 == 0]
    assert any(c[3] for c in wide) and any(not c[3] for c in wide), "the wide-store shape in both layouts"
    sbm, sbn = X.tile_block(tile, swiglu=True)
    sw = [c for c in cases if c[4]]
    assert all(c[1] % 32 == 0 for c in sw) and any(c[1] < sbn for c in sw) and any(c[1] > sbn for c in sw)
    assert all(c[1] % 4 == 0 and c[2] % 64 == 0 for c in cases)
    # more than one block along each axis somewhere
    assert any(c[0] > bm for c in cases) and any(c[1] > bn for c in cases)


def test_tile_table_lists_every_dispatched_id():
    assert sorted(X.TILES) == list(range(1, 14))
    for t, (bm, bn, wm, wn) in X.TILES.items():
        assert bm % (16 * wm) == 0 and bn % (16 * wn) == 0
        # SwiGLU walks (gate, up) pairs of 16-column blocks: a wave tile must hold an even number of them
        assert (t in X.SWIGLU_FALLS_BACK) == (t >= 12 or (bn // wn // 16) % 2 == 1), t
    assert {7, 8, 9} <= set(X.TILES) and all(len(X.gemm_cases(t)) >= 8 for t in (7, 8, 9))


def test_launch_structure_shapes_meet_their_rules():
    M, N, K = X.persistent_shape(N_CU)
    assert -(-M // 256) * -(-N // 256) > N_CU and M % 256 and N % 256
    M, N, K = X.stream_k_shape(N_CU)
    assert X.stream_k_rule(M, N, K, N_CU) == 16 and K * X.A_MAX * X.W_MAX < 2 ** 24
    M, N, K = X.split_shape(N_CU)
    n_main, n_tail = X.split_rule(M, N, N_CU)
    assert n_main % 256 == 0 and 0 < n_tail <= 224
    assert X.split_rule(257, 280, N_CU) is None                 # the per-tile cases of ids 12 / 13 stay on the 256^2 kernel
    for M, N, K, _ in X.f32out_cases():
        assert N % 4 == 0
    assert {X.f32out_tile(M, N) for M, N, K, _ in X.f32out_cases()} == {1, 2}
    assert {c[2] for c in X.fp8_cases()} == set(X.FP8_K_AXIS) and {c[0] for c in X.fp8_cases() if not c[3]} == set(X.m_axis(256))


def test_gemv_cases_take_the_family_they_name():
    """the plan is pure (omchat_op_gemv_plan answers on the host): every form of every case goes to the kernel family it is listed under at 256
    compute units, and the list reaches all six families and the batch edges 1 / 16 / 17 / 32"""
    from omchat_amd import _lib
    l = _lib.lib()
    out = (C.c_int * 20)()
    seen, batches = set(), {}
    for b, N, K, xp, wp, mfma, forms in X.GEMV_CASES:
        for dt in (_lib.F16, _lib.BF16):
            for form, ks, family in forms:
                epi, ks_, flags = X.gemv_plan_args(b, N, K, xp, wp, form, ks)
                assert l.omchat_op_set_tuning(1, mfma) == 0
                try:
                    rc = l.omchat_op_gemv_plan(dt, b, N, K, epi, ks_, flags, 0, N_CU, out)
                finally:
                    assert l.omchat_op_set_tuning(1, 0) == 0
                assert rc == 0, (b, N, K, form, l.omchat_last_error().decode())
                assert out[0] == family, (b, N, K, form, out[0], family)
                seen.add(family); batches.setdefault(family, set()).add(b)
    assert seen == set(X.GEMV_FAMILIES)
    assert batches[X.GF_MFMA] >= {1, 16, 17, 32} and batches[X.GF_PK] >= {1, 16, 17, 32} and batches[X.GF_XS] >= {1, 16, 17, 32}
    assert batches[X.GF_ROWS] == {1} and batches[X.GF_ROWS_LONGK] == {1}      # batch-1 forms


# ---------------------------------------------------------------------------------------------------------------------------------------
# quantised weights and the norm-in-GEMV launches (X.QUANT_CASES; tests/test_gpu_gemv_quant_exact.py runs them)
# ---------------------------------------------------------------------------------------------------------------------------------------
QIDS = [c.id for c in X.QUANT_CASES]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", X.QUANT_CASES, ids=QIDS)
def test_quant_case_preconditions(dt, case):
    """make_quant_operands asserts the round trips through T, the 2^24-granule bound on every partial sum and the exactness of acc * scale (+ bias)
    in fp32; here: the weights survive THEIR storage type, the scales differ between neighbours, and the final rounding is a real one"""
    ops = case.operands(dt, N_CU)
    N, K = case.N(N_CU), case.K
    assert ops["W"].shape == (N, K) and ops["A"].shape == (case.b, K)
    if case.wf == X.WF_E4M3:
        assert torch.equal(X.e4m3_bytes(ops["W"]).view(torch.float8_e4m3fn).double(), ops["W"])
        s = ops["w_scale"]
        assert torch.equal(X.f32(s), s) and bool((s[1:] != s[:-1]).all()) and float(s.min()) >= 0.125 and float(s.max()) <= 1
    if case.wf == X.WF_MX4:
        e = ops["e"]
        assert int(ops["codes"].max()) == 15 and len(ops["codes"].unique()) == 16 and 0 < int(e.min()) + 127 and int(e.max()) + 127 < 255
        assert N == 1 or bool((e[1:] != e[:-1]).all()), "adjacent rows of a block share a scale"
        if case.wide:
            assert bool((e == e[:, :1]).all()) and N >= case.wide and (int(e.min()), int(e.max())) == (-24, case.wide - 25)
            assert case.wide == X.WIDE or not all(form in ("f32", "partial") for form, _, _ in case.forms), "the full window wherever the output is fp32"
        else:
            assert (int(e.min()), int(e.max())) == (case.e_shift - 2, case.e_shift + 2)
            assert bool((e[:, 1:] != e[:, :-1]).all()), "adjacent blocks of a row share a scale (the last block of a ragged chunk included)"
        if not case.packed:
            assert K % 32 == 0 and (K % 64 != 0 or K % 512 == 0), "MXFP4 rows: a ragged K ends inside a 64-k pair of blocks"
    elif not case.packed and K % 512 != 0:
        assert K % 64 == 0
    if not case.wide:      # as for GEMV_CASES: on acc (* scale) + bias, whichever forms the case runs
        v = ops["acc"] if ops["scale"] is None else ops["acc"] * ops["scale"]
        assert X.unrepresentable_share(v + ops["bias"], dt) >= 0.25, X.unrepresentable_share(v + ops["bias"], dt)
    else:                  # the wide cases write fp32 (no rounding to T), but for the one whose output is T(acc): that rounding
        assert all(form in ("f32", "partial") for form, _, _ in case.forms) or X.unrepresentable_share(ops["acc"], dt) >= 0.25, X.unrepresentable_share(ops["acc"], dt)
    for form, ks, _ in case.forms:
        want = X.quant_reference(ops, form, dt)
        assert torch.equal(want.float().double(), want)
        if form.startswith("swiglu"):      # silu(g) * u may leave f16's range on a few outputs (the 16-bit GEMV_CASES: 2-3 %), where 2 ulp bounds nothing
            assert float(torch.isfinite(want).double().mean()) >= 0.97, (form, float(torch.isfinite(want).double().mean()))
        else:
            assert bool(torch.isfinite(want).all()), (form, "an expected value is not finite")
        if form == "partial":
            assert bool((want / ops["granule"] == (want / ops["granule"]).round()).all())


@pytest.mark.parametrize("dt", DTS)
def test_exact_rmsnorm_survives_any_rsqrt(dt):
    """xn = T(nw * T(x * inv)) equals nw * x / 2 for every inv within +-8 fp32 ulps of rsqrt(tot / K + eps), for every norm case: the bits of the
    normalised row do not depend on the device's rsqrtf"""
    seen = set()
    for case in X.QUANT_CASES:
        if not case.norm or (case.K, case.wf) in seen:
            continue
        seen.add((case.K, case.wf))
        ops = case.operands(dt, N_CU, cached=False)
        x, nw = ops["A"], ops["nw"]
        assert case.K % 8 == 0 and float((x * x).sum()) == 4.0 * case.K
        assert set(x.abs().reshape(-1, 8).sort(dim=1).values.unique(dim=0).flatten().tolist()) == {0.0, 1.0, 2.0, 3.0, 4.0}
        tot = (x.float() * x.float()).sum()
        assert float(tot / float(case.K)) == 4.0
        inv0 = X.norm_inv(x)
        assert abs(float(inv0) - 0.5) < 1e-6
        for d in range(-8, 9):
            inv = (inv0.view(torch.int32) + d).view(torch.float32)
            assert torch.equal(X.norm_xn(x, nw, inv, dt), nw[None, :] * x / 2), (case.id, d)
        assert torch.equal(ops["xn"], nw[None, :] * x / 2)
    assert len(seen) >= 9


def test_quant_cases_take_the_family_they_name():
    """the plan at 256 compute units answers the listed family (and waves / rows per wave where the case pins them) for every form of every case,
    under the case's tuning keys; and every family x weight-form pair of the issue is in the list"""
    from omchat_amd import _lib
    l = _lib.lib()
    out = (C.c_int * 20)()
    seen = set()
    for case in X.QUANT_CASES:
        for dt in (_lib.F16, _lib.BF16):
            for form, ks, family in case.forms:
                epi, ks_, flags = case.plan_args(form, ks)
                try:
                    for key, value, _ in case.tuning:
                        assert l.omchat_op_set_tuning(key, value) == 0
                    rc = l.omchat_op_gemv_plan(dt, case.b, case.N(N_CU), case.K, epi, ks_, flags, case.wf, N_CU, out)
                finally:
                    for key, _, back in case.tuning:
                        assert l.omchat_op_set_tuning(key, back) == 0
                assert rc == 0, (case.id, form, l.omchat_last_error().decode())
                assert out[0] == family and out[1] == case.wf, (case.id, form, out[0], family)
                for i, v in case.pins.items():
                    assert out[i] == v, (case.id, form, "plan field", i, out[i], v)
                seen.add((family, case.wf))
    assert seen == X.QUANT_PAIRS, (seen ^ X.QUANT_PAIRS)
    wide = {c.forms[0][2] for c in X.QUANT_CASES if c.wide}
    assert wide == {f for f, w in X.QUANT_PAIRS if w == X.WF_MX4}, "one wide-exponent variant per MXFP4 family"
    norm_rr = {(c.wf, c.forms[0][0] == "swiglu", c.pins.get(8)) for c in X.QUANT_CASES if c.norm and 8 in c.pins}
    for wf in (X.WF_16, X.WF_E4M3, X.WF_MX4):      # every rows-per-wave answer of rows_per_wave for a norm launch (csrc/gemv.hip)
        assert {r for w, s, r in norm_rr if w == wf and not s} == {1, 2, 4}
        assert {r for w, s, r in norm_rr if w == wf and s} == ({1, 2, 3} if wf == X.WF_16 else {1, 2, 4})
    assert {c.b for c in X.QUANT_CASES if c.packed} == {1, 16, 17, 32}


CORRUPTIONS = ("nibbles", "last_scale", "next_row_scale", "drop32", "swap_gate_up")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", X.QUANT_CASES, ids=QIDS)
def test_quant_reference_discriminates(dt, case):
    """a kernel that swaps the nibbles of a byte, takes the neighbouring block's or the next row's scale, drops the last 32 k, crosses gate and up in
    the last block or adds the bias before the e4m3 scale would have computed on other operands: each must change at least one expected
    element of every form it applies to"""
    ops = case.operands(dt, N_CU)
    for form, ks, _ in case.forms:
        want = X.quant_reference(ops, form, dt)
        for kind in CORRUPTIONS:
            if kind == "swap_gate_up" and not form.startswith("swiglu"):
                continue
            bad = X.corrupt(ops, kind, dt)
            if bad is None:
                continue
            other = X.quant_reference(bad, form, dt)
            assert not torch.equal(other, want), (case.id, form, kind, "changes no expected element")
        if form == "bias" and case.wf == X.WF_E4M3:
            assert not torch.equal(X.bias_before_scale(ops, dt), want), (case.id, "bias before the scale changes no expected element")
