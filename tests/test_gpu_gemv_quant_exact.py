"""Exact per-element tests of the skinny GEMV launches that tests/test_gpu_gemv_exact.py leaves out: e4m3 and MXFP4 weights in the whole-row,
long-K, norm, norm-loop, packed, x-stationary and x-stationary split-K families, the 16-bit norm-in-GEMV forms (four-wave, nine-wave, loop, every
rows-per-wave answer) and the seven-wave residual form -- X.QUANT_CASES of tests/gemm_exact_ref.py, on operands for which the expected BITS are
determined: integer / dyadic x, integer e4m3 weights under row scales k / 8, hand-built MXFP4 codes and e8m0 bytes, and for the norm forms the
exact-RMSNorm row whose normalised value does not depend on the last bits of rsqrtf (tests/test_gemm_exact_cpu.py proves all of that).

As in test_gemv_exact: the plan is pinned on the device before each launch (family, weight form, and waves / rows per wave where the case names
them); Y carries a sentinel behind its last element / in its ldy padding and guard rows, which must survive; bias, fp32 output, residual and the
sums of the EPI_PARTIAL slices are asserted with torch.equal, every slice being a multiple of the case's granule; SwiGLU within 2 ulp of T (and
gemm_exact_ref.tail_floor); swiglu_yp equals the row-major SwiGLU bit for bit.  The weight rows behind row N are poison that is never read (the
row index clamps to N - 1): e4m3 bytes 0x7F under NaN scales, MXFP4 scale bytes 0xFF, NaN for 16-bit rows.  No engine, no model."""
import ctypes as C
import pytest
import torch

pytestmark = pytest.mark.gpu
from gpu_util import DT, CODE, ptr, sync
from omchat_amd import _lib
import gemm_exact_ref as X
import mxfp4_ref

DTS = ["bf16", "f16"]
NAN = float("nan")
GUARD = 8


def _dev16(x, ld, guard, T):
    """[rows, cols] float64 -> T [rows + guard, ld] on the device, NaN in the padding and the guard rows"""
    rows, cols = x.shape
    t = torch.full((rows + guard, ld), NAN, dtype=T)
    t[:rows, :cols] = x.to(torch.float32).to(T)
    return t.cuda()


def _dev_bytes(x, guard, poison):
    t = torch.full((x.shape[0] + guard, x.shape[1]), poison, dtype=torch.uint8)
    t[:x.shape[0]] = x
    return t.cuda()


def _sentinel(n, T):
    if T == torch.float32:
        return torch.full((n,), X.SENTINEL32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full((n,), X.SENTINEL16, dtype=torch.int16, device="cuda").view(T)


def _untouched(t):
    if t.dtype == torch.float32:
        return t.view(torch.int32) == X.SENTINEL32
    return t.view(torch.int16) == X.SENTINEL16


def _unpack_x(packed, K, NB):
    """inverse of common.h packed_x_index on the host: [NB * 16, K]"""
    p = packed.view(K // 64, 2, NB, 4, 16, 8)
    return p.permute(2, 4, 0, 1, 3, 5).reshape(NB * 16, K)


class Weights:
    """the device copies of one operand set: x, the weights in their storage form with poisoned guard rows, scales, norm weights, bias, residual"""

    def __init__(self, case, ops, T, N, K):
        b = case.b
        self.ldx = K + 8 if case.packed or case.wf == X.WF_16 and not case.norm else K      # the dense entries take ldx = K
        self.x = _dev16(ops["A"], self.ldx, GUARD if b > 1 or self.ldx > K else 1, T)
        self.nw = ops["nw"].to(torch.float32).to(T).cuda() if case.norm else None
        self.bias = ops["bias"].to(torch.float32).to(T).cuda()
        self.resid = _dev16(ops["resid"], N, 1, T)
        self.scale = self.s = None
        if case.wf == X.WF_E4M3:
            self.w = _dev_bytes(X.e4m3_bytes(ops["W"]), GUARD, 0x7F)
            self.scale = torch.cat((ops["w_scale"].float(), torch.full((GUARD,), NAN))).cuda()
        elif case.wf == X.WF_MX4:
            self.w = _dev_bytes(mxfp4_ref.pack(ops["codes"]), GUARD, 0x77)
            self.s = _dev_bytes((ops["e"] + 127).to(torch.uint8), GUARD, 0xFF)
        else:
            self.ldw = K + 16
            self.w = _dev16(ops["W"], self.ldw, GUARD, T)


def _launch(lib, case, dw, form, ks, epi, dt, Y, ldy, N, K):
    code, f32, bias = CODE[dt], int(form == "f32"), ptr(dw.bias) if form == "bias" else None
    resid = ptr(dw.resid) if form == "resid" else None
    if case.packed:
        return lib.omchat_op_gemv_mxfp4_packed(code, ptr(dw.x), dw.ldx, ptr(dw.w), ptr(dw.s), ptr(Y), ldy, case.b, N, K, bias, epi, f32, ks,
                                               int(form == "swiglu_yp"), None)
    if case.norm:
        if case.wf == X.WF_16:
            return lib.omchat_op_gemv_norm(code, ptr(dw.x), ptr(dw.w), dw.ldw, ptr(Y), N, K, ptr(dw.nw), X.NORM_EPS, bias, epi, f32, None)
        if case.wf == X.WF_E4M3:
            return lib.omchat_op_gemv_fp8_norm(code, ptr(dw.x), ptr(dw.w), ptr(dw.scale), ptr(Y), N, K, ptr(dw.nw), X.NORM_EPS, bias, epi, f32, None)
        return lib.omchat_op_gemv_mxfp4_norm(code, ptr(dw.x), ptr(dw.w), ptr(dw.s), ptr(Y), N, K, ptr(dw.nw), X.NORM_EPS, bias, epi, f32, None)
    if case.wf == X.WF_16:
        return lib.omchat_op_gemv(code, ptr(dw.x), dw.ldx, ptr(dw.w), dw.ldw, ptr(Y), ldy, 1, N, K, bias, resid, N, epi, f32, None)
    if case.wf == X.WF_E4M3:
        return lib.omchat_op_gemv_fp8(code, ptr(dw.x), ptr(dw.w), ptr(dw.scale), ptr(Y), N, K, bias, resid, epi, f32, ks, None)
    return lib.omchat_op_gemv_mxfp4(code, ptr(dw.x), ptr(dw.w), ptr(dw.s), ptr(Y), N, K, bias, resid, epi, f32, ks, None)


def _launch_prepacked(lib, case, dw, dt, Y, ldy, N, K, T):
    """the same launch through the pack-once entries: omchat_op_pack_x, omchat_op_pack_w4, omchat_op_gemv_prepacked (EPI_NONE with bias)"""
    NB = 2 if case.b > 16 else 1
    xp = torch.zeros(NB * 16 * K, dtype=T, device="cuda")
    w4p = torch.zeros(N * K // 2, dtype=torch.uint8, device="cuda")
    sp = torch.zeros(N * K // 32, dtype=torch.uint8, device="cuda")
    _lib.check(lib.omchat_op_pack_x(CODE[dt], ptr(dw.x), dw.ldx, case.b, K, ptr(xp), None))
    _lib.check(lib.omchat_op_pack_w4(ptr(dw.w), ptr(dw.s), N, K, ptr(w4p), ptr(sp), None))
    _lib.check(lib.omchat_op_gemv_prepacked(CODE[dt], ptr(xp), ptr(w4p), ptr(sp), ptr(Y), ldy, case.b, N, K, ptr(dw.bias), X.EPI_NONE, 0, 0, 0, None))
    sync()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ci", range(len(X.QUANT_CASES)), ids=[c.id for c in X.QUANT_CASES])
def test_gemv_quant_exact(gpu_lib, dt, ci):
    case = X.QUANT_CASES[ci]
    T = DT[dt]
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    b, N, K = case.b, case.N(n_cu), case.K
    ops = case.operands(dt, n_cu)
    dw = Weights(case, ops, T, N, K)
    NB = 2 if b > 16 else 1
    plan = (C.c_int * 20)()
    row_major_swiglu = None
    try:
        for key, value, _ in case.tuning:
            _lib.check(gpu_lib.omchat_op_set_tuning(key, value))
        for form, ks, family in case.forms:
            epi, ks_, flags = case.plan_args(form, ks)
            _lib.check(gpu_lib.omchat_op_gemv_plan(CODE[dt], b, N, K, epi, ks_, flags, case.wf, 0, plan))
            assert plan[0] == family and plan[1] == case.wf, (form, "the plan sends this case to family", plan[0], "weight form", plan[1], "not", family, case.wf)
            for i, v in case.pins.items():
                assert plan[i] == v, (form, "plan field", i, "is", plan[i], "not", v)
            what = (case.id, form, "family", family, b, N, K)
            f32 = form in ("f32", "partial")
            cols = N // 2 if epi == X.EPI_SWIGLU else N
            want64 = X.quant_reference(ops, form, dt)
            want = want64.float() if f32 else want64.to(torch.float32).to(T)
            floor = X.quant_tail_floor(ops, dt) if epi == X.EPI_SWIGLU else None
            slices = max(ks, 1) if form == "partial" else 1
            if form == "swiglu_yp":
                rows, ldy = 1, 0
                Y = _sentinel(NB * 16 * cols + GUARD, T)
            else:
                ldy = cols + 8 if case.packed else cols                     # the batch-1 entries write dense rows
                rows = slices * b
                Y = _sentinel((rows + (GUARD if case.packed else 0)) * ldy + GUARD, torch.float32 if f32 else T)
            _lib.check(_launch(gpu_lib, case, dw, form, ks, epi, dt, Y, ldy, N, K))
            sync()
            host = Y.cpu()
            if form == "swiglu_yp":
                assert bool(_untouched(host[NB * 16 * cols:]).all()), (what, "written behind the packed output")
                host = _unpack_x(host[:NB * 16 * cols], cols, NB)
                msg = X.first_mismatch(host[:b], want, 2, floor)
                assert msg is None, (what, msg)
                assert bool(_untouched(host[b:]).all()), (what, "packed rows behind row b were written")
                assert row_major_swiglu is not None and torch.equal(host[:b].view(torch.int16), row_major_swiglu.view(torch.int16)), what
                continue
            grid = host[:(rows + (GUARD if case.packed else 0)) * ldy].reshape(-1, ldy)
            assert bool(_untouched(host[grid.numel():]).all()), (what, "written behind the last element of Y")
            assert bool(_untouched(grid[:rows, cols:]).all()) and bool(_untouched(grid[rows:]).all()), (what, "the ldy padding or a guard row was written")
            got = grid[:rows, :cols]
            if form == "partial":
                part = got.reshape(slices, b, cols).double()
                assert bool(torch.isfinite(part).all()), (what, "a slice is not finite")
                units = part / ops["granule"]
                assert torch.equal(units, units.round()), (what, "a slice is not a multiple of the granule",
                                                          X.first_mismatch(units.reshape(-1, cols).float(), units.round().reshape(-1, cols).float()))
                total = part.sum(0)
                assert torch.equal(total, want64), (what, X.first_mismatch(total.float(), want, 0))
            elif epi == X.EPI_SWIGLU:
                msg = X.first_mismatch(got, want, 2, floor)
                assert msg is None, (what, msg)
                row_major_swiglu = got.contiguous()
            else:
                assert torch.equal(got, want), (what, X.first_mismatch(got, want, 0))
                if form == "bias" and ci == X.PREPACKED_CASE:
                    Y2 = _sentinel(Y.numel(), T)
                    _launch_prepacked(gpu_lib, case, dw, dt, Y2, ldy, N, K, T)
                    assert torch.equal(Y2.cpu().view(torch.int16), host.view(torch.int16)), (what, "the pre-packed launch differs")
    finally:
        for key, _, back in case.tuning:
            gpu_lib.omchat_op_set_tuning(key, back)
