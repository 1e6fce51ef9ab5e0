"""Exact per-element tests of the 16-bit skinny GEMV (omchat_op_gemv, omchat_op_gemv_packed with w_packed / y_packed): one case per kernel
family that the product build reaches without a norm -- MFMA, packed, x-stationary, x-stationary split-K, whole-row and long-K whole-row --
on the integer / dyadic operands of tests/gemm_exact_ref.py, for which the fp32 accumulation is exact in any order (split-K slices and
v_dot2 included).  EPI_NONE with bias, out_f32, EPI_RESID and EPI_PARTIAL are asserted bit for bit, SwiGLU within 2 ulp of T (and, for bf16
results below fp32's smallest normal number, within gemm_exact_ref.tail_floor: the device returns those as signed zeros).

Each form first asks omchat_op_gemv_plan which family the launch takes on this device and asserts the one the case is listed under, so a
later change to the plan cannot silently move a case to another kernel.  Y carries a sentinel in its ldy padding and in guard rows behind
row b, which must survive.  The K ranges of the EPI_PARTIAL slices are the kernels' own business: asserted are that every slice holds
integers (a partial sum of integer products) and that the slices add up to the exact product.  The norm-in-GEMV forms (on an x whose
normalised row does not depend on the last bits of the rsqrt), the quantised weights and the seven-wave residual form are held to the same
standard in tests/test_gpu_gemv_quant_exact.py."""
import ctypes as C
import pytest
import torch

pytestmark = pytest.mark.gpu
from gpu_util import DT, CODE, ptr, sync
from omchat_amd import _lib
import gemm_exact_ref as X

DTS = ["bf16", "f16"]
NAN = float("nan")
GUARD = 8


def _padded(x, ld, guard, T):
    rows, cols = x.shape
    t = torch.full((rows + guard, ld), NAN, dtype=T)
    t[:rows, :cols] = x.to(torch.float32).to(T)
    return t.cuda()


def _sentinel(rows, ld, T):
    if T == torch.float32:
        return torch.full((rows, ld), X.SENTINEL32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full((rows, ld), X.SENTINEL16, dtype=torch.int16, device="cuda").view(T)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16), X.SENTINEL32 if t.dtype == torch.float32 else X.SENTINEL16


def _unpack_x(packed, K, NB):
    """inverse of common.h packed_x_index on the host: [NB * 16, K]"""
    p = packed.view(K // 64, 2, NB, 4, 16, 8)                 # [chunk][half][nb][g][row % 16][j]
    return p.permute(2, 4, 0, 1, 3, 5).reshape(NB * 16, K)    # row = nb * 16 + r ; k = chunk * 64 + half * 32 + g * 8 + j


def _check(Y, rows, cols, want, tol, what, floor=None):
    host = Y.cpu()
    got = host[:rows, :cols]
    msg = X.first_mismatch(got, want, tol, floor)
    if tol == 0:
        assert torch.equal(got, want), (what, msg)
    assert msg is None, (what, msg)
    bits, s = _bits(host)
    assert bool((bits[:rows, cols:] == s).all()), (what, "the ldy padding was written")
    assert bool((bits[rows:] == s).all()), (what, "a guard row behind row b was written")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", range(len(X.GEMV_CASES)), ids=lambda i: "b{}-N{}-K{}-x{}w{}m{}".format(*X.GEMV_CASES[i][:6]))
def test_gemv_exact(gpu_lib, dt, case):
    b, N, K, xp, wp, mfma, forms = X.GEMV_CASES[case]
    T = DT[dt]
    ops = X.make_operands(3, b, N, K, dt)
    dX = _padded(ops["A"], K + 8, GUARD, T)
    dW = _padded(ops["W"], K + 16, GUARD, T)
    ldr = N + 4
    dR = _padded(ops["resid"], ldr, GUARD, T)
    dbias = ops["bias"].to(T).cuda()
    NB = 2 if b > 16 else 1
    plan = (C.c_int * 20)()
    row_major_swiglu = None
    gpu_lib.omchat_op_set_tuning(1, mfma)
    try:
        for form, ks, family in forms:
            epi, ks_, flags = X.gemv_plan_args(b, N, K, xp, wp, form, ks)
            _lib.check(gpu_lib.omchat_op_gemv_plan(CODE[dt], b, N, K, epi, ks_, flags, 0, 0, plan))
            assert plan[0] == family, (form, "the plan sends this case to family", plan[0], "not", family)
            what = (form, "family", family, b, N, K)
            f32 = form in ("f32", "partial")
            cols = N // 2 if epi == X.EPI_SWIGLU else N
            want64 = X.gemv_reference(ops, form, dt)
            want = want64.float() if f32 else want64.to(torch.float32).to(T)
            if form == "swiglu_yp":
                Y = _sentinel(1, NB * 16 * cols, T)
                ldy = 0
            else:
                slices = max(ks, 1) if form == "partial" else 1
                ldy = cols + 8
                Y = _sentinel(slices * b + GUARD, ldy, torch.float32 if f32 else T)
            if xp:
                _lib.check(gpu_lib.omchat_op_gemv_packed(CODE[dt], ptr(dX), K + 8, ptr(dW), K + 16, ptr(Y), ldy, b, N, K,
                                                         ptr(dbias) if form == "bias" else None, epi, int(form == "f32"), ks, wp,
                                                         int(form == "swiglu_yp"), None))
            else:
                _lib.check(gpu_lib.omchat_op_gemv(CODE[dt], ptr(dX), K + 8, ptr(dW), K + 16, ptr(Y), ldy, b, N, K,
                                                  ptr(dbias) if form == "bias" else None, ptr(dR) if form == "resid" else None, ldr, epi,
                                                  int(form == "f32"), None))
            sync()
            if form == "swiglu_yp":
                host = _unpack_x(Y.cpu().reshape(-1), cols, NB)
                msg = X.first_mismatch(host[:b], want, 2, X.tail_floor(ops, X.EPI_SWIGLU, dt))
                assert msg is None, (what, msg)
                bits, s = _bits(host)
                assert bool((bits[b:] == s).all()), (what, "packed rows behind row b were written")
                if row_major_swiglu is not None:      # the same values, packed for the next GEMV
                    assert torch.equal(host[:b].view(torch.int16), row_major_swiglu.view(torch.int16)), what
            elif form == "partial":
                host = Y.cpu()
                part = host[:slices * b, :cols].reshape(slices, b, cols)
                assert torch.isfinite(part).all() and torch.equal(part, part.round()), (what, "a slice is not a sum of integer products")
                total = part.double().sum(0)
                msg = X.first_mismatch(total.float(), want, 0)
                assert torch.equal(total, want64), (what, msg)
                bits, s = _bits(host)
                assert bool((bits[:slices * b, cols:] == s).all()) and bool((bits[slices * b:] == s).all()), (what, "padding / guard rows written")
            else:
                _check(Y, b, cols, want, 2 if form == "swiglu" else 0, what, X.tail_floor(ops, X.EPI_SWIGLU, dt) if form == "swiglu" else None)
                if form == "swiglu":
                    row_major_swiglu = Y.cpu()[:b, :cols].contiguous()
    finally:
        gpu_lib.omchat_op_set_tuning(1, 0)
