"""Device-side helpers of the exact GEMM tests (tests/test_gpu_gemm_exact.py, tests/test_gpu_vit_stats.py): the operands of a case on the device
in the dense or the poisoned strided layout, one launch of an epilogue, and the comparison with the float64 reference of tests/gemm_exact_ref.py
including the sentinel in the padding columns and the guard rows."""
import torch

from gpu_util import DT, CODE, ptr, sync
from omchat_amd import _lib
import gemm_exact_ref as X

NAN = float("nan")
EPI_OF = {"none": X.EPI_NONE, "bias": X.EPI_NONE, "resid": X.EPI_RESID, "ls_resid": X.EPI_LS_RESID, "gelu": X.EPI_GELU, "swiglu": X.EPI_SWIGLU,
          "f32out": X.EPI_F32OUT}
TOL_ULP = {"gelu": 1, "swiglu": 2}
GUARD = 8           # rows allocated behind the last row of a strided operand / output


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _padded(x, ld, guard, T):
    """x [rows, cols] (float64) as a device tensor [rows + guard, ld] of T with NaN in the padding columns and the guard rows"""
    rows, cols = x.shape
    t = torch.full((rows + guard, ld), NAN, dtype=T)
    t[:rows, :cols] = x.to(torch.float32).to(T)
    return t.cuda()


def _sentinel(rows, ld, T):
    if T == torch.float32:
        return torch.full((rows, ld), X.SENTINEL32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full((rows, ld), X.SENTINEL16, dtype=torch.int16, device="cuda").view(T)


class Problem:
    """the operands of one case on the device.  strided: lda, ldw > K with NaN in the padding columns, NaN guard rows behind row M of A and row N of W,
    ldc > N and ldr > N with ldr != ldc (NaN in the residual's padding and guard rows), C pre-filled with a sentinel and eight guard rows"""

    def __init__(self, ops, dt, strided):
        T = DT[dt]
        self.ops, self.dt, self.strided = ops, dt, strided
        self.M, self.K = ops["A"].shape
        self.N = ops["W"].shape[0]
        g = GUARD if strided else 0
        self.lda, self.ldw = (self.K + 8, self.K + 16) if strided else (self.K, self.K)
        self.ldr = self.N + 4 if strided else self.N
        self.A, self.W = _padded(ops["A"], self.lda, g, T), _padded(ops["W"], self.ldw, g, T)
        self.R = _padded(ops["resid"], self.ldr, g, T)
        self.bias, self.ls = ops["bias"].to(T).cuda(), ops["ls"].to(T).cuda()

    def out(self, cols, T):
        ldc = cols + 8 if self.strided else cols      # (+8 keeps ldc % 8 == 0 where N % 8 == 0: the wide-store path stays reachable)
        return _sentinel(self.M + (GUARD if self.strided else 0), ldc, T), ldc


def _check(C, M, cols, want64, tol, what, floor=None):
    """the [M, cols] corner of C against the reference; the padding columns and the guard rows must still carry the sentinel, bit for bit"""
    host = C.cpu()
    T = host.dtype
    got, want = host[:M, :cols], want64.to(torch.float32).to(T)
    msg = X.first_mismatch(got, want, tol, floor)
    if tol == 0:
        assert torch.equal(got, want), (what, msg)
    assert msg is None, (what, msg)
    assert not torch.isnan(got.float()).any(), what
    bits = host.view(torch.int32 if T == torch.float32 else torch.int16)
    s = X.SENTINEL32 if T == torch.float32 else X.SENTINEL16
    assert bool((bits[:M, cols:] == s).all()), (what, "a padding column between N and ldc was written")
    assert bool((bits[M:] == s).all()), (what, "a guard row behind row M was written")


def _launch(lib, P, name, tile, row_scale=None, rs=None, sk=None):
    """one launch of epilogue `name` on problem P; returns (C, columns of the output)"""
    epi = EPI_OF[name]
    cols = P.N // 2 if name == "swiglu" else P.N
    C, ldc = P.out(cols, torch.float32 if name == "f32out" else DT[P.dt])
    bias = ptr(P.bias) if name in ("bias", "ls_resid", "gelu") else None
    resid = ptr(P.R) if name in ("resid", "ls_resid") else None
    head = (CODE[P.dt], ptr(P.A), P.lda, ptr(P.W), P.ldw, ptr(C), ldc, P.M, P.N, P.K, bias, ptr(P.ls), resid, P.ldr, epi, tile)
    if sk is not None:
        _lib.check(lib.omchat_op_gemm_sk(*head, ptr(sk), sk.numel(), 1, None))
    elif row_scale is not None or rs is not None:
        stats, rs_ld, nslots, dim = rs if rs is not None else (None, 0, 0, 0)
        _lib.check(lib.omchat_op_gemm_fused(*head, ptr(row_scale), ptr(stats), rs_ld, nslots, dim, 0.0, None, 0, None, None))
    else:
        _lib.check(lib.omchat_op_gemm(*head, None))
    sync()
    return C, cols


def _run(lib, P, name, tile, scale=None, **kw):
    C, cols = _launch(lib, P, name, tile, **kw)
    has_bias = name in ("bias", "ls_resid", "gelu")
    want = X.reference(P.ops, EPI_OF[name], P.dt, bias=has_bias, scale=scale)
    _check(C, P.M, cols, want, TOL_ULP.get(name, 0), (name, "tile", tile, P.M, P.N, P.K, "strided" if P.strided else "dense"),
           X.tail_floor(P.ops, EPI_OF[name], P.dt, has_bias, scale))
    return C
