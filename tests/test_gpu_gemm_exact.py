"""Exact per-element tests of the MFMA GEMM: every tile id of launch_epi, both types, every epilogue, through omchat_op_gemm,
omchat_op_gemm_fused, omchat_op_gemm_sk and omchat_op_gemm_fp8, against the float64 reference of tests/gemm_exact_ref.py on operands for
which that reference is exact (small integers in A and W, dyadic epilogue operands: the fp32 accumulator holds the exact sum in any order).

EPI_NONE (with and without bias), EPI_RESID, EPI_LS_RESID, EPI_F32OUT and the row-scale forms are asserted with torch.equal: any indexing,
guard or rounding-point error shows as a named element.  GELU may differ by 1 ulp of T and SwiGLU by 2: the device erf / exp are
fp32-accurate, so a result can only fall on the other side of one rounding boundary of T (SwiGLU has two roundings in series); an indexing
error moves values by far more.  Below fp32's smallest normal number that accuracy ends -- bf16 results of 1e-37 and less come back as signed
zeros (measured: 1 to 149 elements per SwiGLU case with gates in [-97, -88]) -- so those two epilogues also pass an element whose absolute
error is within gemm_exact_ref.tail_floor (2^-126 |x| or 2^-126 |g u|); the exact epilogues have no such floor.

tests/test_gemm_exact_cpu.py proves the reference's preconditions for every case list used here."""
import pytest
import torch

pytestmark = pytest.mark.gpu
from gpu_util import DT, CODE, ptr, sync
from omchat_amd import _lib
import gemm_exact_ref as X

DTS = ["bf16", "f16"]
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


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", range(8))
@pytest.mark.parametrize("tile", sorted(X.TILES))
def test_gemm_every_tile_every_epilogue(gpu_lib, dt, tile, case):
    """tile ids 1 .. 13 at the smallest shapes that reach every guard of the tile (gemm_exact_ref.gemm_cases): M in {1, BM - 1, BM + 1, 2 BM + 3},
    N at 4, either side of BN, 8 mod 16 and 4 mod 8, K of one step, an odd step count and a long loop; dense and strided / poisoned layouts.
    SwiGLU on tiles 3, 10, 11, 12 and 13 is the documented fall-back to the 256^2 kernel"""
    M, N, K, strided, swiglu = X.gemm_cases(tile)[case]
    P = Problem(X.cached_operands(1, M, N, K, dt), dt, strided)
    for name in (("swiglu",) if swiglu else ("none", "bias", "resid", "ls_resid", "gelu")):
        _run(gpu_lib, P, name, tile)


@pytest.mark.parametrize("dt", DTS)
def test_tile3_swiglu_falls_back_to_the_256_kernel(gpu_lib, dt):
    """force_tile = 3 under SwiGLU: 48-column wave tiles cannot hold the (gate, up) block pairs; the dispatch falls through to the 256^2
    kernel as it does for tiles 10 / 11 -- the same bits as force_tile = 2, and the reference within 2 ulp"""
    P = Problem(X.cached_operands(1, *X.TILE3_SWIGLU_SHAPE, dt), dt, True)
    c3 = _run(gpu_lib, P, "swiglu", 3)
    c2 = _run(gpu_lib, P, "swiglu", 2)
    assert torch.equal(c3.view(torch.int16), c2.view(torch.int16))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K,strided", X.f32out_cases())
def test_gemm_f32out(gpu_lib, dt, M, N, K, strided):
    """raw fp32 accumulators: the 128^2 kernel below 64 tiles of 256^2, the staggered 256^2 kernel above (the dispatch ignores force_tile)"""
    P = Problem(X.cached_operands(1, M, N, K, dt), dt, strided)
    _run(gpu_lib, P, "f32out", 0)


def _pow2_scale(M):
    """per-row factors 4, 2, 1, 1/2 -- rsqrt of the powers of four 1/16 .. 4"""
    return 2.0 ** (1 - ((torch.arange(M) * 3 + 1) % 4).to(torch.float64))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("tile", X.ROW_SCALE_TILES)
def test_gemm_row_scale(gpu_lib, dt, tile):
    """omchat_op_gemm_fused: T(s[m] * acc + bias ...) with a different dyadic factor per row, finished (row_scale) and as statistics slots
    whose rsqrt is exact: two slots per row with sum / dim a power of four and eps = 0, so rstd = 4, 2, 1 or 1/2"""
    M, N, K = X.row_scale_shape(tile)
    ops = X.cached_operands(1, M, N, K, dt)
    P = Problem(ops, dt, True)
    s8 = ops["row_scale"].float().cuda()
    for name in ("bias", "ls_resid", "resid"):
        _run(gpu_lib, P, name, tile, scale=ops["row_scale"], row_scale=s8)
    s2 = _pow2_scale(M)
    dim, rs_ld = 64, M + 3
    total = dim / (s2 * s2)                                       # sum of the row's slots: dim * 4^e
    stats = torch.full((2, rs_ld), NAN, dtype=torch.float32)
    stats[0, :M], stats[1, :M] = (0.75 * total).float(), (0.25 * total).float()
    stats = stats.cuda()
    for name in ("bias", "ls_resid"):
        _run(gpu_lib, P, name, tile, scale=s2, row_scale=s2.float().cuda())
        _run(gpu_lib, P, name, tile, scale=s2, rs=(stats, rs_ld, 2, dim))


@pytest.mark.parametrize("dt", DTS)
def test_gemm_persistent_form(gpu_lib, dt):
    """tuning key 13: one workgroup per compute unit walks several 256^2 tiles and issues the next tile's loads before its epilogue"""
    M, N, K = X.persistent_shape(_cus())
    assert -(-M // 256) * -(-N // 256) > _cus()
    P = Problem(X.cached_operands(1, M, N, K, dt), dt, False)
    gpu_lib.omchat_op_set_tuning(13, 1)
    try:
        for name in ("bias", "ls_resid"):
            _run(gpu_lib, P, name, 2)
    finally:
        gpu_lib.omchat_op_set_tuning(13, 0)


@pytest.mark.parametrize("dt", DTS)
def test_gemm_stream_k(gpu_lib, dt):
    """stream_k = 1: the K loops of 16 tiles dealt to all workgroups, partial slabs added by the tile's owner -- integers, so the same bits"""
    M, N, K = X.stream_k_shape(_cus())
    assert X.stream_k_rule(M, N, K, _cus()) > 0, "the shape must take the stream-K launch on this device"
    P = Problem(X.cached_operands(1, M, N, K, dt), dt, True)
    ws = torch.empty(gpu_lib.omchat_op_gemm_sk_ws(), dtype=torch.uint8, device="cuda")
    for name in ("bias", "resid", "ls_resid"):
        _run(gpu_lib, P, name, 2, sk=ws)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("tile", [12, 13])
def test_gemm_two_launch_split(gpu_lib, dt, tile):
    """tiles 12 / 13: whole rounds of 256^2 tiles on the leading columns, one round of 192 x 224 tiles (8 or 12 waves) on the tail"""
    M, N, K = X.split_shape(_cus())
    if X.split_rule(M, N, _cus()) is None:
        pytest.skip(f"launch_epi's rule does not split {M} x {N} on {_cus()} compute units")
    P = Problem(X.cached_operands(1, M, N, K, dt), dt, False)
    for name in ("bias", "ls_resid"):
        _run(gpu_lib, P, name, tile)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K,swiglu", X.fp8_cases())
def test_gemm_fp8_exact(gpu_lib, dt, M, N, K, swiglu):
    """omchat_op_gemm_fp8: e4m3 bytes of integers in [-4, 4] built on the host, dyadic per-row scales; T(sa[m] sw[n] acc + bias ...) is exact"""
    T = DT[dt]
    ops = X.make_operands(2, M, N, K, dt, 4, 4)
    sa, sw = X.fp8_scales(M, N, 2)
    A8, W8 = X.e4m3_bytes(ops["A"]).cuda(), X.e4m3_bytes(ops["W"]).cuda()
    dsa, dsw = sa.float().cuda(), sw.float().cuda()
    bias_d = ops["bias"].to(T).cuda()
    strided = M % 2 == 1
    ldr = N + 4 if strided else N
    R = _padded(ops["resid"], ldr, GUARD if strided else 0, T)
    s2 = sa[:, None] * sw[None, :]
    for name in (("swiglu",) if swiglu else ("none", "bias", "resid", "gelu")):
        cols = N // 2 if swiglu else N
        ldc = cols + 8 if strided else cols
        C = _sentinel(M + (GUARD if strided else 0), ldc, T)
        _lib.check(gpu_lib.omchat_op_gemm_fp8(CODE[dt], ptr(A8), ptr(dsa), ptr(W8), ptr(dsw), ptr(C), ldc, M, N, K,
                                              ptr(bias_d) if name in ("bias", "gelu") else None, ptr(R) if name == "resid" else None, ldr,
                                              EPI_OF[name], None))
        sync()
        want = X.reference(ops, EPI_OF[name], dt, bias=name in ("bias", "gelu"), scale=s2)
        _check(C, M, cols, want, TOL_ULP.get(name, 0), ("fp8", name, M, N, K), X.tail_floor(ops, EPI_OF[name], dt, name in ("bias", "gelu"), s2))
