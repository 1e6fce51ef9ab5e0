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
from gemm_exact_gpu import EPI_OF, TOL_ULP, GUARD, Problem, _cus, _padded, _sentinel, _check, _launch, _run      # (shared with test_gpu_vit_stats.py)

DTS = ["bf16", "f16"]
NAN = float("nan")


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
    s2 = X.pow2_scale(M)
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
