"""Operands for which the GEMM / GEMV reference is EXACT, the float64 reference itself, and the case lists of the exact tests.  CPU only.

The kernels accumulate in fp32.  With small integers in A and W every product and every partial sum is an integer below 2^24, so the fp32
accumulator holds the exact value in ANY summation order (every tile shape, stream-K slabs, split-K slices, v_dot2).  The epilogue operands
are dyadic (bias k / 128 or k / 1024 by type, layer scale k / 8, residual k / 4, row scale k / 8), so every remaining step of an epilogue is one IEEE
fp32 operation or one round-to-nearest-even to T, restated below in float64 with an explicit rounding wherever the device rounds.  The
expected BITS of EPI_NONE / EPI_RESID / EPI_LS_RESID / EPI_F32OUT / EPI_PARTIAL / out_f32 and of the row-scale form are then determined;
GELU and SwiGLU go through erf / exp and are compared in ulps of T (ulp_distance).

tests/test_gemm_exact_cpu.py proves the preconditions for every case list below; tests/test_gpu_gemm_exact.py,
tests/test_gpu_gemv_exact.py and tests/test_gpu_gemv_quant_exact.py (quantised weights, norm-in-GEMV: the last section) run the kernels."""
import functools
import math
import torch

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
EPI_NONE, EPI_GELU, EPI_LS_RESID, EPI_RESID, EPI_SWIGLU, EPI_PARTIAL, EPI_F32OUT = 0, 1, 2, 3, 4, 5, 6
A_MAX, W_MAX = 3, 2                      # |A| <= 3, |W| <= 2: K * 6 < 2^24 up to K = 2.7 M
# bias = k / BIAS_DEN, |k| <= BIAS_DEN.  The fraction is chosen per type so that T(acc + bias) really rounds: bf16 keeps 8 significant bits, so
# 1/128 steps are lost from |acc| >= 2 on; f16 keeps 11, and accumulators of a K = 64 problem (|acc| ~ 20) still hold 1/32 -- 1/1024 steps do not
# survive from |acc| >= 2 on (test_gemm_exact_cpu.py::test_final_rounding_is_exercised holds every case, the four-output ones included, to a
# quarter of its outputs)
BIAS_DEN = {"bf16": 128, "f16": 1024}
SENTINEL16 = 0x5A5A                      # bit pattern of untouched 16-bit output (finite in both types); fp32 outputs carry it twice
SENTINEL32 = 0x5A5A5A5A

# ---------------------------------------------------------------------------------------------------------------------------------------
# The tile menu of launch_epi (csrc/gemm.hip), restated: id -> (BM, BN, waves along M, waves along N).  Tiles 12 / 13 run tile 2 on the leading
# columns and tile 10 / 11 on the tail; where that split does not apply, and for every id under an epilogue it does not take, the 256^2 kernel runs.
# ---------------------------------------------------------------------------------------------------------------------------------------
TILES = {1: (128, 128, 2, 2), 2: (256, 256, 2, 4), 3: (256, 192, 2, 4), 4: (224, 256, 2, 4), 5: (192, 256, 2, 4), 6: (256, 256, 2, 4),
         7: (256, 192, 4, 3), 8: (256, 256, 4, 4), 9: (192, 256, 3, 4), 10: (192, 224, 4, 2), 11: (192, 224, 6, 2),
         12: (256, 256, 2, 4), 13: (256, 256, 2, 4)}
SWIGLU_FALLS_BACK = (3, 10, 11, 12, 13)  # wave tiles of 48 / 112 columns would split (gate, up) block pairs: the 256^2 kernel
K_AXIS = (64, 192, 1024)                 # one K step, an odd step count (the double buffer ends on either stage), a long loop
EXACT_EPIS = ("none", "bias", "resid", "ls_resid")      # asserted with torch.equal; "gelu" <= 1 ulp, "swiglu" <= 2 ulp


def tile_block(tile, swiglu=False):
    """(BM, BN) of the kernel that the dispatch runs for this tile id (SwiGLU falls back to 256^2 where the tile cannot hold the pairs)"""
    if swiglu and tile in SWIGLU_FALLS_BACK:
        return 256, 256
    return TILES[tile][:2]


def m_axis(bm):
    return (1, bm - 1, bm + 1, 2 * bm + 3)


def n_axis(bn):
    """4; either side of the tile edge; 8 mod 16 (a wide-store block pair ends inside a block) beyond one tile; 4 mod 8 (narrow-store fall-back)"""
    return (4, bn - 4, bn + 4, bn + 24, 20)


def gemm_cases(tile):
    """Sparse crossing of the M, N and K axes for one tile id: every value of each axis appears, not the full product.  A case is
    (M, N, K, strided, swiglu).  strided: lda, ldw > K and ldc, ldr > N with ldr != ldc, NaN in the padding and the guard rows of A, W and the
    residual, a sentinel in C's padding and guard rows (StridedProblem in the GPU test).  The wide-store shape runs dense AND strided."""
    bm, bn = tile_block(tile)
    ms, ns = m_axis(bm), n_axis(bn)
    out = []
    for i, n in enumerate(ns):
        m = ms[(i + tile) % len(ms)]
        k = K_AXIS[(i + tile) % len(K_AXIS)]
        out.append((m, n, k, i % 2 == 1, False))
        if n % 8 == 0:
            out.append((m, n, k, i % 2 == 0, False))
    bm, bn = tile_block(tile, swiglu=True)
    ms = m_axis(bm)
    for i, n in enumerate((bn - 32, bn + 32)):      # N % 32 == 0 on both sides of the tile edge
        out.append((ms[(i + 1 + tile) % len(ms)], n, K_AXIS[(i + 1 + tile) % len(K_AXIS)], i == 1, True))
    return out


TILE3_SWIGLU_SHAPE = (257, 224, 192)     # force_tile = 3 under SwiGLU: two row tiles, N below one tile, an odd K step count


def row_scale_shape(tile):
    """one row beyond the tile, a wide-store width beyond it, an odd K step count"""
    bm, bn = tile_block(tile)
    return bm + 1, bn + 24, 192


ROW_SCALE_TILES = (1, 2, 7, 8, 9, 10)


def f32out_cases():
    """EPI_F32OUT ignores force_tile: the 128^2 kernel below 64 tiles of 256^2, the staggered 256^2 kernel from there on (launch_gemm)"""
    return [(129, 132, 192, True), (257, 24, 64, False), (2049, 1800, 64, True)]      # (M, N, K, strided); the last: 9 x 8 = 72 tiles


def f32out_tile(M, N):
    return 1 if -(-M // 256) * -(-N // 256) < 64 else 2


FP8_K_AXIS = (128, 384)


def fp8_cases():
    """the fp8 x fp8 kernel is the 256^2 staggered kernel on 128-deep K steps: (M, N, K, swiglu)"""
    ms, ns = m_axis(256), n_axis(256)
    out = [(ms[i % 4], n, FP8_K_AXIS[i % 2], False) for i, n in enumerate(ns)]
    return out + [(257, 224, 128, True), (255, 288, 384, True)]


# launch structures behind the 256^2 kernel, for a device of n_cu compute units ----------------------------------------------------------
def persistent_shape(n_cu):
    """more 256^2 tiles than compute units (tuning key 13: one workgroup per CU walks several tiles), ragged on both axes, one K step"""
    ct = n_cu // 17 + 1
    return 16 * 256 + 4, (ct - 1) * 256 + 4, 64      # 17 row tiles x ct column tiles > n_cu


def stream_k_rule(M, N, K, n_cu):
    """launch_cfg8's use_sk for stream_k = 1 with the full workspace: returns the tiles of the stream-K round (0: data-parallel only)"""
    G = min(n_cu, 256)
    tiles = -(-M // 256) * -(-N // 256)
    R, KT = tiles % G, K // 64
    return R if R > 0 and R * 10 < G * 9 and R * KT >= 4 * G and KT >= 8 else 0


def stream_k_shape(n_cu):
    """16 tiles, ragged, whose K loop is cut into >= 4 K-tiles for each of the G workgroups: every tile is summed from several slabs"""
    G = min(n_cu, 256)
    return 1021, 1020, 64 * max(8, -(-4 * G // 16))


def split_rule(M, N, n_cu):
    """launch_epi's two-launch split of tiles 12 / 13: (n_main, n_tail), or None when the whole problem goes to the 256^2 kernel"""
    rt, ct = -(-M // 256), -(-N // 256)
    full = rt * ct // n_cu
    ct_main = min(ct, full * n_cu // rt) if full >= 1 else 0
    n_main = ct_main * 256
    n_tail = N - n_main
    if n_main > 0 and n_tail > 0 and -(-M // 192) * -(-n_tail // 224) <= n_cu:
        return n_main, n_tail
    return None


def split_shape(n_cu):
    """16 row tiles (ragged) x enough column tiles for one whole round of 256^2 tiles, and a 220-column tail for the 192 x 224 kernel"""
    ct_main = n_cu // 16
    return 16 * 256 - 3, ct_main * 256 + 220, 64


# ---------------------------------------------------------------------------------------------------------------------------------------
# rounding, in float64 containers
# ---------------------------------------------------------------------------------------------------------------------------------------
def f32(x):
    """one IEEE fp32 operation: its exact (float64) result rounded to fp32.  (The sums and products formed here are exact in float64: make_operands bounds their exponent spread.)"""
    return x.to(torch.float32).to(torch.float64)


def rT(x, dt):
    """round-to-nearest-even to T of an fp32 value"""
    return x.to(torch.float32).to(DT[dt]).to(torch.float64)


def representable(x, dt):
    return rT(x, dt) == x


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float64)


randint = _randint


def pow2_scale(M):
    """per-row factors 4, 2, 1, 1/2 -- rsqrt of the powers of four 1/16 .. 4; adjacent rows differ by a factor of at least 2"""
    return 2.0 ** (1 - ((torch.arange(M) * 3 + 1) % 4).to(torch.float64))


def make_operands(seed, M, N, K, dt, a_max=A_MAX, w_max=W_MAX):
    """A [M, K], W [N, K], bias [N], ls [N], resid [M, N], row_scale [M] as float64 tensors of integers and dyadics, with the exactness
    preconditions asserted (see the module docstring).  row_scale differs from row to row; ls is never 0."""
    g = torch.Generator().manual_seed(seed)
    A = _randint(g, -a_max, a_max, (M, K))
    W = _randint(g, -w_max, w_max, (N, K))
    den = BIAS_DEN[dt]
    bias = _randint(g, -den, den, (N,)) / den
    ls = _randint(g, 1, 12, (N,)) / 8 * (1 - 2 * _randint(g, 0, 1, (N,)))
    resid = _randint(g, -64, 64, (M, N)) / 4
    row_scale = (1 + (torch.arange(M) * 5 + seed) % 16).to(torch.float64) / 8
    ops = dict(A=A, W=W, bias=bias, ls=ls, resid=resid, row_scale=row_scale)
    for name in ("A", "W", "bias", "ls", "resid"):
        assert bool(representable(ops[name], dt).all()), (name, "does not survive a round trip through", dt)
    assert bool((f32(row_scale) == row_scale).all())
    assert K * a_max * w_max < 2 ** 24, "partial sums must stay below 2^24"
    acc = A @ W.t()
    assert float(acc.abs().max()) <= K * a_max * w_max
    for s in (None, row_scale):
        v = acc if s is None else acc * s[:, None]
        assert bool((f32(v) == v).all()), "acc * row_scale must be exact in fp32"
        assert bool((f32(v + bias) == v + bias).all()), "acc + bias must be exact in fp32"
    ops["acc"] = acc
    return ops


@functools.lru_cache(maxsize=2)
def cached_operands(seed, M, N, K, dt, a_max=A_MAX, w_max=W_MAX):
    """the same operands for every epilogue / layout of a shape: computed once, read only"""
    return make_operands(seed, M, N, K, dt, a_max, w_max)


def gelu64(x):
    """x Phi(x) through erfc: 1 + erf(z) cancels in the negative tail (at x = -8 float64 keeps two digits of it), erfc(-z) does not"""
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


FLT_MIN = 2.0 ** -126


def tail_floor(ops, epi, dt, bias=True, scale=None):
    """Absolute floor under the ulp bounds of GELU / SwiGLU, per element; None for every other epilogue.

    The 1 / 2 ulp bounds rest on the device erf / exp being fp32-accurate.  fp32 carries that relative accuracy down to FLT_MIN = 2^-126 only: the
    GPU's exp and reciprocal units return zero where the exact result is an fp32 subnormal, and exp(-g) overflows above 88.7.  bf16 has fp32's
    exponent range, so it resolves values far below that (its subnormals reach 2^-133), and integer gates g in about [-97, -88] or GELU arguments
    in about [-13.5, -13.1] have exact results of 1e-37 .. 1e-40 that the device returns as a signed zero.  Where Phi(x) or sigmoid(g) is below
    FLT_MIN the fp32 evaluation may be off by that much, i.e. the output by FLT_MIN |x| (GELU) or FLT_MIN |g u| (SwiGLU): the floor.  It is
    ~1e-35 at most, 30 orders below any value an indexing or rounding-point error would move, and below half an f16 subnormal, so f16 never uses it."""
    v = ops["acc"]
    if scale is not None:
        v = f32(v * (scale if scale.dim() == 2 else scale[:, None]))
    if epi == EPI_GELU:
        return FLT_MIN * rT(f32(v + ops["bias"]) if bias else v, dt).abs()
    if epi == EPI_SWIGLU:
        M, N = v.shape
        blocks = v.reshape(M, N // 32, 2, 16)
        return (1.0 + 2.0 ** -7) * FLT_MIN * (rT(blocks[:, :, 0], dt) * rT(blocks[:, :, 1], dt)).abs().reshape(M, N // 2)
    return None


def reference(ops, epi, dt, bias=True, scale=None):
    """The rounding points of gemm_epilogue (csrc/gemm.hip), restated.  scale: [M] fp32 factor on the accumulators (row scale; for the fp8 x fp8
    kernel pass scale2d = a_scale[m] * w_scale[n] through `scale` as an [M, N] tensor).  Returns float64 values that T (fp32 for EPI_F32OUT /
    EPI_PARTIAL sums) holds exactly.
      EPI_NONE      T(s * acc + bias)
      EPI_RESID     T(resid + T(s * acc + bias))
      EPI_LS_RESID  T(resid + T(fp32(T(s * acc + bias) * ls)))
      EPI_F32OUT    acc
      EPI_GELU      T(gelu_erf(T(s * acc + bias)))
      EPI_SWIGLU    T(T(silu(T(g))) * T(u)), (g, u) = the 16 | 16 interleaved column blocks of s * acc"""
    v = ops["acc"]
    if scale is not None:
        v = f32(v * (scale if scale.dim() == 2 else scale[:, None]))
    if epi == EPI_F32OUT:
        return v
    if epi == EPI_SWIGLU:
        M, N = v.shape
        blocks = v.reshape(M, N // 32, 2, 16)
        g, u = rT(blocks[:, :, 0], dt), rT(blocks[:, :, 1], dt)
        s = rT(g * torch.sigmoid(g), dt)
        return rT(f32(s * u), dt).reshape(M, N // 2)
    if bias:
        v = f32(v + ops["bias"])
    y = rT(v, dt)
    if epi == EPI_NONE:
        return y
    if epi == EPI_GELU:
        return rT(gelu64(y), dt)
    if epi == EPI_RESID:
        return rT(f32(ops["resid"] + y), dt)
    if epi == EPI_LS_RESID:
        return rT(f32(ops["resid"] + rT(f32(y * ops["ls"]), dt)), dt)
    raise ValueError(epi)


def reference_fp32(ops, epi, dt, bias=True, scale=None):
    """the same epilogues as a plain fp32 torch evaluation (what test_gpu_ops._gemm_ref does), for the exact epilogues: the float64 reference
    must equal it bit for bit (test_gemm_exact_cpu.py)"""
    T = DT[dt]
    v = ops["A"].float() @ ops["W"].float().t()
    if scale is not None:
        v = v * scale.float()[:, None]
    if epi == EPI_F32OUT:
        return v
    if bias:
        v = v + ops["bias"].float()
    y = v.to(T).float()
    if epi == EPI_RESID:
        y = (ops["resid"].float() + y).to(T).float()
    elif epi == EPI_LS_RESID:
        y = (ops["resid"].float() + (y * ops["ls"].float()).to(T).float()).to(T).float()
    return y


def unrepresentable_share(x, dt):
    """share of the values of x (float64) that T does not hold: the outputs whose final rounding is a real rounding"""
    return float((~representable(x, dt)).double().mean())


def ulp_distance(a, b):
    """distance in units of T between two tensors of the same 16-bit float type: the bit patterns mapped to a monotone integer line
    (+0 and -0 coincide); NaN is infinitely far from everything"""
    assert a.dtype == b.dtype and a.dtype in (torch.bfloat16, torch.float16)

    def line(t):
        i = t.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
        return torch.where(i >= 0x8000, -(i - 0x8000), i)
    d = (line(a) - line(b)).abs()
    return torch.where(torch.isnan(a.float()) | torch.isnan(b.float()), torch.full_like(d, 1 << 40), d)


def first_mismatch(got, want, tol_ulp=0, floor=None):
    """None, or a text naming the first offending element (row, column, got, want) of two [rows, columns] tensors of one type.
    floor: per-element absolute error that passes whatever its ulp distance (tail_floor; GELU / SwiGLU only)"""
    if got.dtype in (torch.bfloat16, torch.float16):
        bad = ulp_distance(got, want) > tol_ulp
        if floor is not None:
            bad &= ~((got.double() - want.double()).abs() <= floor)
    else:
        bad = ~((got == want) & ~torch.isnan(got))
    if not bool(bad.any()):
        return None
    r, c = (int(v) for v in bad.nonzero()[0])
    return f"{int(bad.sum())} of {bad.numel()} elements differ; first at (row {r}, column {c}): got {float(got[r, c])!r}, want {float(want[r, c])!r}"


# e4m3 (OCP fn) bytes of the integers -4 .. 4, built on the host: 1 = 0x38 (exponent 7, mantissa 0), 2 = 0x40, 3 = 0x44, 4 = 0x48
_E4M3 = {0: 0x00, 1: 0x38, 2: 0x40, 3: 0x44, 4: 0x48}


def e4m3_bytes(x):
    """float64 tensor of integers in [-4, 4] -> uint8 tensor of their e4m3 codes"""
    lut = torch.tensor([(_E4M3[abs(v)] | (0x80 if v < 0 else 0)) for v in range(-4, 5)], dtype=torch.uint8)
    assert float(x.abs().max()) <= 4 and bool((x == x.round()).all())
    return lut[(x + 4).to(torch.int64)]


def fp8_scales(M, N, seed):
    """dyadic per-row scales of the fp8 x fp8 GEMM: a_scale[m] a power of two in 2^-3 .. 2^0, w_scale[n] = k / 8, k in 1 .. 8; their product
    and its product with an accumulator below 2^13 are exact in fp32"""
    a = 2.0 ** (-((torch.arange(M) * 3 + seed) % 4).to(torch.float64))
    w = (1 + (torch.arange(N) * 5 + seed) % 8).to(torch.float64) / 8
    return a, w


# ---------------------------------------------------------------------------------------------------------------------------------------
# skinny GEMV: one case per kernel family that the product build reaches without a norm.  (family, b, N, K, epi, ksplit, flags) with the flag
# bits of omchat_op_gemv_plan (1 x_packed, 2 w_packed, 4 y_packed, 16 out_f32, 32 force_mfma, 64 resid given); found with the plan hook on
# the CPU, pinned again by the GPU test before each launch.  The shapes are the smallest the family accepts with a ragged last N tile where
# the family allows one, and b at 1 / 16 / 17 / 32 where the family takes them.
# ---------------------------------------------------------------------------------------------------------------------------------------
GF_MFMA, GF_PK, GF_XS, GF_XS_SPLIT, GF_ROWS, GF_ROWS_LONGK = 0, 1, 2, 3, 4, 7
PLAN_X_PACKED, PLAN_W_PACKED, PLAN_Y_PACKED, PLAN_OUT_F32, PLAN_RESID = 1, 2, 4, 16, 64
# (b, N, K, x_packed, w_packed, force_mfma, ((form, ksplit, family), ...)); forms: "bias" EPI_NONE with bias, "f32" out_f32, "resid" EPI_RESID,
# "partial" EPI_PARTIAL in ksplit fp32 slices, "swiglu", "swiglu_yp" (the SwiGLU output in the packed x layout of the consumer)
GEMV_CASES = [
    # whole-row streaming form, b = 1: one row per wave, 102 rows = 25 workgroups of 4 and one of 2
    (1, 102, 64, 0, 0, 0, (("bias", 0, GF_ROWS), ("f32", 0, GF_ROWS), ("resid", 0, GF_ROWS))),
    (1, 160, 192, 0, 0, 0, (("swiglu", 0, GF_ROWS),)),
    (1, 102, 1024, 0, 0, 0, (("partial", 0, GF_ROWS),)),                      # four rows per wave: 102 = 6 x 16 + 6 (this entry has no ksplit: one slice)
    # K > 4096 with a residual: x through LDS, 3 rows per workgroup, 1030 = 343 x 3 + 1
    (1, 1030, 4160, 0, 0, 0, (("resid", 0, GF_ROWS_LONGK),)),
    # MFMA form on row-major operands: 16-column tiles (two per workgroup for b > 16 / SwiGLU), 100 = 6 x 16 + 4
    (1, 100, 64, 0, 0, 1, (("bias", 0, GF_MFMA), ("f32", 0, GF_MFMA), ("resid", 0, GF_MFMA))),
    (16, 100, 192, 0, 0, 0, (("bias", 0, GF_MFMA), ("f32", 0, GF_MFMA), ("resid", 0, GF_MFMA), ("partial", 0, GF_MFMA))),
    (17, 100, 192, 0, 0, 0, (("bias", 0, GF_MFMA), ("f32", 0, GF_MFMA), ("resid", 0, GF_MFMA), ("partial", 0, GF_MFMA))),
    (32, 100, 64, 0, 0, 0, (("bias", 0, GF_MFMA), ("resid", 0, GF_MFMA))),
    (16, 160, 192, 0, 0, 0, (("swiglu", 0, GF_MFMA),)),
    (17, 160, 64, 0, 0, 0, (("swiglu", 0, GF_MFMA),)),
    # packed x, row-major or packed W: two 16-column tiles per workgroup, 48 = 32 + 16
    (16, 48, 192, 1, 0, 0, (("bias", 0, GF_PK), ("f32", 0, GF_PK), ("partial", 2, GF_PK))),
    (17, 48, 192, 1, 1, 0, (("bias", 0, GF_PK), ("f32", 0, GF_PK), ("partial", 3, GF_PK))),
    (1, 48, 1024, 1, 0, 0, (("bias", 0, GF_PK), ("partial", 2, GF_PK))),
    (32, 384, 64, 1, 1, 0, (("swiglu", 0, GF_PK), ("swiglu_yp", 0, GF_PK))),
    (1, 384, 64, 1, 0, 0, (("swiglu", 0, GF_PK), ("swiglu_yp", 0, GF_PK))),
    # x-stationary persistent form: packed W, K = 3584 in one piece, fewer tiles than compute units
    (1, 64, 3584, 1, 1, 0, (("bias", 0, GF_XS), ("f32", 0, GF_XS))),
    (17, 64, 3584, 1, 1, 0, (("bias", 0, GF_XS), ("f32", 0, GF_XS))),
    (16, 128, 3584, 1, 1, 0, (("swiglu", 0, GF_XS), ("swiglu_yp", 0, GF_XS))),
    (32, 128, 3584, 1, 1, 0, (("swiglu", 0, GF_XS), ("swiglu_yp", 0, GF_XS))),
    # ... and its split-K form: 56 chunks of K as slices of 40 and 16, two tiles per workgroup (130 tiles x 2 slices on 256 CUs)
    (17, 2080, 3584, 1, 1, 0, (("partial", 2, GF_XS_SPLIT),)),
    (32, 2080, 3584, 1, 1, 0, (("partial", 2, GF_XS_SPLIT),)),
]
GEMV_FAMILIES = (GF_MFMA, GF_PK, GF_XS, GF_XS_SPLIT, GF_ROWS, GF_ROWS_LONGK)


def gemv_plan_args(b, N, K, x_packed, w_packed, form, ksplit):
    """(epi, ksplit, flags) of omchat_op_gemv_plan for one form of a case"""
    epi = {"bias": EPI_NONE, "f32": EPI_NONE, "resid": EPI_RESID, "partial": EPI_PARTIAL, "swiglu": EPI_SWIGLU, "swiglu_yp": EPI_SWIGLU}[form]
    flags = (PLAN_X_PACKED if x_packed else 0) | (PLAN_W_PACKED if w_packed else 0) | (PLAN_Y_PACKED if form == "swiglu_yp" else 0)
    flags |= (PLAN_OUT_F32 if form == "f32" else 0) | (PLAN_RESID if form == "resid" else 0)
    return epi, ksplit, flags


def gemv_reference(ops, form, dt):
    """Y of the skinny GEMV, the rounding points of gemv.hip's epilogues restated (A = X [b, K]): T(acc + bias); acc; T(resid + T(acc));
    sum of the fp32 slices = acc; SwiGLU as the GEMM's"""
    if form == "bias":
        return reference(ops, EPI_NONE, dt, bias=True)
    if form in ("f32", "partial"):
        return ops["acc"]
    if form == "resid":
        return reference(ops, EPI_RESID, dt, bias=False)
    return reference(ops, EPI_SWIGLU, dt)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Quantised weights (e4m3 rows + fp32 row scales, MXFP4) and the norm-in-GEMV launches: operands for which these are exact too.
#
# e4m3: integer weights in [-4, 4] and w_scale[n] = k / 8, never the same on adjacent rows; the kernels compute fp32(sum * scale) per K slice,
# then + bias, T(), resid +  (gemv_rows_body / rw_rows_q in csrc/gemv.hip) -- reference(ops, epi, dt, scale = w_scale[None, :]).
# MXFP4: codes over all 16 e2m1 values and e8m0 bytes built directly; the kernels widen the codes at scale 1 and multiply the fp32 partial of a
# block by 2^e, so every intermediate is a multiple of one granule per row and the accumulation is exact while sum |x w| / granule < 2^24
# (asserted per case, whatever the order).  The wide variant gives all blocks of row n the exponent -24 + n % 33: exact within a row, 2^-24 ..
# 2^8 across rows -- a scale folded into an f16 convert underflows and changes bits.  Its outputs are fp32; the long-K family has no fp32 output,
# so its wide case writes T(acc) (EPI_RESID on a zero residual) with exponents -24 .. +2 and |x| <= 31: every T(acc) is finite in f16 and
# at least a quarter of them are real roundings in both types (test_gemm_exact_cpu.py asserts both).  The SwiGLU cases take block exponents
# lower by 4, so that silu(gate) * up stays inside f16's range and the 2 ulp bound is a bound on nearly every output.
# RMSNorm: x is made of groups of eight magnitudes {4, 3, 2, 1, 1, 1, 0, 0}, permuted, with random signs: the sum of squares is the integer
# 4 K, tot / K == 4.0 exactly, rsqrtf(4 + 1e-6) is 0.5 to a few ulps, every x * inv lies within ~2^-21 of x / 2 in {0, .5, 1, 1.5, 2} -- far
# from a rounding boundary of T -- so T(x * inv) == x / 2 whatever the last bits of the device's rsqrtf are, and with norm weights from
# {.5, 1, 1.5, 2} xn = T(nw * T(x * inv)) == nw * x / 2 exactly: multiples of 1 / 4 up to 4.  The dot products are then exact as above.
# ---------------------------------------------------------------------------------------------------------------------------------------
WF_16, WF_E4M3, WF_MX4 = 0, 1, 2
GF_ROWS_NORM, GF_ROWS_NORM_LOOP = 5, 6
PLAN_NORM = 8
NORM_EPS = 1e-6
NORM_GROUP = (4.0, 3.0, 2.0, 1.0, 1.0, 1.0, 0.0, 0.0)
NORM_W = (0.5, 1.0, 1.5, 2.0)
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def norm_x(g, K):
    """the exact-RMSNorm row [1, K]: K / 8 permuted, signed copies of NORM_GROUP"""
    assert K % 8 == 0
    grp = torch.tensor(NORM_GROUP, dtype=torch.float64).repeat(K // 8, 1)
    perm = torch.rand((K // 8, 8), generator=g).argsort(dim=1)
    sign = 1 - 2 * _randint(g, 0, 1, (K // 8, 8))
    return (grp.gather(1, perm) * sign).reshape(1, K)


def norm_weights(g, K):
    return torch.tensor(NORM_W, dtype=torch.float64)[torch.randint(0, 4, (K,), generator=g)]


def norm_inv(x, eps=NORM_EPS):
    """fp32 rsqrt(tot / K + eps) as torch evaluates it: the centre of the +-8 ulp band the CPU test walks"""
    tot = (x.float() * x.float()).sum()
    return torch.rsqrt(tot / float(x.numel()) + torch.tensor(eps, dtype=torch.float32))


def norm_xn(x, nw, inv, dt):
    """T(nw * T(x * inv)) with fp32 products, the kernel's rounding points (gemv_rows_norm_body); inv an fp32 scalar tensor"""
    T = DT[dt]
    return (nw.float() * (x.float() * inv).to(T).float()).to(T).double()


WIDE = 33                                # exponents of the wide variant: -24 .. +8
WIDE_F16_OUT = 27                        # ... where T(acc) is the output: -24 .. +2, so that |acc| stays inside f16 (QUANT_CASES, the long-K entry)
SWIGLU_E_SHIFT = -4                      # block exponents of the MXFP4 SwiGLU cases: -6 .. -2, so that silu(gate) * up stays inside f16


def mx_exponents(N, K, seed, wide=0, shift=0):
    """block exponents [N, K / 32]: ((3 n + 2 blk + seed) % 5) - 2 + shift.  The block step 2 and the row step 3 are both coprime to 5, so
    adjacent blocks of a row and adjacent rows of a block never share an exponent.  wide > 0: -24 + n % wide in every block of row n"""
    n, blk = torch.arange(N)[:, None], torch.arange(K // 32)[None, :]
    if wide:
        return (-24 + n % wide).expand(N, K // 32).contiguous()
    return (3 * n + 2 * blk + seed) % 5 - 2 + shift


def mx_dequant(codes, e):
    """float64 [N, K] of e2m1 codes [N, K] (sign in bit 3) and block exponents [N, K / 32]"""
    c = codes.to(torch.int64)
    v = torch.where(c >= 8, -E2M1[c & 7], E2M1[c & 7])
    return v * torch.ldexp(torch.ones(e.shape, dtype=torch.float64), e).repeat_interleave(32, dim=1)


def e4m3_row_scales(N, seed):
    """k / 8, k in 1 .. 8, as fp8_scales: the step of 5 keeps adjacent rows apart"""
    return (1 + (torch.arange(N) * 5 + seed) % 8).to(torch.float64) / 8


def quant_finish(ops, dt, need_bias=True):
    """acc, the per-output scale and granule of a quantised / norm operand set, from its x (xn), weights and scales; asserts the exactness bounds"""
    wf, xn = ops["wf"], ops["xn"]
    gx = 0.25 if ops["norm"] else 1.0
    if wf == WF_MX4:
        ops["W"] = mx_dequant(ops["codes"], ops["e"])
        gw = 0.5 * torch.ldexp(torch.ones(len(ops["e"]), dtype=torch.float64), ops["e"].min(dim=1).values)
    else:
        gw = torch.ones(len(ops["W"]), dtype=torch.float64)
    acc = xn @ ops["W"].t()
    bound = (xn.abs() @ ops["W"].abs().t()) / (gx * gw)[None, :]      # every partial sum in any order, in granules
    assert float(bound.max()) < 2 ** 24, ("partial sums must stay below 2^24 granules", float(bound.max()))
    assert bool((acc / (gx * gw) == (acc / (gx * gw)).round()).all())
    scale = ops.get("w_scale")
    s2 = None if scale is None else scale[None, :]
    v = acc if s2 is None else acc * s2
    assert bool((f32(v) == v).all()), "acc * scale must be exact in fp32"
    if need_bias:
        assert bool((f32(v + ops["bias"]) == v + ops["bias"]).all()), "acc * scale + bias must be exact in fp32"
    ops["acc"], ops["scale"] = acc, s2
    ops["granule"] = gx * gw * (0.125 if wf == WF_E4M3 else 1.0)      # of an output and of every EPI_PARTIAL slice (e4m3: each slice is scaled)
    return ops


def make_quant_operands(seed, wf, b, N, K, dt, norm=False, x_max=A_MAX, wide=0, e_shift=0):
    """x [b, K] (norm: the exact-RMSNorm row and its norm weights), the weights of form wf with their scales, bias / resid as make_operands
    defines them (wide: a zero residual), and acc = xn W^T (e4m3: before the row scale).  wide / e_shift: mx_exponents.  Every operand
    survives its storage type; the bounds are asserted."""
    g = torch.Generator().manual_seed(seed)
    ops = dict(wf=wf, norm=norm, wide=wide)
    if norm:
        assert b == 1
        x, nw = norm_x(g, K), norm_weights(g, K)
        xn = nw[None, :] * x / 2
        assert torch.equal(norm_xn(x, nw, norm_inv(x), dt), xn) and float(xn.abs().max()) <= 4 and torch.equal(xn * 4, (xn * 4).round())
        ops.update(A=x, nw=nw, xn=xn)
    else:
        x = _randint(g, -x_max, x_max, (b, K))
        ops.update(A=x, xn=x)
    if wf == WF_MX4:
        assert K % 32 == 0
        ops["codes"] = torch.randint(0, 16, (N, K), generator=g).to(torch.uint8)
        ops["e"] = mx_exponents(N, K, seed, wide, e_shift)      # (W, the de-quantised weights: quant_finish)
    elif wf == WF_E4M3:
        ops["W"] = _randint(g, -4, 4, (N, K))
        ops["w_scale"] = e4m3_row_scales(N, seed)
        assert bool((ops["w_scale"][1:] != ops["w_scale"][:-1]).all())
    else:
        ops["W"] = _randint(g, -W_MAX, W_MAX, (N, K))
        assert bool(representable(ops["W"], dt).all())
    den = BIAS_DEN[dt]
    ops["bias"] = _randint(g, -den, den, (N,)) / den
    ops["resid"] = (torch.zeros((b, N), dtype=torch.float64) if wide else _randint(g, -64, 64, (b, N)) / 4)
    for name in ("A", "xn", "bias", "resid") + (("nw",) if norm else ()):
        assert bool(representable(ops[name], dt).all()), (name, "does not survive a round trip through", dt)
    return quant_finish(ops, dt, need_bias=not wide)


@functools.lru_cache(maxsize=2)
def cached_quant_operands(seed, wf, b, N, K, dt, norm=False, x_max=A_MAX, wide=0, e_shift=0):
    return make_quant_operands(seed, wf, b, N, K, dt, norm, x_max, wide, e_shift)


def quant_reference(ops, form, dt):
    """as gemv_reference, with the e4m3 row scale on the accumulators; "f32" / "partial": fp32(acc * scale) (the sum of the scaled slices)"""
    s = ops["scale"]
    if form == "bias":
        return reference(ops, EPI_NONE, dt, bias=True, scale=s)
    if form in ("f32", "partial"):
        return reference(ops, EPI_F32OUT, dt, scale=s)
    if form == "resid":
        return reference(ops, EPI_RESID, dt, bias=False, scale=s)
    return reference(ops, EPI_SWIGLU, dt, scale=s)


def quant_tail_floor(ops, dt):
    return tail_floor(ops, EPI_SWIGLU, dt, scale=ops["scale"])


# the corruptions that the reference must tell apart (test_gemm_exact_cpu.py): each returns operands a subtly wrong kernel would have computed on
def corrupt(ops, kind, dt):
    """None where the corruption does not apply to this operand set.  nibbles: the two codes of every byte swapped; last_scale: the last
    block's e8m0 byte replaced by its neighbour's; next_row_scale: row n under row n + 1's scale(s); drop32: the last 32 k dropped;
    swap_gate_up: gate and up exchanged in the last 32-row block"""
    o = dict(ops)
    wf = ops["wf"]
    if kind == "nibbles":
        if wf != WF_MX4:
            return None
        c = ops["codes"]
        o["codes"] = torch.stack((c[:, 1::2], c[:, 0::2]), dim=2).reshape(c.shape)
    elif kind == "last_scale":
        if wf != WF_MX4 or ops["wide"]:
            return None
        o["e"] = ops["e"].clone()
        o["e"][:, -1] = ops["e"][:, -2]
    elif kind == "next_row_scale":
        if wf == WF_MX4:
            o["e"] = torch.roll(ops["e"], -1, 0)
        elif wf == WF_E4M3:
            o["w_scale"] = torch.roll(ops["w_scale"], -1, 0)
        else:
            return None
    elif kind == "drop32":
        if wf == WF_MX4:
            o["codes"] = ops["codes"].clone()
            o["codes"][:, -32:] = 0
        else:
            o["W"] = ops["W"].clone()
            o["W"][:, -32:] = 0
    elif kind == "swap_gate_up":
        N = ops["W"].shape[0]
        idx = torch.arange(N)
        idx[N - 32:] = torch.cat((torch.arange(N - 16, N), torch.arange(N - 32, N - 16)))
        for name in ("W", "codes", "e", "w_scale"):
            if name in ops:
                o[name] = ops[name][idx]
    else:
        raise ValueError(kind)
    return quant_finish(o, dt, need_bias=False)


def bias_before_scale(ops, dt):
    """EPI_NONE on e4m3 with the bias added BEFORE the row scale: T(fp32(fp32(acc + bias) * scale))"""
    return rT(f32(f32(ops["acc"] + ops["bias"]) * ops["scale"]), dt)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Case list.  QCase: weight form, b, N (an int, or a function of the compute-unit count where the family depends on it), K, norm, max |x|,
# packed (through omchat_op_gemv_mxfp4_packed), wide (the number of row exponents from -24 up; 0: the narrow form), tuning ((key, value,
# restore), ...), pins ({index into the plan's ints: value}: 5 = waves per
# workgroup, 8 = rows per wave) and forms ((form, ksplit, family), ...) as in GEMV_CASES.  Ragged K: K % 64 == 0 and K % 512 != 0 for 16-bit and
# e4m3 rows, K % 32 == 0 and K % 64 != 0 for MXFP4 rows (the last 512-chunk ends inside a 64-k pair of blocks).
# ---------------------------------------------------------------------------------------------------------------------------------------
class QCase:
    def __init__(self, wf, b, N, K, forms, norm=False, x_max=A_MAX, packed=False, wide=0, tuning=(), pins=None, name=None):
        self.wf, self.b, self._N, self.K, self.forms, self.norm, self.x_max = wf, b, N, K, forms, norm, x_max
        self.packed, self.wide, self.tuning, self.pins = packed, wide, tuning, pins or {}
        self.cu_dependent = callable(N)
        self.e_shift = SWIGLU_E_SHIFT if wf == WF_MX4 and any(f[0].startswith("swiglu") for f in forms) else 0
        self.id = "wf{}-b{}-N{}-K{}{}{}{}{}".format(wf, b, name if callable(N) else N, K, "-norm" if norm else "", "-pk" if packed else "",
                                                    "-wide" if wide else "", "".join("-k{}v{}".format(k, v) for k, v, _ in tuning))

    def N(self, n_cu):
        return self._N(n_cu) if self.cu_dependent else self._N

    def operands(self, dt, n_cu, cached=True):
        f = cached_quant_operands if cached else make_quant_operands
        return f(5, self.wf, self.b, self.N(n_cu), self.K, dt, self.norm, self.x_max, self.wide, self.e_shift)

    def plan_args(self, form, ks):
        epi, ks_, flags = gemv_plan_args(self.b, 0, self.K, self.packed, self.packed, form, ks)
        return epi, ks_, flags | (PLAN_NORM if self.norm else 0)


def balanced7(n_cu):
    return 7 * 2 * n_cu


def balanced9(n_cu):
    return 9 * 2 * n_cu


def loop_rows(n_cu):
    """the smallest output count of at least 8 CUs that does not divide by 2 CUs"""
    return 8 * n_cu + 1


def loop_pairs2(n_cu):
    """N of the SwiGLU loop case: (gate, up) pairs come in blocks of 16, so the smallest such pair count is 8 CUs + 16 (for 2 CUs > 16)"""
    n = 8 * n_cu
    while n % (2 * n_cu) == 0:
        n += 16
    return 2 * n


def _ragged_k(wf, k16, k4):
    return k4 if wf == WF_MX4 else k16


def _quant_cases():
    R, L, NM, LP = GF_ROWS, GF_ROWS_LONGK, GF_ROWS_NORM, GF_ROWS_NORM_LOOP
    out = [QCase(WF_16, 1, balanced7, 64, (("resid", 0, R),), pins={5: 7}, name="14cu")]      # the seven-wave residual form (tuning key 17)
    for wf in (WF_E4M3, WF_MX4):
        out += [
            QCase(wf, 1, 102, _ragged_k(wf, 64, 96), (("bias", 0, R), ("f32", 0, R), ("resid", 0, R)), pins={8: 1}),
            QCase(wf, 1, 160, _ragged_k(wf, 192, 544), (("swiglu", 0, R),), pins={8: 4}),      # four pairs per wave
            QCase(wf, 1, 102, 1024, (("partial", 0, R),), pins={8: 4}),
            QCase(wf, 1, 70, 4096, (("partial", 3, R),), pins={8: 4}),                         # eight chunks cut 2 | 3 | 3
            QCase(wf, 1, 32790, _ragged_k(wf, 64, 96), (("bias", 0, R), ("f32", 0, R)), pins={8: 8}),      # eight rows per wave, ragged last group
            QCase(wf, 1, 1030, _ragged_k(wf, 4160, 4128), (("resid", 0, L),)),
            QCase(wf, 1, 9, 32768, (("resid", 0, L),), x_max=1),                               # the upper K bound, the largest LDS staging
        ]
    for wf in (WF_16, WF_E4M3, WF_MX4):
        kr = _ragged_k(wf, 576, 544)
        out += [
            QCase(wf, 1, 70, kr, (("bias", 0, NM), ("f32", 0, NM)), norm=True, pins={8: 2}),
            QCase(wf, 1, 96, kr, (("swiglu", 0, NM),), norm=True, pins={8: 1}),
            QCase(wf, 1, 70, 4096, (("bias", 0, NM),), norm=True, pins={8: 2}),
            QCase(wf, 1, balanced9, 2048, (("bias", 0, NM),), norm=True, pins={5: 9, 8: 1}, name="18cu"),
            QCase(wf, 1, 32790, _ragged_k(wf, 64, 96), (("bias", 0, NM),), norm=True, pins={8: 4}),      # lm_head's four rows per wave
        ]
        # every other rows-per-wave answer of the SwiGLU norm launch: tuning key 38 (16-bit: 2, 3; quantised, value x 16: 2, 4); 80 pairs
        for v, rr, back in (((2, 2, 1), (3, 3, 1)) if wf == WF_16 else ((32, 2, 16), (64, 4, 16))):
            out.append(QCase(wf, 1, 160, kr, (("swiglu", 0, NM),), norm=True, tuning=((38, v, back),), pins={8: rr}))
        # the loop form (tuning key 16, every bit)
        for k in (2048, _ragged_k(wf, 2112, 2080)):
            out += [
                QCase(wf, 1, loop_rows, k, (("bias", 0, LP),), norm=True, tuning=((16, 15, 0),), name="8cu+1"),
                QCase(wf, 1, loop_pairs2, k, (("swiglu", 0, LP),), norm=True, tuning=((16, 15, 0),), name="16cu+32"),
            ]
    # packed MXFP4 (batched steps): the packed rows of GEMV_CASES with wf = 2
    P, XS, SP = GF_PK, GF_XS, GF_XS_SPLIT
    M = WF_MX4
    out += [
        QCase(M, 16, 48, 192, (("bias", 0, P), ("f32", 0, P), ("partial", 2, P)), packed=True),
        QCase(M, 17, 48, 192, (("bias", 0, P), ("f32", 0, P), ("partial", 3, P)), packed=True),
        QCase(M, 1, 48, 1024, (("bias", 0, P), ("partial", 2, P)), packed=True),
        QCase(M, 32, 384, 64, (("swiglu", 0, P), ("swiglu_yp", 0, P)), packed=True),
        QCase(M, 1, 384, 64, (("swiglu", 0, P), ("swiglu_yp", 0, P)), packed=True),
        QCase(M, 1, 64, 3584, (("bias", 0, XS), ("f32", 0, XS)), packed=True),
        QCase(M, 17, 64, 3584, (("bias", 0, XS), ("f32", 0, XS)), packed=True),
        QCase(M, 16, 128, 3584, (("swiglu", 0, XS), ("swiglu_yp", 0, XS)), packed=True),
        QCase(M, 32, 128, 3584, (("swiglu", 0, XS), ("swiglu_yp", 0, XS)), packed=True),
        QCase(M, 17, 2080, 3584, (("partial", 2, SP),), packed=True),
        QCase(M, 32, 2080, 3584, (("partial", 2, SP),), packed=True),
    ]
    # the wide-exponent variant, one per MXFP4 family: fp32 output (the long-K form has none: EPI_RESID on a zero residual, T(acc))
    out += [
        QCase(M, 1, 102, 96, (("f32", 0, R),), wide=WIDE),
        QCase(M, 1, 1030, 4128, (("resid", 0, L),), x_max=31, wide=WIDE_F16_OUT),
        QCase(M, 1, 70, 544, (("f32", 0, NM),), norm=True, wide=WIDE),
        QCase(M, 1, loop_rows, 2048, (("f32", 0, LP),), norm=True, wide=WIDE, tuning=((16, 15, 0),), name="8cu+1"),
        QCase(M, 16, 48, 192, (("f32", 0, P),), packed=True, wide=WIDE),
        QCase(M, 17, 64, 3584, (("f32", 0, XS),), packed=True, wide=WIDE),
        QCase(M, 17, 2080, 3584, (("partial", 2, SP),), packed=True, wide=WIDE),
    ]
    return out


QUANT_CASES = _quant_cases()
PREPACKED_CASE = next(i for i, c in enumerate(QUANT_CASES) if c.packed and c.b == 16 and not c.wide)      # also run through the pack-once entries
# every (family, weight form) pair that the list must reach
QUANT_PAIRS = ({(GF_ROWS, WF_16)} | {(f, w) for f in (GF_ROWS, GF_ROWS_LONGK) for w in (WF_E4M3, WF_MX4)} |
               {(f, w) for f in (GF_ROWS_NORM, GF_ROWS_NORM_LOOP) for w in (WF_16, WF_E4M3, WF_MX4)} |
               {(f, WF_MX4) for f in (GF_PK, GF_XS, GF_XS_SPLIT)})
