"""The statistics chain of the fused ViT layer (csrc/model.hip vit_layer_fused), restated on the CPU, with operands for which every link's expected
BITS are determined, the mutants the restatement must tell apart, and the case tables of tests/test_gpu_vit_stats.py.  CPU only.

    row_sumsq -> qkv GEMM (row scale from x's slots; EPI_NONE_STATS leaves the q / k slots) -> vit_knorm_slots (K from its slots, leaves the q sums)
              -> attention (Q normed + scaled on load) -> proj GEMM (EPI_LS_RESID_STATS leaves x's slots) -> fc1 GEMM (row scale) -> fc2 GEMM (..._STATS)

Everything is indexed by (slot, row): statistics are SLOT-MAJOR fp32, element (slot s, row m) at [s * ld + m].

Scaled exact-norm rows.  Row r is 2^e_r times a permuted, signed copy of gemm_exact_ref.NORM_GROUP per eight channels: its sum of squares is the
integer 4 C 4^e_r (exact in fp32 in any order: every square is a multiple of 4^e_r and the total is 4 C < 2^24 of them), T(x * rstd) is
group / 2 in {0, .5, 1, 1.5, 2} whatever the last bits of rsqrtf are (test_vit_stats_cpu.py walks +-8 ulp), and the normalised row does not depend
on e_r -- so a statistic taken from ANY other row is wrong by a factor of at least 2 and changes every non-zero output.  row_exponents gives
adjacent rows different exponents, the first row of every batch element and the last row a value no neighbour has, the two batch elements
different values in the same row, and the q rows a value different from the k rows.

Hand-made slots.  A consumer's slots are INPUTS: they need not be the true sums of the data.  split_slots cuts a row's total into nslots
unequal integer shares of total / 1024, different per row and per slot: the shares sum exactly in fp32 in any order (reduction tree, two
half-sums, a shuffle tree), so the total the consumer must arrive at is known to the bit.  With total = 4 * C_total * 4^e the rsqrt is the one
of the scaled rows above even when C_total != C.  Everything behind the last slot and behind the last row is NaN.

GEMM operands for the statistics epilogues (stats_operands): integer outputs |c| <= 63, so every stored value's square is an integer and a
wave tile's total stays below 2^24: the fp32 slot value is exact in any order."""
import functools
import torch

import gemm_exact_ref as X

DT = X.DT
NAN = float("nan")
EPI_LS_RESID_STATS, EPI_NONE_STATS = 7, 8
Q_SCALE = 128 ** -0.5
EPS = 1e-6

# ---------------------------------------------------------------------------------------------------------------------------------------
# scaled exact-norm rows
# ---------------------------------------------------------------------------------------------------------------------------------------
E_CYCLE = (-4, 1, -2, 3, 0)      # five values of [-4, 5]; consecutive entries (cyclically) differ
E_FIRST = (5, 4)                 # first row of batch element b (b % 2): in no cycle
E_LAST = -3                      # last row of all
E_Q = {-4: -1, 1: 2, -2: 0, 3: -4, 0: 3, 5: 1, 4: -2, -3: 5}      # the q row's exponent where the k row has the key: never equal, all in [-4, 5]


def row_exponents(B, S):
    """int64 [B, S]: e of row (b, s).  Adjacent rows (in the flat order b * S + s) differ, row (b, s) and row (1 - b, s) differ, the first row of
    every batch element and the last row of all carry a value no other row has"""
    s = torch.arange(S)[None, :]
    b = torch.arange(B)[:, None]
    e = torch.tensor(E_CYCLE)[(s + 2 * b) % 5]
    e[:, 0] = torch.tensor([E_FIRST[i % 2] for i in range(B)])
    if B * S > 1:
        e[B - 1, S - 1] = E_LAST
    return e


def q_exponents(e):
    """the exponents of the q rows that go with k rows of exponents e: every row differs (q totals are at least 4 x off the k totals)"""
    out = e.clone()
    for k, v in E_Q.items():
        out[e == k] = v
    return out


def groups(seed, rows, C):
    """[rows, C] float64: per row C / 8 permuted, signed copies of NORM_GROUP (a different arrangement per row)"""
    g = torch.Generator().manual_seed(seed)
    return torch.cat([X.norm_x(g, C) for _ in range(rows)], 0)


def scaled_rows(grp, e):
    """grp [rows, C] * 2^e[row]"""
    return grp * torch.ldexp(torch.ones(e.numel(), dtype=torch.float64), e.reshape(-1))[:, None]


def sumsq_of(e, C_total):
    """the sum of squares of a scaled row over C_total channels: 4 C_total 4^e, float64 (an fp32 value)"""
    return 4.0 * C_total * torch.ldexp(torch.ones(e.numel(), dtype=torch.float64), 2 * e.reshape(-1))


def norm_weights(seed, C):
    return X.norm_weights(torch.Generator().manual_seed(seed), C)


def rstd32(total, dim, eps):
    """fp32 rsqrt(total / dim + eps) as torch evaluates it (the kernels: rsqrtf(tot / (float)dim + eps)); total float64 holding fp32 values"""
    return torch.rsqrt(total.float() / float(dim) + torch.tensor(eps, dtype=torch.float32))


def knorm(x, w, inv, dt):
    """T(w * T(x * inv)): the K half (vit_knorm_slots_kernel, vit_qknorm_kernel part 1); x [rows, C], inv fp32 [rows]; returns a tensor of T"""
    T = DT[dt]
    return (w.float()[None, :] * (x.float() * inv[:, None]).to(T).float()).to(T)


def qnorm(x, w, inv, dt, q_scale=Q_SCALE):
    """T(T(w * T(x * inv)) * q_scale): the Q half (vit_qknorm_kernel part 0, attn2_kernel on load); one fp32 product, rounded to T"""
    return (knorm(x, w, inv, dt).float() * torch.tensor(q_scale, dtype=torch.float32)).to(DT[dt])


def exact_knorm(grp, w, dt):
    """what knorm must give on a scaled row whose statistic is right: w * group / 2, exactly representable"""
    v = w[None, :] * grp / 2
    assert bool(X.representable(v, dt).all())
    return v.float().to(DT[dt])


# ---------------------------------------------------------------------------------------------------------------------------------------
# hand-made slots
# ---------------------------------------------------------------------------------------------------------------------------------------
SHARES = 1024


def split_slots(total, nslots, salt=0):
    """[nslots, rows] float64: row m's total cut into integer shares of total / 1024: 1024 // nslots - 2 + (7 m + 3 s + salt) % 5 for every slot
    but the last, which takes the rest -- unequal, but every slot carries more than 1 % of the total, so a slot left out moves the rsqrt by
    more than half an ulp of bf16.  Any partial sum in any order is an integer number of shares below 2^24: exact in fp32"""
    rows = total.numel()
    assert 1 <= nslots <= 128
    m = torch.arange(rows)[None, :]
    s = torch.arange(nslots)[:, None]
    w = (SHARES // nslots - 2 + (7 * m + 3 * s + salt) % 5).to(torch.float64)
    w[nslots - 1] = SHARES - w[:nslots - 1].sum(0)
    assert bool((w >= 1).all()) and bool((w.sum(0) == SHARES).all())
    out = w * (total.reshape(1, -1) / SHARES)
    assert torch.equal(X.f32(out), out)
    return out


def slot_buffer(slots, ld, behind=2):
    """fp32 [nslots + behind, ld], NaN everywhere but [slot < nslots][row < rows]"""
    n, rows = slots.shape
    buf = torch.full((n + behind, ld), NAN, dtype=torch.float32)
    buf[:n, :rows] = slots.float()
    return buf


# ---------------------------------------------------------------------------------------------------------------------------------------
# the row scale finished inside the GEMM launch: which source the tile's slots come from (launch_cfg8 / launch_cfg in csrc/gemm.hip, restated)
# ---------------------------------------------------------------------------------------------------------------------------------------
RS_NSLOTS = (1, 2, 15, 16, 17, 29, 32, 33, 50, 67)
RS_EPIS = ("bias", "ls_resid", "gelu")
RS_DIM = 64
RS_TILES = X.ROW_SCALE_TILES + (4, 5)      # + the 224-row tile (a partial last 64-row group in tile_row_scale_prefetch) and the 8-wave 192-row tile
CFG8_TILES = (2, 12, 13)         # ids that run the staggered 8-wave 256^2 kernel (launch_cfg8); every other id of TILES is a launch_cfg instantiation
LDS_WG = 160 * 1024


def rs_source(tile, nslots):
    """"dma": the tile's slots are fetched by LDS-DMA behind the stage buffers; "global": tile_row_scale reads them from global memory.
    launch_cfg8: LDS = 2 stages x 4 x 128 x 128 bytes, the slots of 256 rows behind it, 160 KiB per workgroup.
    launch_cfg:  LDS = 2 (BM + BN) 128 bytes, the slots of BM rounded up to 64 rows, at most 32 KiB more and at most 160 KiB."""
    if tile in CFG8_TILES:
        lds, rs_bytes, lds_max = 2 * 4 * 128 * 128, nslots * 256 * 4, LDS_WG
    else:
        bm, bn = X.TILES[tile][:2]
        lds = 2 * (bm + bn) * 128
        rs_bytes = nslots * (-(-bm // 64) * 64) * 4
        lds_max = min(lds + 32 * 1024, LDS_WG)
    return "dma" if lds + rs_bytes <= lds_max else "global"


def threads_per_row(tile):
    """tile_row_scale: two threads per row (the first / the second half of the slots) when the workgroup has 2 BM threads"""
    bm, _, wm, wn = X.TILES[tile]
    nt = 512 if tile in CFG8_TILES else wm * wn * 64
    return 2 if nt >= 2 * bm else 1


def rs_slots(M, nslots, dim=RS_DIM):
    """(scale [M] float64, slots [nslots, M] float64): slots whose sum is dim / scale^2 = dim * 4^k, so that rsqrt(sum / dim + 0) == scale"""
    s = X.pow2_scale(M)
    return s, split_slots(dim / (s * s), nslots)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the statistics epilogues
# ---------------------------------------------------------------------------------------------------------------------------------------
NONE_STATS_TILES = (2, 6, 7, 8, 9)     # launch_t: every other id runs tile 2 under EPI_NONE_STATS (64-column slots only)
STATS_K = (64, 192)


def persistent_dispatch(M, N, n_cu, persist, rs_stats):
    """launch_cfg8's choice of the persistent kernel (tuning key 13 = persist), restated for a launch without stream-K (R = 0): more 256^2
    tiles than workgroups G = min(CUs, 256), G >= 8, and NO in-launch row scale -- a statistics epilogue does not enter the condition"""
    G = min(n_cu, 256)
    return bool(persist) and -(-M // 256) * -(-N // 256) > G and G >= 8 and not rs_stats


def slot_width(tile):
    """columns of one wave tile = one statistics slot: BN / (waves along N)"""
    _, bn, _, wn = X.TILES[tile]
    return bn // wn


def stats_tile(tile, epi):
    """the tile id that runs (launch_t's remap of EPI_NONE_STATS)"""
    return tile if epi == EPI_LS_RESID_STATS or tile in NONE_STATS_TILES else 2


def stats_shapes(tile, epi):
    """M in {1, BM + 1}; N = two whole slots and a partial one of 4 or 24 (8 mod 16) columns; K one step and an odd step count"""
    t = stats_tile(tile, epi)
    bm, w = X.TILES[t][0], slot_width(t)
    return [(1, 2 * w + 4, 64), (bm + 1, 2 * w + 24, 192), (bm + 1, 2 * w + 4, 64), (1, 2 * w + 24, 192)]


def slot_edges(tile, epi, M, N, n_cu):
    """[(first column, end column)] of every slot the launch writes, in slot order.  Tiles 12 / 13 where launch_epi's split applies: the
    64-column slots of the 256^2 launch, then the 112-column slots of the 192 x 224 tail, which start at column n_main"""
    t = stats_tile(tile, epi)
    split = X.split_rule(M, N, n_cu) if t in (12, 13) else None
    if split is None:
        w = slot_width(t)
        return [(c, min(c + w, N)) for c in range(0, N, w)]
    n_main, _ = split
    return [(c, c + 64) for c in range(0, n_main, 64)] + [(c, min(c + 112, N)) for c in range(n_main, N, 112)]


def expected_stats(out64, edges):
    """[slots, M] float64: per slot the sum of squares of the stored values of exactly its columns"""
    sq = out64 * out64
    return torch.stack([sq[:, a:b].sum(1) for a, b in edges], 0)


def stats_operands(seed, M, N, K, dt):
    """operands in gemm_exact_ref.make_operands' form whose EPI_NONE and EPI_LS_RESID outputs (with bias) are integers |c| <= 63: A in
    [-3, 3]; every row of W has four entries of +-1 spread over K; integer bias |b| <= 8, ls in {+-1, +-2}, integer residual |r| <= 23:
    |acc| <= 12, |T(acc + b)| <= 20, |. * ls| <= 40, |c| <= 63"""
    g = torch.Generator().manual_seed(seed)
    A = X.randint(g, -3, 3, (M, K))
    W = torch.zeros(N, K, dtype=torch.float64)
    pos = torch.rand((N, K), generator=g).argsort(dim=1)[:, :4]
    W.scatter_(1, pos, 1 - 2 * X.randint(g, 0, 1, (N, 4)))
    bias = X.randint(g, -8, 8, (N,))
    ls = (1 + X.randint(g, 0, 1, (N,))) * (1 - 2 * X.randint(g, 0, 1, (N,)))
    resid = X.randint(g, -23, 23, (M, N))
    ops = dict(A=A, W=W, bias=bias, ls=ls, resid=resid, row_scale=torch.ones(M, dtype=torch.float64), acc=A @ W.t())
    for name in ("A", "W", "bias", "ls", "resid"):
        assert bool(X.representable(ops[name], dt).all())
    return ops


@functools.lru_cache(maxsize=2)
def cached_stats_operands(seed, M, N, K, dt):
    return stats_operands(seed, M, N, K, dt)


def stats_precondition(out64, edges):
    """every stored value is an integer |c| <= 63 (its square a multiple of the granule 1) and every slot's total stays below 2^24 granules"""
    ok = bool((out64 == out64.round()).all()) and float(out64.abs().max()) <= 63
    return ok and float(expected_stats(out64, edges).max()) < 2 ** 24


# ---------------------------------------------------------------------------------------------------------------------------------------
# case tables of the elementwise links
# ---------------------------------------------------------------------------------------------------------------------------------------
SUMSQ_CASES = [(1, 8), (5, 256), (257, 3200), (5, 3200), (257, 8)]                       # (rows, H): rows in {1, 5, 257}, H in {8, 256, 3200}
FINISH_NSLOTS = (1, 16, 17, 50)
# (rows, C, nslots, C_total / C): rows in {1, 19}, C in {128, 384, 3200}, nslots in {1, 2, 50, 63, 64}, C_total in {C, 2 C}
KNORM_CASES = [(1, 128, 1, 1), (19, 128, 2, 2), (19, 384, 50, 1), (1, 384, 63, 2), (19, 3200, 64, 2), (19, 3200, 50, 1), (19, 384, 64, 1)]
QKNORM_CASES = [(1, 128), (19, 384), (5, 3200)]                                          # (rows, C)
# (B, S, H, stride, dim / (H 128)): S = 65, 129 take the peeled key; S = 129 ends in a query block with one live row
MHA_CASES = [(2, 64, 1, 1, 1), (2, 65, 3, 2, 1), (2, 129, 1, 2, 2), (2, 129, 3, 1, 2), (2, 65, 1, 1, 2), (2, 64, 3, 2, 2)]
POISON16 = 0x5A5A


def mha_inputs(B, S, H, dim_mult, dt, seed=7):
    """Q [B, S, H, 128] scaled rows (a row = all heads of a token), K / V [B, H, S, 128] Gaussian rounded to T, w_q, the statistics
    [B * S] = 4 dim 4^e the launch is given, and the exactly known normed Q (T(T(w_q * group / 2) * q_scale)) as a tensor of T"""
    T = DT[dt]
    C = H * 128
    e = q_exponents(row_exponents(B, S))
    grp = groups(seed, B * S, C)
    q = scaled_rows(grp, e)
    assert bool(X.representable(q, dt).all())
    wq = norm_weights(seed + 1, C)
    g = torch.Generator().manual_seed(seed + 2)
    k = torch.randn(B, H, S, 128, generator=g).to(T).float()
    v = torch.randn(B, H, S, 128, generator=g).to(T).float()
    dim = dim_mult * C
    sums = sumsq_of(e, dim)
    qn = (exact_knorm(grp, wq, dt).float() * torch.tensor(Q_SCALE, dtype=torch.float32)).to(T)
    return dict(q=q.reshape(B, S, H, 128), k=k, v=v, wq=wq, sums=sums, dim=dim, qn=qn.reshape(B, S, H, 128), e=e, grp=grp)


def mha_qn_from(inp, sums, dim, dt, eps=EPS):
    """the normed Q a kernel computes that reads `sums` [B * S] and divides by `dim` (the mutants pass other sums / another divisor)"""
    B, S, H, _ = inp["q"].shape
    inv = rstd32(sums, dim, eps)
    return qnorm(inp["q"].reshape(B * S, H * 128), inp["wq"], inv, dt).reshape(B, S, H, 128)


# ---------------------------------------------------------------------------------------------------------------------------------------
# mutants: what a subtly wrong kernel would read.  Each returns the statistic(s) such a kernel uses instead of the right ones.
# ---------------------------------------------------------------------------------------------------------------------------------------
def mutant_row_plus_1(per_row):
    """the statistic of row r + 1 (the last row: the one before it)"""
    out = torch.roll(per_row, -1, 0)
    out[-1] = per_row[-2] if len(per_row) > 1 else per_row[-1]
    return out


def mutant_other_batch(per_row, B, S):
    """the statistic of the same row of the neighbouring batch element ((b * Sq + rr) with b off by one)"""
    return torch.roll(per_row.reshape(B, S, *per_row.shape[1:]), 1, 0).reshape(per_row.shape)


def mutant_stride_ignored(buf, rows, stride):
    """qn_stride taken for 1: row r reads word r of the [rows * stride] buffer"""
    return buf[:rows]


def slot_mutant_totals(buf, rows, q0, nslots, kind):
    """the (q total, k total) [rows] a vit_knorm_slots-like consumer arrives at from the slot buffer (q slots [q0, q0 + nslots), k slots behind
    them) under a mutation: "ok", "swap_groups", "drop_last", "one_behind" """
    q = buf[q0:q0 + nslots, :rows].double()
    k = buf[q0 + nslots:q0 + 2 * nslots, :rows].double()
    if kind == "swap_groups":
        q, k = k, q
    elif kind == "drop_last":
        q, k = q[:-1], k[:-1]
    elif kind == "one_behind":
        q = buf[q0:q0 + nslots + 1, :rows].double()
        k = buf[q0 + nslots:q0 + 2 * nslots + 1, :rows].double()
    elif kind != "ok":
        raise ValueError(kind)
    return q.sum(0), k.sum(0)


def stats_mutant_edges(edges, N, kind):
    """slot column ranges of a statistics epilogue that drops a slot's last column / counts a column >= N into the last slot"""
    e = list(edges)
    if kind == "drop_last_column":
        return [(a, b - 1) for a, b in e]
    if kind == "count_beyond_n":
        return e[:-1] + [(e[-1][0], e[-1][1] + 1)]
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the tower
# ---------------------------------------------------------------------------------------------------------------------------------------
POS_KEY = "embeddings.position_embedding"


def scale_pos_rows(pos):
    """position embedding [1, ntok, C] with row r multiplied by 2^(r % 5 - 2): the residual rows then differ in magnitude"""
    r = torch.arange(pos.shape[1])
    return pos * torch.ldexp(torch.ones(len(r), dtype=pos.dtype), r % 5 - 2)[None, :, None]


def scale_tiles(px):
    """pixel tiles [n, 3, S, S] with tile b multiplied by 4^(b % 3 - 1) (exact): the same token row of neighbouring tiles differs in magnitude too.
    (The branches enter the residual stream through a layer scale of ~0.1, so a statistic off by 2 moves a row by less than ten bounds of bf16;
    one off by 4 or 16 does: test_vit_stats_cpu.py prints both mutants' figures.)"""
    b = torch.arange(px.shape[0])
    return px * torch.ldexp(torch.ones(len(b), dtype=px.dtype), 2 * (b % 3 - 1))[:, None, None, None]


def cdiv(a, b):
    return -(-a // b)

