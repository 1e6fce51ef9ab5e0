"""GPU: the decode attention over the e4m3 KV cache, the cache quantiser and the split-KV merge, each against the fp64 restatement of
tests/kv8_ref.py (checked by tests/test_kv8_cpu.py) on inputs where ONE wrong key, scale or partial misses a head by O(1): tied keys on every
boundary position (first, last, both sides of every tile and split edge), scales that differ by >= 2 between neighbours, partials one of which
owns the row.  out and the workspace are NaN before every call; cache bytes 0x7F, NaN scales and NaN 16-bit rows sit behind every length.

What each part reaches (T = bf16 and f16):
  (a) omchat_op_attn_decode_kv8: key 47 = 1 attn_decode_kernel<T, true> (attn_decode_tile<KV8>: both scale-load branches -- whole tile, ragged tile);
      2 / 3 / 4 attn_decode_kv8_walk_kernel<T, 2 | 3 | 4, 1>; 11 attn_decode_kv8_walk_kernel<T, 3, 4> (dead waves, the LDS fold); 0 the launcher's
      pick; GQA groups 1, 2, 4, 7, 16; merges of 1 .. 26 partials (attn_merge_kernel's one-round-trip branch).
  (b) omchat_op_attn_decode_kv8_append: attn_decode_kv8_walk_kernel<T, 3, 1, true> and <T, 3, 4, true> (key 48 = 1) and rope_kv_kernel's e4m3
      outputs in front of the unfused forms (key 48 = 0, or a launch too short to fuse); the 33 k-key case is the one the launcher fuses by itself.
  (c) omchat_op_attn_decode_kv8_masked: attn_decode_kernel<T, true, true>.
  (d) omchat_op_kv_quant: kv_quant_kernel<T> (pos_lo / pos0, len, max_rows).
  (e) omchat_op_attn_merge: attn_merge_kernel<T> (<= 64 branch; chunk loop, second and third chunk), attn_merge_mid_kernel<T, 4, 1 | 2> and <T, 8, 1 | 4>.
  (f) omchat_op_attn_decode (16-bit cache) with the same boundary witnesses: attn_decode_kernel<T>, attn_decode_multi_kernel<T, false | true>,
      attn_decode_dma_kernel<T, 2>.

Bound of (a), (b), (c), (f): gpu_util.TOL per (sequence, head).  What the kernels' operand rounding alone costs on these inputs (P x value scale
rounded to T, per-split running maximum; test_kv8_cpu.py::test_operand_rounding_stays_under_half_the_bound, worst (sequence, head) per family):
    bf16 (TOL 1.2e-2): plain 2.45e-3  drop 3.26e-3  scale 3.02e-3  smallv 2.27e-3  largev 2.20e-3  masked 2.11e-3
    f16  (TOL 2.5e-3): plain 3.19e-4  drop 4.16e-4  scale 3.45e-4  smallv 3.04e-4  largev 4.00e-4  masked 2.89e-4
    f16 smallv with the value scale folded into P unscaled (the kernels before the fold was rescaled): 9.01e-3, outside the bound
Measured on an MI355X, worst (sequence, head): bf16 plain 3.24e-3  drop 4.16e-3  scale 3.28e-3  smallv 2.80e-3  largev 2.78e-3  masked 2.65e-3
append 4.00e-3; f16 plain 4.01e-4  drop 5.00e-4  scale 3.93e-4  smallv 3.54e-4  largev 4.95e-4  masked 3.43e-4  append 4.44e-4.  f16 smallv before
the fold was rescaled (attn_common.h FoldRescale): 4.89e-3 (tile_edges, key 47 = 1) and 6.21e-3 (nw4).
Bound of (e), per element: half an ulp of T at the reference value (2^-9 resp. 2^-12 of the power of two above it) + 2^-13 relative (fp32 sums of <= 2049 positive terms and exp2f: twice the 2^-14 the CPU test allows a plain
fp32 evaluation); an owner's output within 1 ulp of T(O_s / l_s).  (b) and (d): bytes, scales and 16-bit rows bit for bit."""
import functools
import pytest
import torch

pytestmark = pytest.mark.gpu
from gpu_util import DT, CODE, TOL, ptr, sync
from omchat_amd import _lib
import decode_append_ref as dar
import kv8_ref as kr

DTS = ["bf16", "f16"]
NAN = float("nan")
KEY_DEFAULTS = {10: 0, 12: 0, 19: 64, 21: 1, 25: 1, 26: 0, 47: 0, 48: 1}


def i32(v):
    return torch.as_tensor(v, dtype=torch.int32).to("cuda")


class tuning:
    """set tuning keys for a block, restore the defaults whatever happens"""
    def __init__(self, lib, **keys):
        self.lib, self.keys = lib, {int(k[1:]): v for k, v in keys.items()}

    def __enter__(self):
        for k, v in self.keys.items():
            _lib.check(self.lib.omchat_op_set_tuning(k, v))

    def __exit__(self, *exc):
        for k in self.keys:
            self.lib.omchat_op_set_tuning(k, KEY_DEFAULTS[k])


def poisoned(inp, first=0):
    """device copies of the e4m3 cache with everything from slot lens[i] - first on poisoned: (k8, v8, ks, vs)"""
    k8, v8, ks, vs = inp.k8.clone(), inp.v8.clone(), inp.ks.clone(), inp.vs.clone()
    for i, n in enumerate(inp.lens):
        k8[i, :, n - first:] = 0x7F; v8[i, :, n - first:] = 0x7F; ks[i, :, n - first:] = NAN; vs[i, :, n - first:] = NAN
    return k8.cuda(), v8.cuda(), ks.cuda(), vs.cuda()


def check_heads(out, ref, dt, tag):
    assert torch.isfinite(out.float()).all(), (tag, "unwritten or non-finite output")
    err = kr.rel_heads(out, ref)
    print("kv8", tag, "worst (sequence, head) rel", f"{float(err.max()):.3e}", "bound", TOL[dt])
    assert float(err.max()) < TOL[dt], (tag, err)


# ------------------------------------------------------------------------------------------------ (a) attention over a given e4m3 cache
@functools.lru_cache(maxsize=8)
def _case(name, family, dt, rnd):
    """(inputs, fp64 reference): computed once, shared, never modified"""
    inp = kr.case_inputs(name, family, DT[dt], rnd)
    ref = kr.attend(inp.q, inp.k8, inp.ks, inp.v8, inp.vs, inp.lens, kr.SCALE, inp.mask)
    assert torch.isfinite(ref).all()
    return inp, ref


def run_kv8(lib, dt, inp, cache, mask=None):
    b, Hq = inp.q.shape[:2]
    Hkv, cap = inp.k8.shape[1:3]
    L = max(inp.lens)
    wsb = lib.omchat_op_attn_decode_ws(b, Hq, L)
    ws = torch.full((wsb // 4 + 4,), NAN, dtype=torch.float32, device="cuda")
    out = torch.full((b, Hq, 128), NAN, dtype=DT[dt], device="cuda")
    dq = inp.q.to(DT[dt]).cuda()
    if mask is None:
        dl = i32(inp.lens)
        _lib.check(lib.omchat_op_attn_decode_kv8(CODE[dt], ptr(dq), ptr(cache[0]), ptr(cache[1]), ptr(cache[2]), ptr(cache[3]), ptr(out), b, Hq, Hkv, cap, L,
                                                 ptr(dl), kr.SCALE, ptr(ws), wsb, None))
    else:
        _lib.check(lib.omchat_op_attn_decode_kv8_masked(CODE[dt], ptr(dq), ptr(cache[0]), ptr(cache[1]), ptr(cache[2]), ptr(cache[3]), ptr(out), b, Hq, Hkv,
                                                        cap, L, ptr(mask), mask.shape[1], kr.SCALE, ptr(ws), wsb, None))
    sync()
    return out


def part_a(lib, dt, name, family):
    """[(tag, out, ref)] of every round and form of a case"""
    b, Hq, Hkv, cap, lens, forms = kr.SHAPES[name]
    res = []
    for rnd in range(kr.n_rounds(Hq, lens) if family == "drop" else 1):
        inp, ref = _case(name, family, dt, rnd)
        cache = poisoned(inp)
        for form in forms:
            with tuning(lib, k47=form):
                res.append(((dt, name, family, "round", rnd, "key 47", form), run_kv8(lib, dt, inp, cache), ref))
    return res


A_CASES = [(n, f) for n in kr.SHAPES for f in ("plain", "drop", "scale")] + [(n, f) for n in ("tile_edges", "nw4") for f in ("smallv", "largev")]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name,family", A_CASES)
def test_kv8_decode_attention_per_head(gpu_lib, dt, name, family):
    """(a): every form of the case table on every family; `drop` in as many rounds as it takes for every boundary position to have been owned"""
    for tag, out, ref in part_a(gpu_lib, dt, name, family):
        check_heads(out, ref, dt, tag)


# ------------------------------------------------------------------------------------------------ (b) the fused append
@functools.lru_cache(maxsize=4)
def _append_case(name, dt):
    T = DT[dt]
    b, Hq, Hkv, cap, lens, _ = kr.APPEND_SHAPES[name]
    qkv, inp, owners = kr.append_inputs(name, T)
    # the rotation with the model's roundings, which the kernels keep (rope_chunk): the rows they store, bit for bit.  (With rope_rows' single
    # rounding the rotated key differs by an ulp here and there, some of its e4m3 bytes by one step of 6 %, and a head that weights the new key
    # misses TOL against an attention over THAT cache: measured 1.8e-2 / 9.3e-3 (bf16 / f16) on one_key_and_769, fused or not.)
    res = kr.decode_append_kv8(qkv, inp.k8, inp.ks, inp.v8, inp.vs, inp.k16, inp.v16, Hq, Hkv, lens, kr.THETA, kr.SCALE, T, rope=kr.rope_rows_T)
    assert torch.isfinite(res[0]).all()
    return qkv, inp, res[0], res[1:7]


def part_b(lib, dt, name, form, fuse):
    T = DT[dt]
    b, Hq, Hkv, cap, lens, _ = kr.APPEND_SHAPES[name]
    qkv, inp, ref, stored = _append_case(name, dt)
    k8, v8, ks, vs = poisoned(inp, first=1)
    k16, v16 = inp.k16.clone(), inp.v16.clone()
    for i, n in enumerate(lens):
        k16[i, :, n - 1:] = NAN; v16[i, :, n - 1:] = NAN
    before = [t.cpu().clone() for t in (k8, ks, v8, vs)] + [k16.to(T), v16.to(T)]
    k16, v16 = k16.to(T).cuda(), v16.to(T).cuda()
    dq = qkv.to(T).cuda()
    L, uniform = max(lens), len(lens) == 1
    wsb = lib.omchat_op_attn_decode_ws(b, Hq, L)
    ws = torch.full((wsb // 4 + 4,), NAN, dtype=torch.float32, device="cuda")
    out = torch.full((b, Hq, 128), NAN, dtype=T, device="cuda")
    dl = None if uniform else i32(lens)
    dp = None if uniform else i32([n - 1 for n in lens])
    with tuning(lib, k47=form, k48=fuse):
        _lib.check(lib.omchat_op_attn_decode_kv8_append(CODE[dt], ptr(dq), kr.THETA, ptr(k8), ptr(v8), ptr(ks), ptr(vs), ptr(k16), ptr(v16), ptr(out), b, Hq,
                                                        Hkv, cap, L, ptr(dl), ptr(dp), kr.SCALE, ptr(ws), wsb, None))
        sync()
    return out, [t.cpu() for t in (k8, ks, v8, vs, k16, v16)], before, ref, stored


def raw(t):
    """the bits of a tensor (NaN poison compares equal to itself)"""
    return t if t.dtype == torch.uint8 else t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


B_CASES = [(n, f) for n, s in kr.APPEND_SHAPES.items() for f in s[5]]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("name,form", B_CASES)
def test_kv8_fused_append_against_the_restated_step(gpu_lib, dt, name, form, fuse):
    """(b): the new key is tied to one head per sequence; the output per head against the fp64 step; the appended e4m3 bytes, scales and 16-bit
    rows bit for bit against the restated quantiser on the rotated row (the rotation with the model's roundings, which rope_chunk keeps:
    kv8_ref.rope_rows_T); every other slot, poison included, untouched"""
    lens = kr.APPEND_SHAPES[name][4]
    out, after, before, ref, stored = part_b(gpu_lib, dt, name, form, fuse)
    tag = (dt, name, "key 47", form, "key 48", fuse)
    check_heads(out, ref, dt, tag)
    for what, got, was, want in zip(("k8", "k scales", "v8", "v scales", "k16", "v16"), after, before, stored):
        expect = was.clone()
        for i, n in enumerate(lens):
            expect[i, :, n - 1] = want[i, :, n - 1]
            assert torch.equal(raw(got[i, :, n - 1]), raw(want[i, :, n - 1])), (tag, what, "sequence", i, "the appended row differs from the restated one")
        assert torch.equal(raw(got), raw(expect)), (tag, what, "a slot other than the new one changed")


# ------------------------------------------------------------------------------------------------ (c) masked
def part_c(lib, dt):
    inp, ref = _case("masked", "masked", dt, 0)
    mask = (inp.mask * torch.tensor([1, 2, 128, 255], dtype=torch.uint8).repeat(dar.MASK_SB // 4)).cuda()      # visible is "!= 0", not "== 1"
    return run_kv8(lib, dt, inp, poisoned(inp), mask), ref


@pytest.mark.parametrize("dt", DTS)
def test_kv8_masked_decode_attention(gpu_lib, dt):
    """(c): left pads inside a tile, of one whole tile, of two tiles and two keys; holes; a tied key hidden by the mask with poisoned values
    (leak) and a tied key that is the last visible one in front of a hole / the first behind a pad (drop)"""
    out, ref = part_c(gpu_lib, dt)
    check_heads(out, ref, dt, (dt, "masked"))


@pytest.mark.parametrize("dt", DTS)
def test_kv8_masked_refusals_launch_nothing(gpu_lib, dt):
    inp, _ = _case("masked", "masked", dt, 0)
    cache = poisoned(inp)
    b, Hq, Hkv, cap, L = 4, 4, 2, 256, 200
    mask = inp.mask.cuda()
    out = torch.full((b, Hq, 128), NAN, dtype=DT[dt], device="cuda")
    wsb = gpu_lib.omchat_op_attn_decode_ws(b, Hq, L)
    ws = torch.full((wsb // 4 + 4,), NAN, dtype=torch.float32, device="cuda")
    dq = inp.q.to(DT[dt]).cuda()
    for msb, m, k in ((200, ptr(mask), ptr(cache[0])), (128, ptr(mask), ptr(cache[0])), (256, None, ptr(cache[0])), (256, ptr(mask), None)):
        with pytest.raises(ValueError):
            _lib.check(gpu_lib.omchat_op_attn_decode_kv8_masked(CODE[dt], ptr(dq), k, ptr(cache[1]), ptr(cache[2]), ptr(cache[3]), ptr(out), b, Hq, Hkv, cap, L,
                                                                m, msb, kr.SCALE, ptr(ws), wsb, None))
    sync()
    assert bool(torch.isnan(out.float()).all()) and bool(torch.isnan(ws).all())


# ------------------------------------------------------------------------------------------------ (d) the cache quantiser
def quant_rows(T, b=3, Hkv=2, cap=40):
    """k, v [b, Hkv, cap, 128] values of T: by position % 5 a zero row, a row whose largest element maps to exactly 448 (byte 0x7E), a
    linspace(-1, 1) row (e4m3 subnormals), a row on exact round-to-nearest-even ties of the e4m3 grid, a Gaussian row"""
    g = torch.Generator().manual_seed(77)
    grid = kr.e4m3(torch.arange(0, 127, dtype=torch.uint8)).float()          # 0 .. 448
    ties = torch.cat((torch.tensor([448.0]), (grid[:-1] + grid[1:]) / 2, torch.tensor([-(grid[9] + grid[10]) / 2])))      # 1 + 126 + 1
    x = []
    for which in range(2):
        t = (torch.randn(b, Hkv, cap, 128, generator=g) * 0.05)
        for j in range(cap):
            if j % 5 == 0:
                t[:, :, j] = 0
            elif j % 5 == 1:
                t[:, :, j, (7 + j + which) % 128] = 3.0
            elif j % 5 == 2:
                t[:, :, j] = torch.linspace(-1, 1, 128)
            elif j % 5 == 3:
                for i in range(b):
                    for h in range(Hkv):
                        t[i, h, j] = ties.roll(j + which) * 2.0 ** (i - h - 6)
        x.append(t.to(T).float())
    assert torch.equal(x[0][0, 0, 3].abs().max(), torch.tensor(448.0 * 2.0 ** -6))      # the tie rows survived the rounding to T: s = 2^-6 exactly
    return x


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("max_rows", [1, 4, 5, 23])
def test_kv_quant_rows_bit_exact_and_nothing_else_written(gpu_lib, dt, max_rows):
    """(d): rows [lo, min(lo + max_rows, len)) of every (sequence, head) hold the restated quantiser's bytes and scales; every other byte and
    scale keeps its sentinel.  lo per sequence (pos_lo) or common (pos0); len absent, inside the row range, below lo."""
    T, b, Hkv, cap = DT[dt], 3, 2, 40
    k, v = quant_rows(T)
    (k8r, ksr), (v8r, vsr) = kr.quant(k), kr.quant(v)
    assert int(k8r[0, 0, 1, 8]) == 0x7E and int(k8r[0, 0, 0].max()) == 0 and float(ksr[0, 0, 0]) == 1.0
    dk, dv = k.to(T).cuda(), v.to(T).cuda()
    los = [0, 7, 17]
    for pos_lo, pos0, lens in ((los, 0, None), (None, 9, None), (los, 0, [2, 4, 40]), (None, 9, [10, 9, 12])):
        k8 = torch.full((b, Hkv, cap, 128), 0x55, dtype=torch.uint8, device="cuda"); v8 = k8.clone()
        ks = torch.full((b, Hkv, cap), -7.0, dtype=torch.float32, device="cuda"); vs = ks.clone()
        dlo = None if pos_lo is None else i32(pos_lo)
        dlen = None if lens is None else i32(lens)
        _lib.check(gpu_lib.omchat_op_kv_quant(CODE[dt], ptr(dk), ptr(dv), ptr(k8), ptr(v8), ptr(ks), ptr(vs), b, Hkv, cap, ptr(dlo), pos0, ptr(dlen), max_rows, None))
        sync()
        wk8 = torch.full_like(k8r, 0x55); wv8 = wk8.clone(); wks = torch.full_like(ksr, -7.0); wvs = wks.clone()
        for i in range(b):
            lo = pos_lo[i] if pos_lo is not None else pos0
            hi = min(lo + max_rows, lens[i] if lens is not None else cap)
            if hi > lo:
                wk8[i, :, lo:hi] = k8r[i, :, lo:hi]; wv8[i, :, lo:hi] = v8r[i, :, lo:hi]; wks[i, :, lo:hi] = ksr[i, :, lo:hi]; wvs[i, :, lo:hi] = vsr[i, :, lo:hi]
        tag = (dt, max_rows, pos_lo, pos0, lens)
        assert torch.equal(k8.cpu(), wk8) and torch.equal(v8.cpu(), wv8), tag
        assert torch.equal(ks.cpu(), wks) and torch.equal(vs.cpu(), wvs), tag
    with pytest.raises(ValueError):
        _lib.check(gpu_lib.omchat_op_kv_quant(CODE[dt], ptr(dk), ptr(dv), ptr(k8), ptr(v8), ptr(ks), ptr(vs), b, Hkv, cap, None, cap - 3, None, 4, None))
    with pytest.raises(ValueError):
        _lib.check(gpu_lib.omchat_op_kv_quant(CODE[dt], ptr(dk), None, ptr(k8), ptr(v8), ptr(ks), ptr(vs), b, Hkv, cap, None, 0, None, 4, None))


# ------------------------------------------------------------------------------------------------ (e) the merge
HALF_ULP = {"bf16": 2.0 ** -9, "f16": 2.0 ** -12}      # half an ulp of T, relative to the power of two ABOVE the value (2^-8 / 2^-11 of the one below)
MERGE_KEYS = ({}, {"k21": 0}, {"k21": 2}, {"k19": 1})


def run_merge(lib, dt, mc, nsplit):
    ws = mc.ws.cuda()
    out = torch.full((kr.MERGE_ROWS, kr.MERGE_HEADS, 128), NAN, dtype=DT[dt], device="cuda")
    _lib.check(lib.omchat_op_attn_merge(CODE[dt], ptr(ws), nsplit, kr.MERGE_HEADS, kr.MERGE_ROWS, ptr(i32(mc.lens)), nsplit * kr.MERGE_SPLIT_KEYS, kr.SCALE,
                                        ptr(out), kr.MERGE_SPLIT_KEYS, None))
    sync()
    assert torch.equal(ws.cpu().view(torch.int32), mc.ws.view(torch.int32)), "the partials were modified"
    return out.cpu()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nsplit", kr.MERGE_NSPLITS)
def test_split_merge_on_hand_made_partials(gpu_lib, dt, nsplit):
    """(e): rows of nsplit, nsplit - 1 and 1 live partials (NaN behind them); each (row, head) owned by one partial index -- 0, 1, 7, 8, the
    edges of every kernel's thread groups and chunks, the last and the one before it -- whose weight is 1 - O(2^-60): a partial that is dropped,
    counted twice or weighted by another maximum moves an owner to a different u_s (relative distance O(1))"""
    T = DT[dt]
    for rnd in range(kr.merge_rounds(nsplit)):
        mc = kr.merge_partials(nsplit, rnd)
        ref = torch.stack([torch.stack([kr.merge_ref(mc.ws[r, h, :, 128], mc.ws[r, h, :, 129], mc.ws[r, h, :, :128], mc.ns[r], mc.c)
                                        for h in range(kr.MERGE_HEADS)]) for r in range(kr.MERGE_ROWS)])
        own = torch.stack([torch.stack([mc.ws[r, h, int(mc.owner[r, h]), :128] / mc.ws[r, h, int(mc.owner[r, h]), 129]
                                        for h in range(kr.MERGE_HEADS)]) for r in range(kr.MERGE_ROWS)]).to(T)
        for keys in MERGE_KEYS:
            with tuning(gpu_lib, **keys):
                got = run_merge(gpu_lib, dt, mc, nsplit)
            tag = (dt, "nsplit", nsplit, "round", rnd, keys)
            assert torch.isfinite(got.float()).all(), tag
            bound = torch.exp2(torch.floor(torch.log2(ref)) + 1) * HALF_ULP[dt] + ref * 2.0 ** -13
            over = ((got.double() - ref).abs() / bound).max()
            assert float(over) <= 1.0, (tag, "worst error / bound", float(over))
            ulps = (got.view(torch.int16).int() - own.view(torch.int16).int()).abs()
            assert int(ulps.max()) <= 1, (tag, "an owner's row is not its partial's O / l", int(ulps.max()))


# ------------------------------------------------------------------------------------------------ (f) the 16-bit cache, same witnesses
F_KEYS = [(k10, k25, k12) for k10 in (1, 2, 4) for k25 in (0, 1) for k12 in (0, 1)]


@functools.lru_cache(maxsize=4)
def _case16(name, dt, rnd):
    b, Hq, Hkv, cap, L, lens = dar.SHAPES[name]
    q, k, v, ties = kr.drop_inputs16((b, Hq, Hkv, cap, lens), DT[dt], rnd, 13000 + sorted(dar.SHAPES).index(name), tile=32)
    ref = dar.attend(q, k, v, lens, kr.SCALE)
    for i, n in enumerate(lens):
        k[i, :, n:] = NAN; v[i, :, n:] = NAN
    return q, k, v, ref


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", ["multi4_ragged", "multi2_ragged", "ring_ragged"])
def test_16_bit_decode_attention_with_boundary_witnesses(gpu_lib, dt, name):
    """(f): the first and last key and both sides of every 32-key edge (the ring form's tiles; every 64-key tile and every split edge is one of
    them) owned by a head, under keys 10 x 25 x 12"""
    T = DT[dt]
    b, Hq, Hkv, cap, L, lens = dar.SHAPES[name]
    wsb = gpu_lib.omchat_op_attn_decode_ws(b, Hq, L)
    dl = i32(lens)
    for rnd in range(kr.n_rounds(Hq, lens, 32)):
        q, k, v, ref = _case16(name, dt, rnd)
        dq, dk, dv = q.to(T).cuda(), k.to(T).cuda(), v.to(T).cuda()
        for k10, k25, k12 in F_KEYS:
            ws = torch.full((wsb // 4 + 4,), NAN, dtype=torch.float32, device="cuda")
            out = torch.full((b, Hq, 128), NAN, dtype=T, device="cuda")
            with tuning(gpu_lib, k10=k10, k25=k25, k12=k12):
                _lib.check(gpu_lib.omchat_op_attn_decode(CODE[dt], ptr(dq), ptr(dk), ptr(dv), ptr(out), b, Hq, Hkv, cap, L, ptr(dl), kr.SCALE, ptr(ws), wsb, None))
                sync()
            check_heads(out, ref, dt, (dt, name, "round", rnd, "keys 10 / 25 / 12", (k10, k25, k12)))
