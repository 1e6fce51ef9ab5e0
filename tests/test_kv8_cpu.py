"""CPU (no GPU): what tests/test_gpu_kv8_attn.py rests on, proven before a kernel is judged -- the restated quantiser, the fp64 attention on
the de-quantised cache, the witnesses (every tied key carries its owner head; every boundary position is owned; a scale from the neighbouring
key moves every head), what the kernels' operand rounding alone costs on exactly the GPU test's inputs (calibration, printed), and the
split-KV merge restatement with its owners and its fp32 allowance."""
import math
import pytest
import torch
import kv8_ref as kr
import decode_append_ref as dar
from gpu_util import DT, TOL

DTS = ["bf16", "f16"]
CASES = list(kr.SHAPES)


def _head(inp, i, h, hide=None, see_all=False):
    """(probabilities [n], output [128]) of one (sequence, head) in fp64; hide: a key made invisible"""
    n, rep = inp.lens[i], inp.q.shape[1] // inp.k8.shape[1]
    g = h // rep
    s = kr.dequant(inp.k8[i, g, :n], inp.ks[i, g, :n]) @ inp.q[i, h].double() * kr.SCALE
    if inp.mask is not None and not see_all:
        s = torch.where(inp.mask[i, :n] != 0, s, torch.full_like(s, -math.inf))
    if hide is not None:
        s[hide] = -math.inf
    p = torch.softmax(s, dim=0)
    return p, p @ kr.dequant(inp.v8[i, g, :n], inp.vs[i, g, :n])


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_restated_quantiser_is_quant_ref_bit_for_bit():
    from test_gpu_fp8 import quant_ref
    g = torch.Generator().manual_seed(1)
    for dt in DTS:
        x = (torch.randn(300, 128, generator=g) * 0.05).to(DT[dt]).float()
        x[3] = 0; x[5, 7] = 3.0; x[6] = torch.linspace(-1, 1, 128).to(DT[dt]).float()
        q, s = quant_ref(x)
        b8, s2 = kr.quant(x)
        assert torch.equal(b8, q.view(torch.uint8)) and torch.equal(s, s2)
        assert int(b8[5, 7]) == 0x7E and int(b8[3].max()) == 0 and float(s2[3]) == 1.0
        assert torch.equal(kr.dequant(b8, s2), q.float().double() * s.double()[:, None])


@pytest.mark.parametrize("name", CASES + ["masked"])
def test_attend_is_atens_softmax_on_the_dequantised_cache(name):
    inp = kr.case_inputs(name, "masked" if name == "masked" else "plain", torch.bfloat16)
    ref = kr.attend(inp.q, inp.k8, inp.ks, inp.v8, inp.vs, inp.lens, kr.SCALE, inp.mask)
    rep = inp.q.shape[1] // inp.k8.shape[1]
    for i, n in enumerate(inp.lens):
        kk = kr.dequant(inp.k8[i, :, :n], inp.ks[i, :, :n]).repeat_interleave(rep, 0)
        vv = kr.dequant(inp.v8[i, :, :n], inp.vs[i, :, :n]).repeat_interleave(rep, 0)
        am = None if inp.mask is None else (inp.mask[i, :n] != 0)[None, None, :]
        got = torch.nn.functional.scaled_dot_product_attention(inp.q[i].double()[:, None, :], kk, vv, attn_mask=am, scale=kr.SCALE)[:, 0]
        assert float((got - ref[i]).abs().max()) < 1e-12 * max(1.0, float(ref[i].abs().max()))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", CASES)
def test_every_tied_key_carries_its_owner_and_every_boundary_is_owned(name, dt):
    b, Hq, Hkv, cap, lens, forms = kr.SHAPES[name]
    owned = [set() for _ in lens]
    worst_p, worst_d = 1.0, math.inf
    for rnd in range(kr.n_rounds(Hq, lens)):
        inp = kr.case_inputs(name, "drop", DT[dt], rnd)
        for (i, g, j), (h, kind) in inp.ties.items():
            assert kind == "drop" and h // (Hq // Hkv) == g and j < lens[i]
            owned[i].add(j)
            p, out = _head(inp, i, h)
            worst_p = min(worst_p, float(p[j]))
            if lens[i] > 1:      # (a one-key sequence without its key has no output at all)
                worst_d = min(worst_d, _rel(_head(inp, i, h, hide=j)[1], out))
    print(f"kv8 witnesses {name} {dt}: smallest owner probability {worst_p:.6f}, smallest change when the key is removed {worst_d:.3f}")
    assert worst_p >= 0.999 and worst_d > 50 * TOL[dt]
    for i, n in enumerate(lens):
        assert owned[i] == set(kr.boundary_positions(n)), (name, i)


@pytest.mark.parametrize("name", CASES)
def test_boundary_lists_hold_the_first_and_last_key_and_both_sides_of_every_tile_and_split_edge(name):
    b, Hq, Hkv, cap, lens, forms = kr.SHAPES[name]
    for n in lens:
        lst = set(kr.boundary_positions(n))
        assert {0, n - 1} <= lst and all(0 <= j < n for j in lst)
        for sk in [64] + [kr.FORM_SPLIT[f] for f in (forms if forms != (0,) else (1, 3, 11))] + [128, 192, 256, 768]:
            for e in range(sk, n, sk):
                assert {e - 1, e} <= lst, (name, n, sk, e)
    for n in (33, 97, 512):      # the 32-key tiles of the ring form (part f)
        assert {31, 32} <= set(kr.boundary_positions(n, 32))


@pytest.mark.parametrize("dt", DTS)
def test_masked_witnesses(dt):
    inp = kr.case_inputs("masked", "masked", DT[dt])
    kinds = [k for _, k in inp.ties.values()]
    assert kinds.count("leak") == 6 and kinds.count("drop") == 8
    for (i, g, j), (h, kind) in inp.ties.items():
        if kind == "leak":      # hidden: seen, it would own its head and drag the poison in
            assert inp.mask[i, j] == 0
            p, out = _head(inp, i, h, see_all=True)
            assert float(p[j]) >= 0.999 and _rel(out, _head(inp, i, h)[1]) > 50 * TOL[dt]
        else:
            assert inp.mask[i, j] != 0
            p, out = _head(inp, i, h)
            assert float(p[j]) >= 0.999 and _rel(_head(inp, i, h, hide=j)[1], out) > 50 * TOL[dt]
    assert (1, 0, dar.MASK_HOLES[1][0] - 1) in inp.ties and (1, 0, dar.MASK_HOLES[1][0]) in inp.ties


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", list(kr.APPEND_SHAPES))
def test_the_appended_key_owns_its_head_after_rotation_and_quantisation(name, dt):
    b, Hq, Hkv, cap, lens, _ = kr.APPEND_SHAPES[name]
    qkv, inp, owners = kr.append_inputs(name, DT[dt])
    out, k8, ks, v8, vs, k16, v16, qr = kr.decode_append_kv8(qkv, inp.k8, inp.ks, inp.v8, inp.vs, inp.k16, inp.v16, Hq, Hkv, lens, kr.THETA, kr.SCALE, DT[dt],
                                                            rope=kr.rope_rows_T)
    done = inp._replace(q=qr.float(), k8=k8, ks=ks, v8=v8, vs=vs)
    for i, h in enumerate(owners):
        p, o = _head(done, i, h)
        assert float(p[lens[i] - 1]) >= 0.999, (name, i, float(p[lens[i] - 1]))
        assert torch.allclose(o, out[i, h], rtol=1e-12, atol=0)
        if lens[i] > 1:
            assert _rel(_head(done, i, h, hide=lens[i] - 1)[1], o) > 50 * TOL[dt]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", CASES)
def test_a_scale_from_the_neighbouring_key_moves_every_head(name, dt):
    inp = kr.case_inputs(name, "scale", DT[dt])
    assert not bool(torch.isnan(kr.e4m3(inp.k8)).any() | torch.isnan(kr.e4m3(inp.v8)).any())
    ref = kr.attend(inp.q, inp.k8, inp.ks, inp.v8, inp.vs, inp.lens, kr.SCALE)
    bad = kr.shifted_scales(inp)
    err = kr.rel_heads(kr.attend(bad.q, bad.k8, bad.ks, bad.v8, bad.vs, bad.lens, kr.SCALE), ref)
    print(f"kv8 scale witness {name} {dt}: smallest per-head change {float(err.min()):.3f}")
    assert float(err.min()) > 50 * TOL[dt], err


def _calib_worst(name, family, dt, fold=None):
    shape = kr.MASKED_SHAPE if name == "masked" else kr.SHAPES[name]
    forms = shape[5]
    inp = kr.case_inputs(name, family, DT[dt])
    ref = kr.attend(inp.q, inp.k8, inp.ks, inp.v8, inp.vs, inp.lens, kr.SCALE, inp.mask)
    worst = 0.0
    for sk in sorted({64} | {kr.FORM_SPLIT[f] for f in (forms if forms != (0,) else (1, 3, 11))}):
        c = (DT[dt], sk) if fold is None else (DT[dt], sk, fold)
        got = kr.attend(inp.q, inp.k8, inp.ks, inp.v8, inp.vs, inp.lens, kr.SCALE, inp.mask, calib=c)
        worst = max(worst, float(kr.rel_heads(got, ref).max()))
    return worst


@pytest.mark.parametrize("dt", DTS)
def test_operand_rounding_stays_under_half_the_bound(dt):
    """the calibration table of test_gpu_kv8_attn.py's docstring: worst (sequence, head) over the cases of a family, every split size of its forms"""
    table = {}
    for family in kr.FAMILIES:
        names = CASES if family in ("plain", "drop", "scale") else ["tile_edges", "nw4"]
        table[family] = max(_calib_worst(n, family, dt) for n in names)
    table["masked"] = _calib_worst("masked", "masked", dt)
    if dt == "f16":      # the fold as it was (e * vs rounded to f16: subnormal as soon as V rows are small): recorded, not a bound
        table["smallv, plain fold"] = max(_calib_worst(n, "smallv", dt, "plain") for n in ("tile_edges", "nw4"))
    print(f"kv8 calibration {dt} (bound {TOL[dt]:.1e}): " + "  ".join(f"{k} {v:.2e}" for k, v in table.items()))
    for family, worst in table.items():
        if family != "smallv, plain fold":
            assert worst <= TOL[dt] / 2, (family, worst)
    if dt == "f16":
        assert table["smallv, plain fold"] > TOL[dt], "the plain fold no longer misses the bound on small value rows: drop the rescaling"


@pytest.mark.parametrize("nsplit", kr.MERGE_NSPLITS)
def test_merge_owners_and_the_fp32_allowance(nsplit):
    seen = [set() for _ in range(kr.MERGE_ROWS)]
    worst32 = 0.0
    for rnd in range(kr.merge_rounds(nsplit)):
        mc = kr.merge_partials(nsplit, rnd)
        assert mc.ns[0] == nsplit and mc.ns[1] == max(1, nsplit - 1) and mc.ns[2] == 1
        for r in range(kr.MERGE_ROWS):
            ns = mc.ns[r]
            assert bool(torch.isnan(mc.ws[r, :, ns:]).all()) and bool(torch.isfinite(mc.ws[r, :, :ns, :130]).all())
            for h in range(kr.MERGE_HEADS):
                w = mc.ws[r, h]
                m, l, O = w[:, 128], w[:, 129], w[:, :128]
                o = int(mc.owner[r, h])
                seen[r].add(o)
                wt = torch.exp2((m[:ns].double() - m[:ns].double().max()) * mc.c) * l[:ns].double()
                assert float(wt[o] / wt.sum()) >= 0.999
                assert float(l[:ns].min()) >= 1 and float(l[:ns].max()) <= 64
                ref = kr.merge_ref(m, l, O, ns, mc.c)
                assert float(((ref - O[o].double() / l[o].double()) / ref).abs().max()) < 1e-9
                worst32 = max(worst32, float(((kr.merge_ref_fp32(m, l, O, ns, mc.c).double() - ref) / ref).abs().max()))
    for r in range(kr.MERGE_ROWS):
        ns = kr.merge_ns(nsplit)[r]
        assert seen[r] == {s for s in kr.MERGE_OWNED + (ns - 1, ns - 2) if 0 <= s < ns}
    print(f"merge nsplit {nsplit}: fp32 evaluation within {worst32:.2e} of fp64 (allowance 2^-14 = {2.0 ** -14:.2e})")
    assert worst32 <= 2.0 ** -14


def test_merge_ref_without_an_owner_is_the_plain_weighted_mean():
    """the formula itself, on partials none of which dominates: against a direct softmax over the keys the partials stand for"""
    g = torch.Generator().manual_seed(3)
    n, sk = 1000, 64
    s = torch.randn(n, generator=g, dtype=torch.float64) * 3
    v = torch.randn(n, 128, generator=g, dtype=torch.float64)
    ns = -(-n // sk)
    m = torch.stack([s[i * sk:(i + 1) * sk].max() for i in range(ns)])
    e = [torch.exp(s[i * sk:(i + 1) * sk] - m[i]) for i in range(ns)]
    l = torch.stack([x.sum() for x in e])
    O = torch.stack([e[i] @ v[i * sk:(i + 1) * sk] for i in range(ns)])
    got = kr.merge_ref(m / (kr.SCALE), l, O, ns, kr.SCALE * 1.4426950408889634)      # m in raw-score units: the kernels scale it by c
    assert torch.allclose(got, torch.softmax(s, 0) @ v, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("dt", DTS)
def test_rope_rows_T_is_the_oracles_rotation_bit_for_bit(dt):
    """the rotation whose bits the kernels store (cos / sin and both products rounded to T): the oracle's apply_rope on the host table"""
    import oracle
    T = DT[dt]
    pos = torch.tensor([0, 1, 63, 64, 448, 999, 4160])
    x = torch.randn(len(pos), 5, 128, generator=torch.Generator().manual_seed(3)).to(T)
    cos, sin = dar.rope_table(pos, kr.THETA)
    cos, sin = torch.cat((cos, cos), -1).to(T)[:, None, :], torch.cat((sin, sin), -1).to(T)[:, None, :]      # [n, S = 1, 128]
    want, _ = oracle.apply_rope(x[:, :, None, :], x[:, :, None, :], cos, sin)
    got = kr.rope_rows_T(x, pos, kr.THETA, T)
    assert torch.equal(got.view(torch.int16), want[:, :, 0].contiguous().view(torch.int16))
    one = dar.rope_rows(x, pos, kr.THETA, T)
    assert not torch.equal(one, got) and float((one.double() - got.double()).norm() / got.double().norm()) < 3e-3
