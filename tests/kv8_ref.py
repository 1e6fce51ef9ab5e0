"""CPU restatement in fp64 of the decode attention over the e4m3 KV cache (attention.hip: attn_decode_kernel<T, true[, true]>,
attn_decode_kv8_walk_kernel, the fused RoPE + append + quantise step), of the cache quantiser (kv_quant_kernel) and of the split-KV merge
(attn_merge_kernel, attn_merge_mid_kernel), with the inputs that make one wrong key, scale or partial visible: witness builders in the style
of attn_prefill_ref.py.  Plain torch; tests/test_kv8_cpu.py checks all of it before tests/test_gpu_kv8_attn.py judges a kernel with it.

A tied key: k16[b, g, j] = C_SPIKE * q[b, h] BEFORE quantisation -- its score against head h is ~45 nats against ~4 for the runner-up, so head h's
output IS that key's value row: a kernel that drops it, reads its scale from a neighbour or weights its split wrongly misses the head by O(1)."""
import collections
import math
import torch
import decode_append_ref as dar
from decode_append_ref import rope_rows, rel_heads  # noqa: F401

D = 128
KV_TILE = 64
C_SPIKE = 4.0
V_POISON = 1000.0
SCALE = 128 ** -0.5
THETA = 1e6
FORM_SPLIT = {1: 64, 2: 128, 3: 192, 4: 256, 11: 768}      # tuning key 47 -> keys per split (11: four waves x three tiles)
LARGEV_ABSMAX = {torch.float16: 60000.0, torch.bfloat16: 2.0 ** 116}
# bf16: the kernels hold the UN-normalised sum l x V in fp32 (l = sum of exponentials relative to the maximum, up to a few hundred over the
# lengths below, and the merge adds the partials): 2^116 x 2^11 stays finite, 2^128 does not.  The fp64 reference is finite either way.


# ------------------------------------------------------------------------------------------------ quantiser
def quant(x):
    """x [..., 128] -> (e4m3 bytes uint8 [..., 128], scales fp32 [...]): s = absmax / 448 (1 for a zero row), bytes = e4m3_rne(x / s) in fp32"""
    x = x.float()
    m = x.abs().amax(dim=-1)
    s = torch.where(m > 0, m / 448.0, torch.ones_like(m))
    return (x / s[..., None]).to(torch.float8_e4m3fn).view(torch.uint8), s


def e4m3(b8):
    """the values of e4m3 bytes, fp64"""
    return b8.view(torch.float8_e4m3fn).float().double()


def dequant(b8, s):
    return e4m3(b8) * s.double()[..., None]


# ------------------------------------------------------------------------------------------------ attention
def _round(x, T):
    return x.float().to(T).double()


def attend(q, k8, ks, v8, vs, lens, scale, mask=None, calib=None):
    """q [b, Hq, 128], k8 / v8 [b, Hkv, cap, 128] e4m3 bytes, ks / vs [b, Hkv, cap] -> [b, Hq, 128] fp64 on the DE-QUANTISED cache.  Key j of
    sequence i is visible iff j < lens[i] and (mask is None or mask[i][j] != 0); nothing else of the cache is read.
    calib = (T, split_keys[, fold]): NOT the reference -- the kernels' arithmetic where it differs from exact: a running maximum per split over
    64-key tiles, P x value scale rounded to T before the PV product (the MFMA operand), the exponentials summed unrounded, the splits merged
    exactly.  fold: "plain" = e * vs rounded (bf16; f16 before the fold was rescaled), "pow2" = e * (vs / u) rounded with u = the power of two at
    or below the tile's largest value scale, the tile's product multiplied by u in fp32 (f16).  Default: by T."""
    b, Hq, _ = q.shape
    rep = Hq // k8.shape[1]
    out = torch.zeros(b, Hq, D, dtype=torch.float64)
    for i in range(b):
        n = int(lens[i])
        see = torch.ones(n, dtype=torch.bool) if mask is None else mask[i, :n] != 0
        if calib is None:
            for g in range(k8.shape[1]):      # (per kv head: a 33 k-key cache is not repeated per query head)
                hs = slice(g * rep, (g + 1) * rep)
                s = q[i, hs].double() @ dequant(k8[i, g, :n], ks[i, g, :n]).T * scale
                s = torch.where(see[None, :], s, torch.full_like(s, -math.inf))
                e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
                out[i, hs] = e @ dequant(v8[i, g, :n], vs[i, g, :n]) / e.sum(dim=-1, keepdim=True)
            continue
        kk = dequant(k8[i, :, :n], ks[i, :, :n]).repeat_interleave(rep, 0)            # [Hq, n, 128]
        s = torch.einsum("hd,hnd->hn", q[i].double(), kk) * scale
        s = torch.where(see[None, :], s, torch.full_like(s, -math.inf))
        T, split_keys = calib[0], calib[1]
        fold = calib[2] if len(calib) > 2 else ("pow2" if T == torch.float16 else "plain")
        vb = e4m3(v8[i, :, :n]).repeat_interleave(rep, 0)
        vsc = vs[i, :, :n].double().repeat_interleave(rep, 0)                        # [Hq, n]
        parts = []
        for s0 in range(0, n, split_keys):
            m_run = torch.full((Hq, 1), -math.inf, dtype=torch.float64)
            l_run = torch.zeros(Hq, 1, dtype=torch.float64)
            o = torch.zeros(Hq, D, dtype=torch.float64)
            for t0 in range(s0, min(s0 + split_keys, n), KV_TILE):
                t1 = min(t0 + KV_TILE, n)
                if not bool(see[t0:t1].any()):
                    continue
                st = s[:, t0:t1]
                m_new = torch.maximum(m_run, st.max(dim=-1, keepdim=True).values)
                alpha = torch.exp(m_run - m_new)
                e = torch.exp(st - m_new)
                l_run = l_run * alpha + e.sum(dim=-1, keepdim=True)
                if fold == "pow2":
                    u = torch.exp2(torch.floor(torch.log2(vsc[:, t0:t1].max(dim=-1, keepdim=True).values)))
                    o = o * alpha + u * torch.einsum("hn,hnd->hd", _round(e * (vsc[:, t0:t1] / u), T), vb[:, t0:t1])
                else:
                    o = o * alpha + torch.einsum("hn,hnd->hd", _round(e * vsc[:, t0:t1], T), vb[:, t0:t1])
                m_run = m_new
            if bool(torch.isfinite(m_run).all()):
                parts.append((m_run, l_run, o))
        M = torch.stack([p[0] for p in parts]).max(dim=0).values
        num = sum(torch.exp(p[0] - M) * p[2] for p in parts)
        den = sum(torch.exp(p[0] - M) * p[1] for p in parts)
        out[i] = num / den
    return out


def rope_rows_T(x, pos, theta, dtype):
    """rope_rows with the roundings of the model this project restates, which the kernels keep (attn_common.h rope_chunk): cos / sin rounded to
    dtype, each product rounded to dtype, then the sum -- the BITS of a rotated row (rope_rows rounds once: up to an ulp away)"""
    cos, sin = dar.rope_table(pos, theta)
    cos = torch.cat((cos, cos), dim=-1).to(dtype).float()[:, None, :]
    sin = torch.cat((sin, sin), dim=-1).to(dtype).float()[:, None, :]
    x = x.to(dtype).float()
    partner = x[..., torch.arange(D) ^ 64]
    sign = torch.where(torch.arange(D) < 64, -1.0, 1.0)
    return ((x * cos).to(dtype).float() + (sign * partner * sin).to(dtype).float()).to(dtype)


def decode_append_kv8(qkv, k8, ks, v8, vs, k16, v16, Hq, Hkv, lens, theta, scale, dtype, rope=rope_rows):
    """One fused step (attn_decode_kv8_walk_kernel<FUSE>, or rope_kv_kernel with the e4m3 outputs in front of the attention): qkv
    [b, (Hq + 2 Hkv) * 128] raw projections; sequence i holds lens[i] keys counting the new one; q / k rotated at position lens[i] - 1
    (rope_rows: one rounding to dtype), the rotated k row and the raw v row quantised and stored at slot lens[i] - 1 of k8 / v8 / ks / vs, the
    16-bit rows at the same slot of k16 / v16.  rope = rope_rows_T: the bytes the kernels store (their rotation rounds as the model does).  Returns (out fp64 [b, Hq, 128], k8, ks, v8, vs, k16, v16 completed, rotated q).  Slots at and
    beyond lens[i] - 1 of the given caches are never read."""
    q, kn, vn = dar.split_qkv(qkv.to(dtype), Hq, Hkv)
    pos = torch.tensor([int(n) - 1 for n in lens])
    qr = rope(q, pos, theta, dtype)
    kr = rope(kn, pos, theta, dtype)
    k8, ks, v8, vs, k16, v16 = k8.clone(), ks.clone(), v8.clone(), vs.clone(), k16.to(dtype).clone(), v16.to(dtype).clone()
    kb, ksc = quant(kr.float())
    vb, vsc = quant(vn.float())
    for i, n in enumerate(lens):
        k8[i, :, n - 1] = kb[i]; ks[i, :, n - 1] = ksc[i]; v8[i, :, n - 1] = vb[i]; vs[i, :, n - 1] = vsc[i]
        k16[i, :, n - 1] = kr[i]; v16[i, :, n - 1] = vn[i]
    return attend(qr.float(), k8, ks, v8, vs, lens, scale), k8, ks, v8, vs, k16, v16, qr


# ------------------------------------------------------------------------------------------------ the cases of tests/test_gpu_kv8_attn.py
# name -> (b, Hq, Hkv, cap, lens, tuning key 47 forms).  The smallest shapes that reach each branch.
#   tile_edges: one key; a tile one short of full, full, one over; two tiles, two and a key (a walking form's split ends in empty tiles)
#   walk_edges: a split of a walking form ends in an empty tile (127, 129, 193, 257 ...) or starts with one key (129: form 2, 193: form 3, 257: form 4)
#   nw4: a one-key sequence (three dead waves), a full first wave, a second wave with one key, a full split, a second split of one key, a third
#        split that is one tile (1600 = 2 x 768 + 64)
#   nrep16 / nrep1: the largest and the smallest GQA group
#   auto: whatever the launcher picks at default keys
AUTO_LENS = [1040, 1, 577, 64, 1025, 769, 193, 960]
SHAPES = {
    "tile_edges": (6, 8, 2, 256, [1, 63, 64, 65, 128, 129], (1, 2, 3, 4)),
    "walk_edges": (6, 7, 1, 512, [127, 129, 192, 193, 257, 449], (2, 3, 4)),
    "nw4": (6, 4, 2, 1664, [1, 192, 193, 768, 769, 1600], (11,)),
    "nrep16": (2, 16, 1, 256, [65, 200], (1, 3)),
    "nrep1": (2, 2, 2, 256, [65, 200], (1, 3)),
    "auto": (8, 8, 4, 1088, AUTO_LENS, (0,)),
}
MASKED_SHAPE = (4, 4, 2, 256, [200] * 4, (0,))       # decode_append_ref's masked case: MASK_PADS, MASK_HOLES, mask rows of MASK_SB bytes
# the fused append: the shapes of test_gpu_fp8's fused-equals-unfused test that fuse, plus tile_edges; name -> (b, Hq, Hkv, cap, lens, key 47 values)
APPEND_SHAPES = {
    "tile_edges": SHAPES["tile_edges"][:5] + ((3, 11, 0),),
    "three_seq": (3, 8, 2, 1024, [1000, 513, 65], (3, 11, 0)),
    "one_key_and_769": (2, 7, 1, 1024, [769, 1], (3, 11, 0)),
    "b1_2113": (1, 28, 4, 2304, [2113], (3, 11, 0)),
    "b1_33k": (1, 28, 4, 33024, [32900], (0,)),      # long enough for the launcher to pick the folded four-wave form by itself
}
FAMILIES = ("plain", "drop", "scale", "smallv", "largev")

Inputs = collections.namedtuple("Inputs", "q k8 ks v8 vs k16 v16 lens ties mask")
# q [b, Hq, 128] fp32 holding values of the 16-bit type; k8 / v8 uint8, ks / vs fp32; k16 / v16 the 16-bit source (None for `scale`);
# ties {(b, kv head, key): (query head, kind)}, kind "drop" (visible, owned) or "leak" (hidden, poisoned)


def boundary_positions(n, tile=KV_TILE):
    """the keys of a sequence of n keys at which a kernel can go wrong: the first, the last, both sides of every tile edge below n (every
    split edge of every form is one of them: split sizes are multiples of the tile)"""
    pos = {0, n - 1}
    for e in range(tile, n, tile):
        pos |= {e - 1, e}
    return sorted(pos)


def n_rounds(Hq, lens, tile=KV_TILE):
    return max(-(-len(boundary_positions(n, tile)) // Hq) for n in lens)


def drop_plan(Hq, Hkv, lens, rnd, tile=KV_TILE):
    """{(b, kv head, key): query head}: round `rnd` of the round-robin assignment of boundary positions to query heads.  Head h owns entry
    rnd * Hq + h of its sequence's list (wrapping round only where the list is at least Hq long: owners of one kv head own different keys)."""
    rep = Hq // Hkv
    plan = {}
    for b, n in enumerate(lens):
        lst = boundary_positions(n, tile)
        for h in range(Hq):
            idx = rnd * Hq + h
            if idx >= len(lst) and len(lst) < Hq:
                continue
            key = (b, h // rep, lst[idx % len(lst)])
            assert key not in plan
            plan[key] = h
    return plan


def _gauss(shape, dtype, seed):
    b, Hq, Hkv, cap = shape[:4]
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, Hq, D, generator=g).to(dtype).float()
    k = torch.randn(b, Hkv, cap, D, generator=g).to(dtype).float()
    v = torch.randn(b, Hkv, cap, D, generator=g).to(dtype).float()
    return q, k, v, g


def drop_inputs16(shape, dtype, rnd, seed, tile=KV_TILE):
    """(q, k16, v16, ties) of the `drop` family on a 16-bit cache: Gaussian everything, each planned key tied to its owner"""
    b, Hq, Hkv, cap, lens = shape[:5]
    q, k, v, _ = _gauss(shape, dtype, seed)
    ties = {}
    for (i, g, j), h in drop_plan(Hq, Hkv, lens, rnd, tile).items():
        k[i, g, j] = C_SPIKE * q[i, h]
        ties[(i, g, j)] = (h, "drop")
    assert torch.equal(k, k.to(dtype).float())
    return q, k, v, ties


def _quantised(q, k, v, lens, ties, mask=None):
    k8, ks = quant(k)
    v8, vs = quant(v)
    return Inputs(q, k8, ks, v8, vs, k, v, list(lens), ties, mask)


def case_inputs(name, family, dtype, rnd=0):
    """the inputs of a case: the same Gaussians for every family and round, the family's ties / scales / value ranges on top"""
    shape = MASKED_SHAPE if name == "masked" else SHAPES[name]
    b, Hq, Hkv, cap, lens = shape[:5]
    seed = 7000 + 13 * (sorted(SHAPES).index(name) if name in SHAPES else len(SHAPES))
    if name == "masked":
        assert family == "masked"
        q, k, v, _ = _gauss(shape, dtype, seed)
        mask, _ = dar.masked_case_mask()
        rep, ties = Hq // Hkv, {}
        for i in range(b):
            hidden = [j for j in range(lens[i]) if mask[i, j] == 0]
            # leak: a hidden key (the last of the left pad, or a hole); drop: the last visible key in front of a hole, else the first visible one
            leak = hidden[-1] if hidden and i != dar.MASK_HOLES[0] else (dar.MASK_HOLES[1][0] if i == dar.MASK_HOLES[0] else None)
            drop = dar.MASK_HOLES[1][0] - 1 if i == dar.MASK_HOLES[0] else dar.MASK_PADS[i]
            for g in range(Hkv):
                if leak is not None:
                    k[i, g, leak] = C_SPIKE * q[i, g * rep]; v[i, g, leak] = V_POISON
                    ties[(i, g, leak)] = (g * rep, "leak")
                k[i, g, drop] = C_SPIKE * q[i, g * rep + 1]
                ties[(i, g, drop)] = (g * rep + 1, "drop")
        return _quantised(q, k, v, lens, ties, mask)
    assert family in FAMILIES, family
    if family == "drop":
        q, k, v, ties = drop_inputs16(shape, dtype, rnd, seed)
        return _quantised(q, k, v, lens, ties)
    q, k, v, g = _gauss(shape, dtype, seed)
    if family == "plain":
        return _quantised(q, k, v, lens, {})
    if family == "smallv":
        return _quantised(q, k, (v * 2.0 ** -8).to(dtype).float(), lens, {})
    if family == "largev":
        v = (v / v.abs().amax(dim=-1, keepdim=True) * LARGEV_ABSMAX[dtype]).to(dtype).float()
        assert torch.isfinite(v).all()
        return _quantised(q, k, v, lens, {})
    # scale: bytes and scales built directly.  Random finite e4m3 bytes (rms ~100), q scaled so that the scores of the keys with k scale 1 have
    # a standard deviation of ~4 nats: a handful of them share the top of the softmax, and a scale from a neighbouring key (a factor >= 2 in
    # the score, a factor 4 or 1 / 8 in the value row) moves every head
    k8 = torch.randint(0, 254, (b, Hkv, cap, D), generator=g, dtype=torch.uint8)
    v8 = torch.randint(0, 254, (b, Hkv, cap, D), generator=g, dtype=torch.uint8)
    k8 = torch.where(k8 >= 0x7F, k8 + 1, k8); v8 = torch.where(v8 >= 0x7F, v8 + 1, v8)          # 0x7F / 0xFF are NaN
    j = torch.arange(cap)
    ks = torch.exp2(-(j % 7).float()).expand(b, Hkv, cap).contiguous()
    vs = torch.exp2(-((3 * j) % 5).float()).expand(b, Hkv, cap).contiguous()
    q = (q * (4.0 / (100.0 * math.sqrt(D) * SCALE))).to(dtype).float()
    return Inputs(q, k8, ks, v8, vs, None, None, list(lens), {}, None)


def shifted_scales(inp):
    """the `scale` mutant: every key reads its neighbour's scales"""
    return inp._replace(ks=torch.roll(inp.ks, -1, dims=-1), vs=torch.roll(inp.vs, -1, dims=-1))


def append_inputs(name, dtype):
    """(qkv [b, (Hq + 2 Hkv) * 128], Inputs of the cache in front of the step, owner heads [b]): the new key of sequence i is tied to query
    head i % Hq: k_new = C_SPIKE * q_raw of that head (the rotation preserves the product); lens count the new key"""
    b, Hq, Hkv, cap, lens = APPEND_SHAPES[name][:5]
    rep = Hq // Hkv
    seed = 9000 + 17 * sorted(APPEND_SHAPES).index(name)
    q, k, v, g = _gauss((b, Hq, Hkv, cap), dtype, seed)
    kn = torch.randn(b, Hkv, D, generator=g).to(dtype).float()
    vn = torch.randn(b, Hkv, D, generator=g).to(dtype).float()
    owners = [i % Hq for i in range(b)]
    for i, h in enumerate(owners):
        kn[i, h // rep] = C_SPIKE * q[i, h]
    qkv = torch.cat((q.reshape(b, -1), kn.reshape(b, -1), vn.reshape(b, -1)), dim=1)
    return qkv, _quantised(q, k, v, lens, {}), owners


# ------------------------------------------------------------------------------------------------ the split-KV merge
WS_STRIDE = 132
MERGE_NSPLITS = (1, 2, 63, 64, 65, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049)
MERGE_ROWS, MERGE_HEADS, MERGE_SPLIT_KEYS = 3, 8, 64
MERGE_OWNED = (0, 1, 7, 8, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)
MERGE_RAISE = 60.0       # the owner's maximum stands 60 / c above the rest (c = scale * log2 e): its weight is 1 - 2^-60 x the others'


def merge_ref(m, l, O, ns, c):
    """m, l [nsplit], O [nsplit, 128] -> [128] fp64: w_s = 2^((m_s - max m) c), out = sum w_s O_s / sum w_s l_s over s < ns"""
    m, l, O = m[:ns].double(), l[:ns].double(), O[:ns].double()
    w = torch.exp2((m - m.max()) * c)
    return (w[:, None] * O).sum(dim=0) / (w * l).sum()


def merge_ref_fp32(m, l, O, ns, c):
    """the same formula in plain fp32 torch: what fp32 sums of <= 2049 positive terms and exp2 cost (the allowance of the GPU bound)"""
    m, l, O = m[:ns].float(), l[:ns].float(), O[:ns].float()
    w = torch.exp2((m - m.max()) * torch.tensor(c, dtype=torch.float32))
    return (w[:, None] * O).sum(dim=0) / (w * l).sum()


def merge_lens(nsplit):
    """kv_len of the three rows: full length; one split fewer (as far as there is one); one split"""
    sk = MERGE_SPLIT_KEYS
    return [nsplit * sk, max(1, nsplit - 1) * sk - (sk // 2 if nsplit > 1 else 0), 1]


def merge_ns(nsplit):
    return [min(nsplit, -(-n // MERGE_SPLIT_KEYS)) for n in merge_lens(nsplit)]


def merge_rounds(nsplit):
    want = max(len(_merge_owned(ns)) for ns in merge_ns(nsplit))
    return -(-want // MERGE_HEADS)


def _merge_owned(ns):
    return sorted({s for s in MERGE_OWNED + (ns - 1, ns - 2) if 0 <= s < ns})


MergeCase = collections.namedtuple("MergeCase", "ws lens ns owner c")
# ws [rows, heads, nsplit, 132] fp32 (NaN at and beyond a row's ns, and in the two unused floats of a partial); owner [rows, heads] int


def merge_partials(nsplit, rnd=0, scale=SCALE):
    """hand-made partials in the workspace layout.  l_s in [1, 64]; O_s = l_s u_s with u_s in [0.5, 1.5]^128 (positive terms: no
    cancellation); maxima Gaussian, ~+-30; each (row, head) owns one partial index whose m is raised 60 / c above the rest."""
    c = scale * 1.4426950408889634
    g = torch.Generator().manual_seed(11000 + 31 * nsplit + rnd)
    R, H = MERGE_ROWS, MERGE_HEADS
    ws = torch.full((R, H, nsplit, WS_STRIDE), float("nan"), dtype=torch.float32)
    owner = torch.zeros(R, H, dtype=torch.int64)
    lens, nss = merge_lens(nsplit), merge_ns(nsplit)
    for r in range(R):
        ns = nss[r]
        owned = _merge_owned(ns)
        l = 1.0 + 63.0 * torch.rand(H, ns, generator=g)
        u = 0.5 + torch.rand(H, ns, D, generator=g)
        m = 10.0 * torch.randn(H, ns, generator=g)
        for h in range(H):
            o = owned[(rnd * H + h) % len(owned)]
            owner[r, h] = o
            m[h, o] = m[h].max() + MERGE_RAISE / c
        ws[r, :, :ns, :D] = l[..., None] * u
        ws[r, :, :ns, 128] = m
        ws[r, :, :ns, 129] = l
    return MergeCase(ws, lens, nss, owner, c)
