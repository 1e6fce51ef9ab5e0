"""CPU restatement in fp64 of one decode step's attention with the RoPE + append fused in (attention.hip: launch_attn_decode with `rope` set,
the launch every decoder layer issues per token): raw q / k / v rows of the new token, a cache of earlier keys, per-sequence lengths, an optional
key mask.  Plain torch; tests/test_decode_append_cpu.py checks it against the oracle's RoPE and ATen's attention before it judges a kernel
(tests/test_gpu_decode_append.py).  The packed x layout is restated once, in glue_ref."""
import torch
from glue_ref import unpack_x  # noqa: F401  (re-exported: the packed output of the merge is unpacked with the same restatement as the norms')

D = 128


def rope_table(pos, theta):
    """cos, sin [n, 64] fp32 of capi.hip rope_table_device at the integer positions pos [n]: inv = float(1 / theta^(2i / 128)) with the
    exponent formed in fp32, ang = float(p) * inv in fp32, cos / sin evaluated in double and cast to fp32"""
    i2 = torch.arange(0, D, 2, dtype=torch.float32) / torch.tensor(float(D), dtype=torch.float32)      # (float)(2 i) / 128.0f
    inv = (1.0 / torch.pow(torch.tensor(float(theta), dtype=torch.float64), i2.double())).float()
    ang = (pos.to(torch.float32)[:, None] * inv[None, :]).double()
    return ang.cos().float(), ang.sin().float()


def rope_rows(x, pos, theta, dtype):
    """x [n, heads, 128] (values of `dtype`) rotated at pos [n]: rotate-half pairing d <-> d ^ 64 (first half x cos - partner sin, second half
    x cos + partner sin), fp64 arithmetic on the fp32 table, ONE rounding to dtype.  Returns dtype."""
    cos, sin = rope_table(pos, theta)
    cos = torch.cat((cos, cos), dim=-1).double()[:, None, :]
    sin = torch.cat((sin, sin), dim=-1).double()[:, None, :]
    x = x.double()
    partner = x[..., torch.arange(D) ^ 64]
    sign = torch.where(torch.arange(D) < 64, -1.0, 1.0).double()
    return (x * cos + sign * partner * sin).to(dtype)


def split_qkv(qkv, Hq, Hkv):
    """qkv [b, (Hq + 2 Hkv) * 128] -> q [b, Hq, 128], k, v [b, Hkv, 128]"""
    x = qkv.view(qkv.shape[0], Hq + 2 * Hkv, D)
    return x[:, :Hq], x[:, Hq:Hq + Hkv], x[:, Hq + Hkv:]


def attend(q, k, v, lens, scale, mask=None, p_dtype=None):
    """q [b, Hq, 128], k / v [b, Hkv, cap, 128] -> [b, Hq, 128] fp64.  Key j of sequence i is visible iff j < lens[i] and (mask is None or
    mask[i][j] != 0); nothing else of the cache is read.  p_dtype: the probabilities are rounded to it before the PV product and the sum is
    taken over the unrounded ones -- the MFMA operand of the kernels (calibration of the test's bound, not the reference)."""
    b, Hq, _ = q.shape
    rep = Hq // k.shape[1]
    out = torch.zeros(b, Hq, D, dtype=torch.float64)
    for i in range(b):
        n = int(lens[i])
        idx = torch.arange(n)
        if mask is not None:
            idx = idx[mask[i, :n] != 0]
        kk = k[i][:, idx].double().repeat_interleave(rep, 0)            # [Hq, n', 128]
        vv = v[i][:, idx].double().repeat_interleave(rep, 0)
        s = torch.einsum("hd,hnd->hn", q[i].double(), kk) * scale
        e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
        l = e.sum(dim=-1, keepdim=True)
        if p_dtype is not None:
            e = e.to(p_dtype).double()
        out[i] = torch.einsum("hn,hnd->hd", e, vv) / l
    return out


def decode_append(qkv, k, v, Hq, Hkv, lens, pos, theta, scale, dtype, mask=None, p_dtype=None):
    """One step.  qkv [b, (Hq + 2 Hkv) * 128] and the caches k / v [b, Hkv, cap, 128] hold values of `dtype`; sequence i holds lens[i] keys
    counting the new one, whose rows go to slot lens[i] - 1; the RoPE position of row i is pos[i] (unmasked: the slot).  Returns
    (out [b, Hq, 128] fp64, the completed k, v in dtype, rotated q in dtype).  The slots at and beyond lens[i] - 1 of the given caches are
    never read (they may hold NaN)."""
    q, kn, vn = split_qkv(qkv.to(dtype), Hq, Hkv)
    pos = torch.as_tensor(pos)
    qr = rope_rows(q, pos, theta, dtype)
    kr = rope_rows(kn, pos, theta, dtype)
    k2, v2 = k.to(dtype).clone(), v.to(dtype).clone()
    for i in range(qkv.shape[0]):
        k2[i, :, int(lens[i]) - 1] = kr[i]
        v2[i, :, int(lens[i]) - 1] = vn[i]
    return attend(qr, k2, v2, lens, scale, mask, p_dtype), k2, v2, qr


# ------------------------------------------------------------------------------------------------ the cases of tests/test_gpu_decode_append.py
# name -> (b, Hq, Hkv, cap, L, lens or None (= L for every sequence)).  The smallest shapes that reach each branch of the four kernel
# families; which tuning keys a case runs under is the GPU test's business.  Kept here so that the CPU test can measure what operand
# rounding alone costs per head on exactly these inputs (test_decode_append_cpu.py::test_operand_rounding_stays_under_half_the_bound).
RAGGED_ONE_TILE = [1, 2, 63, 64, 65, 128]      # empty cache; new row last in a tile, first in the next tile; a full last tile
SHAPES = {
    "one_tile_ragged_8_2": (6, 8, 2, 128, 128, RAGGED_ONE_TILE),
    "one_tile_ragged_7_1": (6, 7, 1, 128, 128, RAGGED_ONE_TILE),
    "one_tile_ragged_4_2": (6, 4, 2, 128, 128, RAGGED_ONE_TILE),
    "one_tile_ragged_2_2": (6, 2, 2, 128, 128, RAGGED_ONE_TILE),
    "one_tile_L1": (2, 8, 2, 128, 1, None),
    "one_tile_L64": (2, 8, 2, 64, 64, None),          # cap == L: the new row is the last slot of the cache
    "one_tile_L65": (2, 8, 2, 128, 65, None),
    # key 10 = 4 (256-key splits): owner in the first tile; in the last tile of a split; in the second split's first tile; in a split
    # whose tile loop ends early (449 = 256 + 3 tiles + 1 key: tile 3 of split 1 holds the new key alone)
    "multi4_ragged": (4, 8, 2, 512, 449, [1, 256, 257, 449]),
    "multi2_ragged": (4, 8, 2, 256, 193, [129, 192, 193, 64]),      # key 10 = 2 (128-key splits)
    "multi4_uniform": (2, 8, 2, 512, 321, None),      # key 10 = 4, kv_len = NULL: owner = first row of the second split's second tile
    # the ring form's 32-key tiles: the lens of test_batched_decode_attention_dma_ring_* shifted onto tile edges
    "ring_ragged": (5, 7, 1, 512, 512, [1, 32, 33, 97, 512]),
    "ring_wrap": (16, 8, 4, 1024, 1000, None),        # several tiles per split at one slot per CU: the ring wraps
    "auto_66_splits": (1, 28, 4, 4224, 4161, None),   # default keys: 66 one-tile splits, the owner is the last, the 65..256-split merge
    "masked": (4, 4, 2, 256, 200, None),
    "packed_nb1": (5, 8, 2, 128, 128, [1, 64, 65, 128, 17]),
    "packed_nb2": (20, 8, 2, 128, 128, [1 + (37 * i) % 128 for i in range(20)]),
}
MASK_SB = 256
MASK_PADS = [0, 5, 64, 130]      # left pads of the masked case: none, inside tile 0, one whole tile hidden, two whole tiles (and two keys) hidden
MASK_HOLES = (1, [70, 71, 100, 127, 128, 198])      # (row, hidden keys in the middle of it)


def case_inputs(name, dtype):
    """(qkv [b, (Hq + 2 Hkv) * 128], k, v [b, Hkv, cap, 128], lens [b]) of a case, fp32 values rounded to dtype; the caches are random
    everywhere (the GPU test poisons the slots that must not be read)"""
    b, Hq, Hkv, cap, L, lens = SHAPES[name]
    seed = 1000 + 7 * sorted(SHAPES).index(name)
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(b, (Hq + 2 * Hkv) * D, generator=g).to(dtype).float()
    k = torch.randn(b, Hkv, cap, D, generator=g).to(dtype).float()
    v = torch.randn(b, Hkv, cap, D, generator=g).to(dtype).float()
    return qkv, k, v, (list(lens) if lens is not None else [L] * b)


def masked_case_mask():
    """(mask uint8 [b, MASK_SB], pos [b]) of the masked case: left pads, one row with holes, the new key visible, zero beyond L;
    pos = sum(mask) - 1 (omchat_arch.py: the RoPE position of a padded row is its count of real tokens, not its slot)"""
    b, _, _, _, L, _ = SHAPES["masked"]
    mask = torch.zeros(b, MASK_SB, dtype=torch.uint8)
    for i, pad in enumerate(MASK_PADS):
        mask[i, pad:L] = 1
    mask[MASK_HOLES[0], MASK_HOLES[1]] = 0
    mask[:, L - 1] = 1
    return mask, (mask.sum(1) - 1).to(torch.int32)


def rel_heads(got, ref):
    """relative Frobenius error per (sequence, query head): got, ref [b, Hq, 128] -> [b, Hq]"""
    got = got.detach().cpu().double(); ref = ref.detach().cpu().double()
    return (got - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-30)
