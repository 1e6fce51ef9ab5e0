"""CPU restatement in fp64 of the prefill attention (attention.hip: launch_attn_prefill -- attn_kernel, attn2_kernel and their GQA / head-dim /
key-group instantiations), the inputs that make a mask wrong by ONE key visible in ONE output row, and the table of shapes that
tests/test_gpu_attn_prefill_rows.py runs.  Plain torch; tests/test_attn_prefill_cpu.py checks the restatement against ATen and glue_ref, and
measures on exactly these inputs what operand rounding costs per row and what each one-key mutant of the mask costs, before a kernel is judged.

Visibility (kernels.h AttnArgs): key j is visible to query row i of sequence b iff kv_start[b] <= j < kv_len[b] and (not causal or
j <= i + q_pos0).

Witness inputs.  q, k, v are Gaussian at scale 1, rounded to the 16-bit type.  A boundary key j is then TIED to the row i it concerns:
k[b, g, j] = C_SPIKE * q[b, i, g * n_rep + j % n_rep] (C_SPIKE = 4 is a power of two: no rounding), whose score against that (row, head) is
C_SPIKE * |q|^2 * scale ~ 45 nats at head dim 128 -- the key owns that row's softmax if it is visible and must leave no trace if it is not.
  leak   the tied key is the FIRST HIDDEN one: above the causal limit (j = i + q_pos0 + 1, every row), the key at kv_len[b], the key at
         kv_start[b] - 1 (launches with a kv_start).  Every key hidden by length or start also carries v = V_POISON.
  drop   the tied key is the LAST VISIBLE one: the causal limit itself (j = i + q_pos0, every row), kv_len[b] - 1, kv_start[b]: the row's
         output is essentially v[j], and the running maximum jumps by far more than 2^8 in the last key tile the row walks.
  plain  no ties.
The witnessing query head rotates with j, so every head of a GQA group witnesses in some row."""
import collections
import torch

C_SPIKE = 4.0
V_POISON = 1000.0
FAMILIES = ("plain", "leak", "drop")
KV_TILE = 64


# ------------------------------------------------------------------------------------------------ the restatement
def _bounds(b, Skv, kv_len, kv_start):
    hi = [Skv] * b if kv_len is None else [int(x) for x in kv_len]
    lo = [0] * b if kv_start is None else [int(x) for x in kv_start]
    return lo, hi


def visible(b, Sq, Skv, causal, q_pos0, kv_len, kv_start):
    """bool [b, Sq, Skv]: key j visible to row i of sequence b"""
    lo, hi = _bounds(b, Skv, kv_len, kv_start)
    j = torch.arange(Skv)[None, None, :]
    i = torch.arange(Sq)[None, :, None]
    vis = (j >= torch.tensor(lo)[:, None, None]) & (j < torch.tensor(hi)[:, None, None])
    if causal:
        vis = vis & (j <= i + q_pos0)
    return vis.expand(b, Sq, Skv)


def attend_visible(q, k, v, scale, vis, p_dtype=None):
    """q [b, Sq, Hq, D], k / v [b, Hkv, Skv, D], vis bool [b, Sq, Skv] -> [b, Sq, Hq, D] fp64; a row without a visible key gives 0.
    p_dtype: the probabilities are rounded to it before the PV product and the sum is taken over the unrounded ones -- the MFMA operand of the
    kernels (calibration of the test's bound, not the reference)."""
    rep = q.shape[2] // k.shape[1]
    kk = k.double().repeat_interleave(rep, 1)                                  # [b, Hq, Skv, D]
    vv = v.double().repeat_interleave(rep, 1)
    s = torch.einsum("bihd,bhjd->bhij", q.double(), kk) * scale
    s = s.masked_fill(~vis[:, None], -float("inf"))
    m = s.amax(dim=-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    l = e.sum(dim=-1, keepdim=True)
    if p_dtype is not None:
        e = e.to(p_dtype).double()
    o = torch.einsum("bhij,bhjd->bhid", e, vv) / l.clamp_min(1e-300)
    return o.permute(0, 2, 1, 3).contiguous()


def attend(q, k, v, scale, causal, q_pos0, kv_len, kv_start, p_dtype=None):
    """the reference: fp64 on inputs already rounded to the 16-bit type.  kv_len / kv_start: per-sequence lists or None (Skv / 0)."""
    b, Sq, Skv = q.shape[0], q.shape[1], k.shape[2]
    return attend_visible(q, k, v, scale, visible(b, Sq, Skv, causal, q_pos0, kv_len, kv_start), p_dtype)


def row_rel(got, ref):
    """||got - ref||_2 / ||ref||_2 over the D columns of one (sequence, row, head): [b, Sq, Hq, D] -> [b, Sq, Hq]"""
    got = got.detach().cpu().double(); ref = ref.detach().cpu().double()
    return (got - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-30)


# ------------------------------------------------------------------------------------------------ the cases
# api: which entry point the GPU test calls (omchat_op_attn_prefill | _d | _left, omchat_mha_fwd | _varlen: the last two take the same
# q / k / v packed as qkv [B, S, 3, H, D]).  kv_len / kv_start: per-sequence lists or None.  Which tuning keys a case runs under is the GPU
# test's business (GROUPS there); the shapes are the smallest that reach each branch.
Case = collections.namedtuple("Case", "name api b Hq Hkv Sq Skv D causal q_pos0 kv_len kv_start")
LEFT_STARTS = [0, 63, 64, 65]                  # none; just before, on and just after a 64-key tile edge
LEFT_LENS = [130, 130, 100, 130]


def _cases():
    c = [
        # 1. GQA on the second-generation kernel (32-query blocks, 64-key tiles), causal
        Case("gqa_7_1_s161", "prefill", 1, 7, 1, 161, 161, 128, 1, 0, None, None),                 # a one-row last block, a 33-key last tile
        Case("gqa_4_2_suffix", "prefill", 2, 4, 2, 97, 162, 128, 1, 65, [162, 130], None),        # causal and length limits in one tile walk
        Case("gqa_8_1_tile_edges", "prefill", 1, 8, 1, 64, 128, 128, 1, 64, None, None),          # every limit on a tile edge
    ]
    c += [Case(f"gqa_4_2_qpos{p}", "prefill", 1, 4, 2, 66, 66 + p, 128, 1, p, None, None) for p in (1, 63, 64)]
    # 2. every GQA instantiation (n_rep 2..8), and 9 = the first-generation kernel's GQA path
    c += [Case(f"nrep{n}", "prefill", 1, n, 1, 97, 97, 128, 1, 0, None, None) for n in range(2, 10)]
    c += [
        # 3. head split of the heaviest causal blocks: 17 query blocks
        Case("hsplit_7_1_s513", "prefill", 1, 7, 1, 513, 513, 128, 1, 0, None, None),
        # 4. MHA on the second-generation kernel, not causal: 129 and 65 keys take the peeled-key path, 128 does not
        Case("mha_s129", "prefill", 3, 2, 2, 129, 129, 128, 0, 0, None, None),
        Case("mha_s129_lens", "prefill", 3, 2, 2, 129, 129, 128, 0, 0, [129, 128, 65], None),
        # 5. MHA causal (the three-dimensional grid)
        Case("mha_causal_qpos0", "prefill", 1, 3, 3, 130, 130, 128, 1, 0, None, None),
        Case("mha_causal_qpos63", "prefill", 1, 3, 3, 130, 193, 128, 1, 63, None, None),
        # 6. head dim 64
        Case("d64_mha", "prefill_d", 1, 3, 3, 130, 130, 64, 0, 0, None, None),
        Case("d64_mha_causal", "prefill_d", 1, 3, 3, 130, 130, 64, 1, 0, None, None),
        Case("d64_gqa_4_2_causal", "prefill_d", 1, 4, 2, 130, 130, 64, 1, 0, None, None),
    ]
    # 8. left-padded batches, alone and combined with kv_len
    for Hq, Hkv in ((7, 1), (3, 3)):
        for causal in (1, 0):
            for lens in (None, LEFT_LENS):
                name = f"left_{Hq}_{Hkv}_{'causal' if causal else 'full'}{'_lens' if lens else ''}"
                c.append(Case(name, "left", 4, Hq, Hkv, 130, 130, 128, causal, 0, lens, LEFT_STARTS))
    # 9. the packed-qkv seam
    for causal in (0, 1):
        sfx = "_causal" if causal else ""
        c.append(Case("packed_mha" + sfx, "mha_fwd", 2, 2, 2, 129, 129, 128, causal, 0, None, None))
        c.append(Case("packed_varlen_d128" + sfx, "mha_varlen", 2, 2, 2, 129, 129, 128, causal, 0, [129, 65], None))
        c.append(Case("packed_varlen_d64" + sfx, "mha_varlen", 2, 2, 2, 129, 129, 64, causal, 0, [129, 65], None))
    return collections.OrderedDict((x.name, x) for x in c)


CASES = _cases()


def case_scale(case):
    return 128 ** -0.5 if case.D == 128 else 0.125


Inputs = collections.namedtuple("Inputs", "q k v ties compared zero")
# q [b, Sq, Hq, D], k / v [b, Hkv, Skv, D]: fp32 holding values of the 16-bit type.  ties: {(b, kv head, key): (row, query head)}.
# compared bool [b, Sq]: rows held to the bound; zero bool [b, Sq]: rows without a visible key (the kernels leave exactly 0 there).
# Rows at or beyond kv_len[b] of a sequence with a length are unspecified: in neither.


def _tie_plan(case, family):
    """[(b, key, row)]: which row each boundary key is tied to"""
    lo, hi = _bounds(case.b, case.Skv, case.kv_len, case.kv_start)
    Sq, p0 = case.Sq, case.q_pos0
    plan = []
    for b in range(case.b):
        n_rows = min(Sq, hi[b]) if case.kv_len is not None else Sq             # compared rows are [0, n_rows)
        start_row = max(0, lo[b] - p0) if case.causal else min(lo[b], Sq - 1)  # causal: the first row that sees a key at all
        len_row = min(hi[b], Sq) - 1                                           # not causal: any row would do
        cand = []
        if family == "leak":
            if case.causal:
                cand += [(i + p0 + 1, i) for i in range(n_rows) if lo[b] <= i + p0 + 1 < hi[b]]
            cand.append((hi[b], max(0, hi[b] - p0) if case.causal else len_row))       # causal: the first row whose limit lies beyond kv_len
            start_key = lo[b] - 1
        elif family == "drop":
            if case.causal:
                cand += [(i + p0, i) for i in range(n_rows) if lo[b] <= i + p0 < hi[b]]
            cand.append((hi[b] - 1, max(0, hi[b] - 1 - p0) if case.causal else len_row))   # causal: the first row whose limit reaches the last key
            start_key = lo[b]
        if family != "plain" and case.kv_start is not None:                    # the lower limit is witnessed where the launch has one
            cand.append((start_key, start_row))
        for j, i in cand:
            sees_a_key = lo[b] < hi[b] and (not case.causal or i + p0 >= lo[b])    # (a row that sees none is exactly 0, not a witness)
            if 0 <= j < case.Skv and 0 <= i < n_rows and sees_a_key:
                plan.append((b, j, i))
    return plan


def case_inputs(name, family, dtype):
    """the inputs of a case: the same Gaussians for every family, the family's ties and poison on top"""
    case = CASES[name]
    assert family in FAMILIES
    gen = torch.Generator().manual_seed(4000 + 11 * list(CASES).index(name))
    q = torch.randn(case.b, case.Sq, case.Hq, case.D, generator=gen).to(dtype).float()
    k = torch.randn(case.b, case.Hkv, case.Skv, case.D, generator=gen).to(dtype).float()
    v = torch.randn(case.b, case.Hkv, case.Skv, case.D, generator=gen).to(dtype).float()
    n_rep = case.Hq // case.Hkv
    lo, hi = _bounds(case.b, case.Skv, case.kv_len, case.kv_start)
    ties = {}
    for b, j, i in _tie_plan(case, family):
        for g in range(case.Hkv):
            h = g * n_rep + j % n_rep
            assert ties.get((b, g, j), (i, h)) == (i, h), (name, family, "one key tied to two rows", b, j)
            ties[(b, g, j)] = (i, h)
            k[b, g, j] = C_SPIKE * q[b, i, h]
    if family == "leak":
        for b in range(case.b):
            v[b, :, hi[b]:] = V_POISON
            v[b, :, :lo[b]] = V_POISON
    assert torch.equal(k, k.to(dtype).float()) and torch.equal(v, v.to(dtype).float())
    vis = visible(case.b, case.Sq, case.Skv, case.causal, case.q_pos0, case.kv_len, case.kv_start)
    in_range = torch.ones(case.b, case.Sq, dtype=torch.bool)
    if case.kv_len is not None:
        in_range = torch.arange(case.Sq)[None, :] < torch.tensor(hi)[:, None]
    sees = vis.any(dim=-1)
    return Inputs(q, k, v, ties, in_range & sees, in_range & ~sees)


def pack_qkv(q, k, v):
    """q [B, S, H, D], k / v [B, H, S, D] -> qkv [B, S, 3, H, D] (FlashAttention.forward's operand)"""
    return torch.stack((q, k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)), dim=2).contiguous()


# ------------------------------------------------------------------------------------------------ one-key mutants of the mask
# name -> (family whose ties witness it, what it does to the arguments).  "+1" mutants show a key too many (leak), "-1" a key too few (drop).
MUTANTS = {
    "causal+1": "leak", "kv_len+1": "leak", "kv_start-1": "leak",
    "causal-1": "drop", "kv_len-1": "drop", "kv_start+1": "drop", "peel_dropped": "drop",
}


def peels(case, kv_len_b):
    """attn2_kernel's peeled last key: MHA, head dim 128, not causal, no left padding, one key over whole tiles"""
    return (case.Hq == case.Hkv and case.D == 128 and not case.causal and case.kv_start is None and kv_len_b > KV_TILE
            and kv_len_b % KV_TILE == 1)


def mutant_visible(case, mutant):
    """the visibility of a kernel whose mask is wrong by one key in the way `mutant` names (None: this case cannot show it)"""
    lo, hi = _bounds(case.b, case.Skv, case.kv_len, case.kv_start)
    p0 = case.q_pos0
    if mutant in ("causal+1", "causal-1"):
        if not case.causal:
            return None
        p0 += 1 if mutant == "causal+1" else -1
    elif mutant == "kv_len+1":
        hi = [min(x + 1, case.Skv) for x in hi]
    elif mutant == "kv_len-1":
        hi = [x - 1 for x in hi]
    elif mutant in ("kv_start-1", "kv_start+1") and case.kv_start is None:
        return None
    elif mutant == "kv_start-1":
        lo = [max(x - 1, 0) for x in lo]
    elif mutant == "kv_start+1":
        lo = [x + 1 for x in lo]
    elif mutant == "peel_dropped":
        if not any(peels(case, x) for x in hi):
            return None
        hi = [x - 1 if peels(case, x) else x for x in hi]
    else:
        raise KeyError(mutant)
    return visible(case.b, case.Sq, case.Skv, case.causal, p0, hi, lo)
