"""CPU restatement in fp64 of the split-KV block attention (attention.hip: attn_verify_kernel in its four modes behind launch_attn_block --
ATTN_VERIFY, ATTN_EXTEND, ATTN_SHARED, ATTN_SUFFIX), the inputs that make ONE wrong key visible in ONE (query row, head), the one-slot mutants of
the visibility, and the table of shapes that tests/test_gpu_attn_block_rows.py runs.  Plain torch; tests/test_attn_block_cpu.py checks the
restatement against the older references and measures on exactly these inputs what operand rounding costs and what each mutant moves, before a
kernel is judged.  The style and the helpers are attn_prefill_ref.py's and kv8_ref.py's.

Visibility (kernels.h, the four contracts), over (flat query row, cache row, slot):
  verify / extend   one cache row; query row t (position L + t) sees slots 0 .. L + t
  shared            G groups of N rows; row r sees slots [0, P) of its group's first row and slots [P, len_r) of its own
  suffix            N rows of S tokens; flat row j S + t, t < len_j, sees slots [0, P) of row 0 and slots [P, P + t] of row j; the rows
                    t >= len_j are padding (computed from the row's valid keys, not compared)

Witness inputs.  Everything Gaussian at scale 1, rounded to the 16-bit type.  A boundary key in slot j of cache row b is TIED to one flat query
row r: k[b, g, j] = C_SPIKE * q[r, g * n_rep + j % n_rep] for every kv head g, ~45 nats against ~4 for the runner-up.
  drop   the tied key is the LAST VISIBLE one at a boundary: every row's diagonal key (L + t; P + t; len_r - 1), the first own key P, the last
         prompt key P - 1, key 0, the last cached key L - 1, both sides of a tile edge inside a multi-tile split and of a split edge.  A (row,
         head) owns at most one key; a boundary key whose head is taken in every candidate row stays Gaussian.
  leak   the tied key is the FIRST HIDDEN one: slot L + t + 1 (in verify: the next new row of the same launch), slot len_r of the row itself,
         the leader's slot P as a sibling would see it through the prefix, a sibling's slot P - 1.  Every slot that no row sees holds V_POISON.
  plain  no ties.
The two modes with a fused RoPE + append (verify, shared) are built from RAW rows: qkv [rows, (Hq + 2 Hkv) * 128] as the qkv projection leaves
them, rotated here with the kernels' roundings (kv8_ref.rope_rows_T).  A tie on an appended slot is made on the raw rows (k_new = 4 * q_raw: the
rotation is linear and the factor a power of two, so a key tied to the row it is appended for stays tied bit for bit; a key tied to ANOTHER row is
rotated at another position and keeps the low-frequency half of the product, still tens of nats), a tie on a cached slot on the rotated q."""
import collections

import torch

from attn_prefill_ref import C_SPIKE, KV_TILE, V_POISON, row_rel  # noqa: F401
from kv8_ref import boundary_positions, rope_rows_T

D = 128
SCALE = D ** -0.5
THETA = 1e6
CUS = 256                      # the CU count the case table is derived for (MI355X)
SFX_SPLITS = 4
VERIFY, EXTEND, SHARED, SUFFIX = 0, 1, 2, 3
FAMILIES = ("plain", "drop", "leak")

# lens: shared -- the rows' true lengths [G N] or None (every row holds L keys, the no-lengths form); suffix -- the valid tokens of each row [N].
# want: ((plan field, least value), ...): the branch the case was chosen for
Case = collections.namedtuple("Case", "name mode Hq Hkv G N S P L lens want")


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the launcher's plan (attention.hip)
def plan_of(case, cus=CUS):
    """{tpw, nsp, nss, tps} of attn_block_plan on a device with `cus` CUs"""
    Hkv = case.Hkv
    if case.mode == VERIFY:
        keys = case.L + case.S
        tpw = max(1, min(8, cdiv(cdiv(keys, KV_TILE) * Hkv, 2 * cus)))
        return dict(tpw=tpw, nsp=cdiv(keys, KV_TILE * tpw), nss=0, tps=0)
    if case.mode == EXTEND:
        chunks, tiles = cdiv(case.S, 16), cdiv(case.L + case.S, KV_TILE)
        want = max(1, 2 * cus // max(1, chunks * Hkv))
        tpw = max(1, cdiv(tiles, want))
        return dict(tpw=tpw, nsp=cdiv(tiles, tpw), nss=0, tps=0)
    tiles = cdiv(case.P, KV_TILE)
    if case.mode == SHARED:
        want = max(1, 2 * cus // max(1, case.G * Hkv))
        tpw = max(1, cdiv(tiles, want))
        return dict(tpw=tpw, nsp=cdiv(tiles, tpw), nss=cdiv(case.L - case.P, KV_TILE), tps=0)
    chunks, stiles = cdiv(case.N * case.S, 16), cdiv(case.S, KV_TILE)
    want = max(1, 2 * cus // max(1, chunks * Hkv))
    tpw = max(1, cdiv(tiles, want))
    tps = max(1, cdiv(stiles, SFX_SPLITS))
    return dict(tpw=tpw, nsp=cdiv(tiles, tpw), nss=cdiv(stiles, tps), tps=tps)


# ------------------------------------------------------------------------------------------------ geometry
def n_rows(case):
    return {VERIFY: case.S, EXTEND: case.S, SHARED: case.G * case.N, SUFFIX: case.N * case.S}[case.mode]


def n_cache_rows(case):
    return {VERIFY: 1, EXTEND: 1, SHARED: case.G * case.N, SUFFIX: case.N}[case.mode]


def cap_of(case):
    """slots per cache row: room for the first hidden slot of every row, and (shared) for a grid sized for L + 70"""
    return {VERIFY: case.L + case.S + 2, EXTEND: case.L + case.S + 2, SHARED: case.L + 72, SUFFIX: case.P + case.S + 2}[case.mode]


def row_lens(case):
    return list(case.lens) if case.lens is not None else [case.L] * n_rows(case)


def fuses(case):
    return case.mode in (VERIFY, SHARED)


def new_slots(case):
    """the fused forms: [(cache row, slot)] that flat row r appends to; the slot is also the RoPE position of the row"""
    if case.mode == VERIFY:
        return [(0, case.L + t) for t in range(case.S)]
    return [(r, n - 1) for r, n in enumerate(row_lens(case))]


def compared_rows(case):
    """bool [rows]: the rows the contract defines"""
    c = torch.ones(n_rows(case), dtype=torch.bool)
    if case.mode == SUFFIX:
        c = (torch.arange(case.S)[None, :] < torch.tensor(case.lens)[:, None]).reshape(-1)
    return c


def visibility(case, plan=None, dc=0, dpp=0, dps=0, dl=0, dchunk=0, skip=False, nolast=False):
    """bool [flat query row, cache row, slot].  The keyword arguments are the one-slot mutants (MUTANTS): dc moves the causal bound, dpp the end
    of the prompt on the prefix side, dps the start of the own keys, dl the rows' lengths, dchunk the bound of a 16-row chunk (L + NT); skip: the
    causal bound is not applied in the tile that ends at L + 2 (the condition `key0 + 64 > L + 1` off by one); nolast: the last tile of a split
    of several tiles is not walked.  `plan` (default: 256 CUs) matters to nolast only."""
    pl = plan or plan_of(case)
    R, B, cap = n_rows(case), n_cache_rows(case), cap_of(case)
    vis = torch.zeros(R, B, cap, dtype=torch.bool)
    slot = torch.arange(cap)

    def walked(lo, per):
        if not nolast or per < 2:
            return torch.ones(cap, dtype=torch.bool)
        return ((slot - lo) // KV_TILE) % per != per - 1

    P, L, S, N = case.P, case.L, case.S, case.N
    if case.mode in (VERIFY, EXTEND):
        w = walked(0, pl["tpw"])
        for t in range(S):
            t0 = t // 16 * 16 if case.mode == EXTEND else 0
            NT = min(16, S - t0) if case.mode == EXTEND else S
            hi = L + t + dc
            if dchunk:
                hi = min(hi, L + t0 + NT - 1 + dchunk)
            if skip and (L + t0 + 2) % KV_TILE == 0:
                hi = max(hi, min(L + t0 + 1, L + t0 + NT - 1))
            vis[t, 0] = (slot <= hi) & w
    elif case.mode == SHARED:
        lens = row_lens(case)
        pre = (slot < P + dpp) & walked(0, pl["tpw"])
        for r in range(R):
            vis[r, r // N * N] |= pre
            vis[r, r] |= (slot >= P + dps) & (slot < lens[r] + dl)
    else:
        pre = (slot < P + dpp) & walked(0, pl["tpw"])
        own = (slot >= P + dps) & walked(P, pl["tps"])
        for j in range(N):
            for t in range(S):
                c16 = t // 16 * 16
                hi = min(P + t + dc, P + case.lens[j] - 1 + dl)
                if dchunk:
                    hi = min(hi, P + c16 + min(16, S - c16) - 1 + dchunk)
                vis[j * S + t, 0] |= pre
                vis[j * S + t, j] |= own & (slot <= hi)
    return vis


def attend(q, k, v, vis, p_dtype=None):
    """the reference: q [rows, Hq, 128], k / v [cache rows, Hkv, cap, 128] (values of the 16-bit type), vis bool [rows, cache rows, cap]
    -> [rows, Hq, 128] fp64, evaluated on q's device; a row without a visible key gives 0.  p_dtype: the probabilities are rounded to it before
    the PV product and the sum is taken over the unrounded ones -- the MFMA operand of the kernel (calibration of the bound, not the reference)."""
    R, Hq, _ = q.shape
    B, Hkv, cap, _ = k.shape
    rep = Hq // Hkv
    seen = vis.to(q.device).reshape(R, 1, B * cap)
    out = torch.zeros(R, Hq, D, dtype=torch.float64, device=q.device)
    for g in range(Hkv):
        kk = k[:, g].double().reshape(B * cap, D)
        vv = v[:, g].double().reshape(B * cap, D)
        s = torch.einsum("rhd,jd->rhj", q[:, g * rep:(g + 1) * rep].double(), kk) * SCALE
        s = s.masked_fill(~seen, -float("inf"))
        m = s.amax(dim=-1, keepdim=True)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        e = torch.exp(s - m)
        l = e.sum(dim=-1, keepdim=True)
        if p_dtype is not None:
            e = e.to(p_dtype).double()
        vv = torch.where(seen[:, 0].any(dim=0)[:, None], vv, torch.zeros_like(vv))      # (a slot nobody sees: 0 x poison, not 0 x NaN)
        out[:, g * rep:(g + 1) * rep] = torch.einsum("rhj,jd->rhd", e, vv) / l.clamp_min(1e-300)
    return out


# ------------------------------------------------------------------------------------------------ the cases
def _v(name, Hq, Hkv, T, L, want=()):
    return Case(name, VERIFY, Hq, Hkv, 0, 0, T, 0, L, None, want)


def _e(name, Hq, Hkv, Sq, L, want=()):
    return Case(name, EXTEND, Hq, Hkv, 0, 0, Sq, 0, L, None, want)


def _s(name, Hq, Hkv, G, N, P, own, want=()):
    """own: the own keys of each row, cycled over the G N rows (with lengths), or one int (every row: the no-lengths form)"""
    if isinstance(own, int):
        return Case(name, SHARED, Hq, Hkv, G, N, 0, P, P + own, None, want)
    lens = [P + own[r % len(own)] for r in range(G * N)]
    return Case(name, SHARED, Hq, Hkv, G, N, 0, P, max(lens), lens, want)


def _x(name, Hq, Hkv, N, S, P, lens, want=()):
    assert len(lens) == N and all(1 <= n <= S for n in lens)
    return Case(name, SUFFIX, Hq, Hkv, 0, N, S, P, 0, list(lens), want)


HEADS = {1: (2, 2), 2: (4, 2), 4: (8, 2), 5: (10, 2), 7: (14, 2), 8: (16, 2)}      # n_rep -> (Hq, Hkv): two kv heads everywhere
L_EDGES = (128, 65, 126, 191)              # L % 64 = 0, 1, 62, 63
OWN = (1, 64, 65, 130)


def _cases():
    c = []
    # verify: the four-wave form (T n_rep <= 64) and the eight-wave form; loader-only waves (T n_rep = 9, 18, 63, 72: below 16 NW and no
    # multiple of 16); every L % 64 with every n_rep
    i = 0
    for n_rep in (1, 2, 7, 8):
        for T in (1, 9, 16):
            c.append(_v(f"verify_r{n_rep}_t{T}", *HEADS[n_rep], T, L_EDGES[i % 4] + 64 * (i % 3)))
            i += 1
    c += [
        _v("verify_empty_cache", 4, 2, 16, 0),
        # 66 tiles x 8 kv heads > 512: two tiles per split; the new rows 4150 .. 4165 straddle the tile edge 4160 INSIDE the split [4096, 4224)
        _v("verify_tpw2_tile", 16, 8, 16, 4150, (("tpw", 2),)),
        # 131 tiles x 4 kv heads > 512; the new rows 8312 .. 8327 straddle the SPLIT edge 8320 = 65 x 128
        _v("verify_tpw2_split", 28, 4, 16, 8312, (("tpw", 2),)),
    ]
    # extend: a partial last chunk of 1 row (Sq = 1, 17, 33); n_rep 5 and 8 take the eight-wave form
    i = 0
    for n_rep in (1, 4, 5, 8):
        for Sq in (1, 17, 33):
            c.append(_e(f"extend_r{n_rep}_s{Sq}", *HEADS[n_rep], Sq, L_EDGES[(i + 1) % 4] + 64 * (i % 2)))
            i += 1
    # 16 chunks x 4 kv heads: 8 splits wanted over 13 tiles -> two tiles per split; the early chunks leave neutral partials in the late splits
    c.append(_e("extend_tpw2", 8, 4, 256, 513, (("tpw", 2),)))
    # shared: N n_rep on both sides of 64; P % 64 = 0, 1, 63; own lengths mixed within a group; the no-lengths form
    c += [
        _s("shared_n2_p64", 28, 4, 1, 2, 64, (1, 130)),
        _s("shared_g2_n16_p65", 28, 4, 2, 16, 65, OWN),                  # 112 query rows: eight waves
        _s("shared_g2_n16_p63", 4, 2, 2, 16, 63, OWN),
        _s("shared_n16_r8_p128", 8, 1, 1, 16, 128, OWN),                 # 128 query rows
        _s("shared_g2_n1_p65", 7, 1, 2, 1, 65, (64, 65)),
        _s("shared_r1_p1", 2, 2, 1, 2, 1, (130, 1)),
        _s("shared_nolens_n2", 28, 4, 1, 2, 64, 65),
        _s("shared_nolens_g2_n16", 4, 2, 2, 16, 63, 1),
        _s("shared_nolens_n16_r8", 8, 1, 1, 16, 65, 130),
        # 8 groups x 8 kv heads: 8 prefix splits wanted over 9 tiles -> two tiles per prefix split
        _s("shared_tpw2", 32, 8, 8, 2, 575, (1, 65), (("tpw", 2),)),
    ]
    # suffix: S no multiple of 16 (a flat 16-row prefix chunk crosses a sibling border); lengths 1, 16, 17, S; P % 64 = 0, 1, 63
    c += [
        _x("suffix_n3_s21", 28, 4, 3, 21, 64, (21, 1, 17)),
        _x("suffix_n3_s35", 4, 2, 3, 35, 65, (16, 35, 17)),
        _x("suffix_n1_s70", 8, 1, 1, 70, 63, (70,)),                     # two suffix splits of one tile
        _x("suffix_r1_p1", 2, 2, 3, 17, 1, (17, 16, 1)),
        _x("suffix_r5_p128", 10, 2, 3, 19, 128, (1, 19, 16)),
        # five suffix tiles: three splits, two tiles each (the causal and the length bound inside the tile walk)
        _x("suffix_tps2", 4, 2, 4, 300, 65, (300, 257, 65, 1), (("tps", 2), ("nss", 2))),
        # 7 chunks x 8 kv heads: 9 prefix splits wanted over 11 tiles -> two tiles per prefix split
        _x("suffix_tpw2", 16, 8, 3, 33, 641, (33, 17, 1), (("tpw", 2),)),
    ]
    return collections.OrderedDict((x.name, x) for x in c)


CASES = _cases()


# ------------------------------------------------------------------------------------------------ ties
def _edge_keys(n, tpw):
    """the keys of a walk over n keys in splits of tpw tiles at which it can go wrong: key 0, key n - 1, both sides of the first and the last
    tile edge INSIDE a split (the running-maximum jump across tt > 0) and of the first and the last split edge"""
    if n < 1:
        return []
    tiles = [j for j in boundary_positions(n, KV_TILE) if j not in (0, n - 1)]
    splits = set(boundary_positions(n, KV_TILE * tpw))
    inner = [j for j in tiles if j not in splits]
    outer = [j for j in tiles if j in splits]
    keys = [n - 1, 0]
    for lst in (inner, outer):
        keys += lst[:2] + lst[-2:]
    return [j for j in dict.fromkeys(keys) if 0 <= j < n]


class _Plan:
    def __init__(self, n_rep, exclusive):
        self.n_rep, self.exclusive, self.keys, self.owned = n_rep, exclusive, {}, set()

    def tie(self, b, j, rows):
        """slot j of cache row b goes to the first of `rows` whose head j % n_rep owns nothing yet (leak: to the first)"""
        if (b, j) in self.keys:
            return
        for r in rows:
            if not self.exclusive or (r, j % self.n_rep) not in self.owned:
                self.keys[(b, j)] = r
                self.owned.add((r, j % self.n_rep))
                return


def _rot(rows, i):
    i %= len(rows)
    return rows[i:] + rows[:i]


def tie_plan(case, family):
    """{(cache row, slot): flat query row}"""
    assert family in FAMILIES
    if family == "plain":
        return {}
    drop = family == "drop"
    pl = plan_of(case)
    p = _Plan(case.Hq // case.Hkv, drop)
    P, L, S, N = case.P, case.L, case.S, case.N
    if case.mode in (VERIFY, EXTEND):
        for t in range(S):
            p.tie(0, L + t + (0 if drop else 1), [t])
        if drop:
            for i, j in enumerate(_edge_keys(L, pl["tpw"])):
                p.tie(0, j, _rot(list(range(S)), 5 * i + 1))
    elif case.mode == SHARED:
        lens = row_lens(case)
        for r, n in enumerate(lens):      # the diagonal keys first, then the prompt's edges, then the edges of the own keys
            p.tie(r, n - 1 if drop else n, [r])
            if not drop and r % N:
                p.tie(r, P - 1, [r])
        for lead in range(0, case.G * N, N):
            group = list(range(lead, lead + N))
            if drop:
                for i, j in enumerate(_edge_keys(P, pl["tpw"])):
                    p.tie(lead, j, _rot(group, i + 1))
            elif N > 1:
                p.tie(lead, P, [lead + 1])
        for r, n in enumerate(lens if drop else ()):
            for j in [P] + [e + d for e in range(P + KV_TILE, n, KV_TILE) for d in (-1, 0)]:
                p.tie(r, j, [r])
    else:
        valid = [j * S + t for j in range(N) for t in range(case.lens[j])]
        for j in range(N):
            for t in range(case.lens[j]):
                p.tie(j, P + t + (0 if drop else 1), [j * S + t])
            if not drop and j:
                p.tie(j, P - 1, [j * S])
        if drop:
            for i, j in enumerate(_edge_keys(P, pl["tpw"])):
                p.tie(0, j, _rot(valid, 7 * i + 3))
        elif N > 1:
            p.tie(0, P, [S])
    return p.keys


# ------------------------------------------------------------------------------------------------ inputs
Inputs = collections.namedtuple("Inputs", "q k v vis compared ties qkv k0 v0 pos")
# q [rows, Hq, 128], k / v [cache rows, Hkv, cap, 128]: fp32 holding values of the 16-bit type -- what the attention itself reads (q rotated, the
# caches complete).  ties {(cache row, kv head, slot): (flat row, query head)}.  The fused forms (verify, shared) also have qkv [rows, (Hq + 2 Hkv)
# * 128] raw, k0 / v0 the caches BEFORE the step (the appended slots hold other Gaussians) and pos [rows] (RoPE position = appended slot); the
# others None.


def case_inputs(name, family, dtype):
    """the inputs of a case: the same Gaussians for every family, the family's ties and poison on top"""
    case = CASES[name]
    R, B, cap, Hq, Hkv = n_rows(case), n_cache_rows(case), cap_of(case), case.Hq, case.Hkv
    n_rep = Hq // Hkv
    gen = torch.Generator().manual_seed(6000 + 13 * list(CASES).index(name))
    rnd = lambda *shape: torch.randn(*shape, generator=gen).to(dtype).float()
    q_raw, k, v = rnd(R, Hq, D), rnd(B, Hkv, cap, D), rnd(B, Hkv, cap, D)
    q, kn, vn, pos, fresh = q_raw, None, None, None, {}
    if fuses(case):
        kn, vn = rnd(R, Hkv, D), rnd(R, Hkv, D)
        slots = new_slots(case)
        pos = torch.tensor([s for _, s in slots])
        fresh = {bs: r for r, bs in enumerate(slots)}
        q = rope_rows_T(q_raw, pos, THETA, dtype).float()
    ties = {}
    for (b, j), r in tie_plan(case, family).items():
        for g in range(Hkv):
            h = g * n_rep + j % n_rep
            assert (b, g, j) not in ties, (name, family, "one key tied twice", b, j)
            ties[(b, g, j)] = (r, h)
            if (b, j) in fresh:
                kn[fresh[(b, j)], g] = C_SPIKE * q_raw[r, h]
            else:
                k[b, g, j] = C_SPIKE * q[r, h]
    vis = visibility(case)
    if family == "leak":
        v = torch.where(vis.any(dim=0)[:, None, :, None], v, torch.full_like(v, V_POISON))
    k0, v0, qkv = None, None, None
    if fuses(case):
        k0, v0 = k.clone(), v.clone()
        kr = rope_rows_T(kn, pos, THETA, dtype).float()
        for (b, j), r in fresh.items():
            k[b, :, j] = kr[r]
            v[b, :, j] = vn[r]
        qkv = torch.cat((q_raw.reshape(R, -1), kn.reshape(R, -1), vn.reshape(R, -1)), dim=1)
    assert torch.equal(k, k.to(dtype).float()) and torch.equal(v, v.to(dtype).float()) and torch.equal(q, q.to(dtype).float())
    return Inputs(q, k, v, vis, compared_rows(case), ties, qkv, k0, v0, pos)


def witness_mask(case, inp):
    """bool [rows, Hq]: the tied (row, head) pairs"""
    m = torch.zeros(n_rows(case), case.Hq, dtype=torch.bool)
    for r, h in inp.ties.values():
        m[r, h] = True
    return m


# ------------------------------------------------------------------------------------------------ one-slot mutants
# name -> (the family whose ties witness it, what it changes)
MUTANTS = collections.OrderedDict([
    ("causal+1", ("leak", dict(dc=1))),
    ("causal-1", ("drop", dict(dc=-1))),
    ("P+1_prefix_side", ("leak", dict(dpp=1))),
    ("P-1_prefix_side", ("drop", dict(dpp=-1))),
    ("P-1_suffix_side", ("leak", dict(dps=-1))),
    ("P+1_suffix_side", ("drop", dict(dps=1))),
    ("len+1", ("leak", dict(dl=1))),
    ("len-1", ("drop", dict(dl=-1))),
    ("chunk_bound-1", ("drop", dict(dchunk=-1))),
    ("bound_skipped_in_tile_ending_at_L+2", ("leak", dict(skip=True))),
    ("last_tile_of_split_not_walked", ("drop", dict(nolast=True))),
    ("new_key_from_cache_slot", ("drop", None)),
])


def mutant_output(case, inp, mutant):
    """what a kernel wrong in the way `mutant` names computes on these inputs, [rows, Hq, 128] fp64 -- or None where this case cannot show it
    (the compared rows see the same keys)"""
    change = MUTANTS[mutant][1]
    if change is None:
        return attend(inp.q, inp.k0, inp.v0, inp.vis) if fuses(case) else None
    vis = visibility(case, **change)
    if torch.equal(vis[inp.compared], inp.vis[inp.compared]):
        return None
    return attend(inp.q, inp.k, inp.v, vis)
