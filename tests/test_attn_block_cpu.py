"""CPU: tests/attn_block_ref.py proved before tests/test_gpu_attn_block_rows.py judges attn_verify_kernel with it -- the restatement against the
older references of each mode, the witness inputs (no key tied twice, every tied (row, head) compared and, in the drop family, owning exactly
one key), what operand rounding costs per (row, head) on exactly the inputs the GPU test uses, and what every one-slot mutant of the visibility
moves on them."""
import functools

import pytest
import torch

import attn_block_ref as abr
import attn_prefill_ref as apr
import group_ref as gr
import suffix_ref as sfr
from gpu_util import DT, TOL

DTS = ("bf16", "f16")


@functools.lru_cache(maxsize=None)
def _inputs(name, family, dt):
    return abr.case_inputs(name, family, DT[dt])


@functools.lru_cache(maxsize=None)
def _ref(name, family, dt):
    inp = _inputs(name, family, dt)
    return abr.attend(inp.q, inp.k, inp.v, inp.vis)


def _agree(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("family", abr.FAMILIES)
def test_restatement_agrees_with_the_older_references(family):
    """on the same inputs, to fp64 round-off: attn_prefill_ref.attend with q_pos0 = L (verify, extend), suffix_ref.attn_suffix_ref (suffix),
    suffix_ref.attn_shared_lens_ref and group_ref.attn_shared_ref (shared, with and without lengths)"""
    worst = 0.0
    for name, case in abr.CASES.items():
        if case.mode == abr.VERIFY and case.L > 4000 and family != "drop":
            continue                                     # (the two long cases once)
        inp, mine = _inputs(name, family, "bf16"), _ref(name, family, "bf16")
        if case.mode in (abr.VERIFY, abr.EXTEND):
            keys = case.L + case.S
            other = apr.attend(inp.q[None], inp.k[:, :, :keys], inp.v[:, :, :keys], abr.SCALE, 1, case.L, None, None)[0]
        elif case.mode == abr.SUFFIX:
            q4 = inp.q.view(case.N, case.S, case.Hq, abr.D)
            other = sfr.attn_suffix_ref(q4, inp.k, inp.v, case.P, case.lens).reshape(-1, case.Hq, abr.D)
        elif case.lens is None:
            other = gr.attn_shared_ref(inp.q, inp.k, inp.v, case.G, case.N, case.P, case.L)
        else:
            other = sfr.attn_shared_lens_ref(inp.q, inp.k, inp.v, case.G, case.N, case.P, case.lens)
        e = _agree(mine[inp.compared], other[inp.compared])
        worst = max(worst, e)
        assert e < 1e-12, (name, family, e)
    print(f"\n{family}: restatement against the older references, worst max-abs difference / max-abs {worst:.1e}")


def test_case_table_reaches_its_branches():
    """the plan of every case at 256 CUs (attention.hip's formulas restated): the multi-tile cases get their tiles, every other case one tile
    per split; the table holds what the issue of these tests names"""
    for name, case in abr.CASES.items():
        pl = abr.plan_of(case)
        for field, least in case.want:
            assert pl[field] >= least, (name, pl)
        if not case.want:
            assert pl["tpw"] == 1 and pl["tps"] <= 1, (name, pl)
        print(f"{name}: {pl}")
    by_mode = lambda m: [c for c in abr.CASES.values() if c.mode == m]
    reps = lambda m: {c.Hq // c.Hkv for c in by_mode(m)}
    assert reps(abr.VERIFY) >= {1, 2, 7, 8} and {c.S for c in by_mode(abr.VERIFY)} >= {1, 9, 16}
    assert reps(abr.EXTEND) >= {1, 4, 5, 8} and {c.S for c in by_mode(abr.EXTEND)} >= {1, 17, 33}
    for m in (abr.VERIFY, abr.EXTEND):
        assert {c.L % 64 for c in by_mode(m)} >= {0, 1, 62, 63}
    sh = by_mode(abr.SHARED)
    assert {c.N for c in sh} >= {1, 2, 16} and {c.G for c in sh} >= {1, 2} and {c.P % 64 for c in sh} >= {0, 1, 63}
    assert any(c.N * (c.Hq // c.Hkv) > 64 for c in sh) and any(c.N * (c.Hq // c.Hkv) <= 64 for c in sh)
    assert any(c.lens is None for c in sh) and any(c.lens and {n - c.P for n in c.lens} >= {1, 64, 65, 130} for c in sh)
    sx = by_mode(abr.SUFFIX)
    assert {c.N for c in sx} >= {1, 3} and {c.P % 64 for c in sx} >= {0, 1, 63} and any(c.S % 16 and c.N > 1 for c in sx)
    assert any({1, 16, 17, c.S} <= set(c.lens) | {c.S} and 16 in c.lens and 17 in c.lens for c in sx)
    for m in (abr.VERIFY, abr.EXTEND, abr.SHARED, abr.SUFFIX):
        assert any(("tpw", 2) in c.want for c in by_mode(m)), m
    assert sum(("tpw", 2) in c.want for c in by_mode(abr.VERIFY)) >= 2
    assert any(("tps", 2) in c.want and ("nss", 2) in c.want for c in sx)


# ------------------------------------------------------------------------------------------------ the witnesses
def test_ties_are_well_formed():
    """no key is tied to two rows (case_inputs asserts it while it builds), every tied (row, head) is a compared one; drop: the key is visible to
    its row and the (row, head) owns no other; leak: the key is hidden from its row; every head index of a GQA group witnesses somewhere"""
    heads = {}
    for name, case in abr.CASES.items():
        n_rep = case.Hq // case.Hkv
        for family in ("drop", "leak"):
            inp = _inputs(name, family, "bf16")
            assert inp.ties, (name, family)
            owners = {}
            for (b, g, j), (r, h) in inp.ties.items():
                assert bool(inp.compared[r]), (name, family, "a tied row that is not compared", r)
                assert h == g * n_rep + j % n_rep
                assert bool(inp.vis[r, b, j]) == (family == "drop"), (name, family, b, j, r)
                heads.setdefault((n_rep, family), set()).add(h % n_rep)
                if family == "drop":
                    assert owners.setdefault((r, h), (b, j)) == (b, j), (name, "one (row, head) owns two keys", r, h)
            if family == "leak":          # the poison sits exactly on the slots nobody sees
                assert torch.equal((inp.v == abr.V_POISON).all(dim=-1).all(dim=1), ~inp.vis.any(dim=0)), name
    for (n_rep, family), hs in heads.items():
        assert hs == set(range(n_rep)), (n_rep, family, hs)


@pytest.mark.parametrize("dt", DTS)
def test_operand_rounding_stays_under_half_the_bound(dt):
    """The GPU test holds every defined (row, head) to TOL[dt].  The kernel feeds the PV MFMA probabilities rounded to T and the merge rounds the
    output to T; that alone, on every input the GPU test uses, must stay at or below half the bound"""
    worst = {}
    for name, case in abr.CASES.items():
        for family in abr.FAMILIES:
            inp = _inputs(name, family, dt)
            cal = abr.attend(inp.q, inp.k, inp.v, inp.vis, p_dtype=DT[dt]).to(DT[dt])
            e = float(abr.row_rel(cal, _ref(name, family, dt))[inp.compared].max())
            worst[family] = max(worst.get(family, 0.0), e)
            assert e <= TOL[dt] / 2, (name, family, e)
    print(f"\noperand rounding {dt}: worst (row, head) over all cases, " + ", ".join(f"{f} {worst[f]:.2e}" for f in abr.FAMILIES)
          + f"; bound {TOL[dt]:.1e}")


@pytest.mark.parametrize("mutant", list(abr.MUTANTS))
def test_every_mutant_moves_a_witness(mutant):
    """a kernel wrong by one slot in the way the mutant names misses at least one TIED (row, head) of at least one case by more than 0.5 in the
    family that witnesses it -- no mutant goes without a case that can show it"""
    family = abr.MUTANTS[mutant][0]
    shown, best = [], 0.0
    for dt in DTS:
        for name, case in abr.CASES.items():
            inp = _inputs(name, family, dt)
            got = abr.mutant_output(case, inp, mutant)
            if got is None:
                continue
            rr = abr.row_rel(got, _ref(name, family, dt))
            wit = abr.witness_mask(case, inp) & inp.compared[:, None]
            moved = float(rr[wit].max()) if bool(wit.any()) else 0.0
            if moved > 0.5:
                shown.append(f"{name}/{dt}")
            best = max(best, moved)
    print(f"\nmutant {mutant} ({family}): largest move of a witness head {best:.2f}; shown by {len(shown)} case x type: {', '.join(shown[:8])}"
          + (" ..." if len(shown) > 8 else ""))
    assert shown, (mutant, "no case shows it", best)
    if mutant == "last_tile_of_split_not_walked":      # every multi-tile case shows it, prefix and suffix walks alike
        for name, case in abr.CASES.items():
            if case.want:
                assert f"{name}/bf16" in shown and f"{name}/f16" in shown, (mutant, name)
    assert {s.split("/")[1] for s in shown} == set(DTS), (mutant, "not shown in both types")
