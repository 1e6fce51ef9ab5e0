"""CPU: tests/attn_prefill_ref.py (the fp64 restatement and the witness inputs that judge the prefill attention kernels per output row in
test_gpu_attn_prefill_rows.py) against independent formulations -- ATen's scaled_dot_product_attention, glue_ref.attn_left -- and the two
measurements that say whether that test's inputs are fair, binding on every case of the table:
  * what rounding the MFMA operand (the probabilities) and the output to the 16-bit type costs per row: at most half of the bound;
  * what a mask wrong by ONE key costs in the rows that witness it: more than ten times the bound, for each mutant of the reference, and no
    row with an in-range boundary key is left without a witness."""
import functools
import math
import pytest
import torch
import torch.nn.functional as F

import attn_prefill_ref as apr
import glue_ref
from gpu_util import DT, TOL

DTS = ["bf16", "f16"]


@functools.lru_cache(maxsize=None)
def _ref(name, family, dt):
    case = apr.CASES[name]
    inp = apr.case_inputs(name, family, DT[dt])
    return inp, apr.attend(inp.q, inp.k, inp.v, apr.case_scale(case), case.causal, case.q_pos0, case.kv_len, case.kv_start)


def test_case_table_holds_what_the_gpu_test_needs():
    c = apr.CASES
    assert [c[f"nrep{n}"].Hq for n in range(2, 10)] == list(range(2, 10)) and all(c[f"nrep{n}"].Hkv == 1 for n in range(2, 10))
    assert (c["gqa_7_1_s161"].Sq % 32, c["gqa_7_1_s161"].Skv % 64) == (1, 33)
    assert -(-c["hsplit_7_1_s513"].Sq // 32) >= 16                     # launch_attn_prefill forces the head split from 16 query blocks
    assert [apr.peels(c["mha_s129_lens"], n) for n in c["mha_s129_lens"].kv_len] == [True, False, True]
    for case in c.values():
        assert case.Skv >= case.Sq + case.q_pos0 if case.causal else case.Skv >= 1
        assert case.kv_len is None or (len(case.kv_len) == case.b and all(1 <= n <= case.Skv for n in case.kv_len))
        assert case.kv_start is None or (len(case.kv_start) == case.b and all(0 <= s < case.Skv for s in case.kv_start))
        assert case.api in ("prefill", "prefill_d", "left", "mha_fwd", "mha_varlen") and (case.D == 128 or case.api in ("prefill_d", "mha_varlen"))


@pytest.mark.parametrize("family", apr.FAMILIES)
@pytest.mark.parametrize("name", list(apr.CASES))
def test_attend_against_independent_formulations(name, family):
    case = apr.CASES[name]
    inp, got = _ref(name, family, "f16")
    scale = apr.case_scale(case)
    if case.kv_len is None and case.kv_start is None:
        rep = case.Hq // case.Hkv
        allow = torch.ones(case.Sq, case.Skv, dtype=torch.bool)
        if case.causal:
            allow = allow.tril(diagonal=case.q_pos0)
        want = F.scaled_dot_product_attention(inp.q.double().transpose(1, 2), inp.k.double().repeat_interleave(rep, 1),
                                              inp.v.double().repeat_interleave(rep, 1), attn_mask=allow, scale=scale).transpose(1, 2)
    else:
        lo, hi = apr._bounds(case.b, case.Skv, case.kv_len, case.kv_start)
        want = glue_ref.attn_left(inp.q, inp.k, inp.v, scale, case.causal, case.q_pos0, hi, lo)
    assert torch.isfinite(got).all()
    err = (got - want).abs().amax(dim=-1) / want.abs().amax(dim=-1).clamp_min(1.0)
    assert float(err.max()) < 1e-12, (name, family, float(err.max()))
    assert bool((got[inp.zero] == 0).all())


@pytest.mark.parametrize("dt", DTS)
def test_inputs_tie_each_boundary_key_to_its_row(dt):
    """the ties as the issue states them, read back from the tensors: a tied key is C_SPIKE x the query row it concerns, its score is ~45 nats
    at head dim 128, leak ties are hidden from their row and drop ties are visible to it and own its softmax"""
    for name, case in apr.CASES.items():
        n_rep = case.Hq // case.Hkv
        vis = apr.visible(case.b, case.Sq, case.Skv, case.causal, case.q_pos0, case.kv_len, case.kv_start)
        plain = apr.case_inputs(name, "plain", DT[dt])
        assert not plain.ties
        for family in ("leak", "drop"):
            inp, ref = _ref(name, family, dt)
            assert torch.equal(inp.q, plain.q)
            if not inp.ties:           # nothing is hidden: not causal, every key of the buffer valid
                assert family == "leak" and not case.causal and case.kv_len is None and case.kv_start is None
                continue
            heads = set()
            for (b, g, j), (i, h) in inp.ties.items():
                assert h == g * n_rep + j % n_rep and bool(inp.compared[b, i])
                assert torch.equal(inp.k[b, g, j], apr.C_SPIKE * inp.q[b, i, h])
                assert bool(vis[b, i, j]) == (family == "drop")
                heads.add(h)
                if family == "drop":       # the tied key owns the row: the output is its value row
                    assert float(apr.row_rel(ref[b, i, h], inp.v[b, g, j])) < 1e-3, (name, b, i, h)
            if case.causal and case.Sq >= 2 * n_rep:
                assert heads == set(range(case.Hq)), (name, family, "a head of the group never witnesses")
            score = torch.tensor([float(inp.k[b, g, j] @ inp.q[b, i, h]) for (b, g, j), (i, h) in inp.ties.items()]) * apr.case_scale(case)
            # ~45 nats at head dim 128 (C_SPIKE * 128 * 128^-0.5), ~32 at 64; the weakest still clears twice the 2^8 of the lazy rescale
            assert float(score.min()) > 2 * 8 * math.log(2), (name, family, float(score.min()))
            assert not case.causal or abs(float(score.median()) - apr.C_SPIKE * case.D * apr.case_scale(case)) < 5, (name, family, float(score.median()))
            lo, hi = apr._bounds(case.b, case.Skv, case.kv_len, case.kv_start)
            for b in range(case.b):
                hidden = torch.cat((inp.v[b, :, :lo[b]], inp.v[b, :, hi[b]:]), dim=1)
                assert family != "leak" or bool((hidden == apr.V_POISON).all())


@pytest.mark.parametrize("dt", DTS)
def test_operand_rounding_stays_under_half_the_bound(dt):
    """The GPU test holds every (sequence, row, head) to TOL[dt].  The kernels feed the PV MFMA probabilities rounded to T and round the output
    to T: neither is an error of the kernel.  On the GPU test's own inputs both together must leave at least half of the bound in every row
    -- else the inputs have to change, not the bound."""
    T = DT[dt]
    worst = {f: 0.0 for f in apr.FAMILIES}
    for name, case in apr.CASES.items():
        for family in apr.FAMILIES:
            inp, ref = _ref(name, family, dt)
            rounded = apr.attend(inp.q, inp.k, inp.v, apr.case_scale(case), case.causal, case.q_pos0, case.kv_len, case.kv_start, p_dtype=T)
            rr = apr.row_rel(rounded.to(T), ref)
            rr[~inp.compared] = 0
            e = float(rr.max())
            assert e <= TOL[dt] / 2, (name, family, e)
            worst[family] = max(worst[family], e)
    print(f"operand rounding {dt}: worst row_rel over all cases, " + ", ".join(f"{f} {worst[f]:.2e}" for f in apr.FAMILIES) + f"; bound {TOL[dt]:.1e}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mutant", list(apr.MUTANTS))
def test_one_key_mutants_are_far_outside_the_bound(dt, mutant):
    """A reference whose mask is wrong by one key -- the causal limit, kv_len or kv_start moved either way, the peeled key lost -- on the
    family whose ties witness that direction: every tied (row, head) whose visibility the mutant changes is off by more than 10 x TOL[dt],
    and every row (causal limit) / every sequence (kv_len, kv_start) the mutant changes has such a tie in every kv head."""
    family = apr.MUTANTS[mutant]
    smallest, shown = float("inf"), 0
    for name, case in apr.CASES.items():
        mvis = apr.mutant_visible(case, mutant)
        if mvis is None:
            continue
        inp, ref = _ref(name, family, dt)
        vis = apr.visible(case.b, case.Sq, case.Skv, case.causal, case.q_pos0, case.kv_len, case.kv_start)
        diff = (vis != mvis) & inp.compared[:, :, None]                            # [b, Sq, Skv]
        if not bool(diff.any()):
            continue
        rr = apr.row_rel(apr.attend_visible(inp.q, inp.k, inp.v, apr.case_scale(case), mvis), ref)
        witnesses = [(b, g, j, i, h) for (b, g, j), (i, h) in inp.ties.items() if bool(diff[b, i, j])]
        for b, g, j, i, h in witnesses:
            assert float(rr[b, i, h]) > 10 * TOL[dt], (name, mutant, "sequence, row, head", (b, i, h), float(rr[b, i, h]))
            smallest = min(smallest, float(rr[b, i, h]))
        tied = {(b, g, j, i) for b, g, j, i, h in witnesses}
        if mutant.startswith("causal"):            # the changed key is the row's own
            for b, i, j in diff.nonzero().tolist():
                assert all((b, g, j, i) in tied for g in range(case.Hkv)), (name, mutant, "row without a witness", (b, i, j))
        else:                                       # one changed key per sequence
            for b in range(case.b):
                keys = diff[b].any(dim=0).nonzero().flatten().tolist()
                assert len(keys) <= 1
                for j in keys:
                    assert all(any((b, g, j, i) in tied for i in range(case.Sq)) for g in range(case.Hkv)), (name, mutant, "sequence without a witness", (b, j))
        shown += 1
    assert shown > 0, mutant
    print(f"mutant {mutant} on the {family} family, {dt}: {shown} cases show it, smallest row_rel over all witnessing (row, kv head) {smallest:.2f}; 10 x bound {10 * TOL[dt]:.1e}")


def test_pack_qkv_is_the_flash_attention_layout():
    inp = apr.case_inputs("packed_varlen_d64", "drop", torch.float16)
    qkv = apr.pack_qkv(inp.q, inp.k, inp.v)
    case = apr.CASES["packed_varlen_d64"]
    assert qkv.shape == (case.b, case.Sq, 3, case.Hq, case.D) and qkv.is_contiguous()
    assert torch.equal(qkv[1, 7, 0, 1], inp.q[1, 7, 1]) and torch.equal(qkv[1, 7, 1, 1], inp.k[1, 1, 7]) and torch.equal(qkv[1, 7, 2, 0], inp.v[1, 0, 7])
