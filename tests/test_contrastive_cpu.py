"""CPU: the restatement of contrastive search (tests/contrastive_ref.py) against a literal transcription of HF 4.4x's _ranking_fast; the
witness inputs of the GPU op tests -- every witness owns its candidate's penalty and every one-row mutant moves it by far more than the op
bound (calibration printed); the mode rule, the parameter resolution and every refusal from host data (omchat_amd/contrastive.py); and, on
the tiny decoder's oracle, a prompt whose contrastive ids differ from its greedy ids, so that tests/test_gpu_contrastive.py cannot pass on
greedy output."""
import types

import numpy as np
import pytest
import torch

import contrastive_ref as cr
from omchat_amd import contrastive as cs
from omchat_amd import synth
from omchat_amd.config import tiny

CUS = 256      # an MI355X


# ---------------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("k", cr.OP_K)
@pytest.mark.parametrize("L,H", [(1, 128), (65, 128), (257, 256)])
def test_restatement_equals_ranking_fast(L, H, k):
    rng = np.random.default_rng(L * 100 + k)
    hist = cr.bf16_round(rng.standard_normal((L, H)).astype(np.float32))
    cand = cr.bf16_round(rng.standard_normal((k, H)).astype(np.float32))
    z = cr.logits_inputs(2049, k, seed=L)
    _, p = cr.topk_probs(z, k)
    ctx = torch.from_numpy(hist).double()[None].expand(k, L, H)
    sel, pen = cr.ranking_fast(ctx, torch.from_numpy(cand).double()[:, None, :], torch.from_numpy(p)[None], torch.ones(k, L, dtype=torch.float64),
                               cr.ALPHA, k)
    mine = cr.penalties(hist, cand)
    assert np.abs(pen.numpy() - mine).max() < 1e-12
    assert int(sel[0]) == cr.pick(p, mine, cr.ALPHA)[0]
    # fp32, as HF runs it, gives the same pick on these inputs (the scores are far apart)
    sel32, _ = cr.ranking_fast(ctx.float(), torch.from_numpy(cand)[:, None, :], torch.from_numpy(p.astype(np.float32))[None], torch.ones(k, L), cr.ALPHA, k)
    if cr.pick(p, mine, cr.ALPHA)[1] > 1e-5:
        assert int(sel32[0]) == int(sel[0])


def test_topk_ties_go_to_the_lower_id_and_probabilities_sum():
    z = np.array([1.0, 3.0, 3.0, 2.0, 3.0, -1.0], np.float32)
    ids, p = cr.topk_probs(z, 4)
    assert ids.tolist() == [1, 2, 4, 3]
    full = np.exp(z.astype(np.float64) - 3.0); full /= full.sum()
    assert np.allclose(p, full[ids], rtol=0, atol=1e-15)
    for V in cr.OP_V:
        z = cr.logits_inputs(V, 16)
        ids, p = cr.topk_probs(z, 16)
        assert ids[:3].tolist() == sorted([7, V - 1, min(V - 2, 2047)]) and sorted(ids[3:5].tolist()) == [3, V // 2]
        assert (np.diff(z[ids]) <= 0).all() and len(set(ids.tolist())) == 16
        t = torch.topk(torch.from_numpy(z), 16)
        assert np.array_equal(np.sort(t.values.numpy()), np.sort(z[ids]))
        dev, tol = cr.probs_bound(z, 16)
        print(f"top-k V={V}: fp32 numpy deviates {dev:.3e}, bound {tol:.3e}")
        assert 0 < tol < 1e-6


def test_pick_takes_the_first_maximum():
    p = np.array([0.25, 0.25, 0.25], np.float64)
    assert cr.pick(p, np.array([0.5, 0.5, 0.5]), 0.6)[0] == 0
    assert cr.pick(p, np.array([0.5, 0.2, 0.2]), 0.6) == (1, 0.0)
    assert cr.pick(np.array([0.9, 0.05]), np.array([1.0, 0.1]), 0.6)[0] == 1      # the likelier id repeats the context
    assert cr.pick(np.array([0.9, 0.05]), np.array([1.0, 0.1]), 0.1)[0] == 0


# ---------------------------------------------------------------------------------------------------------------- plan, witnesses, mutants
def test_plan_covers_every_row_once():
    for cus in (1, 8, 256, 304):
        for L in list(cr.OP_L) + [16, 17, 4096, 16384, 16385, cr.OP_L_TWO_GROUPS, 70000]:
            chunks, rpc = cr.plan(L, cus)
            assert rpc % 16 == 0 and (chunks - 1) * rpc < L <= chunks * rpc and chunks <= max(4 * cus, 1) + 0
    assert cr.plan(1025, CUS) == (65, 16) and cr.plan(cr.OP_L_TWO_GROUPS, CUS) == (513, 32) and cr.plan(16384, CUS) == (1024, 16)
    assert cr.edge_rows(1, CUS) == [0] and cr.edge_rows(65, CUS) == [0, 15, 16, 47, 48, 63, 64]
    assert cr.edge_rows(65, CUS, every=True) == [0, 15, 16, 31, 32, 47, 48, 63, 64] and len(cr.edge_rows(1025, CUS, every=True)) == 129


@pytest.mark.parametrize("H", cr.OP_H)
def test_every_witness_owns_its_penalty_and_every_mutant_moves_it(H):
    worst_tol, least_move = 0.0, np.inf
    lengths = list(cr.OP_L) + ([cr.OP_L_TWO_GROUPS] if H == 128 else [])
    for L in lengths:
        k = cr.OP_K[L % len(cr.OP_K)]
        for n, row in enumerate(cr.edge_rows(L, CUS, every=H == 128 and L <= 1025)):      # (as the GPU test takes them)
            i = n % k
            hist, cand = cr.witness_inputs(H, L, k, row, i)
            pen = cr.penalties(hist, cand)
            assert pen[i] >= 0.999 and abs(pen[i] - 1.0) < 1e-12
            if L > 1:
                others = np.delete(pen, i)
                assert others.max() < 0.6, (H, L, others.max())      # roughly 4 / sqrt(H) at these L
            dev, tol = cr.penalty_bound(hist, cand)
            worst_tol = max(worst_tol, tol)
        for name, (rows, wit) in cr.mutants(L, CUS).items():
            hist, cand = cr.witness_inputs(H, L, k, wit, 1)
            dev, tol = cr.penalty_bound(hist, cand)
            move = float(cr.penalties(hist, cand)[1] - cr.penalties(hist[rows], cand)[1])
            least_move = min(least_move, move)
            assert move > 50 * tol, (H, L, name, move, tol)
    print(f"H={H}: op bound (8 x the fp32 evaluation's deviation) at most {worst_tol:.3e}; a one-row mutant moves a witness's penalty by at least {least_move:.3f}")
    assert worst_tol < 1e-5


# ---------------------------------------------------------------------------------------------------------------- host side
GC = types.SimpleNamespace(penalty_alpha=None, top_k=50)


def test_mode_rule():
    assert cs.selects(0.6, 4, False, 1)
    for pa, tk, smp, nb in ((None, 4, False, 1), (0, 4, False, 1), (0.0, 4, False, 1), (-0.5, 4, False, 1), (0.6, 1, False, 1), (0.6, None, False, 1),
                            (0.6, 4, True, 1), (0.6, 4, False, 2)):
        assert not cs.selects(pa, tk, smp, nb), (pa, tk, smp, nb)
        kw = dict(penalty_alpha=pa)
        assert cs.resolve_contrastive(types.SimpleNamespace(penalty_alpha=None, top_k=None), kw, tk, smp, nb, 16) is None and kw == {}


def test_parameter_resolution():
    kw = dict(penalty_alpha=0.6, other=1)
    assert cs.resolve_contrastive(GC, kw, 4, False, 1, 16) == dict(alpha=0.6, k=4) and kw == dict(other=1)
    gc = types.SimpleNamespace(penalty_alpha=0.5, top_k=3)
    assert cs.resolve_contrastive(gc, {}, None, False, 1, 8) == dict(alpha=0.5, k=3)
    assert cs.resolve_contrastive(gc, dict(penalty_alpha=1.0), 16, False, 1, 16) == dict(alpha=1.0, k=16)
    with pytest.raises(ValueError, match=r"\(0, 1\]"):
        cs.resolve_contrastive(GC, dict(penalty_alpha=1.5), 4, False, 1, 16)
    with pytest.raises(ValueError, match="min\\(16, max_batch=16\\) = 16.*default to 50"):
        cs.resolve_contrastive(GC, dict(penalty_alpha=0.6), None, False, 1, 16)      # generation_config.top_k = 50
    with pytest.raises(ValueError, match="= 4"):
        cs.resolve_contrastive(GC, dict(penalty_alpha=0.6), 5, False, 1, 4)
    with pytest.raises(ValueError, match="integer"):
        cs.resolve_contrastive(GC, dict(penalty_alpha=0.6), 2.5, False, 1, 16)
    with pytest.raises(ValueError, match="at most 8 distinct"):
        cs.check_eos(list(range(9)))
    cs.check_eos([1, 2, 2, 3, 4, 5, 6, 7, 8, 8])
    with pytest.raises(ValueError, match="exceed max_seq"):
        cs.check_room(60, 5, 64)
    cs.check_room(59, 5, 64)


@pytest.mark.parametrize("kw,frag", [
    (dict(b=2), "b > 1"), (dict(padded=True), "attention mask"), (dict(num_return_sequences=2), "num_return_sequences"),
    (dict(suffixes=True), "suffixes"), (dict(lookup=True), "prompt_lookup"), (dict(reuse=True), "reuse_cache"), (dict(guidance=True), "guidance_scale"),
    (dict(dola=True), "dola_layers"), (dict(token_fsm=True), "token_fsm"), (dict(banning=True), "token-banning"),
    (dict(repetition_penalty=1.2), "repetition_penalty"), (dict(output_logprobs=True), "output_logprobs"), (dict(tp_size=2), "tensor parallelism"),
    (dict(fp8_kv=True), "e4m3"), (dict(fp8_prefill=True), "fp8 x fp8"), (dict(mxfp4_decode=True), "MXFP4"),
    (dict(share_prompt=True, share_refusal="why not"), "why not")])
def test_every_refusal_from_host_data(kw, frag):
    with pytest.raises(NotImplementedError, match=frag):
        cs.refuse(**kw)


def test_what_is_not_refused():
    cs.refuse()
    cs.refuse(mxfp4_decode=True, mxfp4_batched=True)
    cs.refuse(share_prompt=False, share_refusal="why not")
    cs.refuse(share_prompt=None, share_refusal="why not")
    cs.refuse(repetition_penalty=1.0)
    cs.refuse(repetition_penalty=None)


def test_record_unpacks():
    w = np.zeros((2, cs.REC_WORDS), np.int32)
    w[:, :3] = [[5, 6, 7], [8, 9, 10]]
    w.view(np.float32)[:, 16:19] = [[0.5, 0.25, 0.125]] * 2
    w.view(np.float32)[:, 32:35] = [[0.1, 0.2, 0.3]] * 2
    w[:, 48] = [2, 0]; w[:, 49] = [7, 8]; w[:, 50] = 3; w[:, 51] = [10, 11]
    r = cs.unpack_record(w, 3)
    assert r["ids"].tolist() == [[5, 6, 7], [8, 9, 10]] and r["pick"].tolist() == [2, 0] and r["token"].tolist() == [7, 8]
    assert r["probs"][0].tolist() == [0.5, 0.25, 0.125] and np.allclose(r["penalties"][1], [0.1, 0.2, 0.3]) and r["rows"].tolist() == [10, 11]


# ---------------------------------------------------------------------------------------------------------------- the asserted prompt
def test_contrastive_ids_differ_from_greedy_on_the_tiny_decoders_oracle():
    import oracle
    cfg = tiny(layers_t=cr.TINY_LAYERS)
    sd = {k_: torch.from_numpy(v_).to(torch.bfloat16).float() for k_, v_ in synth.state_dict(cfg, cr.TINY_SEED, only_prefix=("model.layers", "model.norm", "model.embed", "lm_head")).items()}
    ids = torch.tensor([cr.TINY_PROMPT])
    ref = cr.search(cr.oracle_model(oracle, sd, cfg, ids), cr.TINY_K, cr.ALPHA, cr.TINY_NEW)
    greedy, _ = oracle.greedy_generate(ids, None, sd, cfg.vision, cfg.text, cr.TINY_NEW)
    print(f"contrastive {ref['ids']} ranks {ref['ranks']} margins {[f'{m:.2e}' for m in ref['margins']]}\ngreedy      {greedy}")
    assert ref["ids"] != greedy and any(r > 0 for r in ref["ranks"])
    assert len(ref["ids"]) == cr.TINY_NEW
