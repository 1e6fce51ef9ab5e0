"""CPU: the host side of generate(dola_layers=) (omchat_amd/dola.py) against the rules of DESIGN.md section 22 as tests/dola_ref.py restates them
-- the candidate lists for N = 1, 2, 3, 28, 40, 48, tied and untied, the value errors, the refusals --, the identity of the per-row pick with
HF's batch mean at b = 1 (and a b = 2 case where they differ), the a == 0 convention, and the two margins that the inputs of the op-level GPU
cases (tests/test_gpu_dola.py) must keep so that a wrong pick cannot hide behind a near-tie."""
import types
import numpy as np
import pytest

import dola_ref as dr
from omchat_amd import dola


@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("N", [1, 2, 3, 28, 40, 48])
def test_layer_lists_follow_the_rules(N, tied):
    for name in ("low", "high", [0, 1, 2, 5, 27, 39, 47, 48, 99]):
        try:
            want = dr.resolve_layers(name, N, tied)
        except ValueError:
            with pytest.raises(ValueError):
                dola.resolve_layers(name, N, tied)
            continue
        assert dola.resolve_layers(name, N, tied) == want, (name, N, tied)
        assert all(0 <= i < N for i in want) and 1 <= len(want) <= 16


def test_layer_lists_spelled_out():
    assert dola.resolve_layers("low", 28) == list(range(0, 14, 2)) and dola.resolve_layers("high", 28) == list(range(14, 28, 2))
    assert dola.resolve_layers("low", 28, True) == list(range(2, 14, 2))
    assert dola.resolve_layers("low", 40) == list(range(0, 20, 2)) and dola.resolve_layers("high", 40) == list(range(20, 40, 2))
    assert dola.resolve_layers("low", 48) == list(range(0, 20, 2)) and dola.resolve_layers("high", 48) == list(range(28, 48, 2))
    assert dola.resolve_layers("low", 1) == [0] and dola.resolve_layers("high", 1) == [0]
    assert dola.resolve_layers("low", 2, True) == [1] and dola.resolve_layers("high", 2, True) == [1]
    assert dola.resolve_layers("low", 2) == [0]
    assert dola.resolve_layers("high", 3, True) == [1]
    with pytest.raises(ValueError):
        dola.resolve_layers("low", 3, True)                           # range(2, 1, 2) is empty
    assert dola.resolve_layers([1, 3, 4, 9], 4) == [1, 3]             # a list keeps the entries below N
    for bad in ([], [4, 5], [-1, 2], list(range(17)), "middle", 3, [1.5], [True], [1, 1]):
        with pytest.raises(ValueError):
            dola.resolve_layers(bad, 28 if bad != [4, 5] else 4)


def test_resolve_reads_generation_config_and_validates_relative_top():
    gc = types.SimpleNamespace(dola_layers="high", dola_relative_top=None, dola_norm=None)
    kw = dict(other=1)
    assert dola.resolve_dola(gc, kw, 4) == dict(layers=[2], relative_top=0.1, norm=False) and kw == dict(other=1)
    kw = dict(dola_layers=[0], dola_relative_top=1.0, dola_norm=True)
    assert dola.resolve_dola(gc, kw, 4) == dict(layers=[0], relative_top=1.0, norm=True) and kw == {}
    assert dola.resolve_dola(types.SimpleNamespace(), dict(dola_relative_top=0.5), 4) is None      # None: nothing happens
    for bad in (0, 0.0, -0.1, 1.5, float("nan"), "0.1", True):
        with pytest.raises(ValueError):
            dola.resolve_dola(gc, dict(dola_relative_top=bad), 4)


def test_refusals_from_host_data():
    ok = dict(b=1, k=2, max_batch=4)
    dola.refuse(**ok)
    for bad in (dict(num_beams=2), dict(guidance=True), dict(num_return_sequences=2), dict(suffixes=True), dict(lookup=True), dict(reuse=True),
                dict(padded=True), dict(tp_size=2), dict(fp8_decode=True), dict(mxfp4_decode=True)):
        with pytest.raises(NotImplementedError, match="dola_layers with"):
            dola.refuse(**dict(ok, **bad))
    with pytest.raises(ValueError, match="rows go through the head"):
        dola.refuse(b=2, k=2, max_batch=4)
    with pytest.raises(ValueError):
        dola.refuse(b=2, k=16, max_batch=64)                          # 34 rows: more than one head pass takes


def test_generate_refuses_instead_of_dropping_the_keyword():
    """the keyword reaches resolve_dola: a bad value raises from generate() before the engine is touched (engine=None would fail otherwise)"""
    import inspect
    from omchat_amd.model import omchat_qwen2
    src = inspect.getsource(omchat_qwen2.OmChatQwen2ForCausalLM.generate)
    assert "resolve_dola" in src and "dola_premature_layers" in src


def test_b1_identity_with_the_batch_mean_and_a_batch_where_they_differ():
    for k in (1, 2, 7):
        z = dr.op_inputs(1, k, 2049)
        out, picked = dr.stage(z, 1, k, 0.1)
        out_hf, j = dr.stage_batch_mean(z, 1, k, 0.1)
        assert int(picked[0]) == j and np.array_equal(out, out_hf)
    # two rows whose own picks differ: HF gives both the batch-mean layer, here each row gets what it gets alone at b = 1
    rng = np.random.default_rng(5)
    f = (rng.standard_normal((2, 64)) * 3).astype(np.float32)
    near, far = f + 0.01 * rng.standard_normal((2, 64)).astype(np.float32), (rng.standard_normal((2, 64)) * 3).astype(np.float32)
    c0 = np.stack([far[0], near[1]]); c1 = np.stack([near[0], far[1] * 2])
    z = np.concatenate([f, c0, c1])
    out, picked = dr.stage(z, 2, 2, 0.1)
    assert picked.tolist() == [0, 1]
    for r in range(2):
        alone = np.stack([z[r], z[2 + r], z[4 + r]])
        o1, p1 = dr.stage(alone, 1, 2, 0.1)
        assert int(p1[0]) == int(picked[r]) and np.array_equal(o1[0], out[r])
    _, j = dr.stage_batch_mean(z, 2, 2, 0.1)
    assert j in (0, 1) and any(int(p) != j for p in picked)


def test_a_zero_terms_contribute_nothing():
    # both probabilities of the last id underflow to exactly 0 in fp64: a == 0, the term is 0 (torch's kl_div), never NaN
    lm = dr.log_softmax(np.array([0.0, -1.0, -2000.0]))
    lp = dr.log_softmax(np.array([-1.0, 0.0, -3000.0]))
    assert np.exp(lm[2]) == 0 and np.exp(lp[2]) == 0
    full = dr.js(lm, lp)
    part = dr.js(lm[:2], lp[:2]) * 2 / 3                              # the mean runs over V = 3 ids, the last adds 0
    assert np.isfinite(full) and abs(full - part) < 1e-15
    assert abs(dr.js(lm, lm)) < 1e-15                                 # identical rows: zero up to the rounding of log(exp(.))
    z = np.array([[0.0, 1.0, 2.0], [0.0, 1.0, 2.0]], dtype=np.float32)      # a candidate identical to the final row
    out, _ = dr.stage(z, 1, 1, 0.1)
    assert (out[np.isfinite(out)] == 0).all()


@pytest.mark.parametrize("V", sorted(dr.OP_V))
def test_gpu_op_inputs_keep_their_margins(V):
    for b in dr.OP_B:
        for k in dr.OP_K:
            z = dr.op_inputs(b, k, V)
            assert z.dtype == np.float32 and z.shape == ((k + 1) * b, V) and np.isfinite(z).all()
            gap, near = dr.margins(z, b, k, dr.OP_RT)
            assert near >= dr.THRESH_GAP, (b, k, V, near)
            if V == 1:
                assert (dr.divergences(z, b, k) == 0).all()           # point masses: every JS is exactly 0, the tie rule picks position 0
                assert dr.stage(z, b, k, dr.OP_RT)[1].tolist() == [0] * b
            elif k > 1:
                assert gap >= dr.JS_GAP, (b, k, V, gap)
                assert dr.divergences(z, b, k).max(axis=1).min() * V >= dr.JS_MIN
            # the fp32 evaluation keeps the -inf set and the picks under these margins
            ref, picked = dr.stage(z, b, k, dr.OP_RT)
            f32, p32 = dr.stage(z, b, k, dr.OP_RT, np.float32)
            assert np.array_equal(np.isfinite(ref), np.isfinite(f32)) and p32.tolist() == picked.tolist()
