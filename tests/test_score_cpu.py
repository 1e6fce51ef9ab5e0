"""CPU: teacher-forced scoring -- the host label splice against the spliced labels the reference returned
(tests/golden/score_tiny.npz, tools/make_golden_score.py), the fp64 restatement tests/score_ref.py against the reference's loss and
per-token values, and the loss reduction's shift / ignore / empty semantics against torch's cross_entropy."""
import ctypes as C
import numpy as np
import pytest
import torch

import score_ref as sf
from conftest import golden
from omchat_amd import _lib, scoring, synth
from omchat_amd.config import tiny

CASES = ["A", "B", "C", "D", "E"]


def _plan(ids, mask, n_tok, n_tiles, side, ml):
    """omchat_splice_plan (host integers) -> src_index int32 [b, S]"""
    lib = _lib.lib()
    b, T = ids.shape
    a = np.ascontiguousarray(ids.numpy(), np.int64)
    m = None if mask is None else np.ascontiguousarray(mask.numpy() != 0, np.uint8)
    pm = None if m is None else m.ctypes.data_as(C.c_void_p)
    S, lens = C.c_int(0), np.zeros(b, np.int32)
    args = (a.ctypes.data_as(C.c_void_p), pm, b, T, n_tok, n_tiles, 1 if side == "left" else 0, -1 if ml is None else ml)
    _lib.check(lib.omchat_splice_plan(*args, None, lens.ctypes.data_as(C.c_void_p), C.byref(S), 0))
    idx = np.zeros((b, S.value), np.int32)
    _lib.check(lib.omchat_splice_plan(*args, idx.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), C.byref(S), 0))
    return torch.from_numpy(idx)


@pytest.mark.parametrize("name", CASES)
def test_label_splice_equals_reference(name):
    g = golden("score_tiny")
    ids, mask, labels, n_tiles, side, ml, vocab = sf.case_inputs(g, name)
    cfg = tiny(vocab=vocab)
    idx = _plan(ids, mask, cfg.num_image_tokens, n_tiles, side, ml)
    got = scoring.splice_labels(idx, ids, mask, labels)
    want = torch.from_numpy(g[f"{name}_new_labels"].astype(np.int64))
    assert got.dtype == torch.int64 and torch.equal(got, want), (got, want)
    # the restatement on lists agrees as well
    if n_tiles:
        ref = sf.splice_labels(ids.tolist(), None if mask is None else mask.tolist(), labels.tolist(), cfg.num_image_tokens, side, ml)
        assert np.array_equal(ref, want.numpy())
    assert torch.equal(scoring.shift_labels(got), torch.from_numpy(sf.shift(got.numpy())))


def test_label_splice_refuses_bad_shapes_and_ids():
    idx = torch.tensor([[5, 6, -1, -2, 7]], dtype=torch.int32)
    ids = torch.tensor([[5, 6, -200, 7]])
    with pytest.raises(ValueError):
        scoring.splice_labels(idx, ids, None, torch.tensor([[1, 2, 3]]))
    with pytest.raises(ValueError):
        scoring.check_labels(torch.tensor([[0, 320, -100]]), 320)
    with pytest.raises(ValueError):
        scoring.check_labels(torch.tensor([[0, -1, -100]]), 320)
    scoring.check_labels(torch.tensor([[0, 319, -100]]), 320)


@pytest.fixture(scope="module")
def weights():
    g = golden("score_tiny")
    cache = {}

    def get(vocab):
        if vocab not in cache:
            cfg = tiny(vocab=vocab)
            sd = synth.state_dict(cfg, seed=int(g["seed"]))
            cache[vocab] = (cfg, {k: torch.from_numpy(v) for k, v in sd.items() if not k.startswith(synth.TOWER)})
        return cache[vocab]
    return get


@pytest.mark.parametrize("name", CASES)
def test_score_ref_reproduces_reference(name, weights):
    """fp32 oracle against the fp32 reference, the same arithmetic: 1e-5 absolute"""
    g = golden("score_tiny")
    cfg, w = weights(int(g[f"{name}_vocab"]))
    new_labels, tl, loss = sf.oracle_case(g, name, cfg, w)
    assert np.array_equal(new_labels, g[f"{name}_new_labels"])
    err = float(np.abs(tl - g[f"{name}_token_logprobs"].astype(np.float64)).max())
    print(f"SCERR ref-{name} tokens {err:.3e} loss {abs(loss - float(g[f'{name}_loss'])):.3e}")
    assert err <= 1e-5
    assert abs(loss - float(g[f"{name}_loss"])) <= 1e-5
    assert int((new_labels[:, 1:] != sf.IGNORE).sum()) >= 5


def test_loss_semantics_equal_cross_entropy():
    rng = np.random.default_rng(5)
    b, S, V = 3, 9, 37
    logits = (rng.standard_normal((b, S, V)) * 3).astype(np.float32)
    labels = rng.integers(0, V, (b, S))
    labels[0, :4] = -100; labels[1, 6:] = -100; labels[2, ::2] = -100
    labels[1, 0] = 5                                   # column 0 is never scored
    tl = sf.token_logprobs(logits, labels)
    lt, yt = torch.from_numpy(logits), torch.from_numpy(labels)
    want = torch.nn.functional.cross_entropy(lt[:, :-1].reshape(-1, V).double(), yt[:, 1:].reshape(-1), ignore_index=-100)
    assert abs(sf.loss(tl, labels) - float(want)) <= 1e-12
    per = torch.nn.functional.cross_entropy(lt[:, :-1].reshape(-1, V).double(), yt[:, 1:].reshape(-1), ignore_index=-100, reduction="none")
    assert np.allclose(-tl[:, 1:].reshape(-1), per.numpy(), rtol=0, atol=1e-12)
    assert np.all(tl[:, 0] == 0) and np.all(tl[labels == -100] == 0)
    # nothing to score: NaN, as cross_entropy gives
    none = np.full((b, S), -100)
    none[:, 0] = 3
    want = torch.nn.functional.cross_entropy(lt[:, :-1].reshape(-1, V), torch.from_numpy(none)[:, 1:].reshape(-1), ignore_index=-100)
    assert np.isnan(float(want)) and np.isnan(sf.loss(sf.token_logprobs(logits, none), none))
