"""CPU restatement of teacher-forced scoring (omchat_amd/csrc/score.hip, gemm.hip EPI_LSE) in fp64: the log-softmax of
given logits gathered at the shifted labels, Qwen2ForCausalLM's loss reduction, the whole forward(labels=...) of a fixture case through the
oracle (oracle.splice + oracle.decoder), and the tolerance of the GEMM-epilogue op against fp64 from the same 16-bit inputs.
tests/test_score_cpu.py pins it to tests/golden/score_tiny.npz (the reference's own forward) and to torch's cross_entropy."""
import numpy as np
import torch

import logprob_ref as lr

IGNORE = -100


def shift(new_labels):
    """shift[:, t] = new_labels[:, t + 1], last column ignored"""
    out = np.full_like(np.asarray(new_labels), IGNORE)
    out[:, :-1] = np.asarray(new_labels)[:, 1:]
    return out


def row_logprobs(logits, shifted):
    """log_softmax(logits[r])[shifted[r]] in fp64 for every row, 0 where the label is ignored.  logits [..., V], shifted [...]"""
    z = np.asarray(logits, dtype=np.float64)
    lab = np.asarray(shifted)
    m = z.max(axis=-1, keepdims=True)
    lse = (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))[..., 0]
    x = np.take_along_axis(z, np.where(lab == IGNORE, 0, lab)[..., None], axis=-1)[..., 0]
    return np.where(lab == IGNORE, 0.0, x - lse)


def token_logprobs(logits, new_labels):
    """the layout of forward(labels=...).token_logprobs: column t >= 1 = log p(new_labels[:, t] | slots < t), 0 where ignored and in column 0"""
    lp = row_logprobs(logits, shift(new_labels))
    out = np.zeros_like(lp)
    out[:, 1:] = lp[:, :-1]
    return out


def loss(tl, new_labels):
    """mean of -tl over the scored slots (columns >= 1 whose label is not ignored); NaN when there are none, as cross_entropy gives"""
    scored = np.asarray(new_labels)[:, 1:] != IGNORE
    n = int(scored.sum())
    return float("nan") if n == 0 else float(-(np.asarray(tl, dtype=np.float64)[:, 1:][scored]).sum() / n)


def splice_labels(ids, mask, labels, n_tok, side="right", max_length=None):
    """omchat_arch.py:112-199 restated on lists: the labels of the kept tokens, IGNORE over every feature block, cut, padded"""
    rows = []
    for i in range(len(ids)):
        row = []
        for t in range(len(ids[i])):
            if mask is not None and not mask[i][t]:
                continue
            row += [IGNORE] * n_tok if ids[i][t] == -200 else [int(labels[i][t])]
        rows.append(row if max_length is None else row[:max_length])
    S = max(len(r) for r in rows)
    out = np.full((len(rows), S), IGNORE, dtype=np.int64)
    for i, r in enumerate(rows):
        if r:
            if side == "left":
                out[i, S - len(r):] = r
            else:
                out[i, :len(r)] = r
    return out


def case_inputs(g, name):
    """(ids, mask|None, labels, n_tiles, side, max_length|None, vocab) of a case of score_tiny.npz as torch / python values"""
    ids = torch.from_numpy(g[f"{name}_ids"].astype(np.int64))
    mask = g[f"{name}_mask"]
    mask = None if mask.size == 0 else torch.from_numpy(mask.astype(np.int64))
    labels = torch.from_numpy(g[f"{name}_labels"].astype(np.int64))
    ml = int(g[f"{name}_maxlen"])
    return ids, mask, labels, int(g[f"{name}_n_tiles"]), "left" if int(g[f"{name}_left"]) else "right", None if ml < 0 else ml, int(g[f"{name}_vocab"])


def case_feats(name, n_tiles, n_tok, H):
    """the feature rows the fixture's reference run was given (regenerated, not stored)"""
    from omchat_amd import synth
    return None if n_tiles == 0 else torch.from_numpy(synth.uniform("g.score.feats." + name, (n_tiles, n_tok, H), 0, 1.0))


def oracle_case(g, name, cfg, w):
    """forward(labels=...) of a fixture case through the oracle in fp32, log-softmax in fp64 -> (new_labels, token_logprobs, loss).
    w: torch fp32 state dict of cfg (omchat_amd.synth, the fixture's seed)"""
    from oracle import decoder, splice
    ids, mask, labels, n_tiles, side, ml, _ = case_inputs(g, name)
    n_tok, H = cfg.num_image_tokens, cfg.text["hidden_size"]
    feats = case_feats(name, n_tiles, n_tok, H)
    emb = w["model.embed_tokens.weight"]
    if feats is None:          # text only: the reference hands ids, mask and labels to Qwen2 as they are
        x, mask_out, new_labels = emb[ids], mask, labels.numpy()
    else:
        x, mask_out, _ = splice.splice_inputs(ids, mask, list(feats), emb, side, ml)
        new_labels = splice_labels(ids.tolist(), None if mask is None else mask.tolist(), labels.tolist(), n_tok, side, ml)
    h = decoder.qwen2_model(x, w, cfg.text, None, None, mask_out)
    logits = decoder.lm_head(h, w)
    tl = token_logprobs(logits.numpy(), new_labels)
    return new_labels, tl, loss(tl, new_labels)


def op_tolerance(a, w, x_id, lse_):
    """|device - fp64| bound of omchat_op_lse_label for one row: the products of 16-bit inputs are exact in fp32, so only the fp32 summation over
    K differs -- worst case 2 K 2^-24 max_n sum_k |a_k w_nk|, once for the label's logit and once for the log-sum-exp (a common shift of every
    logit moves it by as much) -- plus the fp32 softmax stage (logprob_ref.tolerance).  a [K], w [N, K] fp64"""
    K = a.shape[0]
    worst = float((np.abs(w) @ np.abs(a)).max())
    return 2.0 * K * 2.0 ** -24 * worst + lr.tolerance(x_id, lse_)
