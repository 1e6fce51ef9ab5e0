"""CPU restatement of layer-contrastive decoding (omchat_amd/csrc/dola.hip, omchat_amd/dola.py) in fp64 numpy -- HF 4.4x's
_dola_decoding (candidate layers), _dola_select_contrast and _relative_top_filter, restated from their published text: transformers 5 moved
DoLa out of the library, so nothing here is pinned against an installed HF.

Rows: logits [(k + 1) * b, V], rows [0, b) the final layer's, row (1 + j) * b + r candidate j of sequence r.  Per sequence:
    lm = log_softmax(final), lp_j = log_softmax(cand_j), a_j = 0.5 (exp lm + exp lp_j)
    JS_j = 0.5 * mean_v [a_j (log a_j - lm) + a_j (log a_j - lp_j)]          (a term with a_j == 0 contributes 0: torch's kl_div)
    pick = argmax_j JS_j (first on ties; k == 1: no JS)
    out[v] = -inf where lm[v] < max lm + log(relative_top), else lm[v] - lp_pick[v]
`stage` lets every row pick its own layer (the device's rule); `stage_batch_mean` is HF's: one layer from the batch mean of JS.  `dtype`
float32 evaluates the same formulas in fp32 numpy: the yardstick of the device's tolerance, as tests/guidance_ref.py does for guidance."""
import numpy as np

MAX_LAYERS = 16


def resolve_layers(dola_layers, N, tied=False):
    """HF's candidate list for hidden_states indices (0 = embeddings .. N - 1), by the rules of the issue; ValueError as the project's"""
    start = 0
    if tied:
        start = 2 if N > 2 else (1 if N == 2 else 0)
    if dola_layers == "low":
        if N <= 40:
            out = [start] if start == N // 2 else list(range(start, N // 2, 2))
        else:
            out = list(range(start, 20, 2))
    elif dola_layers == "high":
        out = list(range(N // 2, N, 2)) if N <= 40 else list(range(N - 20, N, 2))
    elif isinstance(dola_layers, (list, tuple)):
        if any(i < 0 for i in dola_layers):
            raise ValueError("negative layer index")
        out = [i for i in dola_layers if i < N]
    else:
        raise ValueError("dola_layers must be 'low', 'high' or a list of integers")
    if not out or len(out) > MAX_LAYERS:
        raise ValueError("no candidate layer, or more than 16")
    return out


def log_softmax(x, dtype=np.float64):
    z = np.asarray(x, dtype=dtype)
    m = z.max(axis=-1, keepdims=True)
    s = np.exp(z - m).sum(axis=-1, keepdims=True, dtype=dtype)
    return (z - (m + np.log(s))).astype(dtype)


def js(lm, lp, dtype=np.float64):
    """[..., V] x [..., V] -> [...]: the Jensen-Shannon divergence as HF writes it (two kl_div(..., reduction='none').mean(-1))"""
    a = (dtype(0.5) * (np.exp(lm) + np.exp(lp))).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        la = np.log(a)
        t1 = np.where(a > 0, a * (la - lm), dtype(0))
        t2 = np.where(a > 0, a * (la - lp), dtype(0))
    return (dtype(0.5) * (t1.mean(axis=-1, dtype=dtype) + t2.mean(axis=-1, dtype=dtype))).astype(dtype)


def _split(logits, b, k, dtype):
    z = np.asarray(logits, dtype=dtype)
    assert z.ndim == 2 and z.shape[0] == (k + 1) * b
    lm = log_softmax(z[:b], dtype)                                     # [b, V]
    lp = log_softmax(z[b:].reshape(k, b, -1), dtype)                   # [k, b, V]
    return lm, lp


def divergences(logits, b, k, dtype=np.float64):
    """-> JS [b, k]"""
    lm, lp = _split(logits, b, k, dtype)
    return np.stack([js(lm, lp[j], dtype) for j in range(k)], axis=1)


def threshold(lm, relative_top, dtype=np.float64):
    return lm.max(axis=-1, keepdims=True) + dtype(np.log(dtype(relative_top)))


def contrast(lm, lp_pick, relative_top, dtype=np.float64):
    with np.errstate(invalid="ignore"):
        return np.where(lm < threshold(lm, relative_top, dtype), dtype(-np.inf), lm - lp_pick).astype(dtype)


def stage(logits, b, k, relative_top=0.1, dtype=np.float64, picked=None):
    """-> (out [b, V], picked positions [b]); every row picks its own layer.  picked: force these positions (the tolerance's yardstick)"""
    lm, lp = _split(logits, b, k, dtype)
    if picked is None:
        picked = np.zeros(b, dtype=np.int64) if k == 1 else np.argmax(divergences(logits, b, k, dtype), axis=1)
    lp_pick = np.stack([lp[int(picked[r]), r] for r in range(b)])
    return contrast(lm, lp_pick, relative_top, dtype), np.asarray(picked, dtype=np.int64)


def stage_batch_mean(logits, b, k, relative_top=0.1, dtype=np.float64):
    """HF: the divergences averaged over the batch, one layer for all rows -> (out [b, V], picked position)"""
    lm, lp = _split(logits, b, k, dtype)
    j = 0 if k == 1 else int(np.argmax(divergences(logits, b, k, dtype).mean(axis=0)))
    return contrast(lm, lp[j], relative_top, dtype), j


def tolerance(logits, b, k, relative_top, picked):
    """(the largest |fp32 numpy - fp64| over the finite scores of these inputs with the fp64 picks, 8 times that): what the device may
    deviate by -- its reduction order and expf differ from numpy's.  The bound tests/test_gpu_guidance.py uses for the guidance stage."""
    ref, _ = stage(logits, b, k, relative_top, picked=picked)
    f32, _ = stage(logits, b, k, relative_top, np.float32, picked=picked)
    fin = np.isfinite(ref) & np.isfinite(f32)
    dev = float(np.abs(f32[fin].astype(np.float64) - ref[fin]).max()) if fin.any() else 0.0
    return dev, 8.0 * dev


def margins(logits, b, k, relative_top):
    """what keeps a comparison with the device honest: (the smallest relative gap between a row's best and second-best JS -- inf at k == 1 --,
    the smallest |lm - thresh| over all ids)"""
    lm, _ = _split(logits, b, k, np.float64)
    gap = np.inf
    if k > 1:
        d = np.sort(divergences(logits, b, k), axis=1)
        with np.errstate(invalid="ignore"):                           # (V == 1: 0 / 0, the caller looks at the divergences themselves)
            gap = float(((d[:, -1] - d[:, -2]) / np.abs(d[:, -1])).min())
    return gap, float(np.abs(lm - threshold(lm, relative_top)).min())


# ---- the tiny decoder: HF's hidden_states of the oracle's layer loop
def hidden_rows(oracle, embeds, w, cfg, cache, layers, norm=False):
    """oracle.qwen2_model's loop (oracle/decoder.py) restated so that it returns, for the LAST position of embeds [1, S, H], the rows the head
    sees: [final normed row, hidden_states[l] for l in layers] -- index 0 the embeddings, l the residual stream behind layer l; norm: the
    candidate rows through the final norm too.  -> [k + 1, H] torch"""
    import torch
    from oracle.decoder import qwen2_layer, rope_cos_sin
    from oracle.vit import rms_norm
    b, S, _ = embeds.shape
    past = cache.get_seq_length()
    pos = (past + torch.arange(S))[None, :].expand(b, S)
    nh = cfg["num_attention_heads"]
    d = cfg.get("head_dim") or cfg["hidden_size"] // nh
    cos, sin = rope_cos_sin(pos, d, cfg.get("rope_theta", 1e6), embeds.dtype)
    eps = cfg.get("rms_norm_eps", 1e-6)
    h, hs = embeds, [embeds]
    for i in range(cfg["num_hidden_layers"]):
        h = qwen2_layer(h, w, i, cfg, cos, sin, cache, None)
        hs.append(h)
    fin = rms_norm(h, w["model.norm.weight"], eps)[0, -1]
    cand = [rms_norm(hs[l], w["model.norm.weight"], eps)[0, -1] if norm else hs[l][0, -1] for l in layers]
    return torch.stack([fin] + cand)


# ---- the inputs of the op-level GPU cases (tests/test_gpu_dola.py), checked on the CPU (tests/test_dola_cpu.py)
OP_V = {1: 3, 7: 8, 2048: 2052, 2049: 2050, 4100: 4103}      # V -> ld: one partial tile, an exact tile, a tile plus one; aligned and misaligned row starts
OP_B, OP_K = (1, 3), (1, 2, 16)
OP_RT = 0.1
JS_GAP, THRESH_GAP = 1e-3, 1e-4
# ... and the gap must be one fp32 can see.  The device compares the sums V * 2 * JS = sum_v a (2 log a - lm - lp) (at most 2 ln 2); a term carries
# about |log| * 6e-8 of its a, |log| below ~30 for these inputs, the a sum to 1: at most ~2e-6 of rounding in a sum.  With the total divergence
# V * JS of the best candidate at JS_MIN or more, a relative gap of JS_GAP is 1e-5 or more in the sums.  A row of near point masses (JS ~ 1e-40
# in fp64: sums of subnormal probabilities) has a relative gap too, but no fp32 evaluation can see it
JS_MIN = 1e-2


def margins_ok(z, b, k, relative_top):
    """the two conditions under which a device in fp32 must reproduce the fp64 pick and -inf set: best and second-best JS a relative JS_GAP
    apart (V == 1: every distribution is the point mass, every JS exactly 0 -- the tie rule decides, on both sides), no lm within THRESH_GAP
    of the threshold"""
    gap, near = margins(z, b, k, relative_top)
    if z.shape[1] == 1:
        return bool((divergences(z, b, k) == 0).all()) and near >= THRESH_GAP
    return gap >= JS_GAP and near >= THRESH_GAP and (k == 1 or float(divergences(z, b, k).max(axis=1).min()) * z.shape[1] >= JS_MIN)


def op_inputs(b, k, V, relative_top=OP_RT):
    """[(k + 1) * b, V] fp32, finite: the final rows, candidate j
    a noisy copy of the final row, noisier with j, so that the divergences are spread.  The first seed of a fixed sequence whose fp64
    reference satisfies margins_ok -- chosen by the reference alone."""
    for seed in range(1000 * V + 100 * b + k, 1000 * V + 100 * b + k + 64):
        rng = np.random.default_rng(seed)
        f = (rng.standard_normal((b, V)) * 3).astype(np.float32)
        c = np.stack([f * np.float32(1.0 - 0.04 * j) + (rng.standard_normal((b, V)) * (0.5 + 0.25 * ((j * 7) % k))).astype(np.float32) for j in range(k)])
        z = np.concatenate([f, c.reshape(k * b, V)]).astype(np.float32)
        if margins_ok(z, b, k, relative_top):
            return z
    raise AssertionError((b, k, V))
