"""CPU restatement of contrastive search (omchat_amd/csrc/contrastive.hip) as HF 4.4x's _contrastive_search computes it for
one prompt -- transformers 5 moved the strategy out of the library, so it is restated here as tests/dola_ref.py restates DoLa:
  p = softmax(z) in fp32, the top-k of p (ties to the lower id: torch.topk leaves the order open, this file fixes it)
  pen_i = max_j cos(h_i, H_ctx[j]) over ALL rows of the context's post-final-norm hidden rows
  pick = argmax_i (1 - alpha) p_i - alpha pen_i, the first maximum
float64 by default; dtype=np.float32 evaluates the same formulas in the order the device uses (dot, times the row's inverse norm, times the
candidate's), which calibrates the op bound of tests/test_gpu_contrastive.py: 8 times the fp32 evaluation's deviation from float64, the bound
of tests/test_gpu_guidance.py / test_gpu_dola.py.  ranking_fast is a literal torch transcription of HF 4.4x's _ranking_fast, to pin the
restatement.  Also here: the penalty launch's plan, the witness inputs and their one-row mutants."""
import numpy as np

KMAX = 16


# ---------------------------------------------------------------------------------------------------------------- the stages
def topk_probs(z, k, dtype=np.float64):
    """z fp32 [V] -> (ids int64 [k] by value descending then id ascending, their softmax probabilities under the (max, sum exp) of the row)"""
    z = np.asarray(z, dtype=np.float32)
    ids = np.lexsort((np.arange(z.shape[0]), -z.astype(np.float64)))[:k]
    x = z.astype(dtype)
    e = np.exp(x - x.max())
    return ids.astype(np.int64), (e[ids] / e.sum(dtype=dtype)).astype(dtype)


def cosines(hist, cand, dtype=np.float64):
    """hist [L, H], cand [k, H] (the 16-bit rows as floats) -> cos [k, L]"""
    h, c = np.asarray(hist, dtype=dtype), np.asarray(cand, dtype=dtype)
    if dtype == np.float64:
        hn = h / np.linalg.norm(h, axis=1, keepdims=True)
        cn = c / np.linalg.norm(c, axis=1, keepdims=True)
        return cn @ hn.T
    one = np.float32(1.0)
    inv_h = one / np.sqrt((h * h).sum(axis=1, dtype=np.float32))
    inv_c = one / np.sqrt((c * c).sum(axis=1, dtype=np.float32))
    return (((c @ h.T) * inv_h[None, :]) * inv_c[:, None]).astype(np.float32)


def penalties(hist, cand, dtype=np.float64):
    """-> pen [k] = max_j cos(cand_i, hist_j)"""
    return cosines(hist, cand, dtype).max(axis=1)


def scores(probs, pen, alpha, dtype=np.float64):
    if dtype == np.float32:      # as torch rounds it: the Python scalars become fp32, every operation is rounded
        return (np.float32(1.0 - alpha) * np.asarray(probs, np.float32) - np.float32(alpha) * np.asarray(pen, np.float32)).astype(np.float32)
    return (1.0 - alpha) * np.asarray(probs, np.float64) - alpha * np.asarray(pen, np.float64)


def pick(probs, pen, alpha, dtype=np.float64):
    """-> (the first maximum's rank, the top-two margin of the scores)"""
    s = scores(probs, pen, alpha, dtype)
    o = np.sort(s.astype(np.float64))
    return int(np.argmax(s)), float(o[-1] - o[-2]) if s.shape[0] > 1 else np.inf


def ranking_fast(context_hidden, next_hidden, next_top_k_probs, cosine_matrix_mask, alpha, beam_width):
    """HF 4.4x generation/utils.py::_ranking_fast, verbatim but for the tensor types (torch, any float dtype): context_hidden
    [B * K, S, E], next_hidden [B * K, 1, E], next_top_k_probs [B, K], cosine_matrix_mask [B * K, S] -> (selected_idx [B], penalties [B * K])"""
    import torch
    norm_context_hidden = context_hidden / context_hidden.norm(dim=2, keepdim=True)
    norm_next_hidden = next_hidden / next_hidden.norm(dim=2, keepdim=True)
    cosine_matrix = torch.matmul(norm_context_hidden, norm_next_hidden.transpose(1, 2)).squeeze(-1)
    cosine_matrix_mask = cosine_matrix_mask.to(dtype=cosine_matrix.dtype)
    cosine_matrix_mask = (1 - cosine_matrix_mask) * torch.finfo(cosine_matrix.dtype).min
    cosine_matrix = cosine_matrix + cosine_matrix_mask
    degeneration_penalty, _ = torch.max(cosine_matrix, dim=-1)
    next_top_k_probs = next_top_k_probs.view(-1)
    contrastive_score = (1.0 - alpha) * next_top_k_probs - alpha * degeneration_penalty
    contrastive_score = torch.stack(torch.split(contrastive_score, beam_width))
    _, selected_idx = contrastive_score.max(dim=-1)
    return selected_idx, degeneration_penalty


def search(model, k, alpha, max_new, eos=(), stop=None):
    """The whole loop over a callable: model(extra) -> (H [L + len(extra), E] the post-final-norm hidden rows of the context followed by the
    ids `extra`, z fp32 [V] the last position's logits).  -> dict(ids, ranks, penalties, margins, steps): steps[t] = (candidate ids,
    probabilities, penalties).  stop(ids so far) -> bool is asked behind every id but the last."""
    H_ctx, z = model([])
    H_ctx = np.asarray(H_ctx, np.float64)
    out = dict(ids=[], ranks=[], penalties=[], margins=[], steps=[])
    for t in range(max_new):
        cids, p = topk_probs(z, k)
        hs, zs = [], []
        for c in cids:
            Hc, zc = model(out["ids"] + [int(c)])
            hs.append(np.asarray(Hc, np.float64)[-1]); zs.append(zc)
        pen = penalties(H_ctx, np.stack(hs))
        i, margin = pick(p, pen, alpha)
        out["ids"].append(int(cids[i])); out["ranks"].append(i); out["penalties"].append(float(pen[i])); out["margins"].append(margin)
        out["steps"].append((cids, p, pen))
        H_ctx = np.concatenate([H_ctx, hs[i][None]])
        z = zs[i]
        if int(cids[i]) in eos or (stop is not None and t + 1 < max_new and stop(out["ids"])):
            break
    return out


# ---------------------------------------------------------------------------------------------------------------- the penalty launch's plan
def plan(L, cus):
    """(chunks, rows_per_chunk): one wave per chunk, up to four per compute unit, chunks of whole 16-row groups (contrastive.hip: cs_plan)"""
    waves = 4 * max(cus, 1)
    groups = (L + 15) // 16
    gpc = max(1, (groups + waves - 1) // waves)
    return max(1, (L + gpc * 16 - 1) // (gpc * 16)), gpc * 16


def edge_rows(L, cus, every=False):
    """row 0, row L - 1 and the rows on both sides of the plan's chunk edges: of every edge with `every`, else of the first, a middle and
    the last one (the kernel treats all chunks alike; the GPU test takes every edge where that is cheap: H = 128, L <= 1025)"""
    chunks, rpc = plan(L, cus)
    edges = [c * rpc for c in range(1, chunks)]
    if len(edges) > 3 and not every:
        edges = [edges[0], edges[len(edges) // 2], edges[-1]]
    rows = {0, L - 1}
    for e in edges:
        rows.update((e - 1, e))
    return sorted(r for r in rows if 0 <= r < L)


# ---------------------------------------------------------------------------------------------------------------- inputs
OP_H = (128, 3584)
OP_L = (1, 2, 63, 64, 65, 257, 1025)
OP_L_TWO_GROUPS = 16400      # with 256 compute units the first length whose chunks hold two 16-row groups (H = 128 only: 4 MB)
OP_K = (2, 5, 16)
OP_V = {2049: 2052, 152064: 152067}      # V -> ld > V: a tile plus one id / the Qwen2 vocabulary; a misaligned second row either way
ALPHA = 0.6


def bf16_round(a):
    """fp32 array rounded to bf16 (round to nearest even), as fp32"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32)


def witness_inputs(H, L, k, row, cand_i, seed=0):
    """Gaussian bf16 history rows [L, H] and candidates [k, H]; history row `row` is 2 * candidate cand_i (exact in bf16), so its cosine
    with that candidate is 1 against roughly 4 / sqrt(H) for every other pair"""
    rng = np.random.default_rng(seed * 7919 + H * 31 + L * 17 + k)
    hist = bf16_round(rng.standard_normal((L, H)).astype(np.float32))
    cand = bf16_round(rng.standard_normal((k, H)).astype(np.float32))
    hist[row] = 2.0 * cand[cand_i]
    return hist, cand


def mutants(L, cus):
    """the one-row mutants of a penalty over L rows: name -> (the rows the mutant still sees, the witness row that shows it)"""
    chunks, rpc = plan(L, cus)
    out = {}
    if L >= 2:
        out["first row dropped"] = (np.arange(1, L), 0)
        out["last row dropped"] = (np.arange(0, L - 1), L - 1)
        out["append not yet visible"] = (np.arange(0, L - 1), L - 1)
    if chunks >= 2:
        e = (chunks // 2) * rpc
        out["edge row dropped (below)"] = (np.delete(np.arange(L), e - 1), e - 1)
        out["edge row dropped (above)"] = (np.delete(np.arange(L), e), e)
    return out


def penalty_bound(hist, cand):
    """(the fp32 evaluation's largest deviation from float64 on these inputs, 8 times that): the op bound.  The deviation is taken over every
    cosine the formulas evaluate, [k, L], not over the k maxima alone: a penalty is whichever of them is the largest, and k numbers are too
    few to measure a rounding error -- a witness cosine that numpy happens to round to exactly 1 would put the bound below one ulp of it."""
    dev = float(np.abs(cosines(hist, cand, np.float32).astype(np.float64) - cosines(hist, cand)).max())
    return dev, 8.0 * dev


def logits_inputs(V, k, seed=0, ties=True):
    """fp32 logits [V] like a head's (a few units of spread); with ties: the maximum three times (tile 0, the last tile, the last id) and the
    runner-up value twice, so that the k best cross equal values"""
    rng = np.random.default_rng(1000 * seed + V + k)
    z = (rng.standard_normal(V) * 2.5).astype(np.float32)
    if ties:
        top = np.float32(z.max() + 1.0)
        z[[7, V - 1, min(V - 2, 2047)]] = top
        z[[3, V // 2]] = np.float32(top - 0.5)
    return z


def probs_bound(z, k):
    ids, ref = topk_probs(z, k)
    dev = float(np.abs(topk_probs(z, k, np.float32)[1].astype(np.float64) - ref).max())
    return dev, 8.0 * dev


# ---------------------------------------------------------------------------------------------------------------- the tiny decoder
def oracle_model(oracle, sd, cfg, input_ids, images=None):
    """model(extra) for search() over the CPU oracle (tests only): the spliced prompt followed by the ids `extra`, recomputed from scratch
    (the tiny decoder: cheap) -> (the post-final-norm rows of row 0 [L, E] as float64 numpy, the last logits fp32 numpy)"""
    import torch
    from oracle.pipeline import encode_images
    from oracle.splice import splice_inputs
    emb = sd["model.embed_tokens.weight"]
    if images is None:
        base = emb[input_ids]
    else:
        feats = [f for f in encode_images(images, sd, cfg.vision)]
        base, _, _ = splice_inputs(input_ids, None, feats, emb, "right", cfg.text.get("tokenizer_model_max_length"))

    def model(extra):
        x = base if not extra else torch.cat([base, emb[torch.tensor([list(extra)])]], dim=1)
        h = oracle.qwen2_model(x, sd, cfg.text, oracle.KVCache(cfg.text["num_hidden_layers"]))
        return h[0].double().numpy(), oracle.lm_head(h[:, -1], sd)[0].float().numpy()
    return model


# the tiny decoder of the model-level tests (tests/test_contrastive_cpu.py asserts that contrastive search leaves the greedy ids on it)
TINY_LAYERS, TINY_SEED, TINY_K, TINY_NEW = 4, 22, 4, 10
TINY_PROMPT = [3, 17, 18, 19, 20, 21, 7, 9]
