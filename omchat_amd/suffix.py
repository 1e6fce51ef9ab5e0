"""Host side of generate(suffixes=[...]) / score(suffixes=[...]): N suffixes over one prefilled prompt.  Pure host
data: the argument resolution with every refusal, the per-row histories, the padded sequences handed to stopping criteria and the label
arithmetic of the scoring form.  Nothing here touches the device."""

SHARE_MAX_N = 16
SHARE_MAX_QROWS = 128


def as_id_lists(suffixes):
    """list / tuple of N token-id sequences (lists or 1-D tensors) -> list of N lists of ints; anything else is a ValueError"""
    if suffixes is None or isinstance(suffixes, (str, bytes)) or not hasattr(suffixes, "__len__"):
        raise ValueError("`suffixes` has to be a list of token-id sequences")
    if hasattr(suffixes, "dim"):      # one tensor: its rows are equal-length suffixes
        if suffixes.dim() != 2:
            raise ValueError("`suffixes` as a tensor has to be [N, S]: pass a list of 1-D sequences for suffixes of different length")
        suffixes = list(suffixes)
    rows = []
    for j, s in enumerate(suffixes):
        if hasattr(s, "dim"):
            if s.dim() != 1:
                raise ValueError(f"`suffixes[{j}]` has to be a 1-D sequence of token ids, but has {s.dim()} dimensions")
            s = s.tolist()
        try:
            rows.append([int(i) for i in s])
        except TypeError:
            raise ValueError(f"`suffixes[{j}]` has to be a sequence of token ids") from None
    return rows


def share_refusal(fp8_kv, tp_size, q_heads, kv_heads, N):
    """why the N suffix rows cannot share the prompt's slots (share_prompt=True), or None.  N == 1 shares trivially (no group is begun)."""
    if fp8_kv:
        return "the e4m3 KV cache"
    if tp_size != 1:
        return "tensor parallelism"
    n_rep = q_heads // max(1, kv_heads)
    if N > SHARE_MAX_N or N * n_rep > SHARE_MAX_QROWS:
        return "N outside N <= 16 and N * (q heads per kv head) <= 128"
    if n_rep > 8:
        return "more than 8 query heads per kv head (the suffix attention's query rows)"
    return None


def check_suffix_args(batch, mask_has_zeros, suffixes, vocab, max_batch, max_prefill_rows, num_beams=1, num_return_sequences=1, lookup=False,
                      reuse=False, streamer=False, fp8_kv=False, fp8_prefill=False, tp_size=1, q_heads=1, kv_heads=1, share_prompt=None):
    """every refusal of generate(suffixes=...) / score(suffixes=...) that host data alone decides, each with its own message, in this order.
    -> the suffixes as lists of ints."""
    if batch != 1:
        raise ValueError(f"`suffixes` continue ONE prompt: input_ids has to be [1, T], but holds {batch} rows")
    if mask_has_zeros:
        raise NotImplementedError("`suffixes` over a padded prompt (attention_mask with zeros) is not implemented: pass the prompt unpadded")
    rows = as_id_lists(suffixes)
    if len(rows) == 0:
        raise ValueError("`suffixes` is empty: pass at least one suffix (or no `suffixes` at all)")
    for j, r in enumerate(rows):
        if len(r) == 0:
            raise ValueError(f"`suffixes[{j}]` is empty: every suffix holds at least one token id")
    for j, r in enumerate(rows):
        bad = [i for i in r if not 0 <= i < vocab]
        if bad:
            raise ValueError(f"`suffixes[{j}]` holds ids outside the vocabulary [0, {vocab}) (suffixes are text ids only; the image "
                             f"sentinel belongs to the prompt): {bad[:8]}")
    N, S_max = len(rows), max(len(r) for r in rows)
    if N > max_batch:
        raise ValueError(f"`suffixes` needs one cache row per suffix: create the model with max_batch >= {N} (it has {max_batch})")
    if N * S_max > max_prefill_rows:
        raise ValueError(f"`suffixes` are prefilled as one block of N * max length = {N * S_max} rows: create the model with "
                         f"max_prefill_rows >= {N * S_max} (it has {max_prefill_rows})")
    if num_beams > 1:
        raise NotImplementedError("`suffixes` with num_beams > 1 is not implemented")
    if num_return_sequences > 1:
        raise NotImplementedError("`suffixes` with num_return_sequences > 1 is not implemented: repeat a suffix to sample it more than once")
    if lookup:
        raise NotImplementedError("`suffixes` with prompt_lookup_num_tokens is not implemented: a verify step runs one sequence")
    if reuse:
        raise NotImplementedError("`suffixes` with reuse_cache=True is not implemented: the cache rows end as siblings, not as one conversation")
    if streamer and N > 1:
        raise ValueError(f"`streamer` cannot be used with more than one suffix: it takes one sequence (N = {N})")
    if fp8_kv or fp8_prefill or tp_size > 1:
        raise NotImplementedError("`suffixes` with the e4m3 KV cache, fp8 x fp8 prefill GEMMs or tensor parallelism is not implemented "
                                  "(DESIGN.md section 7)")
    if share_prompt:
        why = share_refusal(fp8_kv, tp_size, q_heads, kv_heads, N)
        if why is not None:
            raise NotImplementedError(f"share_prompt=True is not available here ({why}): use share_prompt=False (DESIGN.md section 7)")
    return rows


def check_room(prompt_slots, rows, max_seq):
    """P + max S_j + 1 > max_seq: known once the splice plan gave the prompt's slot count, refused before the tower runs"""
    S_max = max(len(r) for r in rows)
    if prompt_slots + S_max + 1 > max_seq:
        raise ValueError(f"`suffixes`: the prompt's {prompt_slots} cache slots + the longest suffix ({S_max}) + one generated token exceed "
                         f"max_seq = {max_seq}")


def histories(prompt_ids, rows):
    """row j's history as HF's processors would see it for the concatenated prompt: prompt ids as passed (-200 sentinels included) + suffix_j"""
    p = [int(i) for i in prompt_ids]
    return [p + list(r) for r in rows]


def seen_sets(prompt_ids, rows):
    """the repetition penalty's seen ids of row j: the ids of prompt + suffix_j; the image sentinel (negative) never counts"""
    return [[i for i in h if i >= 0] for h in histories(prompt_ids, rows)]


def padded_sequences(prompt_ids, rows, new_rows, pad):
    """what stopping criteria are handed: row j = prompt + suffix_j + generated_j, right-padded with the pad id (0 when there is none) to
    the longest row.  new_rows: N lists of the ids generated so far."""
    full = [h + [int(t) for t in g] for h, g in zip(histories(prompt_ids, rows), new_rows)]
    width = max(len(f) for f in full)
    fill = 0 if pad is None else int(pad)
    return [f + [fill] * (width - len(f)) for f in full]


def suffix_token_table(rows, pad_row):
    """the [N, S_max] gather plan of the suffix block: token ids, pad_row behind a row's end (a zero embedding row)"""
    S_max = max(len(r) for r in rows)
    return [list(r) + [pad_row] * (S_max - len(r)) for r in rows]


def score_labels(rows, ignore=-100):
    """scoring form: (first ids [N], shifted labels [N, S_max]).  Token 0 of suffix j is predicted by the prompt's last position; token t + 1
    by suffix row t, so labels[j][t] = suffix_j[t + 1] for t < S_j - 1 and `ignore` from there on."""
    S_max = max(len(r) for r in rows)
    first = [r[0] for r in rows]
    lab = [list(r[1:]) + [ignore] * (S_max - len(r) + 1) for r in rows]
    return first, lab
