"""What sequence 0's KV cache holds, and how much of a new prompt it already covers (generate(reuse_cache=True)).

Host-only code (no torch, no device work).  A cache slot is described by the embedding row that was prefilled or decoded into it:
a token id (int >= 0), or (tile key, row in tile) for an image-feature row.  A tile key names tile CONTENT: the engine compares the
pixel tensors of two calls bit for bit on the device and hands equal tiles the same key (Engine._tile_keys), so an image that moves to
another index, or a conversation that repeats its picture, still matches.  Nothing here hashes floats."""

PAD_ROW = -(2 ** 31)      # omchat_splice_plan's padding row (never part of a b = 1, unpadded plan)


def slots_from_plan(src_index, ntok, tile_keys):
    """src_index: one row of omchat_splice_plan (ints: id >= 0 -> embed_tokens row; -1 - (tile * ntok + r) -> feature row r of tile
    `tile`); tile_keys[tile] = content key.  -> list of slots"""
    out = []
    for v in src_index:
        v = int(v)
        if v >= 0:
            out.append(v)
            continue
        if v == PAD_ROW:
            raise ValueError("padded splice plan: the prefix record describes one unpadded sequence")
        tile, r = divmod(-1 - v, ntok)
        if tile >= len(tile_keys):
            raise ValueError("more <image> sentinels than image tiles")
        out.append((tile_keys[tile], r))
    return out


def slots_from_ids(ids, ntok, tile_keys):
    """the same from token ids with the -200 image sentinel (every sentinel takes the next tile and expands to ntok slots), as
    omchat_splice_plan lays a b = 1 row out"""
    out, tile = [], 0
    for t in ids:
        t = int(t)
        if t == -200:
            if tile >= len(tile_keys):
                raise ValueError("more <image> sentinels than image tiles")
            out.extend((tile_keys[tile], r) for r in range(ntok))
            tile += 1
        else:
            out.append(t)
    return out


def common_prefix(record, new_slots):
    """number of leading slots of new_slots that the record (list of slots, or None) already holds"""
    if not record:
        return 0
    n = min(len(record), len(new_slots))
    i = 0
    while i < n and record[i] == new_slots[i]:
        i += 1
    return i


def keep_count(record, new_slots, cached=None):
    """P of generate(reuse_cache=True): the common prefix, capped at len(new_slots) - 1 (one row must be prefilled to have logits) and
    at `cached` (the slots the cache really holds, when known)"""
    p = min(common_prefix(record, new_slots), max(len(new_slots) - 1, 0))
    return p if cached is None else min(p, int(cached))


def extend_record(prompt_slots, generated, cached):
    """the record after a generate() call: the prompt's slots plus the generated ids that are actually cached (`cached` = kv length after
    the final rewind: the last emitted id is never cached)"""
    n_gen = max(0, int(cached) - len(prompt_slots))
    return (list(prompt_slots) + [int(t) for t in generated[:n_gen]])[:int(cached)]


def check_reuse_args(batch, num_beams, attention_mask_rows=None, padding_side="right"):
    """the refusals of generate(reuse_cache=True), raised before any work: one unpadded right-aligned sequence, no beams"""
    if batch != 1:
        raise ValueError(f"reuse_cache=True keeps ONE conversation in sequence 0's cache: batch size {batch} is not supported")
    if num_beams > 1:
        raise ValueError("reuse_cache=True with num_beams > 1 is not supported: a beam search forks sequence 0's cache")
    if padding_side != "right":
        raise ValueError("reuse_cache=True needs right padding (tokenizer_padding_side='right')")
    if attention_mask_rows is not None and any(int(x) == 0 for row in attention_mask_rows for x in row):
        raise ValueError("reuse_cache=True with a padded batch (attention_mask with zeros) is not supported")
