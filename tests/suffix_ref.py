"""Host restatement of generate(suffixes=[...]) / score(suffixes=[...]): the refusal table, the per-row histories,
the padded sequences of the stopping criteria, the label arithmetic of the scoring form, and the suffix-pass attention and the shared decode
attention over rows of different lengths in fp64."""
import math

import torch


def refusal(batch=1, mask_zeros=False, suffixes=((5, 6),), vocab=320, max_batch=8, max_prefill_rows=1024, num_beams=1, num_return_sequences=1,
            lookup=False, reuse=False, streamer=False, fp8_kv=False, fp8_prefill=False, tp_size=1, q_heads=7, kv_heads=1, share_prompt=None):
    """(exception type, a fragment of its message) that generate(suffixes=...) raises from host data alone, or None; the first that applies"""
    if batch != 1:
        return ValueError, "ONE prompt"
    if mask_zeros:
        return NotImplementedError, "padded prompt"
    rows = [list(s) for s in suffixes]
    if not rows:
        return ValueError, "`suffixes` is empty"
    if any(len(r) == 0 for r in rows):
        return ValueError, "is empty: every suffix"
    if any(not 0 <= i < vocab for r in rows for i in r):
        return ValueError, "outside the vocabulary"
    N, S = len(rows), max(len(r) for r in rows)
    if N > max_batch:
        return ValueError, "max_batch >="
    if N * S > max_prefill_rows:
        return ValueError, "max_prefill_rows >="
    if num_beams > 1:
        return NotImplementedError, "num_beams > 1"
    if num_return_sequences > 1:
        return NotImplementedError, "num_return_sequences > 1"
    if lookup:
        return NotImplementedError, "prompt_lookup_num_tokens"
    if reuse:
        return NotImplementedError, "reuse_cache=True"
    if streamer and N > 1:
        return ValueError, "`streamer` cannot be used with more than one suffix"
    if fp8_kv or fp8_prefill or tp_size > 1:
        return NotImplementedError, "e4m3 KV cache, fp8 x fp8 prefill GEMMs or tensor parallelism"
    if share_prompt and (N > 16 or N * (q_heads // kv_heads) > 128 or q_heads // kv_heads > 8):
        return NotImplementedError, "share_prompt=True is not available"
    return None


def room_refusal(prompt_slots, suffixes, max_seq):
    return prompt_slots + max(len(s) for s in suffixes) + 1 > max_seq


def histories(prompt, suffixes):
    return [[int(i) for i in prompt] + [int(i) for i in s] for s in suffixes]


def seen_sets(prompt, suffixes):
    return [[i for i in h if i >= 0] for h in histories(prompt, suffixes)]


def padded_sequences(prompt, suffixes, new_rows, pad):
    full = [h + list(g) for h, g in zip(histories(prompt, suffixes), new_rows)]
    w = max(map(len, full))
    return [f + [0 if pad is None else pad] * (w - len(f)) for f in full]


def score_from_logits(logits_rows, prompt_len, suffixes):
    """plain log-softmax scoring: logits_rows[j] fp [prompt_len + S_j, V] = the logits of every position of prompt + suffix_j (positions
    counted in cache slots).  -> (token_logprobs [N, S_max] with 0 behind a row's end, sequence_logprobs [N], num_tokens [N])"""
    N, S_max = len(suffixes), max(len(s) for s in suffixes)
    tl = torch.zeros(N, S_max, dtype=torch.float64)
    for j, s in enumerate(suffixes):
        lp = torch.log_softmax(logits_rows[j].double(), dim=-1)
        for t, tok in enumerate(s):
            tl[j, t] = lp[prompt_len + t - 1, tok]      # token t sits at slot prompt_len + t and is predicted by the slot in front
    return tl, tl.sum(dim=1), torch.tensor([len(s) for s in suffixes])


def attn_suffix_ref(q, k, v, P, lengths):
    """fp64 GQA on the 16-bit-rounded inputs: q [N, S, Hq, 128], k / v [>= N rows, Hkv, cap, 128]; query (j, t), t < lengths[j], sees the keys
    [0, P) of row 0 and the keys [P, P + t] of row j.  Rows t >= lengths[j] are left 0 (not compared).  Evaluated on q's device."""
    N, S, Hq, _ = q.shape
    rep = Hq // k.shape[1]
    scale = 1.0 / math.sqrt(128)
    out = torch.zeros(N, S, Hq, 128, dtype=torch.float64, device=q.device)
    for j in range(N):
        n = int(lengths[j])
        kk = torch.cat([k[0, :, :P], k[j, :, P:P + n]], dim=1).double().repeat_interleave(rep, dim=0)      # [Hq, P + n, 128]
        vv = torch.cat([v[0, :, :P], v[j, :, P:P + n]], dim=1).double().repeat_interleave(rep, dim=0)
        s = torch.einsum("thd,hld->htl", q[j, :n].double(), kk) * scale                                      # [Hq, n, P + n]
        key = torch.arange(P + n, device=q.device)[None, :]
        tq = torch.arange(n, device=q.device)[:, None]
        s = s.masked_fill((key > P + tq)[None], float("-inf"))
        out[j, :n] = torch.einsum("htl,hld->thd", torch.softmax(s, -1), vv)
    return out


def attn_suffix_dense(q, k, v, P, lengths):
    """the same through one dense masked softmax over the concatenation of every row's slots (an independent formulation for the CPU check):
    the key axis is [row 0 slots | row 1 slots | ...] and the mask picks row 0's [0, P) and row j's [P, P + t]"""
    N, S, Hq, _ = q.shape
    Hkv, cap = k.shape[1], k.shape[2]
    rep = Hq // Hkv
    kk = k[:N].double().permute(1, 0, 2, 3).reshape(Hkv, N * cap, 128).repeat_interleave(rep, dim=0)
    vv = v[:N].double().permute(1, 0, 2, 3).reshape(Hkv, N * cap, 128).repeat_interleave(rep, dim=0)
    out = torch.zeros(N, S, Hq, 128, dtype=torch.float64)
    slot = torch.arange(cap)
    for j in range(N):
        for t in range(int(lengths[j])):
            mask = torch.zeros(N, cap, dtype=torch.bool)
            mask[0, :P] = True
            mask[j] |= (slot >= P) & (slot <= P + t)
            s = torch.einsum("hd,hld->hl", q[j, t].double(), kk) / math.sqrt(128)
            s = s.masked_fill(~mask.reshape(-1)[None], float("-inf"))
            out[j, t] = torch.einsum("hl,hld->hd", torch.softmax(s, -1), vv)
    return out


def attn_shared_lens_ref(q, k, v, G, N, P, lens):
    """tests/group_ref.py: attn_shared_ref with a length per row: row r sees the keys [0, P) of its group's first row and [P, lens[r]) of its own"""
    rows, Hq, _ = q.shape
    rep = Hq // k.shape[1]
    scale = 1.0 / math.sqrt(128)
    out = torch.empty(rows, Hq, 128, dtype=torch.float64, device=q.device)
    for r in range(G * N):
        lead = (r // N) * N
        L = int(lens[r])
        kk = torch.cat([k[lead, :, :P], k[r, :, P:L]], dim=1).double().repeat_interleave(rep, dim=0)
        vv = torch.cat([v[lead, :, :P], v[r, :, P:L]], dim=1).double().repeat_interleave(rep, dim=0)
        s = torch.einsum("hd,hld->hl", q[r].double(), kk) * scale
        out[r] = torch.einsum("hl,hld->hd", torch.softmax(s, -1), vv)
    return out
