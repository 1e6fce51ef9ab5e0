"""Host restatement of generate(do_sample=True, num_return_sequences=N) with num_beams == 1: the row order, the
expansion of the prompts' seen sets, the refusal table, and the shared-prompt attention in fp64."""
import math

import torch


def expand_rows(rows, N):
    """prompt-major: rows i*N .. i*N+N-1 are copies of prompt i (HF's _expand_inputs_for_generation: repeat_interleave on dim 0)"""
    return [list(r) for r in rows for _ in range(N)]


def prompt_of(row, N):
    return row // N


def seen_sets(rows, N):
    """the repetition penalty's seen ids of the b * N rows: the prompt's ids, per sibling; the image sentinel (negative) never counts"""
    return [[int(i) for i in r if int(i) >= 0] for r in expand_rows(rows, N)]


def share_refusal(fp8_kv, tp_size, q_heads, kv_heads, N):
    return bool(fp8_kv) or tp_size != 1 or not 2 <= N <= 16 or N * (q_heads // kv_heads) > 128


def refusal(N, do_sample=True, num_beams=1, b=1, max_batch=64, padded=False, ragged=False, reuse=False, lookup=False, streamer=False,
            share_prompt=None, fp8_kv=False, tp_size=1, q_heads=7, kv_heads=1):
    """the exception generate() raises before any work for these arguments, or None.  Beam search reads num_return_sequences itself."""
    if num_beams > 1 or N == 1:
        return None
    if not do_sample:
        return ValueError              # HF: greedy methods do not support num_return_sequences != 1
    if b * N > max_batch:
        return ValueError
    if padded or ragged:
        return NotImplementedError     # pad equal or use b = 1
    if reuse or lookup:
        return NotImplementedError
    if streamer:
        return ValueError
    if share_prompt and share_refusal(fp8_kv, tp_size, q_heads, kv_heads, N):
        return NotImplementedError
    return None


def attn_shared_ref(q, k, v, G, N, P, L):
    """fp64 GQA on the 16-bit-rounded inputs: q [G*N, Hq, 128], k / v [>= G*N rows, Hkv, cap, 128]; row g*N + j sees the keys [0, P) of row
    g*N and the keys [P, L) of its own row.  Evaluated in double on q's device."""
    rows, Hq, _ = q.shape
    rep = Hq // k.shape[1]
    scale = 1.0 / math.sqrt(128)
    out = torch.empty(rows, Hq, 128, dtype=torch.float64, device=q.device)
    for r in range(G * N):
        lead = (r // N) * N
        kk = torch.cat([k[lead, :, :P], k[r, :, P:L]], dim=1).double().repeat_interleave(rep, dim=0)      # [Hq, L, 128]
        vv = torch.cat([v[lead, :, :P], v[r, :, P:L]], dim=1).double().repeat_interleave(rep, dim=0)
        s = torch.einsum("hd,hld->hl", q[r].double(), kk) * scale
        out[r] = torch.einsum("hl,hld->hd", torch.softmax(s, -1), vv)
    return out
