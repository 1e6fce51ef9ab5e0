"""CPU restatements of the row / glue kernels (omchat_amd/csrc/elementwise.hip) and of left-padded prefill attention (attention.hip:
AttnArgs.kv_start, launch_attn_uniform_rows) in plain torch.  fp64 where arithmetic happens; the copy kernels are exact indexing; the kernels
whose contract is a rounding sequence (tp_finish, the residual adds, vit_assemble) restate that sequence in fp32 with `.to(T)` at each
rounding point.  tests/test_glue_ref_cpu.py checks every function here against an independent formulation."""
import torch

INT_MIN = -(2 ** 31)
EPI_NONE, EPI_LS_RESID, EPI_RESID = 0, 2, 3


# ------------------------------------------------------------------------------------------------ attention
def attn_left(q, k, v, scale, causal, q_pos0, kv_len, kv_start):
    """q [b, Sq, Hq, D], k / v [b, Hkv, Skv, D] -> [b, Sq, Hq, D] in fp64.  Key j of sequence i is visible to query row r iff
    kv_start[i] <= j < kv_len[i] and (not causal or j <= r + q_pos0) (kernels.h AttnArgs).  A row without a visible key gives 0:
    what the flash kernel leaves there (attn_common.h M_FLOOR)."""
    q, k, v = q.double(), k.double(), v.double()
    b, Sq, Hq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    rep = Hq // Hkv
    out = torch.zeros(b, Sq, Hq, D, dtype=torch.float64)
    for i in range(b):
        lo, hi = int(kv_start[i]), int(kv_len[i])
        for h in range(Hq):
            kh, vh = k[i, h // rep], v[i, h // rep]
            s = (q[i, :, h] @ kh.t()) * scale                                   # [Sq, Skv]
            j = torch.arange(Skv)[None, :]
            vis = (j >= lo) & (j < hi)
            if causal:
                vis = vis & (j <= torch.arange(Sq)[:, None] + q_pos0)
            else:
                vis = vis.expand(Sq, Skv)
            s = torch.where(vis, s, torch.full_like(s, -float("inf")))
            m = s.max(dim=1, keepdim=True).values
            m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
            e = torch.exp(s - m)
            l = e.sum(dim=1, keepdim=True)
            p = torch.where(l > 0, e / l.clamp_min(1e-300), torch.zeros_like(e))
            out[i, :, h] = p @ vh
    return out


def uniform_rows(v, dtype):
    """the fill of launch_attn_uniform_rows: sum_j T(1 / Skv) * V[j] over ALL Skv keys, v [b, Hkv, Skv, D] -> [b, Hkv, D] fp64"""
    Skv = v.shape[2]
    w = torch.tensor(1.0 / Skv, dtype=torch.float32).to(dtype).double()
    return (v.double() * w).sum(dim=2)


# ------------------------------------------------------------------------------------------------ RoPE
def rope_rotate(x, pos, theta):
    """rotate-half RoPE of x [rows, heads, d] at the integer positions pos [rows], fp64 arithmetic on the fp32 angle of the table
    (capi.hip rope_table_device: inv_freq and position * inv_freq in fp32)"""
    d = x.shape[-1]
    inv = (1.0 / (torch.tensor(float(theta), dtype=torch.float64) ** (torch.arange(0, d, 2, dtype=torch.float32).double() / d))).float()
    ang = (pos.float()[:, None] * inv[None, :]).double()                        # [rows, d / 2]
    cos = torch.cat((ang.cos(), ang.cos()), dim=-1)[:, None, :]
    sin = torch.cat((ang.sin(), ang.sin()), dim=-1)[:, None, :]
    x = x.double()
    rot = torch.cat((-x[..., d // 2:], x[..., :d // 2]), dim=-1)
    return x * cos + rot * sin


def rope_slots(b, S, pos, pos0, slot0):
    """(position, cache slot) of every row r = i * S + s as rope_kv_kernel derives them: position pos[r] or pos0 + s, slot slot0 + s or the position"""
    s = torch.arange(b * S) % S
    pr = pos.long() if pos is not None else pos0 + s
    pp = slot0 + s if slot0 >= 0 else pr
    return pr, pp


# ------------------------------------------------------------------------------------------------ copies
def im2col(px, patch, Kpad):
    """pixels [B, 3, HW, HW] -> cols [B * g * g, Kpad]: row (b, py, px), column (channel, ky, kx), zeros beyond 3 * patch^2"""
    B, Cn, HW, _ = px.shape
    g = HW // patch
    c = px.view(B, Cn, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, Cn * patch * patch)
    out = torch.zeros(B * g * g, Kpad, dtype=px.dtype)
    out[:, :c.shape[1]] = c
    return out


def vit_assemble(pe, cls, pos, B, np_, dtype):
    """x [B, np + 1, C]: x[b, 0] = cls + pos[0], x[b, 1 + p] = pe[b * np + p] + pos[1 + p]; the fp32 sum rounded once to dtype"""
    C = pe.shape[-1]
    tok = torch.cat((cls.float().view(1, 1, C).expand(B, 1, C), pe.float().view(B, np_, C)), dim=1)
    return (tok + pos.float()[None]).to(dtype)


def gather_rows(idx, table, feats):
    """out[r] = table[idx[r]] (idx >= 0) | feats[-1 - idx[r]] (idx < 0) | zeros (idx == INT_MIN); exact indexing"""
    i = idx.long()
    pad = i == INT_MIN
    from_table = i >= 0
    t = table[torch.where(from_table, i, torch.zeros_like(i))]
    f = feats[torch.where(~from_table & ~pad, -1 - i, torch.zeros_like(i))]
    out = torch.where(from_table[:, None], t, f)
    return torch.where(pad[:, None], torch.zeros_like(out), out)


def copy_rows_map(rows, group, skip):
    """source row of destination row r: (r / group) * (group + skip) + skip + r % group"""
    r = torch.arange(rows)
    return (r // group) * (group + skip) + skip + r % group


# ------------------------------------------------------------------------------------------------ epilogues / residual adds
def tp_finish(sum_, bias, ls, resid, epi, dtype):
    """elementwise.hip tp_finish_kernel: EPI_NONE T(sum + b), EPI_RESID T(r + T(sum + b)), EPI_LS_RESID T(r + T(T(sum + b) * ls)); fp32 adds and
    products, no contraction.  16-bit operands, fp32 sum [M, N]."""
    v = sum_.float()
    if bias is not None:
        v = v + bias.float()[None]
    if epi == EPI_NONE:
        return v.to(dtype)
    v = v.to(dtype).float()
    if epi == EPI_LS_RESID:
        v = (v * ls.float()[None]).to(dtype).float()
    return (resid.float() + v).to(dtype)


def resid_sum(x, part, dtype):
    """resid_rmsnorm_kernel's first half: T(x + T(sum_s part[s])), the fp32 slices [ks, rows, H] added in slice order"""
    a = torch.zeros_like(part[0])
    for s in range(part.shape[0]):
        a = a + part[s]
    return (x.float() + a.to(dtype).float()).to(dtype)


def resid16(x, y, dtype):
    return (x.float() + y.float()).to(dtype)


# ------------------------------------------------------------------------------------------------ packed x layout
def packed_x_index(row, k, NB):
    """common.h packed_x_index, elementwise on integer tensors"""
    return ((((k >> 6) * 2 + ((k >> 5) & 1)) * NB + (row >> 4)) * 64 + (row & 15) + 16 * ((k >> 3) & 3)) * 8 + (k & 7)


def unpack_x(packed, rows, K, NB):
    """row-major [rows, K] view of a buffer in the packed x layout (flat, NB * 16 * K elements)"""
    r = torch.arange(rows)[:, None].expand(rows, K)
    k = torch.arange(K)[None, :].expand(rows, K)
    return packed.reshape(-1)[packed_x_index(r, k, NB)]
