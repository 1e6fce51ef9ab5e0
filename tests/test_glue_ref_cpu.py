"""CPU (no GPU): every reference of tests/glue_ref.py against an independent formulation of the same operation, so that a reference cannot be
wrong in the same way as the kernel it judges (tests/test_gpu_glue_ops.py)."""
import pytest
import torch
import torch.nn.functional as F

import glue_ref as gr
import oracle
from gpu_util import randn


def test_im2col_is_unfold_and_conv2d():
    for B, HW, patch, Kpad in [(2, 28, 14, 640), (2, 12, 4, 64)]:
        px = randn((B, 3, HW, HW), 1)
        cols = gr.im2col(px, patch, Kpad)
        K = 3 * patch * patch
        unf = F.unfold(px, kernel_size=patch, stride=patch).transpose(1, 2).reshape(-1, K)      # [B * g * g, (channel, ky, kx)]
        assert torch.equal(cols[:, :K], unf)
        assert Kpad > K and float(cols[:, K:].abs().max()) == 0.0
        W = randn((5, 3, patch, patch), 2).double()
        conv = F.conv2d(px.double(), W, stride=patch)                                       # [B, 5, g, g]
        got = (cols[:, :K].double() @ W.reshape(5, K).t()).view(B, HW // patch, HW // patch, 5).permute(0, 3, 1, 2)
        assert torch.allclose(got, conv, rtol=1e-12, atol=1e-12)


def test_rope_at_arbitrary_positions_is_the_oracle_rope():
    b, S, H, theta = 3, 5, 4, 1e6
    pos = torch.tensor([[0, 89, 17, 3, 40], [17, 0, 88, 89, 5], [2, 2 + 60, 1, 0, 89]])
    x = randn((b * S, H, 128), 3)
    got = gr.rope_rotate(x, pos.reshape(-1), theta).view(b, S, H, 128).transpose(1, 2)
    cos, sin = oracle.rope_cos_sin(pos, 128, theta, torch.float32)
    xq = x.view(b, S, H, 128).transpose(1, 2)
    ref, _ = oracle.apply_rope(xq, xq, cos, sin)
    # the oracle evaluates inv_freq, the angle, cos / sin and the rotation in fp32: the angle (<= 89 rad) carries up to ~2 ulp of relative error
    # (inv_freq's pow, the product), i.e. 89 * 2 * 2^-23 rad, which moves a rotated value by that times |x|; the rotation adds a few fp32 ulp of |x|
    bound = (89 * 2 * 2.0 ** -23 + 4 * 2.0 ** -23) * float(x.abs().max()) * 2 ** 0.5
    assert float((got - ref.double()).abs().max()) < bound
    # position 0 is the identity
    z = gr.rope_rotate(x, torch.zeros(b * S, dtype=torch.long), theta)
    assert torch.equal(z, x.double())


def test_rope_slots():
    pr, pp = gr.rope_slots(2, 3, None, 5, -1)
    assert pr.tolist() == [5, 6, 7, 5, 6, 7] and pp.tolist() == pr.tolist()
    pos = torch.tensor([9, 0, 4, 4, 7, 1])
    pr, pp = gr.rope_slots(2, 3, pos, 5, -1)
    assert pr.tolist() == pos.tolist() and pp.tolist() == pos.tolist()
    pr, pp = gr.rope_slots(2, 3, pos, 5, 20)
    assert pr.tolist() == pos.tolist() and pp.tolist() == [20, 21, 22, 20, 21, 22]


def _inputs(b, Sq, Skv, Hq, Hkv, seed):
    return randn((b, Sq, Hq, 16), seed), randn((b, Hkv, Skv, 16), seed + 1), randn((b, Hkv, Skv, 16), seed + 2)


@pytest.mark.parametrize("causal", [0, 1])
def test_attn_without_left_padding_is_the_ops_reference(causal):
    from test_gpu_ops import _attn_ref
    b, Sq, Skv, Hq, Hkv = 2, 37, 37, 4, 2
    q, k, v = _inputs(b, Sq, Skv, Hq, Hkv, 10)
    lens = [37, 20]
    got = gr.attn_left(q, k, v, 0.25, causal, 0, lens, [0, 0])
    ref = _attn_ref(q.double(), k.double(), v.double(), 0.25, causal, 0, lens)
    for i in range(b):
        n = lens[i]      # beyond the length the two differ by design (NaN there against 0 here when nothing is visible)
        assert torch.allclose(got[i, :n], ref[i, :n], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("causal", [0, 1])
def test_attn_with_left_padding_is_an_additive_mask(causal):
    b, Sq, Skv, Hq, Hkv = 3, 41, 41, 6, 2
    q, k, v = _inputs(b, Sq, Skv, Hq, Hkv, 20)
    start, lens = [0, 7, 30], [41, 41, 36]
    got = gr.attn_left(q, k, v, 0.3, causal, 0, lens, start)
    neg = torch.finfo(torch.float64).min
    for i in range(b):
        mask = torch.zeros(Sq, Skv, dtype=torch.float64)
        for r in range(Sq):
            for j in range(Skv):
                if j < start[i] or j >= lens[i] or (causal and j > r):
                    mask[r, j] = neg
        for h in range(Hq):
            s = (q[i, :, h].double() @ k[i, h // 3].double().t()) * 0.3 + mask
            ref = torch.softmax(s, dim=-1) @ v[i, h // 3].double()
            live = (mask > neg).any(dim=1)           # a fully masked row: uniform under an additive mask, 0 here
            assert torch.allclose(got[i, live, h], ref[live], rtol=1e-10, atol=1e-12)
            assert float(got[i, ~live, h].abs().max()) == 0.0 if (~live).any() else True
            if causal:
                assert (~live).sum() == start[i]
    # a leaked padding key would show: the visible set does not depend on what the masked rows hold
    k2, v2 = k.clone(), v.clone()
    k2[1, :, :7] = 50.0; v2[1, :, :7] = 1000.0
    again = gr.attn_left(q, k2, v2, 0.3, causal, 0, lens, start)
    assert torch.equal(again, got)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_uniform_rows_are_the_softmax_of_a_fully_masked_row(dtype):
    """modeling_qwen2.py:150-172 on a row whose scores are all finfo.min: softmax in fp32, cast to the activation dtype, times V"""
    Skv = 330
    v = randn((2, 3, Skv, 8), 5).to(dtype)
    s = torch.full((Skv,), torch.finfo(dtype).min, dtype=dtype)
    p = torch.softmax(s.float(), dim=-1).to(dtype)
    assert float(p.float().min()) == float(p.float().max())
    ref = torch.einsum("k,bhkd->bhd", p.double(), v.double())
    got = gr.uniform_rows(v, dtype)
    assert torch.allclose(got, ref, rtol=1e-12, atol=1e-14)


def test_copy_rows_map_is_the_loop():
    for rows, group, skip in [(12, 4, 1), (15, 5, 0), (7, 1, 2), (13, 4, 1)]:
        want = []
        for r in range(rows):
            blk, inside = divmod(r, group)
            want.append(blk * (group + skip) + skip + inside)
        assert gr.copy_rows_map(rows, group, skip).tolist() == want
    # the ViT's use: drop the CLS row of every image
    assert gr.copy_rows_map(6, 3, 1).tolist() == [1, 2, 3, 5, 6, 7]


def test_gather_rows_and_vit_assemble():
    table = randn((5, 8), 1); feats = randn((3, 8), 2)
    idx = torch.tensor([4, -1, gr.INT_MIN, 0, -3], dtype=torch.int32)
    out = gr.gather_rows(idx, table, feats)
    loop = torch.zeros(5, 8)
    for r, i in enumerate(idx.tolist()):
        if i != gr.INT_MIN:
            loop[r] = table[i] if i >= 0 else feats[-1 - i]
    assert torch.equal(out, loop)
    assert torch.equal(out[0], table[4]) and torch.equal(out[1], feats[0]) and torch.equal(out[4], feats[2]) and torch.equal(out[3], table[0])
    assert float(out[2].abs().max()) == 0.0
    B, np_, C = 3, 4, 8
    T = torch.bfloat16
    pe = randn((B * np_, C), 3).to(T); cls = randn((C,), 4).to(T); pos = randn((np_ + 1, C), 5).to(T)
    x = gr.vit_assemble(pe, cls, pos, B, np_, T)
    for b in range(B):
        assert torch.equal(x[b, 0], (cls.float() + pos[0].float()).to(T))
        for p in range(np_):
            assert torch.equal(x[b, 1 + p], (pe[b * np_ + p].float() + pos[1 + p].float()).to(T))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_tp_finish_is_the_gemm_epilogue_reference(dt):
    """the rounding sequence restated two ways: glue_ref.tp_finish and test_gpu_ops._gemm_ref (which starts from A and W)"""
    from test_gpu_ops import _gemm_ref
    from gpu_util import DT, rnd
    M, N, K = 9, 16, 32
    A = rnd(randn((M, K), 1), dt); W = rnd(randn((N, K), 2, 0.05), dt)
    bias = rnd(randn((N,), 3, 0.1), dt); ls = rnd(randn((N,), 4, 0.1) + 0.1, dt); resid = rnd(randn((M, N), 5), dt)
    T = DT[dt]
    for epi in (gr.EPI_NONE, gr.EPI_RESID, gr.EPI_LS_RESID):
        for bb in (None, bias):
            got = gr.tp_finish(A @ W.t(), None if bb is None else bb.to(T), ls.to(T), resid.to(T), epi, T)
            ref = _gemm_ref(A, W, bb, ls, resid, epi, dt).to(T)
            assert torch.equal(got, ref), (epi, bb is None)


def test_residual_adds():
    T = torch.bfloat16
    x = randn((3, 16), 1).to(T); part = randn((3, 3, 16), 2)
    want = (x.float() + ((part[0] + part[1]) + part[2]).to(T).float()).to(T)
    assert torch.equal(gr.resid_sum(x, part, T), want)
    y = randn((3, 16), 3).to(T)
    assert torch.equal(gr.resid16(x, y, T), (x.float() + y.float()).to(T))


def test_packed_x_index_inverts_the_view_form():
    """the index formula of common.h against the reshape / permute statement of the same layout (tests/test_gpu_round2.py)"""
    for rows, K, NB in [(3, 128, 1), (16, 2048, 1), (19, 192, 2), (32, 64, 2)]:
        x = torch.arange(rows * K, dtype=torch.float32).view(rows, K)
        full = torch.zeros(NB * 16, K); full[:rows] = x
        packed = full.view(NB, 16, K // 64, 2, 4, 8).permute(2, 3, 0, 4, 1, 5).reshape(-1)      # [chunk][half][nb][g][row % 16][j]
        assert torch.equal(gr.unpack_x(packed, rows, K, NB), x)
