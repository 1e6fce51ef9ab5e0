"""CPU: tests/decode_append_ref.py (the fp64 restatement that judges the fused RoPE + append decode attention in test_gpu_decode_append.py)
against independent formulations -- the oracle's RoPE, ATen's scaled_dot_product_attention -- and the calibration of that test's per-head
bound: what rounding the MFMA operands alone costs on the inputs the GPU test uses.  Also the argument checks of the C hook, which refuse
before anything touches a device."""
import ctypes as C
import pytest
import torch
import torch.nn.functional as F

import decode_append_ref as dar
import glue_ref
import oracle
from gpu_util import DT, CODE, TOL
from omchat_amd import _lib

DTS = ["bf16", "f16"]
THETA = 1e6


@pytest.mark.parametrize("dt", DTS)
def test_rope_rows_against_the_oracle(dt):
    """the bound of test_rope_kv (3e-3): the oracle rounds cos / sin and each product to T, the restatement rounds once"""
    T = DT[dt]
    pos = torch.tensor([0, 1, 63, 64, 448, 999, 4160])
    x = torch.randn(len(pos), 5, 128, generator=torch.Generator().manual_seed(3)).to(T)
    got = dar.rope_rows(x, pos, THETA, T)
    cos, sin = oracle.rope_cos_sin(pos[:, None], 128, THETA, T)               # [n, 1, 128]
    xq = x[:, :, None, :]                                                      # [n, heads, S = 1, 128]
    want, _ = oracle.apply_rope(xq, xq, cos, sin)
    err = float((got.double() - want[:, :, 0].double()).norm() / want.double().norm())
    print("rope_rows vs oracle", dt, err)
    assert err < 3e-3
    assert torch.equal(got[0], x[0])                                           # position 0 is the identity
    # a neighbouring position is far outside that bound: the comparison can tell table rows apart
    off = dar.rope_rows(x, pos + 1, THETA, T)
    assert float((off.double() - want[:, :, 0].double()).norm() / want.double().norm()) > 0.1


def test_rope_table_is_the_host_table_formula():
    """capi.hip rope_table_device written out element by element in Python floats"""
    import math
    import numpy as np
    pos = torch.tensor([0, 7, 4160])
    cos, sin = dar.rope_table(pos, THETA)
    for n, p in enumerate(pos.tolist()):
        for i in (0, 1, 31, 63):
            inv = np.float32(1.0 / math.pow(float(np.float32(THETA)), float(np.float32(2 * i) / np.float32(128.0))))
            ang = np.float32(p) * inv
            assert float(cos[n, i]) == float(np.float32(math.cos(float(ang)))) and float(sin[n, i]) == float(np.float32(math.sin(float(ang))))


@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (7, 1), (2, 2)])
def test_attend_against_aten(Hq, Hkv):
    g = torch.Generator().manual_seed(5)
    b, cap = 4, 200
    q = torch.randn(b, Hq, 128, generator=g); k = torch.randn(b, Hkv, cap, 128, generator=g); v = torch.randn(b, Hkv, cap, 128, generator=g)
    lens = [1, 64, 65, 200]
    mask = (torch.rand(b, cap, generator=g) > 0.3).to(torch.uint8)
    for i, n in enumerate(lens):
        mask[i, n - 1] = 1
    rep = Hq // Hkv
    for m in (None, mask):
        got = dar.attend(q, k, v, lens, 128 ** -0.5, m)
        vis = torch.arange(cap)[None, :] < torch.tensor(lens)[:, None]
        if m is not None:
            vis = vis & (m != 0)
        want = F.scaled_dot_product_attention(q.double()[:, :, None, :], k.double().repeat_interleave(rep, 1), v.double().repeat_interleave(rep, 1),
                                              attn_mask=vis[:, None, None, :], scale=128 ** -0.5)[:, :, 0]
        assert float((got - want).abs().max()) < 1e-12


@pytest.mark.parametrize("dt", DTS)
def test_decode_append_places_the_rows_and_reads_nothing_behind_them(dt):
    T = DT[dt]
    qkv, k, v, lens = dar.case_inputs("one_tile_ragged_8_2", T)
    b, Hq, Hkv, cap, L, _ = dar.SHAPES["one_tile_ragged_8_2"]
    kp, vp = k.clone(), v.clone()
    for i, n in enumerate(lens):
        kp[i, :, n - 1:] = float("nan"); vp[i, :, n - 1:] = float("nan")
    pos = torch.tensor(lens) - 1
    out, k2, v2, qr = dar.decode_append(qkv, kp, vp, Hq, Hkv, lens, pos, THETA, 128 ** -0.5, T)
    ref, _, _, _ = dar.decode_append(qkv, k, v, Hq, Hkv, lens, pos, THETA, 128 ** -0.5, T)
    assert torch.isfinite(out).all() and torch.equal(out, ref)
    q, kn, vn = dar.split_qkv(qkv.to(T), Hq, Hkv)
    for i, n in enumerate(lens):
        assert torch.equal(v2[i, :, n - 1], vn[i])
        assert torch.equal(k2[i, :, n - 1], dar.rope_rows(kn[i:i + 1], pos[i:i + 1], THETA, T)[0])
        assert torch.equal(k2[i, :, :n - 1], k[i, :, :n - 1].to(T)) and bool(torch.isnan(k2[i, :, n:].float()).all())
    assert torch.equal(out[0], vn[0].double().repeat_interleave(Hq // Hkv, 0))      # one key: the output is its value row
    assert dar.unpack_x is glue_ref.unpack_x                                        # one restatement of the packed layout


def _case_mask(name):
    return dar.masked_case_mask() if name == "masked" else (None, None)


@pytest.mark.parametrize("dt", DTS)
def test_operand_rounding_stays_under_half_the_bound(dt):
    """The GPU test holds every (sequence, head) to TOL[dt].  The kernels feed the PV MFMA probabilities rounded to T and rotate q / k with
    cos, sin and both products rounded to T (rope_chunk): neither is an error of the kernel.  On the GPU test's own inputs the first alone,
    and both together, must leave at least half of the bound -- else the inputs have to change, not the bound."""
    T = DT[dt]
    worst_p, worst_both = 0.0, 0.0
    for name, (b, Hq, Hkv, cap, L, _) in dar.SHAPES.items():
        qkv, k, v, lens = dar.case_inputs(name, T)
        mask, mpos = _case_mask(name)
        pos = mpos if mask is not None else torch.tensor(lens) - 1
        ref, k2, v2, qr = dar.decode_append(qkv, k, v, Hq, Hkv, lens, pos, THETA, 128 ** -0.5, T, mask)
        prounded, _, _, _ = dar.decode_append(qkv, k, v, Hq, Hkv, lens, pos, THETA, 128 ** -0.5, T, mask, p_dtype=T)
        e_p = float(dar.rel_heads(prounded, ref).max())
        # ... and with q and the fresh key rotated as the oracle (and rope_chunk) round them
        q, kn, _ = dar.split_qkv(qkv.to(T), Hq, Hkv)
        cos, sin = oracle.rope_cos_sin(pos.long()[:, None], 128, THETA, T)
        q16, k16 = oracle.apply_rope(q[:, :, None, :], kn[:, :, None, :], cos, sin)
        k3 = k2.clone()
        for i, n in enumerate(lens):
            k3[i, :, n - 1] = k16[i, :, 0]
        both = dar.attend(q16[:, :, 0], k3, v2, lens, 128 ** -0.5, mask, p_dtype=T)
        e_b = float(dar.rel_heads(both, ref).max())
        print(f"operand rounding {dt} {name}: P alone {e_p:.3e}, P and 16-bit RoPE {e_b:.3e}")
        worst_p, worst_both = max(worst_p, e_p), max(worst_both, e_b)
    print(f"operand rounding {dt}: worst per head, P alone {worst_p:.3e}, P and 16-bit RoPE {worst_both:.3e}, bound {TOL[dt]:.1e}")
    assert worst_p <= TOL[dt] / 2 and worst_both <= TOL[dt] / 2


def test_masked_case_hides_whole_tiles():
    mask, pos = dar.masked_case_mask()
    b, _, _, _, L, _ = dar.SHAPES["masked"]
    assert mask.shape == (b, dar.MASK_SB) and dar.MASK_SB % 64 == 0 and int(mask[:, L:].sum()) == 0 and bool((mask[:, L - 1] == 1).all())
    hidden_tiles = [int((mask[i].view(-1, 64).sum(1) == 0)[: (L + 63) // 64].sum()) for i in range(b)]
    assert hidden_tiles == [0, 0, 1, 2]
    assert pos.tolist() == [int(mask[i].sum()) - 1 for i in range(b)] and all(int(p) != L - 1 for p in pos[1:])


def test_hook_refuses_bad_arguments_before_touching_a_device():
    """every refusal of omchat_op_attn_decode_append comes before the RoPE table is allocated: it must answer on a machine without a GPU,
    with pointers that are never dereferenced"""
    lib = _lib.lib()
    P = C.c_void_p(4096)

    def call(qkv=P, k=P, v=P, out=P, ws=P, cap=128, L=64, kv_len=None, pos=None, mask=None):
        return lib.omchat_op_attn_decode_append(CODE["bf16"], qkv, THETA, k, v, out, 2, 8, 2, cap, L, kv_len, pos, mask, 64, 0, 128 ** -0.5, ws, 1 << 20, None)

    for kw in (dict(qkv=None), dict(k=None), dict(v=None), dict(out=None), dict(ws=None), dict(L=0), dict(L=-3), dict(L=129), dict(mask=P),
               dict(mask=P, pos=P, kv_len=P)):
        assert call(**kw) != 0, kw
        assert len(lib.omchat_last_error()) > 0, kw
