"""The MXFP4 reference quantiser (tests/mxfp4_ref.py) pinned by hand-written vectors, and the generate() refusal that needs no device."""
import types
import pytest
import torch

from mxfp4_ref import quant_ref, pack, GRID


def _block(vals, fill=0.0):
    w = torch.full((1, 32), fill, dtype=torch.float32)
    w[0, :len(vals)] = torch.tensor(vals, dtype=torch.float32)
    return w


def test_ties_go_to_the_even_code_and_7p9_saturates():
    # 7.9 is the block's absmax: floor(log2) = 2, e = 0, so the other values are their own scaled values
    vals = [7.9, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    codes, s, deq = quant_ref(_block(vals))
    assert int(s[0, 0]) == 127
    assert deq[0, :8].tolist() == want
    assert codes[0, :8].tolist() == [7, 0, 2, 2, 4, 4, 6, 6]
    # just off the ties: the nearer neighbour
    codes, _, deq = quant_ref(_block([7.9, 0.26, 0.74, 1.26, 1.74, 2.51, 3.49, 5.01]))
    assert deq[0, :8].tolist() == [6.0, 0.5, 0.5, 1.5, 1.5, 3.0, 3.0, 6.0]


def test_scales():
    _, s, deq = quant_ref(_block([8.0, 1.0]))                # absmax 8: floor(log2) = 3, e = 1
    assert int(s[0, 0]) == 128 and deq[0, :2].tolist() == [8.0, 1.0]
    _, s, deq = quant_ref(_block([7.999]))                   # just below: e = 0, saturates at 6
    assert int(s[0, 0]) == 127 and float(deq[0, 0]) == 6.0
    codes, s, deq = quant_ref(_block([]))                    # a zero block: byte 127, codes 0
    assert int(s[0, 0]) == 127 and int(codes.max()) == 0 and float(deq.abs().max()) == 0.0
    _, s, _ = quant_ref(_block([2.0 ** -20]))
    assert int(s[0, 0]) == 127 - 20 - 2
    _, s, _ = quant_ref(_block([3.0e38]))                    # floor(log2) = 127: e = 125
    assert int(s[0, 0]) == 252
    # two blocks of one row scale independently
    w = torch.cat([_block([4.0, 1.0]), _block([0.5, 0.125])], dim=1)
    _, s, deq = quant_ref(w)
    assert s[0].tolist() == [127, 124] and deq[0, [0, 1, 32, 33]].tolist() == [4.0, 1.0, 0.5, 0.125]


def test_negative_values_and_the_sign_bit():
    codes, s, deq = quant_ref(_block([-7.9, -0.25, -0.75, -2.5, -5.0, 3.0, -3.0, -0.0]))
    assert int(s[0, 0]) == 127
    assert deq[0, :8].tolist() == [-6.0, 0.0, -1.0, -2.0, -4.0, 3.0, -3.0, 0.0]
    assert codes[0, :8].tolist() == [15, 0, 10, 12, 14, 5, 13, 0]      # no sign on a zero code
    assert pack(codes)[0, :4].tolist() == [0x0f, 0xca, 0x5e, 0x0d]     # the even k in the low nibble


def test_requantising_the_dequantised_values_is_a_fixed_point():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(64, 256, generator=g) * 0.02
    w[3] = 0
    w[5, 7] = 3.0
    w[6] = torch.linspace(-1, 1, 256)
    w[7] *= 1e-6
    w[8] *= 1e3
    c0, s0, d0 = quant_ref(w)
    c1, s1, d1 = quant_ref(d0)
    assert torch.equal(c0, c1) and torch.equal(s0, s1) and torch.equal(d0, d1)
    # every code is used, and the relative RMS element error on Gaussian weights is the format's ~0.11
    assert len(torch.unique(c0)) >= 15
    r = torch.randn(512, 3584, generator=g) * 0.02
    err = float((quant_ref(r)[2] - r.double()).norm() / r.double().norm())
    assert 0.09 < err < 0.13, err


def test_grid_is_e2m1():
    # e2m1: 1 sign, 2 exponent (bias 1), 1 mantissa bit
    vals = []
    for code in range(8):
        ex, man = code >> 1, code & 1
        vals.append(man * 0.5 if ex == 0 else (1 + man * 0.5) * 2.0 ** (ex - 1))
    assert vals == GRID.tolist()


class _RefusalOnly:
    """an engine generate() must not reach before it refuses: MXFP4 decode is on, everything else fails the test"""
    c = types.SimpleNamespace(t_vocab_total=320, max_seq=64)
    tp_size = 1
    _fp8_kv = False

    def __init__(self, on):
        self._mxfp4_decode = on

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} used before the refusal")


def test_generate_refuses_prompt_lookup_while_mxfp4_decode_is_on():
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    m = object.__new__(OmChatQwen2ForCausalLM)
    gc = types.SimpleNamespace(eos_token_id=None, pad_token_id=None, max_new_tokens=4, do_sample=False)
    m.__dict__.update(generation_config=gc, engine=_RefusalOnly(True), config=types.SimpleNamespace(tokenizer_padding_side="right"))
    ids = torch.tensor([[1, 2, 3, 4]])
    with pytest.raises(NotImplementedError, match="MXFP4"):
        m.generate(ids, prompt_lookup_num_tokens=4, max_new_tokens=2)
