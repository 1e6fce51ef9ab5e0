"""Host side of MXFP4 decode mode 2 (Engine.enable_mxfp4_decode(batched=True)): generate() refuses
prompt_lookup_num_tokens only while the verify step would still read the 16-bit weights, i.e. in mode 1."""
import types

import numpy as np
import pytest
import torch


# ---- the packed MXFP4 layout (csrc/common.h: packed_w4_index / packed_s4_index), restated; vectorised over numpy arrays
def packed_w4_index(row, k, K):
    """index of the dword that holds code (row, k), in nibble k & 7"""
    return (((row >> 4) * (K >> 6) + (k >> 6)) * 2 + ((k >> 5) & 1)) * 64 + (row & 15) + 16 * ((k >> 3) & 3)


def packed_s4_index(row, blk, K):
    """index of the e8m0 byte of (row, block of 32 k)"""
    return ((((row >> 4) * (K >> 6) + (blk >> 1)) * 4 + ((row & 15) >> 2)) * 2 + (blk & 1)) * 4 + (row & 3)


@pytest.mark.parametrize("N,K", [(16, 64), (48, 192), (32, 576)])
def test_packed_layout_index_against_a_brute_force_walk(N, K):
    """walk the layout as the documents state it -- codes [tile][chunk][half][lane], lane l = row 16 tile + (l & 15), k = 64 chunk + 32 half +
    8 (l >> 4); scales [tile][chunk][lane group][half][4 rows] -- and compare every position with the index formulas; both are bijections"""
    pos, seen = 0, np.full((N, K // 8), -1)
    for tile in range(N // 16):
        for chunk in range(K // 64):
            for half in range(2):
                for lane in range(64):
                    row, k = 16 * tile + (lane & 15), 64 * chunk + 32 * half + 8 * (lane >> 4)
                    assert packed_w4_index(row, k, K) == pos and packed_w4_index(row, k + 7, K) == pos
                    seen[row, k // 8] = pos
                    pos += 1
    assert pos == N * K // 8 and (seen >= 0).all()
    pos, seen = 0, np.full((N, K // 32), -1)
    for tile in range(N // 16):
        for chunk in range(K // 64):
            for g in range(4):
                for half in range(2):
                    for r in range(4):
                        row, blk = 16 * tile + 4 * g + r, 2 * chunk + half
                        assert packed_s4_index(row, blk, K) == pos
                        seen[row, blk] = pos
                        pos += 1
    assert pos == N * K // 32 and (seen >= 0).all()
    rows, blk = np.meshgrid(np.arange(N), np.arange(K // 32), indexing="ij")
    assert np.array_equal(packed_s4_index(rows, blk, K), seen)               # the vectorised use of the GPU test


class _RefusalOnly:
    """an engine generate() must not reach before it refuses; past the MXFP4 refusal the first engine use fails with AssertionError"""
    c = types.SimpleNamespace(t_vocab_total=320, max_seq=64)
    tp_size = 1
    _fp8_kv = False

    def __init__(self, **flags):
        self.__dict__.update(flags)

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} used")


def _model(engine):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    m = object.__new__(OmChatQwen2ForCausalLM)
    gc = types.SimpleNamespace(eos_token_id=None, pad_token_id=None, max_new_tokens=4, do_sample=False)
    m.__dict__.update(generation_config=gc, engine=engine, config=types.SimpleNamespace(tokenizer_padding_side="right"))
    return m


IDS = torch.tensor([[1, 2, 3, 4]])


def test_generate_accepts_prompt_lookup_in_batched_mode():
    m = _model(_RefusalOnly(_mxfp4_decode=True, _mxfp4_batched=True))
    # past the refusal: the stub fails the first real engine call, which is not the NotImplementedError that names MXFP4
    with pytest.raises(AssertionError, match="engine"):
        m.generate(IDS, prompt_lookup_num_tokens=4, max_new_tokens=2)


@pytest.mark.parametrize("flags", [dict(_mxfp4_decode=True, _mxfp4_batched=False), dict(_mxfp4_decode=True)])
def test_generate_still_refuses_prompt_lookup_in_mode_1(flags):
    m = _model(_RefusalOnly(**flags))
    with pytest.raises(NotImplementedError, match="MXFP4"):
        m.generate(IDS, prompt_lookup_num_tokens=4, max_new_tokens=2)


def test_enable_passes_the_mode_and_keeps_the_flags_on_a_refusal():
    from omchat_amd.engine import Engine
    calls = []

    class Lib:
        rc = 0

        def omchat_enable_mxfp4_decode(self, h, mode):
            calls.append(mode)
            return self.rc

        def omchat_last_error(self):
            return b"refused"

    e = object.__new__(Engine)
    e.__dict__.update(lib=Lib(), h=None)
    e.enable_mxfp4_decode(True)
    assert calls == [1] and e._mxfp4_decode and not e._mxfp4_batched
    e.enable_mxfp4_decode(True, batched=True)
    assert calls == [1, 2] and e._mxfp4_decode and e._mxfp4_batched
    e.lib.rc = 1
    with pytest.raises(Exception):
        e.enable_mxfp4_decode(False)
    assert e._mxfp4_decode and e._mxfp4_batched                 # a refusal leaves the flags as they were
    e.lib.rc = 0
    e.enable_mxfp4_decode(False, batched=True)
    assert calls[-1] == 0 and not e._mxfp4_decode and not e._mxfp4_batched
