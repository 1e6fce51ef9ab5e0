"""The weight-format table of the decode step (csrc/ctx.h: one table per format of omchat_weight_format): every replica is allocated exactly once
with exactly its derived size, rebuilt in place after a weight reload, and switching formats leaves no residue in the 16-bit step."""
import pytest
import torch

pytestmark = pytest.mark.gpu
from gpu_util import rnd, randn, sync
from test_gpu_mxfp4 import _decoder_sd
from omchat_amd.config import tiny
from omchat_amd.engine import Engine


def _shapes(cfg):
    """(N, K) of the layers * 4 + 1 matrices a decode step streams: qkv, o_proj, gate|up, down_proj per layer, then the lm_head"""
    t = cfg.text
    H, It, V = t["hidden_size"], t["intermediate_size"], t["vocab_size"]
    qd, kvd = t["num_attention_heads"] * 128, t["num_key_value_heads"] * 128
    return [(qd + 2 * kvd, H), (H, qd), (2 * It, H), (H, It)] * t["num_hidden_layers"] + [(V, H)]


def _engine(dt="bf16"):
    cfg = tiny()
    e = Engine(cfg, dtype=dt, max_seq=64, max_batch=2, vision=False)
    sd = _decoder_sd(cfg, 7)
    e.load_state_dict(sd)
    return cfg, sd, e


def test_replica_bytes_are_counted_once_and_rebuilt_in_place(gpu_lib):
    cfg, sd, e = _engine()
    shapes = _shapes(cfg)
    e4m3 = sum(N * K + 4 * N for N, K in shapes)
    mx4 = sum(N * K // 2 + N * K // 32 for N, K in shapes)
    pk16 = sum(2 * N * K for N, K in shapes)
    x = rnd(randn((2, 8, 256), 1, 0.5), "bf16")
    toks = torch.tensor([5, 6], dtype=torch.int32)
    e.prefill(x[:1]); e.decode_step(toks[:1]); sync()              # a 16-bit b = 1 step builds nothing
    base = e.device_bytes()

    def grew():
        nonlocal base
        now = e.device_bytes()
        d, base = now - base, now
        return d

    e.enable_fp8_decode(True)
    assert grew() == e4m3
    e.enable_fp8_decode(True); e.decode_step(toks[:1])
    assert grew() == 0
    e.enable_fp8_decode(False)
    e.enable_mxfp4_decode(True)
    assert grew() == mx4
    e.enable_mxfp4_decode(True); e.decode_step(toks[:1])
    assert grew() == 0
    e.enable_mxfp4_decode(True, batched=True)                      # mode 2: the same codes and scales once more, packed
    assert grew() == mx4
    e.enable_mxfp4_decode(True, batched=True)
    e.prefill(x); e.decode_step(toks)                              # a b = 2 step on the packed MXFP4 replica: no 16-bit packed one
    assert grew() == 0
    e.enable_mxfp4_decode(False)
    e.decode_step(toks)                                            # the first b = 2 step with no MXFP4
    assert grew() == pk16
    e.decode_step(toks); sync()
    assert grew() == 0
    # a reload leaves every replica stale; the next step of each format rebuilds its own in place
    key = "model.layers.1.mlp.down_proj.weight"
    e.load_tensor(key, rnd(randn(tuple(sd[key].shape), 9, 0.05), "bf16"))
    e.decode_step(toks)                                            # 16-bit packed
    assert grew() == 0
    e.enable_mxfp4_decode(True, batched=True); e.decode_step(toks)           # MXFP4, row-major and packed
    assert grew() == 0
    e.enable_mxfp4_decode(False); e.enable_fp8_decode(True)
    e.prefill(x[:1]); e.decode_step(toks[:1]); sync()              # e4m3
    assert grew() == 0
    e.close()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_switching_formats_leaves_no_residue(gpu_lib, dt):
    cfg, sd, e = _engine(dt)
    x = rnd(randn((1, 10, 256), 3, 0.5), dt)
    tok = torch.tensor([11], dtype=torch.int32)
    e.prefill(x)
    n16, l16 = e.decode_step(tok, want_logits=True); e.kv_rewind(1)
    e.enable_fp8_decode(True)
    n8, l8 = e.decode_step(tok, want_logits=True); e.kv_rewind(1)
    e.enable_fp8_decode(False); e.enable_mxfp4_decode(True)
    n4, l4 = e.decode_step(tok, want_logits=True); e.kv_rewind(1)
    e.enable_mxfp4_decode(False)
    n, l = e.decode_step(tok, want_logits=True); sync()
    assert torch.equal(l, l16) and torch.equal(n, n16)
    assert not torch.equal(l8, l16) and not torch.equal(l4, l16) and not torch.equal(l4, l8)      # each replica was really read
    e.close()
