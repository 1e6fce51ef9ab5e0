"""GPU: the four-wave form of the 16-bit one-tile decode attention (attention.hip attn_decode_4w_kernel, tuning key 52) against the one-wave form
(attn_decode_kernel, key 52 = 0) through omchat_op_attn_decode (q rotated, cache complete) and omchat_op_attn_decode_append (fused RoPE + append).
The four-wave form splits a tile's loads, LDS traffic, PV product and stores among four waves without changing the order of any sum, so everything
is compared BIT FOR BIT (integer views: the poison is NaN):
  * the fp32 partial workspace -- o, m, l of every split, the neutral (m, l) of empty trailing splits, and the poison everywhere else;
  * the merged output rows;
  * the K / V caches after the call: the appended rows equal, every slot outside [0, kv_len) -- NaN before the call -- untouched.
kv_len covers a partial first 16-key sub-block (1, 15), sub-block and tile edges (16, 17, 63, 64, 65, 127, 128, 129: the new position first / last
in its tile) and 57 splits (3585); the launch is sized for kv_len + 70 keys, so one or two trailing splits are empty.  GQA groups of 7, 4 and 1."""
import functools
import pytest
import torch

pytestmark = pytest.mark.gpu
from gpu_util import DT, CODE, ptr, sync
from omchat_amd import _lib

NAN = float("nan")
THETA = 1e6
SCALE = 128 ** -0.5
KV_LENS = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 3585]
HEADS = [(28, 4), (8, 2), (4, 4)]
SLACK = 70          # keys the launch is sized for beyond kv_len: the workspace has more splits than the length uses
KEY_4W = 52


def lens_of(kv_len, b):
    """sequence 0 holds kv_len keys; a second sequence a shorter cache with the new position elsewhere in its tile"""
    return [kv_len, max(1, kv_len - 37)][:b]


@functools.lru_cache(maxsize=2)
def _inputs(dt, Hq, Hkv, b, kv_len, rope, big_row):
    """(qkv, k, v, lens, L, cap) on the device, seeded, poison in place; shared and never modified (every call works on clones)"""
    T = DT[dt]
    lens = lens_of(kv_len, b)
    L = kv_len + SLACK
    cap = (L + 63) // 64 * 64
    g = torch.Generator(device="cuda").manual_seed(1000 * kv_len + 10 * Hq + b)
    qkv = torch.randn(b, Hq + 2 * Hkv, 128, device="cuda", generator=g).to(T)
    k = torch.randn(b, Hkv, cap, 128, device="cuda", generator=g).to(T)
    v = torch.randn(b, Hkv, cap, 128, device="cuda", generator=g).to(T)
    if big_row is not None:      # one key far above the rest: its split's maximum dwarfs the others', the merge rescales them to ~0
        k[:, :, big_row] *= 30.0
    for i, n in enumerate(lens):
        first_free = n - 1 if rope else n      # fused append: slot n - 1 is the one being written
        k[i, :, first_free:] = NAN; v[i, :, first_free:] = NAN
    return qkv, k, v, lens, L, cap


def run(lib, dt, Hq, Hkv, b, kv_len, rope, key, big_row=None):
    """one launch under tuning key 52 = key on fresh copies -> (workspace, out, k, v) as integer views on the host"""
    T = DT[dt]
    qkv, k0, v0, lens, L, cap = _inputs(dt, Hq, Hkv, b, kv_len, rope, big_row)
    k, v = k0.clone(), v0.clone()
    dlens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    wsb = lib.omchat_op_attn_decode_ws(b, Hq, L)
    ws = torch.full((wsb // 4,), NAN, dtype=torch.float32, device="cuda")
    out = torch.full((b, Hq, 128), NAN, dtype=T, device="cuda")
    # key 10 = 1, key 25 = 0: the one-tile plan whatever the device's size (as tests/test_gpu_decode_append.py pins it)
    for kk, vv in ((10, 1), (25, 0), (KEY_4W, key)):
        _lib.check(lib.omchat_op_set_tuning(kk, vv))
    try:
        if rope:
            _lib.check(lib.omchat_op_attn_decode_append(CODE[dt], ptr(qkv), THETA, ptr(k), ptr(v), ptr(out), b, Hq, Hkv, cap, L, ptr(dlens), None, None, 0, 0,
                                                        SCALE, ptr(ws), wsb, None))
        else:
            q = qkv[:, :Hq].contiguous()
            _lib.check(lib.omchat_op_attn_decode(CODE[dt], ptr(q), ptr(k), ptr(v), ptr(out), b, Hq, Hkv, cap, L, ptr(dlens), SCALE, ptr(ws), wsb, None))
        sync()
    finally:
        for kk, vv in ((10, 0), (25, 1), (KEY_4W, 1)):
            lib.omchat_op_set_tuning(kk, vv)
    return ws.view(torch.int32).cpu(), out.view(torch.int16).cpu(), k.view(torch.int16).cpu(), v.view(torch.int16).cpu()


def compare(lib, dt, Hq, Hkv, b, kv_len, rope, big_row=None):
    tag = (dt, (Hq, Hkv), "batch", b, "kv_len", kv_len, "rope", rope)
    four = 1 if b == 1 else 2      # batch 1: the default selects the four-wave form; beyond, the key forces it
    ws1, out1, k1, v1 = run(lib, dt, Hq, Hkv, b, kv_len, rope, 0, big_row)
    ws4, out4, k4, v4 = run(lib, dt, Hq, Hkv, b, kv_len, rope, four, big_row)
    qkv, k0, v0, lens, L, cap = _inputs(dt, Hq, Hkv, b, kv_len, rope, big_row)
    nsplit = (L + 63) // 64
    # ---- partials: [b, Hq, nsplit, 132] = o[128], m, l, 2 pad
    w1, w4 = ws1.view(b, Hq, nsplit, 132), ws4.view(b, Hq, nsplit, 132)
    assert torch.equal(w4[..., :128], w1[..., :128]), (tag, "partial o differs")
    assert torch.equal(w4[..., 128], w1[..., 128]), (tag, "partial m differs")
    assert torch.equal(w4[..., 129], w1[..., 129]), (tag, "partial l differs")
    assert torch.equal(ws4, ws1), (tag, "workspace differs outside the partials")
    wf = w4.view(torch.float32)
    for i, n in enumerate(lens):
        used = (n + 63) // 64
        assert used < nsplit, (tag, "the case has no empty trailing split")
        assert torch.isfinite(wf[i, :, :used, :130]).all(), (tag, i, "a partial of a used split was not written")
        assert bool((wf[i, :, used:, 128] == -1e30).all()) and bool((wf[i, :, used:, 129] == 0).all()), (tag, i, "empty split: not the neutral partial")
        assert bool(torch.isnan(wf[i, :, used:, :128]).all()), (tag, i, "empty split: o was written")
    # ---- merged output
    assert torch.isfinite(out4.view(DT[dt]).float()).all(), (tag, "unwritten or non-finite output")
    assert torch.equal(out4, out1), (tag, "merged output differs")
    # ---- caches: the appended rows equal, nothing else touched
    assert torch.equal(k4, k1) and torch.equal(v4, v1), (tag, "cache bytes differ between the forms")
    want_k, want_v = k0.view(torch.int16).cpu().clone(), v0.view(torch.int16).cpu().clone()
    if rope:
        for i, n in enumerate(lens):
            assert torch.isfinite(k4.view(DT[dt])[i, :, n - 1].float()).all() and torch.isfinite(v4.view(DT[dt])[i, :, n - 1].float()).all(), (tag, i, "the new rows were not written")
            want_k[i, :, n - 1] = k4[i, :, n - 1]; want_v[i, :, n - 1] = v4[i, :, n - 1]
            assert torch.equal(v4[i, :, n - 1], qkv[i, Hq + Hkv:].view(torch.int16).cpu()), (tag, i, "the appended v row is not the projection's")
    assert torch.equal(k4, want_k) and torch.equal(v4, want_v), (tag, "a cache slot other than the new one changed")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("kv_len", KV_LENS)
def test_four_waves_give_the_one_wave_bits(gpu_lib, kv_len, heads, b, rope, dt):
    compare(gpu_lib, dt, heads[0], heads[1], b, kv_len, rope)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("b", [1, 2])
def test_a_key_row_of_large_magnitude(gpu_lib, b, rope, dt):
    """key 70 (second split of three) is 30 x the others: scaled scores of ~+-30 against ~+-1, so that split's maximum sets the merged row's and
    the other splits' partials are rescaled by exp2 of a large negative number"""
    compare(gpu_lib, dt, 28, 4, b, 129, rope, big_row=70)
