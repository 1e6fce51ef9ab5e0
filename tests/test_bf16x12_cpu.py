"""bf16x12 reference codec (tests/bf16x12_ref.py): bit layout by hand, exact round trips, every edge the format names, and the condition
the decode relies on -- on the weight distributions in use no row needs the 16-bit fallback."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16x12_ref as ref      # noqa: E402
from omchat_amd import synth      # noqa: E402


def bits(sign, e, m):
    return np.uint16((sign << 15) | (e << 7) | m)


def filled(K, e=120, N=1):
    """rows of +2^(e-127) * 1.0-ish values with a running mantissa: no misses, top = e >> 1"""
    k = np.arange(N * K, dtype=np.uint32).reshape(N, K)
    return (np.uint16(e << 7) | (k % 128).astype(np.uint16)).astype(np.uint16)


def roundtrip(w):
    coded, top, cnt, pat, ok = ref.encode(w)
    assert ok
    assert np.array_equal(ref.decode(coded, top, cnt, pat), w)
    return coded, top, cnt, pat


def test_hand_vectors_bit_layout():
    K = 1024
    w = filled(K, e=121)                       # e[7:1] = 60 everywhere: top = 60
    # record 1, lane 5, weights i = 0..7: signs, exponents around top, one zero
    base = 512 + 8 * 5
    w[0, base + 0] = bits(1, 121, 0x55)        # e71 = 60 -> code 7, sign 1 -> nibble 0xF, low byte 0x80 | 0x55
    w[0, base + 1] = bits(0, 120, 0x01)        # e71 = 60 -> code 7, e[0] = 0      -> nibble 0x7, low byte 0x01
    w[0, base + 2] = bits(0, 109, 0x7F)        # e71 = 54 -> code 1                 -> nibble 0x1, low byte 0xFF
    w[0, base + 3] = bits(1, 0, 0x00)          # -0: code 0, sign kept              -> nibble 0x8, low byte 0x00
    w[0, base + 4] = bits(0, 1, 0x02)          # first binade (e71 = 0): code 0     -> nibble 0x0, low byte 0x82
    w[0, base + 5] = bits(1, 119, 0x10)        # e71 = 59 -> code 6                 -> nibble 0xE, low byte 0x90
    w[0, base + 6] = bits(0, 107, 0x33)        # e71 = 53: below the window -> MISS -> nibble 0, low byte 0, patch
    w[0, base + 7] = bits(0, 0, 0x7F)          # denormal: code 0                   -> nibble 0x0, low byte 0x7F
    coded, top, cnt, pat = roundtrip(w)
    assert coded.shape == (1, K * 3 // 2) and top[0] == 60 and cnt[0] == 1
    rec = coded[0, 768:1536]
    assert list(rec[8 * 5:8 * 5 + 8]) == [0xD5, 0x01, 0xFF, 0x00, 0x82, 0x90, 0x00, 0x7F]
    # nibble word of lane 5: byte i = weight i (low half) | weight i + 4 (high half)
    assert list(rec[512 + 4 * 5:512 + 4 * 5 + 4]) == [0x0F, 0xE7, 0x01, 0x08]
    assert pat[0, 0] == ((base + 6) << 16 | int(bits(0, 107, 0x33)))
    assert not pat[0, 1:].any()
    # the first record holds the filler only: code 7, positive
    assert (coded[0, 512:768] == 0x77).all()


def weights_synth(N, K, name="model.layers.0.mlp.down_proj.weight"):
    return ref.bf16_bits(synth.uniform_range(name, 0, N * K).reshape(N, K))


def weights_gauss(N, K, seed=1):
    return ref.bf16_bits((np.random.default_rng(seed).standard_normal((N, K)) * 0.02).astype(np.float32))


@pytest.mark.parametrize("K", [3584, 18944])
@pytest.mark.parametrize("dist", ["synth", "gauss"])
def test_roundtrip_and_no_fallback(K, dist):
    """exact round trip, and the condition of the decode: no row of these distributions needs the 16-bit fallback (the maxima measured for
    the issue at 4.2 M elements: 6 patches per row of synthetic weights, 13 of Gaussian ones)"""
    N = 4_200_000 // K + 1      # the 4.2 M elements the maxima were measured on
    w = weights_synth(N, K) if dist == "synth" else weights_gauss(N, K)
    coded, top, cnt, pat = roundtrip(w)
    assert int(cnt.max()) <= 16, f"max patches per row {int(cnt.max())}"
    assert float(cnt.sum()) / w.size < 1e-3


def test_zero_row_and_signed_zeros():
    w = np.zeros((2, 512), np.uint16)
    w[1, ::3] = 0x8000
    coded, top, cnt, pat = roundtrip(w)
    assert not top.any() and not cnt.any()
    assert not coded[0].any()
    assert coded[1, 512] == 0x08 and coded[1, 0] == 0      # -0 at k = 0: sign nibble, zero low byte


def test_denormals_and_low_top():
    w = np.zeros((3, 512), np.uint16)
    w[0, :] = (np.arange(512) % 128).astype(np.uint16)                            # denormals only: top = 0
    w[0, 1::2] |= 0x8000
    w[1, :] = ((np.arange(512) % 7).astype(np.uint16) << 7) | 0x15                 # e = 0..6: top = 3 (< 7), codes 4..7 and 0
    w[2, :] = ((np.arange(512) % 14).astype(np.uint16) << 7) | 0x8041              # e = 0..13: top = 6, every e71 in 0..6 has a code
    coded, top, cnt, pat = roundtrip(w)
    assert list(top) == [0, 3, 6] and not cnt.any()


def test_inf_nan_are_patches():
    w = filled(512)
    w[0, 7] = 0x7F80; w[0, 8] = 0xFF80; w[0, 100] = 0x7FC1; w[0, 511] = 0xFFFF
    coded, top, cnt, pat = roundtrip(w)
    assert top[0] == 60 and cnt[0] == 4
    assert [int(p >> 16) for p in pat[0, :4]] == [7, 8, 100, 511]
    assert [int(p & 0xFFFF) for p in pat[0, :4]] == [0x7F80, 0xFF80, 0x7FC1, 0xFFFF]
    w2 = np.full((1, 512), 0x7F80, np.uint16)      # no finite element at all: top = 0, everything a miss -> over the cap
    assert ref.encode(w2)[4] is False


def miss():
    return bits(1, 60, 0x2A)      # e71 = 30: far below a top of 60, and not zero


def test_miss_positions():
    K = 1536
    w = filled(K, N=4)
    w[0, 0] = miss(); w[0, K - 1] = miss()                     # first and last element of the row
    w[1, 512 + 8 * 9 + 1] = miss(); w[1, 512 + 8 * 9 + 6] = miss()      # two in one lane's eight weights
    w[2, 8 * 20 + 7] = miss(); w[2, 8 * 21] = miss(); w[2, 8 * 22 + 3] = miss()      # adjacent lanes of one chunk
    coded, top, cnt, pat = roundtrip(w)
    assert list(cnt) == [2, 2, 3, 0]
    assert [int(p >> 16) for p in pat[0, :2]] == [0, K - 1]
    assert [int(p >> 16) for p in pat[1, :2]] == [512 + 73, 512 + 78]
    assert coded[0, 0] == 0 and coded[0, 512] == 0x70      # the miss is stored as +0 next to an untouched neighbour nibble


def test_patch_cap():
    K = 1024
    w = filled(K, N=2)
    ks = np.arange(33) * 31
    w[0, ks[:32]] = miss()
    w[1, ks] = miss()
    coded, top, cnt, pat, ok = ref.encode(w)
    assert list(cnt) == [32, 33] and not ok
    c0, t0, n0, p0, ok0 = ref.encode(w[:1])
    assert ok0 and n0[0] == 32 and np.array_equal(ref.decode(c0, t0, n0, p0), w[:1])
    assert np.array_equal(p0[0] >> 16, ks[:32])
    with pytest.raises(AssertionError):
        ref.decode(coded, top, cnt, pat)
