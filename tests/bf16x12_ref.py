"""bf16x12: the lossless 12-bit row coding of bf16 weights that the batch-1 decode GEMVs stream.  This numpy
restatement is the ONE definition of the format: the device encoder (gemv.hip: encode_bf16x12_kernel) and the CPU tests are held to it.

A bf16 weight w = sign | e[7:0] | m[6:0].  Per row of K weights (K % 512 == 0):

  top     the largest e[7:1] over the row's FINITE elements (0 for a row without any), one byte per row
  code    0           e[7:1] == 0 (exact for +-0, denormals and the first binade)
          c in 1..7   e[7:1] == top - 7 + c   (only values >= 1 are coded this way)
  nibble  sign << 3 | code
  low     the low byte of w (e[0] and the mantissa), untouched
  miss    every other element (an exponent more than 6 steps of two binades below top, inf, NaN): nibble 0 and low byte 0 in the row, and
          the entry (k << 16 | the 16 bits) in the row's patch list -- sorted by k, at most 32 per row, fixed stride [N][32] uint32, with a
          count per row (stored as min(misses, 33): 33 says "over the cap").  A tensor with any row over the cap is NOT coded (ok == False).

Layout: a row is K * 3 / 2 contiguous bytes, records of 512 weights = 768 bytes: 512 low bytes (weight j of the record at byte j), then
256 nibble bytes.  Lane l (0..63) of a wave owns weights j = 8 l .. 8 l + 7 of a record: its low bytes are the 8 bytes at 8 l, its nibbles
the 4-byte word at 512 + 4 l, byte i of that word holding weight i in its low half and weight i + 4 in its high half.
"""
import numpy as np

REC = 512            # weights per record
REC_BYTES = 768
MAX_PATCH = 32


def row_bytes(K):
    return K // REC * REC_BYTES


def encode(w_bits):
    """w_bits: uint16 [N, K] (the bf16 bit patterns).  Returns (coded uint8 [N, K * 3 / 2], top uint8 [N], count uint8 [N],
    patches uint32 [N, 32], ok)."""
    w = np.ascontiguousarray(w_bits, dtype=np.uint16)
    N, K = w.shape
    assert K % REC == 0, "K must be a multiple of 512"
    e = ((w >> 7) & 0xFF).astype(np.int32)
    e71 = e >> 1
    finite = e != 0xFF
    top = np.where(finite, e71, 0).max(axis=1).astype(np.int32)            # [N]
    c = e71 - (top[:, None] - 7)
    code = np.where(e71 == 0, 0, c)
    hit = finite & ((e71 == 0) | ((c >= 1) & (c <= 7)))
    sign = (w >> 15).astype(np.int32)
    nib = np.where(hit, (sign << 3) | code, 0).astype(np.uint8)             # [N, K]
    low = np.where(hit, w & 0xFF, 0).astype(np.uint8)
    coded = np.zeros((N, K // REC, REC_BYTES), np.uint8)
    coded[:, :, :REC] = low.reshape(N, K // REC, REC)
    nb = nib.reshape(N, K // REC, 64, 2, 4)                                 # [.., lane, half (i >> 2), i & 3]
    coded[:, :, REC:] = (nb[:, :, :, 0, :] | (nb[:, :, :, 1, :] << 4)).reshape(N, K // REC, 256)
    misses = (~hit).sum(axis=1)
    count = np.minimum(misses, MAX_PATCH + 1).astype(np.uint8)
    patches = np.zeros((N, MAX_PATCH), np.uint32)
    for n in np.nonzero(misses)[0]:
        ks = np.nonzero(~hit[n])[0][:MAX_PATCH]
        patches[n, :len(ks)] = (ks.astype(np.uint32) << 16) | w[n, ks].astype(np.uint32)
    return coded.reshape(N, -1), top.astype(np.uint8), count, patches, bool((misses <= MAX_PATCH).all())


def decode(coded, top, count, patches):
    """The inverse: uint16 [N, K].  Needs every count <= 32."""
    coded = np.asarray(coded, np.uint8)
    N = coded.shape[0]
    rec = coded.reshape(N, -1, REC_BYTES)
    R = rec.shape[1]
    low = rec[:, :, :REC].reshape(N, R * REC).astype(np.uint16)
    nw = rec[:, :, REC:].reshape(N, R, 64, 1, 4)
    nib = np.concatenate([nw & 0xF, nw >> 4], axis=3).reshape(N, R * REC).astype(np.int32)
    code = nib & 7
    e71 = np.where(code == 0, 0, (top.astype(np.int32)[:, None] - 7 + code) & 0x7F)
    w = (((nib >> 3) << 15) | (e71 << 8)).astype(np.uint16) | low
    assert (np.asarray(count) <= MAX_PATCH).all(), "a row over the patch cap is not coded"
    for n in np.nonzero(count)[0]:
        p = patches[n, :count[n]]
        w[n, (p >> 16).astype(np.int64)] = (p & 0xFFFF).astype(np.uint16)
    return w


def bf16_bits(x):
    """float32 array -> bf16 bit patterns, round to nearest even (NaN stays NaN)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(x)
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)
