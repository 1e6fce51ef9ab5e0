"""CPU reference of the MXFP4 weight format (OCP Microscaling v1.0) as include/omchat_hip.h states it, in torch:

  per row and per block of 32 consecutive k:  e = floor(log2(max|w|)) - 2 clamped to [-127, 127], stored as the e8m0 byte e + 127
  (a zero block stores 127); codes = w / 2^e rounded to the nearest of {0, .5, 1, 1.5, 2, 3, 4, 6}, ties to the even code, saturating at 6;
  sign in bit 3, never on a zero code.  Packed: two codes per byte, the even k in the low nibble."""
import torch

GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def quant_ref(w):
    """w [N, K] (K % 32 == 0) -> (codes [N, K] uint8 with the sign in bit 3, e8m0 [N, K / 32] uint8, dequant [N, K] float64)"""
    w = w.double()
    N, K = w.shape
    assert K % 32 == 0
    blk = w.view(N, K // 32, 32)
    m = blk.abs().amax(dim=2)
    _, ex = torch.frexp(m)                                   # m = mant * 2^ex, mant in [0.5, 1): floor(log2 m) = ex - 1
    e = (ex.to(torch.int64) - 1 - 2).clamp(-127, 127)
    e = torch.where(m > 0, e, torch.zeros_like(e))
    scale = torch.ldexp(torch.ones_like(m), e)               # 2^e, exact in float64
    a = (blk.abs() / scale[:, :, None]).reshape(N, K)        # exact: a power of two
    lo = (torch.searchsorted(GRID, a, right=True) - 1).clamp(0, 7)      # largest grid value <= a
    hi = (lo + 1).clamp(max=7)                               # above 6: lo == hi == 7 (saturation)
    dl, dh = a - GRID[lo], GRID[hi] - a
    even = torch.where(lo % 2 == 0, lo, hi)                  # a tie goes to the even code of the two neighbours
    mag = torch.where(dh < dl, hi, torch.where(dl < dh, lo, even))
    mag = torch.where(lo == hi, lo, mag)
    neg = (w < 0) & (mag != 0)
    codes = (mag + 8 * neg.to(torch.int64)).to(torch.uint8)
    deq = torch.where(neg, -GRID[mag], GRID[mag]).view(N, K // 32, 32) * scale[:, :, None]
    return codes, (e + 127).to(torch.uint8), deq.reshape(N, K)


def pack(codes):
    """codes [N, K] -> bytes [N, K / 2]: the even k in the low nibble"""
    c = codes.to(torch.int32)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).to(torch.uint8)


def dequant_ref(w):
    return quant_ref(w)[2]
