"""The long-K GEMV launch (down_proj + residual: gemv_rows_longk_body, DESIGN.md section 17 "The long-K form's pass") at every pass count, in
every weight form, as output bits:
    OMCHAT_LIB=<a library built from the commit to pin> python tools/longk_golden.py [--out tests/golden/longk_parent_bits.npz]
writes the seed and, per case, the output half-words of the launch on seeded inputs.  tests/test_gpu_longk_pipeline.py recomputes every case
on the library it loaded and compares half-words for equality: how the passes are scheduled changes no bit.  The golden in the tree was written
by the build of the commit BEFORE the counted pipeline.
Cases: N = 48 rows (one wave per workgroup) + a residual at K = 4608 .. 32768 -- every count of passes from 2 to 8 (passes of eight chunks) and
from 4 to 16 (passes of four), so every peeled ending and both parities of the repeated part, the two K % 4096 == 0 shapes, the K of the real
step -- in 16-bit bf16 and f16, e4m3, MXFP4 and bf16x12; and the real grid, N = 3584 at K = 18944, in bf16 and bf16x12.  The bf16 and bf16x12
cases share the planted rows of tests/test_gpu_bf16x12_longk.py (32 patches, five in one decode group, -inf among the first eight weights, ...)
+ row 16 with +inf at weight 2."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)

SEED = 11
KS = (4608, 8192, 8704, 12800, 16896, 18944, 20992, 25088, 29184, 32768)
FORMS = ("bf16", "f16", "e4m3", "mxfp4", "bf16x12")
CASES = [(f, 48, K) for f in FORMS for K in KS] + [("bf16", 3584, 18944), ("bf16x12", 3584, 18944)]
EPI_RESID = 3


def key(form, N, K):
    return f"{form}_{N}_{K}"


def _planted(N, K):
    """the bf16 bit patterns (int16, device) shared by the bf16 and the bf16x12 case of a shape, x and the residual"""
    import torch
    from test_gpu_bf16x12_longk import planted, _inputs
    w, hot, _ = planted(N, K, SEED)
    w[16, 2] = 0x7F80
    x, res = _inputs(K, N, hot, SEED)
    return w, x, res


def _random(N, K, dt):
    import torch
    g = torch.Generator().manual_seed(SEED + K)
    w = (torch.randn(N, K, generator=g) * 0.02).to(dt).cuda()
    x = (torch.randn(K, generator=g) * 0.5).to(dt).cuda()
    res = (torch.randn(N, generator=g) * 0.5).to(dt).cuda()
    return w, x, res


def run(lib, form, N, K):
    """the launch of one case on `lib`: N output half-words (numpy uint16)"""
    import torch
    from omchat_amd import _lib
    from gpu_util import ptr
    check = _lib.check
    dt = torch.float16 if form == "f16" else torch.bfloat16
    code = _lib.F16 if form == "f16" else _lib.BF16
    y = torch.ones(N, device="cuda", dtype=dt)
    if form in ("bf16", "bf16x12"):
        w, x, res = _planted(N, K)
        if form == "bf16":
            check(lib.omchat_op_gemv(code, ptr(x), K, ptr(w), K, ptr(y), N, 1, N, K, None, ptr(res), N, EPI_RESID, 0, None))
        else:
            from test_gpu_bf16x12_longk import dev_encode
            coded, top, cnt, patch = dev_encode(w)
            c = cnt.cpu().numpy()
            assert c[5] == 32 and c[6] == 5 and c[16] >= 1      # 32 patches; five in the decode group of chunks 2 and 3; the planted +inf
            check(lib.omchat_op_gemv_bf16x12(ptr(x), ptr(coded), ptr(top), ptr(cnt), ptr(patch), ptr(y), N, K, None, 1e-6, ptr(res), EPI_RESID, 0, None))
    else:
        w, x, res = _random(N, K, dt)
        if form == "f16":
            check(lib.omchat_op_gemv(code, ptr(x), K, ptr(w), K, ptr(y), N, 1, N, K, None, ptr(res), N, EPI_RESID, 0, None))
        elif form == "e4m3":
            w8 = torch.empty(N, K, dtype=torch.uint8, device="cuda")
            sc = torch.empty(N, dtype=torch.float32, device="cuda")
            check(lib.omchat_op_quant_fp8(code, ptr(w), N, K, ptr(w8), ptr(sc), None))
            check(lib.omchat_op_gemv_fp8(code, ptr(x), ptr(w8), ptr(sc), ptr(y), N, K, None, ptr(res), EPI_RESID, 0, 1, None))
        else:
            w4 = torch.empty(N, K // 2, dtype=torch.uint8, device="cuda")
            sc = torch.empty(N, K // 32, dtype=torch.uint8, device="cuda")
            check(lib.omchat_op_quant_mxfp4(code, ptr(w), N, K, ptr(w4), ptr(sc), None))
            check(lib.omchat_op_gemv_mxfp4(code, ptr(x), ptr(w4), ptr(sc), ptr(y), N, K, None, ptr(res), EPI_RESID, 0, 1, None))
    torch.cuda.synchronize()
    return y.view(torch.int16).cpu().numpy().view(np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "longk_parent_bits.npz"))
    args = ap.parse_args()
    import torch
    from omchat_amd import _lib
    assert torch.cuda.is_available(), "longk_golden needs a GPU"
    lib = _lib.lib()
    out = {"seed": np.int64(SEED)}
    for form, N, K in CASES:
        out[key(form, N, K)] = run(lib, form, N, K)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {len(CASES)} cases from {_lib.LIB_PATH}, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
