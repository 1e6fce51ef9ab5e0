"""The three long GEMV launches of a batch-1 decode step on 16-bit rows and on their bf16x12 coding, alone, at the
real shapes of the full-width decoder, alternating on one device:
    python tools/bench_bf16x12.py [--roles gate_up,down_proj,lm_head] [--repeats 7] [--iters 56] [--copies 28]
Per role one JSON line: microseconds per launch (median, min, max over the windows; the two formats take turns window by window), GB/s of
the bytes the format streams (coded rows + top + counts + patch lists for bf16x12), the ratio of the medians, whether the outputs were
bit-equal, and the patch statistics of the random N(0, 0.02^2) weights.  Every launch of a window reads another copy of the weights --
`copies` of them, the 28-layer footprint by default -- so that no launch finds its rows in the L2 or the memory-side cache, as in a real
step.  "spread_us" is the largest max - min of a cell: a difference between the formats below it is not a difference."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def encode(lib, w):
    import torch
    from omchat_amd._lib import check, ptr
    N, K = w.shape
    coded = torch.empty(N, K * 3 // 2, dtype=torch.uint8, device="cuda")
    top = torch.empty(N, dtype=torch.uint8, device="cuda")
    cnt = torch.empty(N, dtype=torch.uint8, device="cuda")
    patch = torch.empty(N, 32, dtype=torch.int32, device="cuda")
    over = torch.zeros(1, dtype=torch.int32, device="cuda")
    check(lib.omchat_op_encode_bf16x12(ptr(w), N, K, ptr(coded), ptr(top), ptr(cnt), ptr(patch), ptr(over), None))
    torch.cuda.synchronize()
    return coded, top, cnt, patch, int(over.item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roles", default="gate_up,down_proj,lm_head")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=56)
    ap.add_argument("--copies", type=int, default=28)
    args = ap.parse_args()
    import torch
    from omchat_amd import _lib
    from omchat_amd._lib import check, ptr
    from omchat_amd.config import omchat13b
    assert torch.cuda.is_available(), "bench_bf16x12 needs a GPU"
    lib = _lib.lib()
    cfg = omchat13b()
    H, It, V = cfg.text["hidden_size"], cfg.text["intermediate_size"], cfg.text["vocab_size"]
    BF16, NONE, RESID, SWIGLU = _lib.BF16, _lib.EPI_NONE, _lib.EPI_RESID, _lib.EPI_SWIGLU
    ROLES = dict(gate_up=(2 * It, H, SWIGLU, True, False, args.copies), down_proj=(H, It, RESID, False, False, args.copies),
                 lm_head=(V, H, NONE, True, True, 2))
    g = torch.Generator(device="cuda").manual_seed(2)
    for name in args.roles.split(","):
        N, K, epi, has_norm, f32, ncopy = ROLES[name]
        w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).bfloat16()
        xr = (torch.randn(K, device="cuda", generator=g) * 0.5).bfloat16()
        nw = (1 + 0.1 * torch.randn(K, device="cuda", generator=g)).bfloat16()
        n_y = N // 2 if epi == SWIGLU else N
        res = (torch.randn(N, device="cuda", generator=g) * 0.5).bfloat16() if epi == RESID else None
        enc = encode(lib, w)
        assert enc[4] == 0, "a row of the random weights went over the patch cap"
        cnt = enc[2]
        byts = dict(bf16=N * K * 2, x12=N * K * 3 // 2 + N * (2 + 128))
        sets = dict(bf16=[(w.clone(),) for _ in range(ncopy)], x12=[tuple(t.clone() for t in enc[:4]) for _ in range(ncopy)])
        ys = {f: torch.zeros(n_y, device="cuda", dtype=torch.float32 if f32 else torch.bfloat16) for f in sets}

        def launch(fmt, c):
            y = ys[fmt]
            if fmt == "x12":
                return lib.omchat_op_gemv_bf16x12(ptr(xr), ptr(c[0]), ptr(c[1]), ptr(c[2]), ptr(c[3]), ptr(y), N, K, ptr(nw) if has_norm else None,
                                                  1e-6, ptr(res), epi, int(f32), None)
            if has_norm:
                return lib.omchat_op_gemv_norm(BF16, ptr(xr), ptr(c[0]), K, ptr(y), N, K, ptr(nw), 1e-6, None, epi, int(f32), None)
            return lib.omchat_op_gemv(BF16, ptr(xr), K, ptr(c[0]), K, ptr(y), n_y, 1, N, K, None, ptr(res), N, epi, int(f32), None)

        times = {f: [] for f in sets}
        for r in range(args.repeats):
            for fmt, cs in sets.items():
                for i in range(len(cs)):
                    check(launch(fmt, cs[i]))
                torch.cuda.synchronize()
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for i in range(args.iters):
                    check(launch(fmt, cs[i % len(cs)]))
                z.record()
                z.synchronize()
                times[fmt].append(a.elapsed_time(z) * 1e3 / args.iters)
        equal = bool(torch.equal(ys["bf16"].view(torch.int32 if f32 else torch.int16), ys["x12"].view(torch.int32 if f32 else torch.int16)))
        out, spread = {}, 0.0
        for fmt, v in times.items():
            us = statistics.median(v)
            out[fmt] = dict(us=round(us, 2), min=round(min(v), 2), max=round(max(v), 2), GBps=round(byts[fmt] / us / 1e3, 1))
            spread = max(spread, max(v) - min(v))
        print(json.dumps(dict(role=name, N=N, K=K, copies=ncopy, MB={k: round(v / 1e6, 1) for k, v in byts.items()}, **out,
                              x12_over_bf16=round(out["x12"]["us"] / out["bf16"]["us"], 4), spread_us=round(spread, 2), bit_equal=equal,
                              patches=dict(mean=round(float(cnt.float().mean()), 3), max=int(cnt.max())))), flush=True)
        del sets, w, enc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
