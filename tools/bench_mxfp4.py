"""Batch-1 decode with the three weight formats a step can stream -- 16-bit, the e4m3 replica, the MXFP4 replica -- on
the full-width synthetic decoder (28 layers, vocabulary 152064, one GPU), in one process and on one context:
    python tools/bench_mxfp4.py [--steps 200] [--repeats 5] [--iters 50] [--layers 28]
Prints JSON lines:
  {"step": ...}   ms per decode step, eager and as the captured graph: the formats are measured alternately, `repeats` windows of `steps`
                  steps each (device events around a window); median, min and max over the windows.  "spread_ms" is the largest max - min
                  of any cell: a difference between two formats below it is not a difference.
  {"role": ...}   each of the five GEMV roles of a step alone (qkv, o_proj, gate|up, down_proj, lm_head), per format: microseconds per launch
                  and GB/s of WEIGHT bytes (codes + scales).  Every launch reads another copy of the weights (>= 768 MB of copies per role and
                  format) so that no launch finds its rows in the L2 / the memory-side cache, as in a real step.  form "plain": x arrives
                  normalised; form "norm": the RMSNorm runs in the GEMV's registers (what a step launches for qkv, gate|up and lm_head;
                  the e4m3 format has no op-level entry for it).
  {"drift": ...}  relative difference of the first decode step's logits against the 16-bit step on the same prefill.
Batched section (--sections batched; MXFP4 mode 2, Engine.enable_mxfp4_decode(True, batched=True)): one context with 32 cache rows, the 16-bit
packed path and the packed MXFP4 path alternating:
  {"batched_step": ...}    ms per decode step at b = 8 and b = 32, eager and as the captured graph, windows as above
  {"verify": ...}          ms per prompt-lookup verify step of T = 8 tokens (host clock: the call ends in a device synchronise)
  {"batched_role": ...}    the five GEMV roles alone at b = 8 and b = 32 on PRE-PACKED operands (omchat_op_gemv_prepacked: the launch a step
                           makes, nothing packed or allocated in the timed loop), o_proj and down_proj with the step's split-K slice counts
                           (2 and 8), microseconds per launch and GB/s of weight bytes, rotating copies as above; --batched-iters launches per
                           window (default 1000: 10 to 200 ms of work), median, min and max over the windows
  {"batched_drift": ...}   relative difference of a b = 32 step's logits against the 16-bit packed step on the same prefill."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--prompt", type=int, default=64)
    ap.add_argument("--batched-iters", type=int, default=1000, help="launches per timed window of a batched role (10 to 200 us each)")
    ap.add_argument("--sections", default="batch1,batched", help="comma list of: batch1, batched")
    args = ap.parse_args()
    sections = set(args.sections.split(","))
    import torch
    from omchat_amd import _lib
    from omchat_amd._lib import check, ptr
    from omchat_amd.config import omchat13b
    from omchat_amd.engine import Engine
    assert torch.cuda.is_available(), "bench_mxfp4 needs a GPU"
    lib = _lib.lib()
    cfg = omchat13b()
    cfg.text["num_hidden_layers"] = args.layers
    H, It, V = cfg.text["hidden_size"], cfg.text["intermediate_size"], cfg.text["vocab_size"]
    if "batched" in sections:
        batched(args, cfg, lib)
    if "batch1" not in sections:
        return
    e = Engine(cfg, dtype="bf16", max_seq=args.prompt + args.steps + 64, max_batch=1, vision=False)
    e.fill_synthetic(0)
    x = (torch.randn(1, args.prompt, H, generator=torch.Generator().manual_seed(1)) * 0.5).bfloat16()

    FORMATS = ["bf16", "e4m3", "mxfp4"]

    def select(fmt):
        e.enable_fp8_decode(False)
        e.enable_mxfp4_decode(False)
        if fmt == "e4m3":
            e.enable_fp8_decode(True)
        elif fmt == "mxfp4":
            e.enable_mxfp4_decode(True)

    # ---- drift of the first step against the 16-bit step, same prefill
    logits = {}
    for fmt in FORMATS:
        select(fmt)
        e.prefill(x)
        _, lg = e.decode_step(torch.tensor([3]), want_logits=True)
        torch.cuda.synchronize()
        logits[fmt] = lg[0].double().cpu()
    rel = lambda a, b: float((a - b).norm() / b.norm())
    print(json.dumps(dict(drift=dict(e4m3=round(rel(logits["e4m3"], logits["bf16"]), 5), mxfp4=round(rel(logits["mxfp4"], logits["bf16"]), 5),
                                     argmax_equal=dict(e4m3=bool(logits["e4m3"].argmax() == logits["bf16"].argmax()),
                                                       mxfp4=bool(logits["mxfp4"].argmax() == logits["bf16"].argmax()))))), flush=True)

    # ---- the decode step: windows of `steps` steps, the formats alternating inside every repeat
    def window(n):
        e.prefill(x)                                    # every window decodes the same positions: prompt .. prompt + 8 + n
        tok = torch.tensor([3], dtype=torch.int32, device="cuda")
        for _ in range(8):
            tok, _ = e.decode_step(tok)
        torch.cuda.synchronize()
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            tok, _ = e.decode_step(tok)
        z.record()
        z.synchronize()
        return a.elapsed_time(z) / n

    table, spread = {}, 0.0
    for graph in (False, True):
        e.enable_decode_graph(graph)
        cells = {f: [] for f in FORMATS}
        for _ in range(args.repeats):
            for fmt in FORMATS:
                select(fmt)
                cells[fmt].append(window(args.steps))
        for fmt in FORMATS:
            v = cells[fmt]
            table[f"{fmt}/{'graph' if graph else 'eager'}"] = dict(ms=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
            spread = max(spread, max(v) - min(v))
    e.enable_decode_graph(False)
    select("bf16")
    print(json.dumps(dict(step=table, spread_ms=round(spread, 4), layers=args.layers, steps=args.steps, repeats=args.repeats)), flush=True)
    e.close()

    # ---- the five GEMV roles alone
    BF16, NONE, RESID, SWIGLU = _lib.BF16, _lib.EPI_NONE, _lib.EPI_RESID, _lib.EPI_SWIGLU
    qkvd = (cfg.text["num_attention_heads"] + 2 * cfg.text["num_key_value_heads"]) * 128
    ROLES = [("qkv", qkvd, H, NONE, True, False), ("o_proj", H, H, RESID, False, False), ("gate|up", 2 * It, H, SWIGLU, True, False),
             ("down_proj", H, It, RESID, False, False), ("lm_head", V, H, NONE, True, True)]
    g = torch.Generator(device="cuda").manual_seed(2)
    for name, N, K, epi, has_norm, f32 in ROLES:
        w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).bfloat16()
        xr = (torch.randn(K, device="cuda", generator=g) * 0.5).bfloat16()
        nw = torch.ones(K, device="cuda", dtype=torch.bfloat16)
        bias = torch.zeros(N, device="cuda", dtype=torch.bfloat16) if name == "qkv" else None
        n_y = N // 2 if epi == SWIGLU else N
        y = torch.zeros(n_y, device="cuda", dtype=torch.float32 if f32 else torch.bfloat16)
        res = torch.zeros(N, device="cuda", dtype=torch.bfloat16) if epi == RESID else None
        w8 = torch.empty(N, K, dtype=torch.uint8, device="cuda"); s8 = torch.empty(N, dtype=torch.float32, device="cuda")
        w4 = torch.empty(N, K // 2, dtype=torch.uint8, device="cuda"); s4 = torch.empty(N, K // 32, dtype=torch.uint8, device="cuda")
        check(lib.omchat_op_quant_fp8(BF16, ptr(w), N, K, ptr(w8), ptr(s8), None))
        check(lib.omchat_op_quant_mxfp4(BF16, ptr(w), N, K, ptr(w4), ptr(s4), None))
        torch.cuda.synchronize()
        byts = dict(bf16=N * K * 2, e4m3=N * K + N * 4, mxfp4=N * K // 2 + N * K // 32)

        def copies(ts, nbytes):
            n = max(2, -(-768 * 2 ** 20 // nbytes))
            return [tuple(t.clone() for t in ts) for _ in range(n)]
        sets = dict(bf16=copies((w,), byts["bf16"]), e4m3=copies((w8, s8), byts["e4m3"]), mxfp4=copies((w4, s4), byts["mxfp4"]))

        def launch(fmt, form, c):
            if fmt == "bf16" and form == "plain":
                return lib.omchat_op_gemv(BF16, ptr(xr), K, ptr(c[0]), K, ptr(y), n_y, 1, N, K, ptr(bias), ptr(res), N, epi, int(f32), None)
            if fmt == "bf16":
                return lib.omchat_op_gemv_norm(BF16, ptr(xr), ptr(c[0]), K, ptr(y), N, K, ptr(nw), 1e-6, ptr(bias), epi, int(f32), None)
            if fmt == "e4m3":
                return lib.omchat_op_gemv_fp8(BF16, ptr(xr), ptr(c[0]), ptr(c[1]), ptr(y), N, K, ptr(bias), ptr(res), epi, int(f32), 1, None)
            if form == "plain":
                return lib.omchat_op_gemv_mxfp4(BF16, ptr(xr), ptr(c[0]), ptr(c[1]), ptr(y), N, K, ptr(bias), ptr(res), epi, int(f32), 1, None)
            return lib.omchat_op_gemv_mxfp4_norm(BF16, ptr(xr), ptr(c[0]), ptr(c[1]), ptr(y), N, K, ptr(nw), 1e-6, ptr(bias), epi, int(f32), None)

        cases = [(f, "plain") for f in FORMATS] + ([("bf16", "norm"), ("mxfp4", "norm")] if has_norm else [])
        out = {}
        for fmt, form in cases:
            cs, times = sets[fmt], []
            for r in range(args.repeats):
                for i in range(len(cs)):
                    check(launch(fmt, form, cs[i]))
                torch.cuda.synchronize()
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for i in range(args.iters):
                    check(launch(fmt, form, cs[i % len(cs)]))
                z.record()
                z.synchronize()
                times.append(a.elapsed_time(z) * 1e3 / args.iters)
            us = statistics.median(times)
            out[f"{fmt}/{form}"] = dict(us=round(us, 2), min=round(min(times), 2), max=round(max(times), 2), GBps=round(byts[fmt] / us / 1e3, 1))
        print(json.dumps(dict(role=name, N=N, K=K, weight_MB={k: round(v / 2 ** 20, 1) for k, v in byts.items()}, **out)), flush=True)
        del sets, w, w8, w4
        torch.cuda.empty_cache()


def batched(args, cfg, lib):
    import time
    import torch
    from omchat_amd import _lib
    from omchat_amd._lib import check, ptr
    from omchat_amd.engine import Engine
    H, It, V = cfg.text["hidden_size"], cfg.text["intermediate_size"], cfg.text["vocab_size"]
    B = 32
    e = Engine(cfg, dtype="bf16", max_seq=args.prompt + max(args.steps, 8 * 24) + 64, max_batch=B, vision=False)
    e.fill_synthetic(0)
    x = (torch.randn(B, args.prompt, H, generator=torch.Generator().manual_seed(1)) * 0.5).bfloat16()
    FORMATS = ["bf16", "mxfp4"]

    def select(fmt):
        e.enable_mxfp4_decode(fmt == "mxfp4", batched=True)

    logits = {}
    for fmt in FORMATS:
        select(fmt)
        e.prefill(x)
        _, lg = e.decode_step(torch.arange(3, 3 + B), want_logits=True)
        torch.cuda.synchronize()
        logits[fmt] = lg.double().cpu()
    d = float((logits["mxfp4"] - logits["bf16"]).norm() / logits["bf16"].norm())
    print(json.dumps(dict(batched_drift=dict(mxfp4=round(d, 5), argmax_equal_rows=int((logits["mxfp4"].argmax(1) == logits["bf16"].argmax(1)).sum()),
                                             rows=B))), flush=True)

    def window(b, n):
        e.prefill(x[:b].contiguous())
        tok = torch.arange(3, 3 + b, dtype=torch.int32, device="cuda")
        for _ in range(8):
            tok, _ = e.decode_step(tok)
        torch.cuda.synchronize()
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            tok, _ = e.decode_step(tok)
        z.record()
        z.synchronize()
        return a.elapsed_time(z) / n

    table, spread = {}, 0.0
    for graph in (False, True):
        e.enable_decode_graph(graph)
        for b in (8, 32):
            cells = {f: [] for f in FORMATS}
            for _ in range(args.repeats):
                for fmt in FORMATS:
                    select(fmt)
                    cells[fmt].append(window(b, args.steps))
            for fmt in FORMATS:
                v = cells[fmt]
                table[f"b{b}/{fmt}/{'graph' if graph else 'eager'}"] = dict(ms=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
                spread = max(spread, max(v) - min(v))
    e.enable_decode_graph(False)
    print(json.dumps(dict(batched_step=table, spread_ms=round(spread, 4), layers=args.layers, steps=args.steps, repeats=args.repeats)), flush=True)

    # ---- one verify step of T = 8 tokens (keep_all: every call appends 8 positions; 24 calls per window, the first 4 not timed)
    T, calls = 8, 24
    toks = torch.arange(5, 5 + T, dtype=torch.int32)
    cells = {f: [] for f in FORMATS}
    for _ in range(args.repeats):
        for fmt in FORMATS:
            select(fmt)
            e.prefill(x[:1].contiguous())
            for i in range(calls):
                if i == 4:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                e.decode_verify(toks, keep_all=True)
            torch.cuda.synchronize()
            cells[fmt].append((time.perf_counter() - t0) * 1e3 / (calls - 4))
    print(json.dumps(dict(verify={f: dict(ms=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4)) for f, v in cells.items()},
                          T=T, layers=args.layers)), flush=True)
    select("bf16")
    e.close()

    # ---- the five GEMV roles alone, pre-packed operands, the launches a batched step makes
    BF16, NONE, SWIGLU, PARTIAL = _lib.BF16, _lib.EPI_NONE, _lib.EPI_SWIGLU, 5
    qkvd = (cfg.text["num_attention_heads"] + 2 * cfg.text["num_key_value_heads"]) * 128
    ROLES = [("qkv", qkvd, H, NONE, 1, False), ("o_proj", H, H, PARTIAL, 2, False), ("gate|up", 2 * It, H, SWIGLU, 1, False),
             ("down_proj", H, It, PARTIAL, 8, False), ("lm_head", V, H, NONE, 1, True)]
    g = torch.Generator(device="cuda").manual_seed(2)
    for name, N, K, epi, ks, f32 in ROLES:
        w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).bfloat16()
        w4 = torch.empty(N, K // 2, dtype=torch.uint8, device="cuda"); s4 = torch.empty(N, K // 32, dtype=torch.uint8, device="cuda")
        check(lib.omchat_op_quant_mxfp4(BF16, ptr(w), N, K, ptr(w4), ptr(s4), None))
        wp = torch.empty_like(w); w4p = torch.empty_like(w4); s4p = torch.empty_like(s4)
        check(lib.omchat_op_pack_w(BF16, ptr(w), K, N, K, ptr(wp), None))
        check(lib.omchat_op_pack_w4(ptr(w4), ptr(s4), N, K, ptr(w4p), ptr(s4p), None))
        torch.cuda.synchronize()
        del w, w4, s4
        byts = dict(bf16=N * K * 2, mxfp4=N * K // 2 + N * K // 32)
        bias = torch.zeros(N, device="cuda", dtype=torch.bfloat16) if name == "qkv" else None

        def copies(ts, nbytes):
            n = max(2, -(-768 * 2 ** 20 // nbytes))
            return [tuple(t.clone() for t in ts) for _ in range(n)]
        sets = dict(bf16=copies((wp,), byts["bf16"]), mxfp4=copies((w4p, s4p), byts["mxfp4"]))
        out = {}
        for b in (8, 32):
            NB = 2 if b > 16 else 1
            xr = (torch.randn(b, K, device="cuda", generator=g) * 0.5).bfloat16()
            xp = torch.empty(NB * 16 * K, device="cuda", dtype=torch.bfloat16)
            check(lib.omchat_op_pack_x(BF16, ptr(xr), K, b, K, ptr(xp), None))
            n_y = N // 2 if epi == SWIGLU else N
            y = torch.zeros(ks * NB * 16 * n_y, device="cuda", dtype=torch.float32 if (f32 or epi == PARTIAL) else torch.bfloat16)

            def launch(fmt, c):
                return lib.omchat_op_gemv_prepacked(BF16, ptr(xp), ptr(c[0]), ptr(c[1]) if fmt == "mxfp4" else None, ptr(y), n_y, b, N, K, ptr(bias),
                                                    epi, int(f32), ks, int(epi == SWIGLU), None)
            times = {f: [] for f in FORMATS}
            for r in range(args.repeats):
                for fmt in FORMATS:
                    cs = sets[fmt]
                    for i in range(len(cs)):
                        check(launch(fmt, cs[i]))
                    torch.cuda.synchronize()
                    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for i in range(args.batched_iters):
                        check(launch(fmt, cs[i % len(cs)]))
                    z.record()
                    z.synchronize()
                    times[fmt].append(a.elapsed_time(z) * 1e3 / args.batched_iters)
            for fmt in FORMATS:
                us = statistics.median(times[fmt])
                out[f"b{b}/{fmt}"] = dict(us=round(us, 2), min=round(min(times[fmt]), 2), max=round(max(times[fmt]), 2),
                                          GBps=round(byts[fmt] / us / 1e3, 1))
        print(json.dumps(dict(batched_role=name, N=N, K=K, ksplit=ks, weight_MB={k: round(v / 2 ** 20, 1) for k, v in byts.items()}, **out)), flush=True)
        del sets, wp, w4p, s4p
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
