"""Cost of classifier-free guidance on the device:
    python tools/bench_guidance.py [--iters 200] [--repeats 5] [--model 13b|tiny] [--context 1024] [--steps 64]
Part 1, the stage per pick on [2b, 152064] fp32 logits (the OmChat vocabulary), b = 1 and b = 16, in one context: microseconds per pick
(GPU time of a back-to-back loop, events around it; median and spread over the repeats) of the plain greedy pick of b rows, of the guided
greedy pick of 2b rows (two stage launches + the twin launch more), what that adds, and the two stage launches alone (omchat_op_guidance).
Part 2, the decode step: the guided b = 1 step (2 rows at their own lengths) against the plain b = 1 step and the plain b = 2 step, all
over the same context length in one context, alternating, host-timed windows of --steps steps that end in a synchronise.  One JSON line
per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V = 152064
SCALE = 1.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--model", choices=("13b", "tiny"), default="13b")
    ap.add_argument("--context", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=64)
    args = ap.parse_args()
    import torch
    from omchat_amd import _lib
    from omchat_amd.config import omchat13b, tiny
    from omchat_amd.engine import Engine

    def spread(xs, nd=2):
        return dict(us=round(statistics.median(xs), nd), min=round(min(xs), nd), max=round(max(xs), nd))

    def timed(fn):
        out = []
        for _ in range(args.repeats):
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            z.record()
            z.synchronize()
            out.append(a.elapsed_time(z) * 1e3 / args.iters)
        return spread(out)

    # ---- part 1: the stage per pick
    e = Engine(tiny(vocab=V), dtype="bf16", max_seq=16, max_batch=32, max_tiles=1, vision=False)
    lib = e.lib
    for b in (1, 16):
        lg = (torch.randn(2 * b, V, device="cuda") * 3).contiguous()
        e.guidance_off()
        plain = timed(lambda: e.argmax(lg[:b]))
        e.set_guidance(b, SCALE)
        guided = timed(lambda: e.argmax(lg))
        e.guidance_off()
        ws = torch.empty(int(lib.omchat_op_guidance_ws(b, V)), dtype=torch.uint8, device="cuda")
        out = torch.empty(b, V, dtype=torch.float32, device="cuda")
        stage = timed(lambda: _lib.check(lib.omchat_op_guidance(_lib.ptr(lg), V, b, V, SCALE, _lib.ptr(ws), _lib.ptr(out), V, _lib.cur_stream())))
        print(json.dumps(dict(part="pick", logits=[2 * b, V], greedy_b_rows=plain, guided_2b_rows=guided,
                              added_us=round(guided["us"] - plain["us"], 2), stage_alone=stage,
                              stage_bytes=2 * b * V * 4 * 2 + b * V * 4)), flush=True)
    e.close()

    # ---- part 2: the decode step
    cfg = omchat13b() if args.model == "13b" else tiny(vocab=V)
    S, n = args.context, args.steps
    e = Engine(cfg, dtype="bf16", max_seq=S + n + 64, max_batch=2, max_tiles=1, vision=False)
    e.fill_synthetic(0)
    H = cfg.text["hidden_size"]
    x = (torch.randn(2, S, H, device="cuda") * 0.5).to(torch.bfloat16)

    def window(rows, guided):
        """n timed steps of `rows` rows behind 4 warm-up steps, then the rows go back to where they started"""
        e.guidance_off()
        if guided:
            e.set_guidance(1, SCALE)
        tok = torch.full((rows,), 17, dtype=torch.int32, device="cuda")
        for _ in range(4):
            tok, _ = e.decode_step(tok)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            tok, _ = e.decode_step(tok)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n * 1e6
        e.kv_rewind(rows, n + 4)                                      # every window starts from the prefill's S slots
        return dt

    for graph in (False, True):
        e.enable_decode_graph(graph)
        e.guidance_off()
        e.prefill(x)                                                  # both rows at S slots: every form starts from the same context
        cols = dict(plain_b1=[], plain_b2=[], guided_b1=[])
        window(1, False); window(2, False); window(2, True)          # every form's first step (replica build, graph capture) outside the timing
        for _ in range(args.repeats):                                 # alternating
            cols["plain_b1"].append(window(1, False))
            cols["plain_b2"].append(window(2, False))
            cols["guided_b1"].append(window(2, True))
        row = {k: spread(v, 1) for k, v in cols.items()}
        print(json.dumps(dict(part="step", model=args.model, context=S, graph=graph, **row,
                              guided_over_plain_b1=round(row["guided_b1"]["us"] / row["plain_b1"]["us"], 3),
                              guided_over_plain_b2_us=round(row["guided_b1"]["us"] - row["plain_b2"]["us"], 1))), flush=True)
    e.enable_decode_graph(False)
    e.close()


if __name__ == "__main__":
    main()
