"""Cost of layer-contrastive decoding on the device:
    python tools/bench_dola.py [--iters 200] [--repeats 5] [--model 13b|tiny] [--context 1024] [--steps 64]
Part 1, the stage alone (omchat_op_dola) on [(k + 1), 152064] fp32 logits (the OmChat vocabulary, b = 1) at k = 1, 7 and 16: microseconds
per call (GPU time of a back-to-back loop, events around it; median and spread over the repeats) -- three launches, two at k = 1.
Part 2, the decode step: the b = 1 step with dola_layers='high' (at 28 layers: 7 candidates, 8 rows through the 16-bit head) against the
plain b = 1 step over the same context length in one context, alternating, host-timed windows of --steps steps that end in a synchronise,
eager and with the decode graph.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V = 152064


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--model", choices=("13b", "tiny"), default="13b")
    ap.add_argument("--context", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=64)
    args = ap.parse_args()
    import torch
    from omchat_amd import _lib, dola
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

    # ---- part 1: the stage alone
    lib = _lib.lib()
    for k in (1, 7, 16):
        lg = (torch.randn(k + 1, V, device="cuda") * 3).contiguous()
        n = int(lib.omchat_op_dola_ws(1, k, V))
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        out = torch.empty(1, V, dtype=torch.float32, device="cuda")
        picked = torch.empty(1, dtype=torch.int32, device="cuda")
        stage = timed(lambda: _lib.check(lib.omchat_op_dola(_lib.ptr(lg), V, V, 1, k, 0.1, _lib.ptr(out), V, _lib.ptr(picked), _lib.ptr(ws), n,
                                                            _lib.cur_stream())))
        # bytes: every row once for the partials, the final row and every candidate once for the divergences (k > 1), two rows and the output
        # for the contrast
        nbytes = (k + 1) * V * 4 + (2 * k * V * 4 if k > 1 else 0) + 3 * V * 4
        print(json.dumps(dict(part="stage", logits=[k + 1, V], k=k, stage_alone=stage, stage_bytes=nbytes)), flush=True)

    # ---- part 2: the decode step
    cfg = omchat13b() if args.model == "13b" else tiny(vocab=V, layers_t=4)
    layers = dola.resolve_layers("high", cfg.text["num_hidden_layers"])
    S, n = args.context, args.steps
    e = Engine(cfg, dtype="bf16", max_seq=S + n + 64, max_batch=len(layers) + 1, max_tiles=1, vision=False)
    e.fill_synthetic(0)
    H = cfg.text["hidden_size"]
    x = (torch.randn(1, S, H, device="cuda") * 0.5).to(torch.bfloat16)

    def window(on):
        """n timed steps behind 4 warm-up steps, then the row goes back to where it started"""
        e.dola_off()
        if on:
            e.set_dola(1, layers)
        tok = torch.full((1,), 17, dtype=torch.int32, device="cuda")
        for _ in range(4):
            tok, _ = e.decode_step(tok)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            tok, _ = e.decode_step(tok)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n * 1e6
        e.kv_rewind(1, n + 4)                                          # every window starts from the prefill's S slots
        return dt

    for graph in (False, True):
        e.enable_decode_graph(graph)
        e.dola_off()
        e.prefill(x)
        cols = dict(plain_b1=[], dola_b1=[])
        window(False); window(True)                                    # every form's first step (coding, graph capture) outside the timing
        for _ in range(args.repeats):                                  # alternating
            cols["plain_b1"].append(window(False))
            cols["dola_b1"].append(window(True))
        row = {k: spread(v, 1) for k, v in cols.items()}
        print(json.dumps(dict(part="step", model=args.model, context=S, graph=graph, layers=layers, head_rows=len(layers) + 1, **row,
                              dola_over_plain=round(row["dola_b1"]["us"] / row["plain_b1"]["us"], 3),
                              dola_minus_plain_us=round(row["dola_b1"]["us"] - row["plain_b1"]["us"], 1))), flush=True)
    e.enable_decode_graph(False)
    e.close()


if __name__ == "__main__":
    main()
