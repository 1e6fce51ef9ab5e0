"""Cost of generate(do_sample=True, num_return_sequences=N):
    python tools/bench_group.py [--steps 32] [--passes 5] [--N 4 8 16] [--P 64 1024 3584 16384] [--no-once]
One JSON line per measurement, at the configs[1] decoder geometry (OmChat-2.1-8B's Qwen2-7B, synthetic bf16 weights, one GPU, one prompt):
  decode_step  one decode step of the N sibling rows with the prompt's cache slots shared (omchat_group_begin share = 1) against the same
               step on forked rows (share = 0), on the same context and prompt: `passes` alternating passes of `steps` steps each (greedy
               picks, no logits copied out, no prefill in the timed region), medians, and the spread (max - min) / median of each side
  once         what a call pays once: prefill of one prompt + the fork of its slots into N rows, against the prefill of the
               repeat_interleave'd batch of N prompts"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--N", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--P", type=int, nargs="+", default=[64, 1024, 3584, 16384])
    ap.add_argument("--no-once", action="store_true")
    ap.add_argument("--once-max-rows", type=int, default=32768, help="skip the repeat_interleave'd prefill beyond N * P rows")
    args = ap.parse_args()
    import torch
    from omchat_amd.config import omchat8b_21
    from omchat_amd.engine import Engine

    c8 = omchat8b_21()
    H = c8.text["hidden_size"]
    Nmax = max(args.N)

    def timed(fn):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        z.record()
        z.synchronize()
        return a.elapsed_time(z)

    for P in args.P:
        once_rows = max([n * P for n in args.N if n * P <= args.once_max_rows and not args.no_once] or [P])
        eng = Engine(c8, dtype="bf16", max_seq=P + args.steps + 8, max_batch=Nmax, max_tiles=1, vision=False, max_prefill_rows=max(P, once_rows))
        eng.fill_synthetic(0)
        emb = torch.randn(1, P, H, device="cuda").to(eng.torch_dtype) * 0.5
        for N in args.N:
            lg, _ = eng.prefill(emb, [P])
            tok0 = eng.argmax(lg).repeat(N)
            ms = {0: [], 1: []}

            def loop():
                tok = tok0
                for _ in range(args.steps):
                    tok, _ = eng.decode_step(tok)

            for p in range(args.passes + 1):              # pass 0 warms both forms up (packed weight replica, workspace)
                for share in ((0, 1) if p % 2 == 0 else (1, 0)):
                    eng.group_begin(1, N, P, share=bool(share))
                    t = timed(loop) / args.steps
                    eng.kv_rewind(N, args.steps)
                    if p:
                        ms[share].append(t)
            med = {s: statistics.median(v) for s, v in ms.items()}
            spread = {s: (max(v) - min(v)) / med[s] for s, v in ms.items()}
            print(json.dumps(dict(what="decode_step", N=N, P=P, steps=args.steps, passes=args.passes, forked_ms=round(med[0], 4),
                                  shared_ms=round(med[1], 4), forked_spread=round(spread[0], 4), shared_spread=round(spread[1], 4),
                                  shared_over_forked=round(med[1] / med[0], 4))), flush=True)
            eng.group_end()
            if args.no_once or N * P > args.once_max_rows:
                continue
            embN = emb.repeat(N, 1, 1)
            fork, full = [], []
            for p in range(4):
                def once_fork():
                    eng.prefill(emb, [P])
                    eng.group_begin(1, N, P, share=False)
                a = timed(once_fork)
                b = timed(lambda: eng.prefill(embN, [P] * N))
                if p:
                    fork.append(a); full.append(b)
            print(json.dumps(dict(what="once", N=N, P=P, prefill_once_plus_fork_ms=round(statistics.median(fork), 3),
                                  prefill_expanded_ms=round(statistics.median(full), 3),
                                  ratio=round(statistics.median(fork) / statistics.median(full), 4))), flush=True)
        eng.close()
        del eng, emb
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
