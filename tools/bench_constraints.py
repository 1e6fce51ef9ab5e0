"""Per-pick cost of the on-device logits constraints over the plain greedy pick, on [b, 152064] fp32 logits (the OmChat vocabulary) in one
context:
    python tools/bench_constraints.py [--iters 200]
Prints one line per (batch, history length, constraint): microseconds per pick (GPU time of a back-to-back loop, events around it) and the
extra over greedy.  The pick is the first-token seam (omchat_greedy): ban pass + apply pass + argmax, the history as long as stated."""
import argparse
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V = 152064


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    import torch
    from omchat_amd.config import tiny
    from omchat_amd.engine import Engine
    cfg = tiny(vocab=V)
    e = Engine(cfg, dtype="bf16", max_seq=16, max_batch=32, max_tiles=1, vision=False)
    rng = random.Random(0)
    words = [[rng.randrange(V) for _ in range(1 + i % 4)] for i in range(64)]
    sets = [("ngram3", dict(no_repeat_ngram_size=3)), ("bad_words64", dict(bad_words_ids=words)),
            ("min_new", dict(min_new_tokens=8, eos=[151643, 151645])), ("suppress16", dict(suppress_tokens=list(range(100, 116)))),
            ("begin_suppress", dict(begin_suppress_tokens=[1, 2])),
            ("all", dict(no_repeat_ngram_size=3, bad_words_ids=words, min_new_tokens=8, eos=[151643, 151645], suppress_tokens=list(range(100, 116)),
                         begin_suppress_tokens=[1, 2]))]

    def timed(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        z.record()
        z.synchronize()
        return a.elapsed_time(z) * 1e3 / args.iters

    for b in (1, 32):
        lg = (torch.randn(b, V, device="cuda") * 3).contiguous()
        e.constraints_off()
        g = timed(lambda: e.argmax(lg))
        print(json.dumps(dict(batch=b, pick="greedy", us=round(g, 2))))
        for L in (512, 4096, 33000):
            hist = [[rng.randrange(2000) for _ in range(L)] for _ in range(b)]      # a small span: the tail's first id matches often
            for name, p in sets:
                e.set_constraints(b, hist, 1, **p)
                t = timed(lambda: e.argmax(lg))
                print(json.dumps(dict(batch=b, history=L, pick=name, us=round(t, 2), over_greedy_us=round(t - g, 2))))
    e.close()


if __name__ == "__main__":
    main()
