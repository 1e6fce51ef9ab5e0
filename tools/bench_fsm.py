"""Per-pick cost of the on-device token-FSM stage over the plain greedy pick, on [b, 152064] fp32 logits (the OmChat vocabulary) in one
context:
    python tools/bench_fsm.py [--iters 200]
Prints one line per (batch, pick): microseconds per pick (GPU time of a back-to-back loop, events around it) and the extra over greedy, for
rows in a state of 16, 4 096 and 152 064 edges -- and, in the same run, the plain greedy pick and the no_repeat_ngram_size=3 row of
tools/bench_constraints.py (history 4 096), the stage of the same two launches and the same copy that is the yardstick here.  The pick is
the first-token seam (omchat_greedy): mark pass + apply pass + argmax; the state does not advance."""
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
    from omchat_amd.fsm import TokenFSM
    cfg = tiny(vocab=V)
    e = Engine(cfg, dtype="bf16", max_seq=16, max_batch=32, max_tiles=1, vision=False)
    rng = random.Random(0)
    sizes = (16, 4096, V)
    off, tok, nxt = [0], [], []
    for s, n in enumerate(sizes):      # every edge of a state leads back to it
        tok += sorted(rng.sample(range(V), n)) if n < V else list(range(V))
        nxt += [s] * n
        off.append(len(tok))
    e.load_token_fsm(TokenFSM.from_arrays(off, tok, nxt, vocab_size=V))

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
        e.token_fsm_off()
        g = timed(lambda: e.argmax(lg))
        print(json.dumps(dict(batch=b, pick="greedy", us=round(g, 2))))
        hist = [[rng.randrange(2000) for _ in range(4096)] for _ in range(b)]
        e.set_constraints(b, hist, 1, no_repeat_ngram_size=3)
        t = timed(lambda: e.argmax(lg))
        print(json.dumps(dict(batch=b, history=4096, pick="ngram3", us=round(t, 2), over_greedy_us=round(t - g, 2))))
        e.constraints_off()
        for s, n in enumerate(sizes):
            e.token_fsm_begin(b, s, 1)
            t = timed(lambda: e.argmax(lg))
            print(json.dumps(dict(batch=b, edges=n, pick="fsm", us=round(t, 2), over_greedy_us=round(t - g, 2))))
        e.token_fsm_off()
    e.close()


if __name__ == "__main__":
    main()
