"""Per-pick cost of recording per-token log-probabilities, on [b, 152064] fp32 logits (the OmChat vocabulary) in one
context:
    python tools/bench_logprob.py [--iters 200] [--repeats 5]
Prints one JSON line per (batch, pick): microseconds per pick (GPU time of a back-to-back loop, events around it; median and spread over the
repeats) with logprobs off and on, and the added microseconds; then with the record's extras on -- top_n = 5, top_n = 20, 4 scored ids --
and what each adds to "on".  On a commit without Engine.set_logprobs only the "off" column is measured (run it there for the parent's
column); on one without the extras the three further columns are left out."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETS = [("greedy", None), ("T", dict(temperature=0.8)), ("T,k=50,p=0.9", dict(temperature=0.8, top_k=50, top_p=0.9)),
        ("T,k=50,p=0.9,rep=1.3", dict(temperature=0.8, top_k=50, top_p=0.9, repetition_penalty=1.3))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    from omchat_amd.config import tiny
    from omchat_amd.engine import Engine
    cfg = tiny(vocab=152064)
    e = Engine(cfg, dtype="bf16", max_seq=16, max_batch=32, max_tiles=1, vision=False)
    has = hasattr(e, "set_logprobs")
    extras = hasattr(e, "read_logprob_extras")
    EXTRAS = [("top5", dict(top_n=5)), ("top20", dict(top_n=20)), ("scored4", dict(score_token_ids=[32, 33, 34, 35]))]

    def timed(fn, arm):
        out = []
        for _ in range(args.repeats):
            arm()
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
        return dict(us=round(statistics.median(out), 2), min=round(min(out), 2), max=round(max(out), 2))

    for b in (1, 32):
        lg = (torch.randn(b, 152064, device="cuda") * 3).contiguous()
        for name, p in SETS:
            if p is None:
                e.sampling_off()
                fn = lambda: e.argmax(lg)
            else:
                e.set_sampling(b, seed=1, seen=[list(range(0, 4000, 7))] * b, **p)
                fn = lambda: e.sample(lg)
            off = timed(fn, e.logprobs_off if has else (lambda: None))
            row = dict(batch=b, pick=name, off=off)
            if has:
                row["on"] = timed(fn, lambda: e.set_logprobs(b, args.iters + 10))
                row["added_us"] = round(row["on"]["us"] - off["us"], 2)
            if has and extras:
                for col, kw in EXTRAS:
                    row[col] = timed(fn, lambda: e.set_logprobs(b, args.iters + 10, **kw))
                    row[col + "_added_us"] = round(row[col]["us"] - row["on"]["us"], 2)
            print(json.dumps(row))
    if has:
        e.logprobs_off()
    e.close()


if __name__ == "__main__":
    main()
