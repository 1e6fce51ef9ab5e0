"""Per-token cost of the on-device sampler over the greedy pick, on [b, 152064] fp32 logits (the OmChat vocabulary) in one context:
    python tools/bench_sample.py [--iters 200]
Prints one line per (batch, parameter set): microseconds per pick (GPU time of a back-to-back loop, events around it) and the extra over
greedy."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETS = [("T", dict(temperature=0.8)), ("T,k=50", dict(temperature=0.8, top_k=50)),
        ("T,k=50,p=0.9", dict(temperature=0.8, top_k=50, top_p=0.9)), ("T,p=0.9", dict(temperature=0.8, top_p=0.9)),
        ("T,k=50,p=0.9,rep=1.3", dict(temperature=0.8, top_k=50, top_p=0.9, repetition_penalty=1.3)),
        ("T,min_p=0.05", dict(temperature=0.8, min_p=0.05)), ("T,typical_p=0.9", dict(temperature=0.8, typical_p=0.9)),
        ("T,eta=3e-4", dict(temperature=0.8, eta_cutoff=3e-4)),
        ("T,k=50,p=0.9,min_p,typical,eps,eta", dict(temperature=0.8, top_k=50, top_p=0.9, min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4,
                                                    eta_cutoff=3e-4))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    import torch
    from omchat_amd.config import tiny
    from omchat_amd.engine import Engine
    cfg = tiny(vocab=152064)
    e = Engine(cfg, dtype="bf16", max_seq=16, max_batch=32, max_tiles=1, vision=False)

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
        lg = (torch.randn(b, 152064, device="cuda") * 3).contiguous()
        e.sampling_off()
        g = timed(lambda: e.argmax(lg))
        print(json.dumps(dict(batch=b, pick="greedy", us=round(g, 2))))
        for name, p in SETS:
            e.set_sampling(b, seed=1, seen=[list(range(0, 4000, 7))] * b, **p)
            t = timed(lambda: e.sample(lg))
            print(json.dumps(dict(batch=b, pick=name, us=round(t, 2), over_greedy_us=round(t - g, 2))))
    e.close()


if __name__ == "__main__":
    main()
