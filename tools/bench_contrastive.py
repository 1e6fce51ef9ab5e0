"""Cost of contrastive search on the device:
    python tools/bench_contrastive.py [--iters 200] [--repeats 5] [--model 7b|tiny] [--steps 32]
Part 1, the added launches alone at Qwen2-7B width (H = 3584, V = 152064) for k = 4 / 8 / 16 candidates and L = 1024 / 3584 history rows:
microseconds per call of the penalty launch, the select-and-commit launch and the top-k (two launches), each as the GPU time of a back-to-back
loop with events around it (median and spread over the repeats); the penalty's bytes -- L rows, the norm table and k candidates -- and
its achieved bytes per second.
Part 2, the whole step on a Qwen2-7B-wide decoder over a context of L positions: the k-row decode step plus omchat_contrastive_step (penalty,
select, one-slot KV gather, top-k) against the plain k-row group step on the same context, alternating, host-timed windows of --steps steps
that end in a synchronise, fork and shared-prompt form, and the contrastive step again with the host reading the emitted id behind every
step as generate()'s loop does (it does not run a step ahead); and the gate|up GEMV's rate of a batch-1 step of the same run (HIP-event brackets,
Engine.prof_read), to set the penalty's rate against.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, V = 3584, 152064


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--model", choices=("7b", "tiny"), default="7b")
    ap.add_argument("--steps", type=int, default=32)
    args = ap.parse_args()
    import torch
    from omchat_amd import _lib
    from omchat_amd.config import omchat8b_21, tiny
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

    lib = _lib.lib()
    check, ptr, cs = _lib.check, _lib.ptr, _lib.cur_stream
    # ---- part 1: the launches alone
    for L in (1024, 3584):
        hist = torch.randn(L + 1, H, device="cuda").to(torch.bfloat16)
        inv = torch.empty(L + 1, dtype=torch.float32, device="cuda")
        ch, rpc = _lib.C.c_int(0), _lib.C.c_int(0)
        check(lib.omchat_op_contrastive_plan(L, _lib.C.byref(ch), _lib.C.byref(rpc)))
        chunks = ch.value
        for k in (4, 8, 16):
            cand = torch.randn(k, H, device="cuda").to(torch.bfloat16)
            part = torch.empty(chunks, 16, dtype=torch.float32, device="cuda")
            cinv = torch.empty(16, dtype=torch.float32, device="cuda")
            check(lib.omchat_op_contrastive_penalty(_lib.BF16, ptr(hist), ptr(inv), 1, L, H, ptr(cand), 0, k, ptr(part), ptr(cinv), cs()))
            pen = timed(lambda: check(lib.omchat_op_contrastive_penalty(_lib.BF16, ptr(hist), ptr(inv), 0, L, H, ptr(cand), 0, k, ptr(part), ptr(cinv), cs())))
            lg = (torch.randn(k, V, device="cuda") * 3).contiguous()
            ids = torch.empty(k, dtype=torch.int32, device="cuda")
            probs = torch.empty(k, dtype=torch.float32, device="cuda")
            sel = torch.full((1,), k - 1, dtype=torch.int32, device="cuda")
            ws = torch.empty(int(lib.omchat_op_contrastive_topk_ws(V)), dtype=torch.uint8, device="cuda")
            topk = timed(lambda: check(lib.omchat_op_contrastive_topk(ptr(lg), V, ptr(sel), V, k, ptr(ids), ptr(probs), ptr(ws), cs())))
            rec = torch.empty(52, dtype=torch.int32, device="cuda")
            par = torch.empty(k, dtype=torch.int32, device="cuda")
            one = torch.empty(1, dtype=torch.int32, device="cuda")
            select = timed(lambda: check(lib.omchat_op_contrastive_select(_lib.BF16, ptr(part), chunks, k, 0.6, ptr(ids), ptr(probs), ptr(cinv), ptr(cand), 0,
                                                                          H, ptr(hist), ptr(inv), L, None, 0, 0, ptr(rec), ptr(par), ptr(sel), ptr(one), ptr(one),
                                                                          cs())))
            nbytes = L * H * 2 + L * 4 + k * H * 2
            print(json.dumps(dict(part="launches", L=L, k=k, chunks=chunks, rows_per_chunk=rpc.value, penalty=pen, select=select, topk=topk,
                                  penalty_bytes=nbytes, penalty_GBps=round(nbytes / pen["us"] / 1e3, 1))), flush=True)

    # ---- part 2: the whole step
    cfg = omchat8b_21() if args.model == "7b" else tiny(vocab=V, layers_t=4)
    n = args.steps
    Hm = cfg.text["hidden_size"]
    It = cfg.text["intermediate_size"]
    for L in (1024, 3584):
        e = Engine(cfg, dtype="bf16", max_seq=L + n + 72, max_batch=16, max_tiles=1, vision=False)
        e.fill_synthetic(0)
        x = (torch.randn(1, L, Hm, device="cuda") * 0.5).to(torch.bfloat16)
        # the gate|up GEMV of a batch-1 step in this context: HIP-event brackets on one layer per eager step
        e.prefill(x)
        tok = torch.full((1,), 17, dtype=torch.int32, device="cuda")
        for _ in range(4):
            tok, _ = e.decode_step(tok)
        e.prof_enable(True)
        e.prof_read(_lib.PROF_DECODE_GATEUP)
        for _ in range(24):
            tok, _ = e.decode_step(tok)
        torch.cuda.synchronize()
        ms, cnt = e.prof_read(_lib.PROF_DECODE_GATEUP)
        e.prof_enable(False)
        gu_us = ms * 1e3 / max(cnt, 1)
        gu_bytes = 2 * It * Hm * 2
        print(json.dumps(dict(part="gate_up_b1", context=L, launches=cnt, us=round(gu_us, 2), bytes=gu_bytes, GBps=round(gu_bytes / gu_us / 1e3, 1))), flush=True)
        for k in (4, 8, 16):
            for share in (False, True):
                def window(on, host_read=False):
                    """n timed steps behind 2 warm-up steps over a fresh prefill of the same context; host_read: the host reads the emitted
                    id behind every step before it enqueues the next one, as generate()'s loop does"""
                    e.group_end(); e.contrastive_off()
                    if on:
                        e.set_contrastive(k, 0.6, n + 2, share)
                    lgp, _ = e.prefill(x)
                    if on:
                        cand = e.contrastive_step(lgp)
                    else:
                        e.group_begin(1, k, L, share)
                        cand = torch.arange(17, 17 + k + 1, dtype=torch.int32, device="cuda")
                    def step(c):
                        nxt, lg = e.decode_step(c[:k], want_logits=True)
                        out = e.contrastive_step(lg) if on else nxt
                        if host_read:
                            int(out[k])
                        return out
                    for _ in range(2):
                        cand = step(cand)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(n):
                        cand = step(cand)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) / n * 1e6
                cols = dict(group_step=[], contrastive_step=[], contrastive_step_host_read=[])
                window(False); window(True)
                for _ in range(args.repeats):
                    cols["group_step"].append(window(False))
                    cols["contrastive_step"].append(window(True))
                    cols["contrastive_step_host_read"].append(window(True, host_read=True))
                row = {kk: spread(v, 1) for kk, v in cols.items()}
                print(json.dumps(dict(part="step", model=args.model, context=L, k=k, share=share, **row,
                                      added_us=round(row["contrastive_step"]["us"] - row["group_step"]["us"], 1),
                                      ratio=round(row["contrastive_step"]["us"] / row["group_step"]["us"], 3),
                                      host_read_stall_us=round(row["contrastive_step_host_read"]["us"] - row["contrastive_step"]["us"], 1))), flush=True)
        e.group_end(); e.contrastive_off()
        e.close()
        del e
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
