"""Cost of the on-device beam search (csrc/beam.hip):
    python tools/bench_beam.py [--iters 100] [--no-e2e]
One JSON line per measurement: the selection (select + finish kernels) per step at b = 1 and N in {2, 4, 8} on [N, 152064] fp32 logits;
the KV gather (straight copy kernel) against the suffix length, with its bytes over an 8 TB/s HBM rate; and one beam decode step (4 beam
rows: decode_step + beam_step, its KV gather included) against one 4-row greedy decode step at the configs[1] decoder geometry (OmChat-2.1-8B's
Qwen2-7B, synthetic weights, 64-slot prompt), decode loops alone, no prefill in the timed region.
--processed: the step on processed scores (omchat_beam_processors, repetition_penalty 1.1 + no_repeat_ngram_size 3: ban, statistics, select,
finish and history move) against the plain step at b = 1, N in {2, 4, 8}, histories from 64 and from 1024 ids -- two contexts in one process,
alternating windows, medians -- and a 4-row processed beam decode step between two plain ones."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--processed", action="store_true", help="also the search on processed scores (omchat_beam_processors) against the plain one")
    args = ap.parse_args()
    import torch
    from omchat_amd import _lib
    from omchat_amd._lib import check, ptr
    from omchat_amd.config import tiny, omchat8b_21
    from omchat_amd.engine import Engine

    def timed(fn, iters):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        z.record()
        z.synchronize()
        return a.elapsed_time(z) * 1e3 / iters

    # selection per step: prefill-shaped first step excluded, then b*N rows every step (no EOS: nothing freezes before max_new)
    cfg = tiny(vocab=152064)
    e = Engine(cfg, dtype="bf16", max_seq=2048, max_batch=8, max_tiles=1, vision=False)
    for N in (2, 4, 8):
        lg0 = (torch.randn(1, 152064, device="cuda") * 3).contiguous()
        lg = (torch.randn(N, 152064, device="cuda") * 3).contiguous()
        e.beam_begin(1, N, 1.0, False, [], args.iters + 16, prompt_len=4)
        e.beam_step(lg0)
        us = timed(lambda: e.beam_step(lg), args.iters)
        print(json.dumps(dict(what="select+finish", b=1, N=N, V=152064, us_per_step=round(us, 2))), flush=True)
    e.close()

    if args.processed:
        # the step's selection on processed scores (ban + statistics + select + finish + history move: omchat_beam_processors with
        # repetition_penalty 1.1 and no_repeat_ngram_size 3) against the plain step, two contexts in one process, alternating windows
        import statistics
        W, it = 5, 20
        ea = Engine(cfg, dtype="bf16", max_seq=2048, max_batch=8, max_tiles=1, vision=False)
        eb = Engine(cfg, dtype="bf16", max_seq=2048, max_batch=8, max_tiles=1, vision=False)
        for N in (2, 4, 8):
            for H in (64, 1024):
                g = torch.Generator().manual_seed(N + H)
                prompt = [torch.randint(0, 152064, (H,), generator=g).tolist()]
                lg0 = (torch.randn(1, 152064, device="cuda") * 3).contiguous()
                lg = (torch.randn(N, 152064, device="cuda") * 3).contiguous()
                for eng, proc in ((ea, False), (eb, True)):
                    eng.beam_begin(1, N, 1.0, False, [], W * (it + 5) + 8, prompt_len=4)
                    if proc:
                        eng.beam_processors(prompt, repetition_penalty=1.1, no_repeat_ngram_size=3)
                    eng.beam_step(lg0)
                wa, wb = [], []
                for _ in range(W):
                    wa.append(timed(lambda: ea.beam_step(lg), it))
                    wb.append(timed(lambda: eb.beam_step(lg), it))
                print(json.dumps(dict(what="processed select step", b=1, N=N, V=152064, history=[H + 1, H + W * (it + 5)],
                                      plain_us=round(statistics.median(wa), 2), processed_us=round(statistics.median(wb), 2),
                                      plain_windows=[round(x, 1) for x in wa], processed_windows=[round(x, 1) for x in wb])), flush=True)
        ea.close()
        eb.close()

    # KV gather at the configs[1] per-rank cache geometry (28 layers, 4 kv heads): N - 1 = 3 rows <- one parent over the suffix
    c8 = omchat8b_21()
    layers, kvh, S, R = c8.text["num_hidden_layers"], c8.text["num_key_value_heads"], 1088, 4
    k = torch.zeros(layers, R, kvh, S, 128, dtype=torch.bfloat16, device="cuda")
    v = torch.zeros_like(k)
    for n in (16, 64, 256, 1024):
        fn = lambda: check(e.lib.omchat_op_kv_gather(_lib.BF16, ptr(k), ptr(v), None, None, None, None, layers, R, kvh, S, None, 1, 3, 0, 64,
                                                    64 + n, _lib.cur_stream()))
        us = timed(fn, 20)
        nbytes = 2 * 3 * layers * kvh * n * 256 * 2          # K and V, read + write
        print(json.dumps(dict(what="kv_gather", suffix=n, us=round(us, 2), bytes=nbytes, byte_time_us=round(nbytes / HBM * 1e6, 2),
                              note="includes one stream sync per call")), flush=True)
    del k, v

    if args.no_e2e:
        return
    # one decode step of the 4 beam rows (decode_step + beam_step with its KV gather) against one 4-row greedy decode step, same cache
    # length, the loops alone (no prefill in the timed region)
    eng = Engine(c8, dtype="bf16", max_seq=256, max_batch=4, max_tiles=1, vision=False)
    eng.fill_synthetic(0)
    emb = torch.randn(1, 64, c8.text["hidden_size"], device="cuda").to(eng.torch_dtype) * 0.5
    steps = 32
    res = {}
    for name in ("greedy_b4", "beam4") + (("beam4_processed", "beam4") if args.processed else ()):
        lg, _ = eng.prefill(emb.repeat(4 if name == "greedy_b4" else 1, 1, 1), [64] * (4 if name == "greedy_b4" else 1))
        if name != "greedy_b4":
            eng.beam_begin(1, 4, 1.0, False, [], steps + 2, prompt_len=64)
            if name == "beam4_processed":
                eng.beam_processors([list(range(100, 164))], repetition_penalty=1.1, no_repeat_ngram_size=3)
            tok = eng.beam_step(lg)
        else:
            tok = eng.argmax(lg)
        eng.decode_step(tok, want_logits=True)          # warm-up (packed replica, first batched step)
        torch.cuda.synchronize()
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            nxt, lg = eng.decode_step(tok, want_logits=True)
            tok = nxt if name == "greedy_b4" else eng.beam_step(lg)
        z.record()
        z.synchronize()
        res.setdefault(name, []).append(a.elapsed_time(z) / steps)
        print(json.dumps(dict(what="decode_step", mode=name, ms_per_step=round(res[name][-1], 4), rows=4)), flush=True)
    print(json.dumps(dict(what="decode_step", ratio_beam4_over_greedy_b4=round(res["beam4"][0] / res["greedy_b4"][0], 4))), flush=True)
    if args.processed:      # the processed loop sits between two plain ones
        plain = sum(res["beam4"]) / len(res["beam4"])
        print(json.dumps(dict(what="decode_step", processed_minus_plain_us=round((res["beam4_processed"][0] - plain) * 1e3, 1),
                              ratio_processed_over_plain=round(res["beam4_processed"][0] / plain, 4))), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
