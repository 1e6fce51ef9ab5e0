"""Cost of shared-prefix batches, N suffixes over one prefilled prompt:
    python tools/bench_suffix.py [--N 4 8 16] [--suffix 32] [--passes 5] [--steps 32] [--iters 25] [--no-ttft] [--no-decode] [--no-attn]
One JSON line per measurement, synthetic bf16 weights, configs[1] decoder and tower (omchat8b_21()), one GPU; the prompt is 3 tiles + 512 ids
(3 584 cache slots), every suffix `--suffix` ids:
  suffix_attention  the suffix-pass attention alone over forked rows, bf16, 28 q / 4 kv heads: omchat_op_attn_suffix (one launch + merge)
                    against the batched prefill kernel with q_pos0 = P (omchat_op_attn_prefill) on identical inputs, A B A B in one process;
                    median and min .. max of --iters launches timed with HIP events after warm-up, and the form the rule picks
  ttft              time to the first token of all N rows: the new path (tower on 3 tiles + splice + prefill of the prompt + fork or share +
                    the suffix pass), forked and shared, against the same N concatenated prompts as a plain equal-length batch through the
                    existing prefill path (tower on 3 N tiles + splice + prefill of N x (P + S) rows); `passes` alternating passes, medians and
                    the spread (max - min) / median of each side
  decode_step       one decode step of the N rows after suffixes of DIFFERENT lengths (S / 4 .. S): forked rows, shared rows, and the plain
                    batch's rows (all at P + S); alternating passes of `steps` steps, medians and spreads as above"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--suffix", type=int, default=32)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--no-ttft", action="store_true")
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--no-attn", action="store_true")
    args = ap.parse_args()
    import torch
    from omchat_amd import _lib
    from omchat_amd._lib import check, ptr
    from omchat_amd.config import omchat8b_21
    from omchat_amd.engine import Engine

    def out(**kw):
        print(json.dumps(kw), flush=True)

    def timed(fn):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        z.record()
        z.synchronize()
        return a.elapsed_time(z)

    def launches_us(fn, iters, warm=5):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); z.record(); z.synchronize()
            ts.append(a.elapsed_time(z) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    def summary(ms):
        med = {k: statistics.median(v) for k, v in ms.items()}
        return med, {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}

    lib = _lib.lib()
    cfg = omchat8b_21()
    ntiles, S = 3, args.suffix
    Hq, Hkv, scale = cfg.text["num_attention_heads"], cfg.text["num_key_value_heads"], 1.0 / 128 ** 0.5
    Nmax = max(args.N)

    if not args.no_attn:
        P = ntiles * cfg.num_image_tokens + 512
        cap = P + S
        for N in args.N:
            k = torch.randn(N, Hkv, cap, 128, device="cuda", dtype=torch.bfloat16)
            v = torch.randn(N, Hkv, cap, 128, device="cuda", dtype=torch.bfloat16)
            k[1:, :, :P] = k[0, :, :P]; v[1:, :, :P] = v[0, :, :P]                  # forked rows: every row holds the prompt's bits
            q = torch.randn(N, S, Hq, 128, device="cuda", dtype=torch.bfloat16)
            o = torch.empty_like(q)
            lens = torch.full((N,), S, dtype=torch.int32)
            scratch = torch.zeros(N, dtype=torch.int32, device="cuda")
            kvl = torch.full((N,), cap, dtype=torch.int32, device="cuda")
            wsb = lib.omchat_op_attn_suffix_ws(N, S, Hq, Hkv, P)
            ws = torch.empty(wsb // 4 + 64, device="cuda", dtype=torch.float32)
            args_ = (_lib.BF16, ptr(q), ptr(k), ptr(v), ptr(o), N, S, Hq, Hkv, cap, P)
            check(lib.omchat_op_attn_suffix(*args_, ptr(lens), ptr(scratch), scale, ptr(ws), wsb, None))      # uploads the lengths once
            sfx = lambda: check(lib.omchat_op_attn_suffix(*args_, None, ptr(scratch), scale, ptr(ws), wsb, None))      # device lengths: no sync
            pre = lambda: check(lib.omchat_op_attn_prefill(_lib.BF16, ptr(q), ptr(k), ptr(v), ptr(o), N, S, cap, Hq, Hkv, ptr(kvl), 1, P, scale, None))
            s1, p1, s2, p2 = (launches_us(f, args.iters) for f in (sfx, pre, sfx, pre))
            out(metric="suffix_attention", N=N, S=S, P=P, suffix_us=round(min(s1[0], s2[0]), 2), prefill_us=round(min(p1[0], p2[0]), 2),
                suffix_passes=[round(s1[0], 2), round(s2[0], 2)], prefill_passes=[round(p1[0], 2), round(p2[0], 2)],
                suffix_range=[round(min(s1[1], s2[1]), 2), round(max(s1[2], s2[2]), 2)],
                prefill_range=[round(min(p1[1], p2[1]), 2), round(max(p1[2], p2[2]), 2)],
                rule_picks="suffix" if lib.omchat_suffix_attn_form(0, Hq // Hkv) else "prefill", ws_mb=round(wsb / 2 ** 20, 1))
            del k, v, q, o, ws
        torch.cuda.empty_cache()
    if args.no_ttft and args.no_decode:
        return

    P = ntiles * cfg.num_image_tokens + 512
    e = Engine(cfg, dtype="bf16", max_seq=P + S + args.steps + 8, max_batch=Nmax, max_tiles=min(24, ntiles * Nmax),
               max_prefill_rows=Nmax * (P + S))
    e.fill_synthetic(0)
    H = cfg.text["hidden_size"]
    px = torch.randn(ntiles, 3, cfg.vision["image_size"], cfg.vision["image_size"], device="cuda", dtype=torch.bfloat16)
    g = torch.Generator().manual_seed(0)
    head = [-200] * ntiles + torch.randint(0, 150000, (512,), generator=g).tolist()
    for N in args.N:
        sufs = [torch.randint(0, 150000, (S,), generator=g).tolist() for _ in range(N)]
        ids1 = torch.tensor([head])
        idsN = torch.tensor([head + s for s in sufs])
        pxN = px.repeat(N, 1, 1, 1)
        sidx = torch.tensor(sufs, dtype=torch.int32).view(-1)

        def new_path(share, lens=None):
            emb, l1, _ = e.splice(ids1, None, e.encode_images(px))
            e.prefill(emb, l1, want_logits=False)
            e.group_begin(1, N, l1[0], share=share)
            return e.prefill_suffixes(e.gather_rows(sidx, None).view(N, S, H), lens or [S] * N, l1[0])[0]

        def plain():
            emb, lN, _ = e.splice(idsN, None, e.encode_images(pxN))
            return e.prefill(emb, lN)[0]

        forms = dict(forked=lambda: new_path(False), shared=lambda: new_path(True), plain_batch=plain)
        if not args.no_ttft:
            ms = {k_: [] for k_ in forms}
            order = list(forms)
            for p in range(args.passes + 1):                  # pass 0 warms every form up
                for name in (order if p % 2 == 0 else order[::-1]):
                    t = timed(forms[name])
                    if p:
                        ms[name].append(t)
            med, spread = summary(ms)
            out(metric="ttft", N=N, P=P, S=S, passes=args.passes, **{f"{k_}_ms": round(med[k_], 3) for k_ in forms},
                **{f"{k_}_spread": round(spread[k_], 4) for k_ in forms},
                forked_over_plain=round(med["forked"] / med["plain_batch"], 4), shared_over_plain=round(med["shared"] / med["plain_batch"], 4))
        if not args.no_decode:
            ragged = [max(1, S // 4 + (j * (S - S // 4)) // max(1, N - 1)) for j in range(N)]      # S / 4 .. S
            ms = {k_: [] for k_ in forms}
            order = list(forms)

            def loop(tok0):
                tok = tok0
                for _ in range(args.steps):
                    tok, _ = e.decode_step(tok)

            for p in range(args.passes + 1):
                for name in (order if p % 2 == 0 else order[::-1]):
                    lg = plain() if name == "plain_batch" else new_path(name == "shared", ragged)
                    tok0 = e.argmax(lg)
                    t = timed(lambda: loop(tok0)) / args.steps
                    if p:
                        ms[name].append(t)
            med, spread = summary(ms)
            out(metric="decode_step", N=N, P=P, suffix_lengths=ragged, steps=args.steps, passes=args.passes,
                **{f"{k_}_ms": round(med[k_], 4) for k_ in forms}, **{f"{k_}_spread": round(spread[k_], 4) for k_ in forms},
                forked_over_plain=round(med["forked"] / med["plain_batch"], 4), shared_over_plain=round(med["shared"] / med["plain_batch"], 4),
                shared_over_forked=round(med["shared"] / med["forked"], 4))
        e.group_end()
    e.close()


if __name__ == "__main__":
    main()
