"""Cost of teacher-forced scoring at the configs[1] decoder geometry (Qwen2-7B shape, vocabulary 152064, synthetic
weights), one sequence of S = 3584 and of S = 512 slots:
    python tools/bench_score.py [--repeats 5] [--out table.md]
Three forms, timed in alternating passes (a, b, c, a, b, c, ...; wall clock around a synchronised call, median over the repeats):
  (a) prefill with want_hidden -- what forward() runs without labels, plus the hidden rows
  (b) (a) + Engine.score_hidden -- the lm_head GEMM whose epilogue keeps (max, sum exp) partials, its finishing kernel, the loss reduction
  (c) (a) + the unfused form built from entries that existed before: omchat_lm_head into fp32 logits in chunks of --chunk rows, then
      omchat_op_token_logprob on every chunk
and, for scale, the lm_head GEMM alone through omchat_op_gemm with EPI_F32OUT at the same shape (it stores the 2.2 GB of logits that (b)
never does).  Prints one JSON line per S and a markdown table with the device memory each form adds."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--seqs", type=int, nargs="*", default=[3584, 512])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from omchat_amd import _lib
    from omchat_amd._lib import check, ptr, cur_stream
    from omchat_amd.config import omchat13b
    from omchat_amd.engine import Engine
    cfg = omchat13b()
    H, V = cfg.text["hidden_size"], cfg.text["vocab_size"]
    Smax = max(args.seqs)
    e = Engine(cfg, dtype="bf16", max_seq=Smax + 8, max_batch=1, max_tiles=1, max_prefill_rows=Smax, vision=False)
    e.fill_synthetic(seed=1)
    lib = e.lib
    g = torch.Generator().manual_seed(5)
    rows_out = []

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for S in args.seqs:
        emb = (torch.randn(1, S, H, generator=g) * 0.02).to(torch.bfloat16).cuda()
        labels = torch.randint(0, V, (1, S), generator=g)
        labels[:, ::9] = -100
        keep = {}

        def form_a():
            keep["h"] = e.prefill(emb, [S], want_hidden=True)[1]

        def form_b():
            form_a()
            keep["b"] = e.score_hidden(keep["h"], labels)

        chunk = min(args.chunk, S)
        logits = torch.empty(chunk, V, dtype=torch.float32, device="cuda")
        raw = torch.empty(S, dtype=torch.float32, device="cuda")
        proc = torch.empty(S, dtype=torch.float32, device="cuda")
        ids = labels.clamp_min(0).to(torch.int32).contiguous().view(-1)      # the op takes no ignore index: ignored rows score id 0

        def form_c():
            form_a()
            h = keep["h"].view(S, H)
            for r0 in range(0, S, chunk):
                n = min(chunk, S - r0)
                check(lib.omchat_lm_head(e.h, ptr(h[r0:r0 + n]), n, ptr(logits), cur_stream()))
                check(lib.omchat_op_token_logprob(ptr(logits), n, V, V, ptr(ids[r0:r0 + n]), None, 1.0, 1.0, None, None, None, None,
                                                  ptr(raw[r0:r0 + n]), ptr(proc[r0:r0 + n]), cur_stream()))

        full = torch.empty(S, V, dtype=torch.float32, device="cuda")
        w = torch.empty(V, H, dtype=torch.bfloat16, device="cuda").normal_(0, 0.02)

        def gemm_f32():
            check(lib.omchat_op_gemm(_lib.BF16, ptr(keep["h"]), H, ptr(w), H, ptr(full), V, S, V, H, None, None, None, 0, _lib.EPI_F32OUT, 0,
                                     cur_stream()))

        for fn in (form_a, form_b, form_c, gemm_f32):      # first calls: allocations, attributes
            fn()
        # the two forms agree on the scored rows (the unfused one reads GEMV logits: another summation order)
        lp = keep["b"][0].view(-1)
        m = labels.view(-1) != -100
        agree = float((lp[m.cuda()] - raw[m.cuda()]).abs().max())
        t = {"a": [], "b": [], "c": [], "gemm": []}
        for _ in range(args.repeats):
            t["a"].append(wall(form_a)); t["b"].append(wall(form_b)); t["c"].append(wall(form_c)); t["gemm"].append(wall(gemm_f32))
        med = {k: statistics.median(v) for k, v in t.items()}
        ws_b = lib.omchat_op_lse_label_ws(S, V) + S * 4 + (2 + 2) * 4
        ws_c = chunk * V * 4 + 2 * S * 4 + chunk * 64 * 16
        row = dict(S=S, a_ms=round(med["a"], 3), b_ms=round(med["b"], 3), c_ms=round(med["c"], 3), gemm_f32out_ms=round(med["gemm"], 3),
                   b_minus_a_ms=round(med["b"] - med["a"], 3), c_minus_a_ms=round(med["c"] - med["a"], 3),
                   spread_a_ms=[round(min(t["a"]), 3), round(max(t["a"]), 3)], spread_b_ms=[round(min(t["b"]), 3), round(max(t["b"]), 3)],
                   spread_c_ms=[round(min(t["c"]), 3), round(max(t["c"]), 3)], added_bytes_b=int(ws_b), added_bytes_c=int(ws_c),
                   full_logits_bytes=S * V * 4, max_abs_diff_b_vs_c=agree, chunk=chunk, repeats=args.repeats)
        print(json.dumps(row), flush=True)
        rows_out.append(row)
        del full, w, logits
    e.close()
    lines = ["| S | (a) prefill + hidden ms | (b) - (a) fused ms | (c) - (a) unfused ms | lm_head GEMM, fp32 logits stored ms | (b) adds MB | (c) adds MB | full logits MB |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows_out:
        lines.append(f"| {r['S']} | {r['a_ms']} | {r['b_minus_a_ms']} | {r['c_minus_a_ms']} | {r['gemm_f32out_ms']} | {r['added_bytes_b'] / 1e6:.1f} | "
                     f"{r['added_bytes_c'] / 1e6:.1f} | {r['full_logits_bytes'] / 1e6:.1f} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
