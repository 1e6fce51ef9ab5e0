"""Cost of continuing a KV cache:
    python tools/bench_extend.py [--iters 25] [--no-ttft]
One JSON line per measurement, synthetic weights, configs[1] geometry (omchat13b(): 28 q / 4 kv heads, 3 tiles, S = 3584):
  extend_attention  attention of Sq new rows at q_pos0 = keys - Sq over `keys` cached keys, bf16: the split-KV block attention + merge
                    (omchat_op_attn_extend) against the prefill kernel with q_pos0 (omchat_op_attn_prefill) on identical inputs, back to
                    back in one process; median and min .. max of --iters single launches timed with HIP events after warm-up, and the
                    form omchat_prefill_extend's rule picks (omchat_extend_attn_form);
  turn2_ttft        a follow-up turn on top of a 3 584-slot first turn: the whole path without reuse (tower + projector + splice + prefill of
                    all slots) against the reuse path (gather + omchat_prefill_extend of the suffix rows), suffixes of 16 / 64 / 256 / 1 024 rows."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--no-ttft", action="store_true")
    args = ap.parse_args()
    import torch
    from omchat_amd import _lib
    from omchat_amd._lib import check, ptr
    from omchat_amd.config import omchat13b
    from omchat_amd.engine import Engine

    def out(**kw):
        print(json.dumps(kw), flush=True)

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

    lib = _lib.lib()
    Hq, Hkv, scale = 28, 4, 1.0 / 128 ** 0.5
    for keys in (3600, 8192, 33000):
        k = torch.randn(1, Hkv, keys, 128, device="cuda", dtype=torch.bfloat16)
        v = torch.randn(1, Hkv, keys, 128, device="cuda", dtype=torch.bfloat16)
        for Sq in (16, 64, 256, 512, 1024, 4096):
            if Sq >= keys:
                continue
            L = keys - Sq
            q = torch.randn(Sq, Hq, 128, device="cuda", dtype=torch.bfloat16)
            o = torch.empty_like(q)
            wsb = lib.omchat_op_attn_extend_ws(Sq, Hq, Hkv, L)
            ws = torch.empty(wsb // 4 + 64, device="cuda", dtype=torch.float32)
            split = lambda: check(lib.omchat_op_attn_extend(_lib.BF16, ptr(q), ptr(k), ptr(v), ptr(o), Sq, Hq, Hkv, keys, L, scale, ptr(ws), wsb, None))
            pre = lambda: check(lib.omchat_op_attn_prefill(_lib.BF16, ptr(q), ptr(k), ptr(v), ptr(o), 1, Sq, keys, Hq, Hkv, None, 1, L, scale, None))
            # A, B, A, B: a drift of the clocks would show as a difference between the two passes of one form
            s1, p1, s2, p2 = (launches_us(f, args.iters) for f in (split, pre, split, pre))
            out(metric="extend_attention", Sq=Sq, keys=keys, split_us=round(min(s1[0], s2[0]), 2), prefill_us=round(min(p1[0], p2[0]), 2),
                split_passes=[round(s1[0], 2), round(s2[0], 2)], prefill_passes=[round(p1[0], 2), round(p2[0], 2)],
                split_range=[round(min(s1[1], s2[1]), 2), round(max(s1[2], s2[2]), 2)],
                prefill_range=[round(min(p1[1], p2[1]), 2), round(max(p1[2], p2[2]), 2)],
                rule_picks="split" if lib.omchat_extend_attn_form(Sq, L, Hkv) else "prefill", ws_mb=round(wsb / 2 ** 20, 1))
            del q, o, ws
        del k, v
    if args.no_ttft:
        return

    cfg = omchat13b()
    P, ntiles = 3584, 3
    e = Engine(cfg, dtype="bf16", max_seq=P + 1024 + 64, max_batch=1, max_tiles=ntiles)
    e.fill_synthetic(0)
    px = torch.randn(ntiles, 3, 448, 448, device="cuda", dtype=torch.bfloat16)
    g = torch.Generator().manual_seed(0)
    n_text = P - ntiles * e.ntok
    head = [-200] * ntiles + torch.randint(0, 150000, (n_text,), generator=g).tolist()
    for suffix in (16, 64, 256, 1024):
        ids = torch.tensor([head + torch.randint(0, 150000, (suffix,), generator=g).tolist()])

        def fresh():
            emb, lens, _ = e.splice(ids, None, e.encode_images(px))
            e.prefill(emb, lens)

        feats = e.encode_images(px)
        idx = e.splice_plan(ids, ntiles)

        def reuse():
            e.prefill_extend(e.gather_rows(idx[P:], feats), P)

        f = launches_us(fresh, 5, warm=2)
        r = launches_us(reuse, 5, warm=2)      # (the state left by `fresh` holds P + suffix slots: keep = P trims it)
        out(metric="turn2_ttft", first_turn_slots=P, suffix_rows=suffix, fresh_ms=round(f[0] / 1e3, 3), reuse_ms=round(r[0] / 1e3, 3),
            fresh_range_ms=[round(f[1] / 1e3, 3), round(f[2] / 1e3, 3)], reuse_range_ms=[round(r[1] / 1e3, 3), round(r[2] / 1e3, 3)],
            speedup=round(f[0] / r[0], 2), attn_form="split" if e.extend_attn_form(suffix, P) else "prefill")
    e.close()


if __name__ == "__main__":
    main()
