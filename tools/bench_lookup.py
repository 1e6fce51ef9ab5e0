"""Cost of prompt-lookup decoding:
    python tools/bench_lookup.py [--iters 50] [--ctx 3600] [--gen 64] [--no-e2e] [--sample]
One JSON line per measurement, at the configs[1] decoder geometry (Qwen2-7B shapes of omchat13b(), synthetic weights, text-only context of
--ctx slots), after warm-up (the packed weight replica is built by the first verify step, before any timing):
  verify_step      one omchat_decode_verify of T = 2..16 tokens (drafts rejected at once: the cache grows by one slot per call) against one
                   batch-1 omchat_decode_step; both timed per call with the host synchronised (a verify step always synchronises);
  verify_attention the multi-query attention launch + merge (omchat_op_attn_verify, T = 8) against the single-token one
                   (omchat_op_attn_decode, b = 1) at 3.6 k and 33 k keys, 28 q / 4 kv heads;
  e2e_forced       generate() tokens/s with drafts supplied by a hook from the recorded greedy chain, the first wrong token placed so that
                   0 / 25 / 50 / 75 / 100 % of the drafted tokens are accepted, against plain greedy generate();
  e2e_no_match     generate(prompt_lookup_num_tokens=10) with a drafter that never matches, against plain greedy generate().
--sample measures the sampled form instead ("Sampling"; temperature 0.8, top_k = 50, top_p = 0.9):
  verify_step_sampled  one sampled verify step (Engine.decode_verify(sample=True)) of T = 2 / 8 / 16 tokens against the greedy verify step of
                       the same build and T, drafts rejected at once;
  e2e_sampled_forced   generate(do_sample=True, prompt_lookup_sample=True) tokens/s with drafts forced from the recorded sampled chain at
                       0 / 25 / 50 / 75 / 100 % acceptance, against plain sampled generate() with the same seed."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--ctx", type=int, default=3600)
    ap.add_argument("--gen", type=int, default=64)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--sample", action="store_true")
    args = ap.parse_args()
    import torch
    from omchat_amd import _lib
    from omchat_amd._lib import check, ptr
    from omchat_amd.config import omchat13b
    from omchat_amd.engine import Engine
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM

    def out(**kw):
        print(json.dumps(kw), flush=True)

    def events_us(fn, iters):
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

    # ---- attention launch: multi-query (T = 8) against single-token
    lib = _lib.lib()
    Hq, Hkv, scale = 28, 4, 1.0 / 128 ** 0.5
    if not args.sample:
        for L in (3600, 33000):
            cap = L + 16
            q = torch.randn(16, Hq, 128, device="cuda", dtype=torch.bfloat16)
            k = torch.randn(Hkv, cap, 128, device="cuda", dtype=torch.bfloat16)
            v = torch.randn(Hkv, cap, 128, device="cuda", dtype=torch.bfloat16)
            o = torch.empty(16, Hq, 128, device="cuda", dtype=torch.bfloat16)
            wsb = lib.omchat_op_attn_decode_ws(16, Hq, cap)
            ws = torch.empty(wsb // 4 + 64, device="cuda", dtype=torch.float32)
            one = events_us(lambda: check(lib.omchat_op_attn_decode(_lib.BF16, ptr(q), ptr(k), ptr(v), ptr(o), 1, Hq, Hkv, cap, L + 1, None, scale,
                                                                    ptr(ws), wsb, None)), args.iters * 4)
            for T in (2, 4, 8, 16):
                t = events_us(lambda: check(lib.omchat_op_attn_verify(_lib.BF16, ptr(q), ptr(k), ptr(v), ptr(o), T, Hq, Hkv, cap, L + 1 - T, scale,
                                                                      ptr(ws), wsb, None)), args.iters * 4)
                out(metric="verify_attention", keys=L + 1, T=T, us=round(t, 2), single_token_us=round(one, 2), ratio=round(t / one, 3),
                    target_T8="<= 1.5")
            del q, k, v, o, ws

    # ---- decoder: verify step against batch-1 decode step
    cfg = omchat13b()
    S = args.ctx
    e = Engine(cfg, dtype="bf16", max_seq=S + 16 * (args.iters + 10) + 4 * args.gen + 64, max_batch=1, max_tiles=1, max_prefill_rows=S + 8,
               vision=False)
    e.fill_synthetic(0)
    m = OmChatQwen2ForCausalLM(cfg.clone(), e)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, cfg.text["vocab_size"], (1, S), generator=g)
    m.forward(input_ids=ids, use_cache=True)
    bad = [151000] * 15                       # drafts that are rejected at once: n = 0, the cache grows by one slot per verify step
    e.decode_verify([1] + bad[:1])            # first verify step: builds the packed replica (outside any timing)
    torch.cuda.synchronize()

    def per_call_ms(fn, iters):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    if args.sample:
        sample_part(args, e, m, ids, S, bad, per_call_ms, out)
        e.close()
        return
    tok1 = torch.tensor([1], dtype=torch.int32, device="cuda")

    def plain():
        nxt, _ = e.decode_step(tok1)
        int(nxt[0])                            # host sync, as the verify step has
    base = per_call_ms(plain, args.iters)
    out(metric="decode_step_b1", ctx=S, ms=round(base, 3))
    for T in range(2, 17):
        toks = [1] + bad[:T - 1]
        t = per_call_ms(lambda: e.decode_verify(toks), args.iters)
        out(metric="verify_step", ctx=S, T=T, ms=round(t, 3), decode_step_ms=round(base, 3), ratio=round(t / base, 3), target_T8="<= 1.3")
    if args.no_e2e:
        return

    # ---- end to end
    ids = ids[:, :S]
    def gen_time(**kw):
        m.generate(ids, max_new_tokens=args.gen, **kw)      # warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = m.generate(ids, max_new_tokens=args.gen, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    tg, greedy = gen_time()
    out(metric="e2e_greedy", ctx=S, gen=args.gen, tok_s=round(args.gen / tg, 1))
    k = 8
    # the chain the verify rows themselves pick: a verify row and a batch-1 step may differ in the last bits, and synthetic weights leave
    # near-ties in the greedy chain, so the forced drafts follow the prompt-lookup run's own ids (fixed point of "draft = last run's ids")
    chain = greedy[0, S:].tolist()
    for _ in range(4):
        m._lookup_draft_hook = lambda cur, budget: list(chain[len(cur) - S:len(cur) - S + budget])
        r = m.generate(ids, max_new_tokens=args.gen, prompt_lookup_num_tokens=k)[0, S:].tolist()
        if r == chain:
            break
        chain = r
    diff = next((i for i in range(args.gen) if chain[i] != int(greedy[0, S + i])), None)
    out(metric="e2e_lookup_chain", first_diff_vs_greedy=diff, fixed_point=r == chain)
    for acc in (0.0, 0.25, 0.5, 0.75, 1.0):
        j = int(round(acc * k))

        def hook(cur, budget, j=j):
            pos = len(cur) - S
            d = list(chain[pos:pos + budget])
            if j < len(d):
                d[j] = (d[j] + 1) % 151000
            return d
        m._lookup_draft_hook = hook
        e.lookup_stats(reset=True)
        t, r = gen_time(prompt_lookup_num_tokens=k)
        st = e.lookup_stats()
        out(metric="e2e_forced", ctx=S, gen=args.gen, k=k, target_acceptance=acc,
            acceptance=round(st["accepted"] / max(1, st["drafted"]), 3), verify_steps=st["verify_steps"], tok_s=round(args.gen / t, 1),
            speedup=round(tg / t, 3), same_ids_as_lookup_chain=r[0, S:].tolist() == chain)
    m._lookup_draft_hook = lambda cur, budget: []
    t, r = gen_time(prompt_lookup_num_tokens=10)
    m._lookup_draft_hook = None
    out(metric="e2e_no_match", ctx=S, gen=args.gen, tok_s=round(args.gen / t, 1), ratio=round(tg / t, 3), target=">= 0.97",
        same_ids=bool(torch.equal(r, greedy)))
    e.close()


def sample_part(args, e, m, ids, S, bad, per_call_ms, out):
    import torch
    P = dict(temperature=0.8, top_k=50, top_p=0.9)
    seed = 7
    # ---- sampled verify step against the greedy verify step (both reject their drafts at once: one slot and one committed pick per call)
    for T in (2, 8, 16):
        toks = [1] + bad[:T - 1]
        e.sampling_off()
        tg = per_call_ms(lambda: e.decode_verify(toks), args.iters)
        e.set_sampling(1, seed=seed, seen=[[]], **P)
        ts = per_call_ms(lambda: e.decode_verify(toks, sample=True), args.iters)
        out(metric="verify_step_sampled", ctx=S, T=T, ms=round(ts, 3), greedy_verify_ms=round(tg, 3), extra_us=round((ts - tg) * 1e3, 1),
            ratio=round(ts / tg, 3))
    e.sampling_off()
    if args.no_e2e:
        return

    # ---- end to end against plain sampled generate()
    def gen_time(**kw):
        m.generate(ids, max_new_tokens=args.gen, do_sample=True, seed=seed, **P, **kw)      # warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = m.generate(ids, max_new_tokens=args.gen, do_sample=True, seed=seed, **P, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    tp_, plain = gen_time()
    out(metric="e2e_sampled", ctx=S, gen=args.gen, tok_s=round(args.gen / tp_, 1))
    k = 8
    lk = dict(prompt_lookup_num_tokens=k, prompt_lookup_sample=True)
    # forced drafts follow the lookup run's own ids (a verify row and a batch-1 step can differ in the last bits: the fixed point of
    # "draft = last run's ids", as in the greedy part)
    chain = plain[0, S:].tolist()
    for _ in range(4):
        m._lookup_draft_hook = lambda cur, budget: list(chain[len(cur) - S:len(cur) - S + budget])
        r = m.generate(ids, max_new_tokens=args.gen, do_sample=True, seed=seed, **P, **lk)[0, S:].tolist()
        if r == chain:
            break
        chain = r
    diff = next((i for i in range(args.gen) if chain[i] != int(plain[0, S + i])), None)
    out(metric="e2e_sampled_lookup_chain", first_diff_vs_plain_sampled=diff, fixed_point=r == chain)
    for acc in (0.0, 0.25, 0.5, 0.75, 1.0):
        j = int(round(acc * k))

        def hook(cur, budget, j=j):
            pos = len(cur) - S
            d = list(chain[pos:pos + budget])
            if j < len(d):
                d[j] = (d[j] + 1) % 151000
            return d
        m._lookup_draft_hook = hook
        e.lookup_stats(reset=True)
        t, r = gen_time(**lk)
        st = e.lookup_stats()
        out(metric="e2e_sampled_forced", ctx=S, gen=args.gen, k=k, target_acceptance=acc,
            acceptance=round(st["accepted"] / max(1, st["drafted"]), 3), verify_steps=st["verify_steps"], tok_s=round(args.gen / t, 1),
            speedup=round(tp_ / t, 3), same_ids_as_lookup_chain=r[0, S:].tolist() == chain)
    m._lookup_draft_hook = None


if __name__ == "__main__":
    main()
