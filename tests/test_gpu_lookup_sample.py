"""GPU: prompt-lookup decoding with do_sample=True ("Sampling").  The sampler's verify form against
tests/lookup_sample_ref.py bit for bit; the sampled verify step against that reference on its own logits, with its commit and its rewind;
sampled verify steps reproducing a plain sampled chain; generate(prompt_lookup_sample=True) against plain sampled generate() on tiny models
(decode graph, streamer / stopping criterion, EOS, MXFP4 mode 2); TP 2 / 4 rank contexts on one device; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import lookup_sample_ref as lsr
import sampling_ref as sr
import sampling_ref2 as sr2
from gpu_util import sync
from omchat_amd import _lib, synth
from omchat_amd._lib import check, ptr
from omchat_amd.config import tiny
from omchat_amd.engine import Engine
from test_gpu_lookup import BOUND, PROMPT, _tiny_model

ALL4 = dict(min_p=0.02, typical_p=0.6, epsilon_cutoff=1e-3, eta_cutoff=3e-3)
OP_SETS = {
    "T": dict(temperature=0.8),
    "T-k-p": dict(temperature=0.8, top_k=20, top_p=0.9),
    "penalty": dict(temperature=0.8, top_k=20, top_p=0.9, repetition_penalty=1.3),
    "all4": dict(temperature=0.7, top_k=50, top_p=0.9, repetition_penalty=1.3, **ALL4),
}
GEN_SETS = {
    "T": dict(temperature=0.8),
    "T-k-p": dict(temperature=0.8, top_k=20, top_p=0.9),
    "penalty": dict(temperature=0.8, top_k=20, top_p=0.9, repetition_penalty=1.3),
}


# ---------------------------------------------------------------------------------------------------------------- op level
def _c_filters(kw):
    cut = lambda v: 1.0 if v is None or not 0.0 < v < 1.0 else float(v)
    return (-1.0 if kw.get("min_p") is None else float(kw["min_p"]), cut(kw.get("typical_p")), cut(kw.get("epsilon_cutoff")),
            cut(kw.get("eta_cutoff")))


def _op_verify(lib, logits, tokens, seed, step0, params, seen, rank, V_total):
    """omchat_op_sample_verify -> (ids, lo, hi)"""
    T, V = logits.shape
    temp, pen, kw = lsr.split_params(params)
    dev = torch.from_numpy(logits).cuda()
    tk = torch.tensor(tokens, dtype=torch.int32, device="cuda")
    out = torch.empty(T, dtype=torch.int32, device="cuda")
    lo = torch.zeros(T, dtype=torch.int32, device="cuda")
    hi = torch.zeros(T, dtype=torch.int32, device="cuda")
    flat = torch.tensor(list(seen) or [0], dtype=torch.int32)
    check(lib.omchat_op_sample_verify(ptr(dev), T, V, V, ptr(tk), seed, step0, temp, kw["top_k"], kw["top_p"], pen, *_c_filters(kw), ptr(flat),
                                      len(seen), rank, V_total, ptr(out), ptr(lo), ptr(hi), _lib.cur_stream()))
    torch.cuda.synchronize()
    u = lambda t: t.cpu().numpy().view(np.uint32).astype(np.int64)
    return out.cpu().numpy().astype(np.int64), u(lo), u(hi)


_ROWS = {}


def _rows(V):
    """16 tie-free rows of seeded normal logits (built as tests/test_sampling2_cpu.py builds its rows)"""
    if V not in _ROWS:
        rng = np.random.default_rng(V)
        rows = []
        for _ in range(16):
            x = rng.permutation(np.unique((rng.standard_normal(V + V // 8) * 3.0).astype(np.float32)))[:V]
            assert len(np.unique(x)) == V
            rows.append(x)
        _ROWS[V] = np.stack(rows)
    return _ROWS[V]


MARGIN = 1e-4      # as tests/test_sampling2_cpu.py: no value within this relative distance of a threshold (other than the value that sets it)


def _check_margin(logits, tokens, base, params, gbase, V_total, los, his):
    """the rows keep their distance from both ends of the kept interval, so that the comparison does not hang on a last-bit decision"""
    temp, pen, _ = lsr.split_params(params)
    V = logits.shape[1]
    for j in range(logits.shape[0]):
        seen = lsr.local_seen(list(base) + [int(t) for t in tokens[1:j + 1]], gbase, V, V_total)
        x = sr.processed(logits[j], temp, seen, pen).astype(np.float64)
        for key in (int(los[j]), int(his[j])):
            if key in (0, sr2.TOP):
                continue
            thr = float(sr.unkey(key))
            others = x[x != thr]
            gap = float((np.abs(others - thr) / abs(thr)).min())
            assert gap > MARGIN, f"row {j}: a value sits within {gap:.2e} (relative) of the interval end {thr}"


def _op_tokens(T, gbase, V, V_total):
    """the last emitted id and T - 1 drafts: ids on both sides of 32-bit word boundaries of the slice's bitmap and of the slice's two ends, an id
    twice, and (T = 16) ids outside the vocabulary"""
    d = [gbase + 31, gbase + 32, gbase, gbase + V - 1, gbase + 63, gbase + 64, gbase + 31, gbase + V - 33, gbase + V - 32, gbase - 1, gbase + V,
         -200, V_total, gbase + 95, gbase + 96]
    return [gbase + 7] + d[:T - 1]


@pytest.mark.parametrize("T", [2, 5, 16])
@pytest.mark.parametrize("shard", ["V320", "V152064-rank3"])
@pytest.mark.parametrize("name", sorted(OP_SETS))
def test_op_sample_verify_equals_ref(gpu_lib, name, shard, T):
    V, rank, V_total = (320, 0, 320) if shard == "V320" else (19008, 3, 152064)
    gbase = rank * V
    params = OP_SETS[name]
    tokens = _op_tokens(T, gbase, V, V_total)
    logits = _rows(V)[:T].copy()
    # the drafts and the base seen ids are candidates: a missing or a stray seen bit changes the kept interval, not only a far tail value
    base = [gbase + 3, gbase + 40, gbase + V - 2, gbase - 5, gbase + V + 5, -200, V_total + 1, (gbase + V_total // 2) % V_total]
    for i in set(tokens + base):
        if 0 <= i - gbase < V:
            logits[:, i - gbase] = np.abs(logits[:, i - gbase]) + np.float32(4.0) + np.float32(0.001) * (i - gbase)
    assert all(len(np.unique(r)) == V for r in logits)
    for seed, step0 in ((11, 0), (12345678901, 7)):
        ids, lo, hi = _op_verify(gpu_lib, logits, tokens, seed, step0, params, base, rank, V_total)
        want, wlo, whi = lsr.verify_sample_ref(logits, tokens, seed, step0, base, params, gbase, V_total, want_interval=True)
        assert np.array_equal(ids, want), (seed, ids, want)
        assert np.array_equal(lo, wlo) and np.array_equal(hi, whi), (lo, wlo, hi, whi)
        _check_margin(logits, tokens, base, params, gbase, V_total, wlo, whi)
    if "repetition_penalty" in params and T > 2:
        # the rows' seen sets differ: without the drafts in them at least one row's interval or id is another
        w0 = lsr.verify_sample_ref(logits, [tokens[0]] * T, seed, step0, base, params, gbase, V_total, want_interval=True)
        assert not all(np.array_equal(a, b) for a, b in zip((want, wlo, whi), w0))


# ---------------------------------------------------------------------------------------------------------------- verify step
PEN = dict(temperature=0.8, top_k=20, top_p=0.9, repetition_penalty=1.3)
SEED = 4242


def _begin(e, m, ids, seed, p):
    """prefill, sampler on with the prompt as the seen set, first pick -> (id, the logits it was drawn from)"""
    out = m.forward(input_ids=ids, use_cache=True)
    e.set_sampling(1, seed=seed, seen=[[int(i) for i in ids[0].tolist() if int(i) >= 0]], **p)
    lg = out.local_logits
    return int(e.sample(lg)[0]), lg[0].float().cpu().numpy()


def _sampled_chain(e, m, ids, n, seed, p):
    """n plain sampled picks and, per pick, the single-step logits it was drawn from (pick i at step i)"""
    tok, lg = _begin(e, m, ids, seed, p)
    chain, rows = [tok], [lg]
    for _ in range(n - 1):
        nxt, l2 = e.decode_step(torch.tensor([chain[-1]]), want_logits=True)
        chain.append(int(nxt[0])); rows.append(l2[0].float().cpu().numpy())
    return chain, rows


def _row_pick(lg, step, seed, seen, p):
    temp, pen, kw = lsr.split_params(p)
    return sr2.sample_row(lg, 0, step, seed, temp, sorted(set(seen)), pen, **kw)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("q,kv", [(7, 1), (4, 2)])
@pytest.mark.parametrize("T", [2, 5, 16])
def test_verify_step_equals_ref_on_its_own_logits(gpu_lib, dt, q, kv, T):
    _, e, m = _tiny_model(q, kv, dt=dt)
    ids = torch.tensor([PROMPT])
    chain, _ = _sampled_chain(e, m, ids, T + 1, SEED, PEN)
    # the draft = the plain chain, corrupted in the middle by an id that nothing has seen
    c = (T - 1) // 2
    bogus = next(i for i in range(300, 0, -1) if i not in PROMPT and i not in chain)
    toks = list(chain[:T])
    if T > 2:
        toks[1 + c] = bogus

    def step():
        tok, _ = _begin(e, m, ids, SEED, PEN)
        assert tok == chain[0]
        L = e.kv_lengths(1)[0]
        s, base = e.sampling_state()
        assert s == 1 and base == sorted(set(PROMPT + [tok]))
        picks, n, lg = e.decode_verify(toks, want_logits=True, sample=True)
        return L, base, picks.tolist(), n, lg.float().cpu().numpy()

    L, base, picks, n, lg = step()
    want = lsr.verify_sample_ref(lg, toks, SEED, 1, base, PEN).tolist()
    assert picks == want, (picks, want)
    lead = 0
    while lead < T - 1 and toks[lead + 1] == picks[lead]:
        lead += 1
    assert n == lead
    if T > 2 and picks[c] != bogus:
        assert n <= c
    assert e.kv_lengths(1)[0] == L + 1 + n
    emitted = picks[:n + 1]
    state = (1 + n + 1, sorted(set(base + emitted)))
    assert e.sampling_state() == state
    if T > 2 and bogus not in emitted:
        assert bogus not in e.sampling_state()[1]            # a rejected draft leaves no trace
    print(f"\n{dt} {q}q/{kv}kv T={T}: n = {n}")
    # three plain steps go on from the committed state
    seen, tok = list(state[1]), emitted[-1]
    for k in range(3):
        nxt, l1 = e.decode_step(torch.tensor([tok]), want_logits=True)
        ref = _row_pick(l1[0].float().cpu().numpy(), state[0] + k, SEED, seen, PEN)
        assert int(nxt[0]) == ref, (k, int(nxt[0]), ref)
        seen.append(ref); tok = ref
    assert e.sampling_state() == (state[0] + 3, sorted(set(seen)))
    # the rewind of r of the committed picks: counter, seen set and slots
    for r in range(1, n + 2):
        L2, base2, picks2, n2, _ = step()
        assert (L2, base2, picks2, n2) == (L, base, picks, n)
        e.kv_rewind(1, r)
        assert e.sampling_state() == (1 + n + 1 - r, sorted(set(base + emitted[:n + 1 - r]))), r
        assert e.kv_lengths(1)[0] == L + 1 + n - r
    e.close()


# seeds (model, sampler) for which no position of the chain is left out on the MI355X
CHAIN_SEEDS = {"bf16": (21, 4242), "f16": (21, 4242)}


def _chain_left_out(dt, mseed, sseed):
    """a 40-token plain sampled chain, then sampled verify steps with corrupted drafts and plain steps over the same prompt: everything is
    asserted here; -> how many of the 40 positions were left out (0 or 1)"""
    _, e, m = _tiny_model(seed=mseed, dt=dt)
    ids = torch.tensor([PROMPT])
    N = 40
    chain, rows = _sampled_chain(e, m, ids, N, sseed, PEN)
    P = len(PROMPT)
    left_out = 0

    def same_or_flip(pick, pos, lg_verify):
        """True: the pick is the chain's.  False: it differs and the reference itself flips between the two logit rows (left out)"""
        if pick == chain[pos]:
            return True
        seen = PROMPT + chain[:pos]
        a, b = _row_pick(lg_verify, pos, sseed, seen, PEN), _row_pick(rows[pos], pos, sseed, seen, PEN)
        assert a == pick and b == chain[pos] and a != b, (pos, pick, chain[pos], a, b)
        return False

    tok, _ = _begin(e, m, ids, sseed, PEN)
    got = [tok]
    assert got == chain[:1]
    ok = True
    for ln, j in ((7, None), (6, 2), (6, 0), (6, 5), (6, 3)):
        L = len(got)
        draft = list(chain[L:L + ln])
        if j is not None:
            draft[j] = (draft[j] + 7) % 320
        picks, n, lg = e.decode_verify([got[-1]] + draft, want_logits=True, sample=True)
        picks, lg = picks.tolist(), lg.float().cpu().numpy()
        upto = ln if j is None else j
        for i in range(upto + 1):
            ok = same_or_flip(picks[i], L + i, lg[i])
            if not ok:
                break
        if not ok:
            break
        assert n == upto and picks[:n + 1] == chain[L:L + n + 1]
        got += picks[:n + 1]
        assert e.kv_lengths(1)[0] == P + len(got) - 1
        assert e.sampling_state() == (len(got), sorted(set(PROMPT + got)))
    while ok and len(got) < N:
        nxt, _ = e.decode_step(torch.tensor([got[-1]]))
        got.append(int(nxt[0]))
    left_out = 0 if ok else 1
    if ok:
        assert got == chain
    e.close()
    return left_out


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_sampled_verify_steps_reproduce_the_plain_chain(gpu_lib, dt):
    left_out = _chain_left_out(dt, *CHAIN_SEEDS[dt])
    print(f"\n{dt}: {left_out} of 40 positions left out (a pick that the reference flips between verify-row and single-step logits)")
    assert left_out <= 1


# ---------------------------------------------------------------------------------------------------------------- generate
def _explained(e, m, ids, base, got, dt, seed, p):
    """the first differing position, judged on the single-step logits: a near-tie of the race or a logit next to an end of the kept interval"""
    P = ids.shape[1]
    j = next(i for i in range(min(base.shape[1], got.shape[1])) if base[0, i] != got[0, i])
    e.sampling_off()
    out = m.forward(input_ids=ids, use_cache=True)
    lg = out.local_logits[0]
    for t in base[0, P:j].tolist():
        _, l2 = e.decode_step(torch.tensor([t]), want_logits=True)
        lg = l2[0]
    # the parameters generate() resolved: what the call leaves open comes from generation_config (top_k = 50, as in HF)
    eff = m._sampling_params(p.get("temperature"), p.get("top_k"), p.get("top_p"), p.get("repetition_penalty"), seed, None, {})
    eff.pop("seed")
    temp, pen, kw = lsr.split_params(eff)
    seen = sorted(set(i for i in base[0, :j].tolist() if i >= 0))
    x = sr.processed(lg.float().cpu().numpy(), temp, seen, pen)
    lo, hi = sr2.interval(x, **kw)
    k = sr.key(x).astype(np.int64)
    keep = (k >= lo) & (k <= hi)
    g = np.sort((x + sr.noise(sr.row_key(seed, 0, j - P), np.arange(x.shape[0]))).astype(np.float32)[keep])
    gap = float(g[-1] - g[-2]) if g.shape[0] > 1 else float("inf")
    eps = 2 * BOUND[dt] / temp
    ends = [float(sr.unkey(lo))] + ([float(sr.unkey(hi))] if hi != sr2.TOP else [])
    edge = min(float(np.abs(x[~keep].astype(np.float64) - v).min()) if (~keep).any() else float("inf") for v in ends)
    assert gap < eps or edge < eps, (j, gap, edge, eps)
    return f"explained at {j} (race gap {gap:.3e}, distance to an interval end {edge:.3e}, bound {eps:.3e})"


def _pair(m, ids, k, seed, p, **kw):
    e = m.engine
    base = m.generate(ids, do_sample=True, seed=seed, **p, **kw)
    st0 = e.sampling_state()
    e.lookup_stats(reset=True)
    got = m.generate(ids, do_sample=True, seed=seed, prompt_lookup_num_tokens=k, prompt_lookup_sample=True, **p, **kw)
    return base, got, e.lookup_stats(), st0, e.sampling_state()


# sampler seeds per parameter set for which every k gives equal ids and accepted drafts on the MI355X (model seed 5)
GEN_SEEDS = {"T": 1, "T-k-p": 4, "penalty": 3}


@pytest.mark.parametrize("k", [1, 4, 10])
@pytest.mark.parametrize("name", sorted(GEN_SETS))
def test_generate_lookup_sample_equals_sampled_generate(gpu_lib, name, k):
    _, e, m = _tiny_model(seed=5)
    ids = torch.tensor([PROMPT])
    p, seed = GEN_SETS[name], GEN_SEEDS[name]
    base, got, st, s0, s1 = _pair(m, ids, k, seed, p, max_new_tokens=60)
    if torch.equal(base, got):
        case = "equal"
        assert s0 == s1                       # the sampler's state is left as the plain loop leaves it
    else:
        case = _explained(e, m, ids, base, got, "bf16", seed, p)
    print(f"\n{name} k={k}: {case}; {st}")
    assert st["verify_steps"] > 0 and st["accepted"] > 0
    e.close()


# a peaked parameter set (the tiny synthetic model then repeats itself more often) and the sampler seed for which the MXFP4 case gives equal
# ids and accepted drafts on the MI355X
PEAKED, PEAKED_SEED = dict(temperature=0.4, top_k=20, top_p=0.9), 3


def _logged_lookup(m, ids, **kw):
    """generate() with the verify steps and rewinds of its lookup loop logged: -> (ids, [(emitted before the step, n)], [rewound picks])"""
    e = m.engine
    steps, rewinds, emitted = [], [], [1]
    verify, step, rewind = e.decode_verify, e.decode_step, e.kv_rewind

    def dv(tokens, **k2):
        picks, n = verify(tokens, **k2)
        steps.append((emitted[0], n)); emitted[0] += n + 1
        return picks, n

    def ds(tokens, **k2):
        emitted[0] += 1
        return step(tokens, **k2)

    def rw(b, n=1):
        rewinds.append(n)
        return rewind(b, n)
    e.decode_verify, e.decode_step, e.kv_rewind = dv, ds, rw
    try:
        out = m.generate(ids, **kw)
    finally:
        del e.decode_verify, e.decode_step, e.kv_rewind
    return out, steps, rewinds


def test_generate_lookup_sample_graph_streamer_stopping_eos(gpu_lib):
    _, e, m = _tiny_model(seed=5)
    ids = torch.tensor([PROMPT])
    p, seed = GEN_SETS["penalty"], GEN_SEEDS["penalty"]
    kw = dict(do_sample=True, seed=seed, max_new_tokens=60, **p)
    lk = dict(prompt_lookup_sample=True)
    base = m.generate(ids, **kw)
    e.enable_decode_graph(True)
    e.lookup_stats(reset=True)
    g = m.generate(ids, prompt_lookup_num_tokens=4, **lk, **kw)
    assert e.decode_graph_stats()["replays"] > 0 and e.lookup_stats()["accepted"] > 0
    e.enable_decode_graph(False)
    case = "equal" if torch.equal(g, base) else _explained(e, m, ids, base, g, "bf16", seed, p)
    print(f"\ndecode graph: {case}")

    class S:
        def __init__(self):
            self.got = []
        def put(self, t):
            self.got.extend(int(x) for x in t.view(-1))
        def end(self):
            self.got.append("end")

    # Long accepted runs for the two stops below: the drafts come from the recorded plain chain (the loop's draft hook), so every verify step
    # accepts what it is given, the id of the stop included (the prompt-lookup drafter itself cuts its drafts before an EOS id).  The stop
    # sits inside an accepted run (an emitted pick of a verify step with accepted drafts behind it), at an id that occurs there first.
    P = ids.shape[1]
    chain = base[0, P:].tolist()
    m._lookup_draft_hook = lambda cur, budget: list(chain[len(cur) - P:len(cur) - P + budget])
    full, steps, _ = _logged_lookup(m, ids, prompt_lookup_num_tokens=10, **lk, **kw)
    new = full[0, P:].tolist()
    at = next((pos + i for pos, n in steps for i in range(n) if new.index(new[pos + i]) == pos + i), None)
    assert at is not None, (steps, new)
    # a stopping criterion there, with a streamer
    crit = lambda ids_, s: ids_.shape[1] >= P + at + 1
    s1, s2 = S(), S()
    a = m.generate(ids, streamer=s1, stopping_criteria=[crit], **kw)
    st_a = e.sampling_state()
    b, _, rewinds = _logged_lookup(m, ids, streamer=s2, stopping_criteria=[crit], prompt_lookup_num_tokens=10, **lk, **kw)
    if torch.equal(a, b):
        assert s1.got == s2.got and e.sampling_state() == st_a and b.shape[1] == P + at + 1
        assert e.kv_lengths(1)[0] == b.shape[1] - 1
        print(f"streamer / stopping criterion at {at}: equal; rewinds {rewinds}")
    else:
        print(f"streamer / stopping criterion at {at}:", _explained(e, m, ids, a, b, "bf16", seed, p))
    # an EOS there, kept in the output; sampler state and cache as the plain loop leaves them
    eos = new[at]
    a = m.generate(ids, eos_token_id=eos, **kw)
    st_a = e.sampling_state()
    b, _, rewinds = _logged_lookup(m, ids, eos_token_id=eos, prompt_lookup_num_tokens=10, **lk, **kw)
    if torch.equal(a, b):
        assert int(b[0, -1]) == eos and e.sampling_state() == st_a
        assert e.kv_lengths(1)[0] == b.shape[1] - 1
        assert torch.equal(b, full[:, :b.shape[1]]) and rewinds and max(rewinds) >= 1      # the stop fell inside the accepted run
        print(f"EOS at {at}: equal; rewinds {rewinds}")
    else:
        print(f"EOS at {at}:", _explained(e, m, ids, a, b, "bf16", seed, p))
    m._lookup_draft_hook = None
    e.close()


def test_generate_lookup_sample_in_mxfp4_mode_2(gpu_lib):
    _, e, m = _tiny_model(seed=5)
    m.enable_mxfp4_decode(True, batched=True)
    ids = torch.tensor([PROMPT])
    p, seed = PEAKED, PEAKED_SEED
    base, got, st, s0, s1 = _pair(m, ids, 4, seed, p, max_new_tokens=60)
    case = "equal" if torch.equal(base, got) else _explained(e, m, ids, base, got, "bf16", seed, p)
    if case == "equal":
        assert s0 == s1 and e.kv_lengths(1)[0] == got.shape[1] - 1
    print(f"\nMXFP4 mode 2: {case}; {st}")
    assert st["verify_steps"] > 0 and st["accepted"] > 0
    e.close()


# ---------------------------------------------------------------------------------------------------------------- tensor parallelism
@pytest.mark.parametrize("tp", [2, 4])
def test_tp_sampled_verify_equals_ref(gpu_lib, tp):
    from test_gpu_tp_single import Group, _run_ranks
    cfg = tiny(q_heads=4, kv_heads=2)
    sd = synth.state_dict(cfg, 13)
    ids = torch.tensor([PROMPT])
    plan = [(3, None), (7, 4), (15, 9), (5, 0)]

    def begin(e):
        embeds, lengths, _ = e.splice(ids, None, None)
        logits, _ = e.prefill(embeds, lengths)
        e.set_sampling(1, seed=SEED, seen=[PROMPT], **PEN)
        return int(e.sample(logits)[0])

    def drive(e, chain):
        got = [begin(e)]
        res = []
        for ln, j in plan:
            d = list(chain[len(got):len(got) + ln])
            if j is not None:
                d[j] = (d[j] + 1) % 320
            toks = [got[-1]] + d
            s0, seen0 = e.sampling_state()
            picks, n, lg = e.decode_verify(toks, want_logits=True, sample=True)
            s1, seen1 = e.sampling_state()
            res.append((picks.tolist(), n, e.kv_lengths(1)[0], s0, s1, toks, seen0, seen1, lg.float().cpu()))
            got += picks.tolist()[:n + 1]
        return res

    e1 = Engine(cfg, dtype="bf16", max_seq=128, max_batch=1, max_tiles=1, vision=False)
    e1.load_state_dict(sd, strict=False)
    chain = [begin(e1)]
    for _ in range(60):
        nxt, _ = e1.decode_step(torch.tensor([chain[-1]]))
        chain.append(int(nxt[0]))
    e1.close()
    grp = Group(tp)
    engines, hooks = [], []
    for r in range(tp):
        e = Engine(cfg, dtype="bf16", max_seq=128, max_batch=1, max_tiles=1, tp_rank=r, tp_size=tp, comm=C.c_void_p(1), vision=False)
        h = grp.hook_for(r)
        _lib.check(gpu_lib.omchat_set_allreduce_hook(e.h, C.cast(h, C.c_void_p), None))
        e.load_state_dict(sd, strict=False)
        engines.append(e); hooks.append(h)
    res = _run_ranks(lambda r: drive(engines[r], chain), tp)
    for r in range(1, tp):
        assert [x[:6] for x in res[r]] == [x[:6] for x in res[0]]      # picks, n, cache length, step before / after, tokens
    acc = []
    for k in range(len(plan)):
        picks, n, L, s0, s1, toks = res[0][k][:6]
        full = torch.cat([res[r][k][8] for r in range(tp)], dim=-1).numpy()
        base = sorted(i for r in range(tp) for i in res[r][k][6])          # the ranks' slices of the seen set before the step
        want = lsr.verify_sample_ref(full, toks, SEED, s0, base, PEN).tolist()
        assert picks == want, (k, picks, want)
        assert s1 == s0 + n + 1
        after = sorted(i for r in range(tp) for i in res[r][k][7])
        assert after == sorted(set(base + picks[:n + 1]))
        acc.append(n)
    print(f"\nTP = {tp}: accepted per sampled verify step {acc}")
    for e in engines:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(gpu_lib):
    _, e, m = _tiny_model()
    ids = torch.tensor([PROMPT])
    m.forward(input_ids=ids, use_cache=True)
    before = e.kv_lengths(1)
    toks = [5, 6, 7]
    # the flag without sampling on
    e.sampling_off()
    with pytest.raises(ValueError, match="sampling is off"):
        e.decode_verify(toks, sample=True)
    assert e.kv_lengths(1) == before
    tok, _ = _begin(e, m, ids, SEED, PEN)
    state = e.sampling_state()
    # without the flag the refusal of a verify step while sampling is on stays
    with pytest.raises(ValueError, match="greedy only"):
        e.decode_verify(toks)
    with pytest.raises(ValueError, match="KEEP_ALL"):
        e.decode_verify(toks, keep_all=True, sample=True)
    e.set_constraints(1, [PROMPT], 8, no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="constraints are on"):
        e.decode_verify(toks, sample=True)
    e.constraints_off()
    e.set_logprobs(1, 8)
    with pytest.raises(ValueError, match="logprobs are on"):
        e.decode_verify(toks, sample=True)
    e.logprobs_off()
    assert e.kv_lengths(1) == before and e.sampling_state() == state
    # a rewind of more picks than the last sampled verify step committed, with the penalty on
    picks, n = e.decode_verify([tok] + toks, sample=True)
    after, st_after = e.kv_lengths(1), e.sampling_state()
    assert st_after[0] == state[0] + n + 1
    with pytest.raises(ValueError, match="more than one step"):
        e.kv_rewind(1, n + 2)
    assert e.kv_lengths(1) == after and e.sampling_state() == st_after
    # once another pick ran, the one-step rule holds again
    e.decode_step(torch.tensor([int(picks[n])]))
    with pytest.raises(ValueError, match="more than one step"):
        e.kv_rewind(1, 2)
    e.kv_rewind(1, 1)
    assert e.kv_lengths(1) == after and e.sampling_state() == st_after
    # generate: the keyword with beams; do_sample=True without the keyword names it
    m.forward(input_ids=ids, use_cache=True)
    with pytest.raises(NotImplementedError, match="num_beams"):
        m.generate(ids, prompt_lookup_num_tokens=4, prompt_lookup_sample=True, num_beams=2)
    with pytest.raises(NotImplementedError, match="prompt_lookup_sample"):
        m.generate(ids, prompt_lookup_num_tokens=4, do_sample=True, seed=1)
    assert e.kv_lengths(1) == before
    # greedy: the keyword has no effect
    a = m.generate(ids, max_new_tokens=24, prompt_lookup_num_tokens=4)
    b = m.generate(ids, max_new_tokens=24, prompt_lookup_num_tokens=4, prompt_lookup_sample=True)
    assert torch.equal(a, b)
    # generation_config carries the keyword too
    m.generation_config.prompt_lookup_sample = True
    e.lookup_stats(reset=True)
    m.generate(ids, max_new_tokens=24, prompt_lookup_num_tokens=4, do_sample=True, seed=1, temperature=0.8)      # (raises without it)
    m.generation_config.prompt_lookup_sample = False
    e.close()
