"""GPU: shared-prefix batches, N suffixes over one prefilled prompt.  The suffix-pass attention (omchat_op_attn_suffix)
against an fp64 restatement and against poisoned cache slots; the shared decode attention over rows of different lengths
(omchat_op_attn_shared_lens); omchat_prefill_suffixes on the tiny decoder, forked and shared, in both attention forms, against the fp32
oracle, with decode steps on top (eager, captured, rewound); and generate(suffixes=) / score(suffixes=) themselves."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from gpu_util import CODE, DT, TOL, TOL_DEEP, ptr, rel, sync
import suffix_ref as sfr
import oracle
from omchat_amd import _lib, synth
from omchat_amd.config import tiny
from omchat_amd.engine import Engine

SCALE = 1.0 / np.sqrt(128.0)
HEADS = [(28, 4), (7, 1), (4, 2)]


# ---------------------------------------------------------------------------------------------------------------- op level
def _run_suffix(lib, dt, q, k, v, P, lengths):
    N, S, Hq, _ = q.shape
    Hkv, cap = k.shape[1], k.shape[2]
    ws_b = lib.omchat_op_attn_suffix_ws(N, S, Hq, Hkv, P)
    assert ws_b > 0
    ws = torch.empty(ws_b // 4 + 64, dtype=torch.float32, device="cuda")
    out = torch.empty(N, S, Hq, 128, dtype=DT[dt], device="cuda")
    lens = torch.tensor(lengths, dtype=torch.int32)
    scratch = torch.zeros(N, dtype=torch.int32, device="cuda")
    _lib.check(lib.omchat_op_attn_suffix(CODE[dt], ptr(q), ptr(k), ptr(v), ptr(out), N, S, Hq, Hkv, cap, P, ptr(lens), ptr(scratch), float(SCALE),
                                         ptr(ws), ws_b, None))
    sync()
    assert scratch.tolist() == [P + n for n in lengths]
    return out


PS = [1, 63, 64, 65, 200]
# the tile edge (64 / 65), the 16-token chunk edge (15 / 16 / 17), one-row suffixes, and N * n_rep on both sides of the four- / eight-wave forms
ROWS = [(1, [17]), (2, [1, 16]), (5, [15, 16, 17, 64, 65]), (16, [(23 * j) % 70 + 1 for j in range(16)])]
CAP = max(PS) + 131 + 70      # (the longest own part of the shared-attention test + a wider grid)


def _valid(lengths, S):
    return torch.tensor([[t < n for t in range(S)] for n in lengths], device="cuda")


def _kv(dt, Hkv, seed, rows=16):
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(rows, Hkv, CAP, 128, generator=g).to("cuda", DT[dt])
    v = torch.randn(rows, Hkv, CAP, 128, generator=g).to("cuda", DT[dt])
    return g, k, v


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_op_attn_suffix_vs_fp64_reference(gpu_lib, dt, Hq, Hkv):
    g, k, v = _kv(dt, Hkv, Hq * 100 + Hkv)
    worst = 0.0
    for N, lengths in ROWS:
        S = max(lengths)
        q = torch.randn(N, S, Hq, 128, generator=g).to("cuda", DT[dt])
        ok = _valid(lengths, S)
        for P in PS:
            out = _run_suffix(gpu_lib, dt, q, k, v, P, lengths)
            ref = sfr.attn_suffix_ref(q, k, v, P, lengths)
            o, r = out[ok].double(), ref[ok]                              # [valid rows, Hq, 128]: only rows t < len_j are compared
            e = float((o - r).norm() / r.norm())
            e_rows = float(((o - r).flatten(1).norm(dim=1) / r.flatten(1).norm(dim=1)).max())
            print(f"{dt} Hq={Hq} Hkv={Hkv} N={N} S={S} P={P}: rel err {e:.3e} worst row {e_rows:.3e}")
            worst = max(worst, e, e_rows)
            assert torch.isfinite(out.float()).all(), (N, P)             # the padding rows are computed from finite q: finite too
            assert e < TOL[dt] and e_rows < TOL[dt], (N, P, e, e_rows)
    print(f"\n{dt} Hq={Hq} Hkv={Hkv}: worst rel err {worst:.2e}")


@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_op_attn_suffix_reads_only_its_key_set(gpu_lib, Hq, Hkv):
    """what the contract says is never read may hold anything -- huge finite values or NaN -- without changing a bit of the valid rows"""
    dt = "bf16"
    g, k, v = _kv(dt, Hkv, 7 * Hq + Hkv)
    bits = lambda x: x.view(torch.int16)
    for N, lengths in ROWS[1:]:
        S = max(lengths)
        q = torch.randn(N, S, Hq, 128, generator=g).to("cuda", DT[dt])
        ok = _valid(lengths, S)
        for P in (1, 64, 65, 200):
            base = _run_suffix(gpu_lib, dt, q, k, v, P, lengths)
            for poison in (3e4, float("nan")):
                # 1. the leader's slots >= P are its own suffix: the prefix pass stops at exactly P, so the OTHER rows keep their bits
                kp, vp = k.clone(), v.clone()
                kp[0, :, P:] = poison; vp[0, :, P:] = -poison
                got = _run_suffix(gpu_lib, dt, q, kp, vp, P, lengths)
                assert torch.equal(bits(got[1:][ok[1:]]), bits(base[1:][ok[1:]])), (N, P, poison, "leader's suffix")
                assert not torch.equal(bits(got[0][ok[0]]), bits(base[0][ok[0]]))          # (the leader itself reads them)
                # 2. every sibling's slots < P, and every row's slots from its own end on: nobody's
                kp, vp = k.clone(), v.clone()
                kp[1:N, :, :P] = poison; vp[1:N, :, :P] = -poison
                for j, n in enumerate(lengths):
                    kp[j, :, P + n:] = poison; vp[j, :, P + n:] = -poison
                got = _run_suffix(gpu_lib, dt, q, kp, vp, P, lengths)
                assert torch.equal(bits(got[ok]), bits(base[ok])), (N, P, poison, "siblings below P / beyond the end")
                # 4. the padding query rows
                qp = q.clone()
                qp[~ok] = poison
                got = _run_suffix(gpu_lib, dt, qp, k, v, P, lengths)
                assert torch.equal(bits(got[ok]), bits(base[ok])), (N, P, poison, "padding queries")
            # 3. causality inside a row: looking at row (j, t), the slots > P + t of row j -- its own later tokens, which share the row's tiles
            #    and are masked, so a finite value there weighs exactly 0
            for j, n in enumerate(lengths):
                for t in sorted({0, n // 2, n - 1}):
                    kp, vp = k.clone(), v.clone()
                    kp[j, :, P + t + 1:] = 3e4; vp[j, :, P + t + 1:] = -3e4
                    got = _run_suffix(gpu_lib, dt, q, kp, vp, P, lengths)
                    assert torch.equal(bits(got[j, :t + 1]), bits(base[j, :t + 1])), (N, P, j, t)
                    if N > 1:
                        o = [i for i in range(N) if i != j]
                        assert torch.equal(bits(got[o][ok[o]]), bits(base[o][ok[o]])), (N, P, j, t)


def test_op_attn_suffix_refuses_bad_geometry(gpu_lib):
    q = torch.zeros(2, 8, 28, 128, dtype=torch.bfloat16, device="cuda")
    k = torch.zeros(2, 4, 16, 128, dtype=torch.bfloat16, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    sc = torch.zeros(2, dtype=torch.int32, device="cuda")

    def call(P, lengths, Hq=28, Hkv=4, ws_b=1 << 22):
        lens = torch.tensor(lengths, dtype=torch.int32)
        return gpu_lib.omchat_op_attn_suffix(CODE["bf16"], ptr(q), ptr(k), ptr(k), ptr(q), 2, 8, Hq, Hkv, 16, P, ptr(lens), ptr(sc), 0.1, ptr(ws), ws_b, None)
    assert call(0, [1, 8]) != 0              # no prompt
    assert call(9, [1, 8]) != 0              # P + S beyond the capacity
    assert call(4, [0, 8]) != 0              # an empty row
    assert call(4, [1, 9]) != 0              # a row longer than S
    assert call(4, [1, 8], Hq=27, Hkv=3) != 0      # 9 query heads per kv head
    assert call(4, [1, 8], ws_b=64) != 0     # workspace
    assert call(4, [1, 8]) == 0
    sync()


def _run_shared(lib, dt, q, k, v, G, N, P, L, lens=None):
    rows, Hq, _ = q.shape
    Hkv, cap = k.shape[1], k.shape[2]
    ws_b = lib.omchat_op_attn_shared_ws(G, N, Hq, Hkv, P, L)
    ws = torch.empty(ws_b // 4 + 64, dtype=torch.float32, device="cuda")
    out = torch.empty(rows, Hq, 128, dtype=DT[dt], device="cuda")
    if lens is None:
        _lib.check(lib.omchat_op_attn_shared(CODE[dt], ptr(q), ptr(k), ptr(v), ptr(out), G, N, Hq, Hkv, cap, P, L, float(SCALE), ptr(ws), ws_b, None))
    else:
        ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
        _lib.check(lib.omchat_op_attn_shared_lens(CODE[dt], ptr(q), ptr(k), ptr(v), ptr(out), G, N, Hq, Hkv, cap, P, L, ptr(ld), float(SCALE),
                                                  ptr(ws), ws_b, None))
    sync()
    return out


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_op_attn_shared_lens_vs_fp64_reference(gpu_lib, dt, Hq, Hkv):
    """rows of different lengths: one with a single own key next to one 130 keys longer (two suffix tiles of the short row are empty)"""
    g, k, v = _kv(dt, Hkv, 3 * Hq + Hkv)
    for G, N, own in ((1, 2, [1, 131]), (1, 5, [1, 131, 64, 65, 2]), (2, 3, [70, 1, 131, 3, 130, 64]), (1, 16, [(37 * j) % 131 + 1 for j in range(16)])):
        q = torch.randn(G * N, Hq, 128, generator=g).to("cuda", DT[dt])
        for P in (1, 63, 64, 65, 200):
            lens = [P + d for d in own]
            L = max(lens)
            out = _run_shared(gpu_lib, dt, q, k, v, G, N, P, L, lens)
            ref = sfr.attn_shared_lens_ref(q, k, v, G, N, P, lens)
            e_rows = float(((out.double() - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)).max())
            print(f"{dt} Hq={Hq} Hkv={Hkv} G={G} N={N} P={P}: worst row rel err {e_rows:.3e}")
            assert torch.isfinite(out.float()).all() and e_rows < TOL[dt], (G, N, P, e_rows)
            # a grid sized for a longer L (the step's 256-key bucket) gives the same bits: the extra splits are neutral
            wide = _run_shared(gpu_lib, dt, q, k, v, G, N, P, min(CAP, L + 70), lens)
            assert torch.equal(wide.view(torch.int16), out.view(torch.int16)), (G, N, P)
            # equal lengths: the bits of omchat_op_attn_shared
            same = _run_shared(gpu_lib, dt, q, k, v, G, N, P, L, [L] * (G * N))
            assert torch.equal(same.view(torch.int16), _run_shared(gpu_lib, dt, q, k, v, G, N, P, L).view(torch.int16)), (G, N, P)


# ---------------------------------------------------------------------------------------------------------------- model level (C ABI)
def _decoder(q=7, kv=1, dt="bf16", seed=3, max_seq=512, max_batch=8, **kw):
    cfg = tiny(q_heads=q, kv_heads=kv)
    sd = synth.state_dict(cfg, seed)
    e = Engine(cfg, dtype=dt, max_seq=max_seq, max_batch=max_batch, max_tiles=1, vision=False, **kw)
    e.load_state_dict(sd, strict=False)
    sdt = {k_: torch.from_numpy(v_).to(DT[dt]).float() for k_, v_ in sd.items()}      # the oracle on the 16-bit-rounded weights
    return cfg, e, sdt


def _embeds(sdt, ids, dt):
    return sdt["model.embed_tokens.weight"][torch.as_tensor(ids)].to(DT[dt])


def _oracle(cfg, sdt, emb):
    """fp32 full forward over all rows: (hidden [S, H], logits [S, V], cache)"""
    cache = oracle.decoder.KVCache(cfg.text["num_hidden_layers"])
    h = oracle.qwen2_model(emb.float()[None], sdt, cfg.text, cache)
    return h[0], oracle.lm_head(h, sdt)[0], cache


def _ids(n, seed):
    return torch.randint(0, 320, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


def _snap(e, cfg, N, n):
    """slots [0, n) of the cache rows 0 .. N - 1, every layer, K and V"""
    return [[[e.kv_read_row(j, l, w, 0, n).clone() for w in (0, 1)] for l in range(cfg.text["num_hidden_layers"])] for j in range(N)]


def _block(embs, dt):
    S = max(x.shape[0] for x in embs)
    blk = torch.zeros(len(embs), S, embs[0].shape[1], dtype=DT[dt])
    for j, x in enumerate(embs):
        blk[j, :x.shape[0]] = x
    return blk.cuda()


@pytest.fixture
def force_form(gpu_lib):
    def set_(v):
        _lib.check(gpu_lib.omchat_op_set_tuning(51, v))
    yield set_
    _lib.check(gpu_lib.omchat_op_set_tuning(51, -1))


def _suffix_state(e, sdt, dt, P, lengths, share, seed):
    """prefill P prompt rows, fork / share them among the N rows -> (prompt embeds, per-row suffix embeds)"""
    N = len(lengths)
    emb_p = _embeds(sdt, _ids(P, seed), dt)
    embs = [_embeds(sdt, _ids(n, seed + 17 * (j + 1)), dt) for j, n in enumerate(lengths)]
    e.prefill(emb_p[None].cuda(), [P])
    if N > 1:
        e.group_begin(1, N, P, bool(share))
    return emb_p, embs


SHAPES = [(40, [23, 1, 9]), (100, [64, 17]), (7, [1])]
bits = lambda x: x.view(torch.int16)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("q,kv", [(7, 1), (4, 2)])
@pytest.mark.parametrize("share,form", [(0, 1), (0, 0), (1, 1)])      # form 1 = the suffix kernel, 0 = the batched prefill kernel (forked rows only)
@pytest.mark.parametrize("P,lengths", SHAPES)
def test_prefill_suffixes_vs_oracle(gpu_lib, force_form, dt, q, kv, share, form, P, lengths):
    cfg, e, sdt = _decoder(q, kv, dt)
    N, S = len(lengths), max(lengths)
    force_form(form)
    assert e.suffix_attn_form(share and N > 1) == form
    emb_p, embs = _suffix_state(e, sdt, dt, P, lengths, share, P * 7 + S)
    assert e.kv_lengths(N) == [P] * N
    span = P + S + 2
    before = _snap(e, cfg, N, span)
    logits, hidden = e.prefill_suffixes(_block(embs, dt), lengths, P, want_hidden=True); sync()
    assert e.kv_lengths(N) == [P + n for n in lengths]
    after = _snap(e, cfg, N, span)
    for j, n in enumerate(lengths):
        h_ref, lg_ref, _ = _oracle(cfg, sdt, torch.cat([emb_p, embs[j]]))
        e_h, e_l = rel(hidden[j, :n], h_ref[P:]), rel(logits[j], lg_ref[-1])
        print(f"\n{dt} {q}q/{kv}kv share {share} form {form} P={P} row {j} S={n}: hidden rel err {e_h:.3e}, last logits {e_l:.3e}")
        assert e_h < TOL_DEEP[dt] and e_l < TOL_DEEP[dt], (j, e_h, e_l)
        for l in range(cfg.text["num_hidden_layers"]):
            for w in (0, 1):
                b4, af = before[j][l][w], after[j][l][w]
                # the prompt's slots: the leader's are never written, a sibling's neither (its copy when forked, nobody's when shared)
                assert torch.equal(bits(b4[:, :P]), bits(af[:, :P])), (j, l, w, "slots < P")
                # nothing behind the row's own suffix -- the padding rows of the block write no slot
                assert torch.equal(bits(b4[:, P + n:]), bits(af[:, P + n:])), (j, l, w, "slots >= P + len")
                assert torch.isfinite(af[:, P:P + n].float()).all()
    assert torch.isfinite(hidden.float()).all()
    e.close()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("q,kv", [(7, 1), (4, 2)])
@pytest.mark.parametrize("share", [0, 1])
def test_decode_steps_on_ragged_rows_eager_graph_and_rewind(gpu_lib, dt, q, kv, share):
    """three teacher-forced steps on the oracle's argmax ids over rows of lengths P + 23 / 1 / 9: every step's logits against the oracle,
    eager and captured steps bit for bit, and a rewound step taken again gives the same bits"""
    cfg, e, sdt = _decoder(q, kv, dt)
    P, lengths = 40, [23, 1, 9]
    N = len(lengths)
    e.sampling_off()
    runs = {}
    for graph in (False, True):
        e.enable_decode_graph(graph)
        emb_p, embs = _suffix_state(e, sdt, dt, P, lengths, share, 5)
        logits, _ = e.prefill_suffixes(_block(embs, dt), lengths, P); sync()
        if not graph:
            caches, toks, refs = [], [], []
            for j in range(N):
                _, lg_ref, cache = _oracle(cfg, sdt, torch.cat([emb_p, embs[j]]))
                row_t, row_r, last = [], [], lg_ref[-1]
                for _ in range(3):
                    row_t.append(int(torch.argmax(last)))
                    last = oracle.lm_head(oracle.qwen2_model(_embeds(sdt, [row_t[-1]], dt).float()[None], sdt, cfg.text, cache), sdt)[0, 0]
                    row_r.append(last)
                toks.append(row_t); refs.append(row_r)
        got = []
        for t in range(3):
            _, lg = e.decode_step(torch.tensor([toks[j][t] for j in range(N)], dtype=torch.int32), want_logits=True)
            got.append(lg.clone())
            assert e.kv_lengths(N) == [P + n + t + 1 for n in lengths]
        e.kv_rewind(N, 1)
        assert e.kv_lengths(N) == [P + n + 2 for n in lengths]
        _, again = e.decode_step(torch.tensor([toks[j][2] for j in range(N)], dtype=torch.int32), want_logits=True); sync()
        assert torch.equal(again, got[2]), "a rewound step taken again"
        runs[graph] = got
        if not graph:
            for t in range(3):
                errs = [rel(got[t][j], refs[j][t]) for j in range(N)]
                print(f"\n{dt} {q}q/{kv}kv share {share} step {t}: logits vs the oracle, rows {['%.3e' % x for x in errs]}")
                assert max(errs) < TOL_DEEP[dt], (t, errs)
    assert e.decode_graph_stats()["replays"] > 0
    for t in range(3):
        assert torch.equal(runs[False][t], runs[True][t]), t
    e.enable_decode_graph(False)
    e.close()


def test_refusals_leave_the_state_alone(gpu_lib):
    cfg, e, sdt = _decoder(max_seq=128, max_batch=4, max_prefill_rows=64)
    emb = _embeds(sdt, _ids(64, 5), "bf16").cuda()
    blk = lambda N, S: emb[:1].expand(N * S, -1).reshape(N, S, -1).contiguous()

    def refused(match, N, S, lengths, keep, rows=4):
        kv = e.kv_lengths(rows)
        with pytest.raises((ValueError, _lib.OmchatError), match=match):
            e.prefill_suffixes(blk(N, S), lengths, keep)
        assert e.kv_lengths(rows) == kv

    refused("no live state|must each hold exactly keep", 2, 4, [4, 2], 10)
    e.prefill(emb[None, :30], [30])
    refused("must each hold exactly keep", 2, 4, [4, 2], 30)               # no fork yet: row 1 does not hold the prompt
    refused("must each hold exactly keep", 1, 4, [4], 29)
    e.group_begin(1, 3, 30, True)
    refused("lengths must be in", 3, 4, [4, 0, 2], 30)
    refused("lengths must be in", 3, 4, [4, 5, 2], 30)
    refused("not one prompt of keep slots with N rows", 2, 4, [4, 2], 30)
    refused("N outside", 5, 4, [4] * 5, 30)
    refused("max_prefill_rows", 3, 22, [22] * 3, 30)
    refused("keep < 1", 3, 4, [4] * 3, 0)
    e2_kv = e.kv_lengths(3)
    assert e2_kv == [30] * 3
    with pytest.raises((ValueError, _lib.OmchatError), match="sampled group shares its prompt"):      # omchat_prefill_extend's refusal is still in force
        e.prefill_extend(emb[:4], 10)
    # the group survived all of it: the suffix pass and a ragged step still run, then the step's own refusals
    lg, _ = e.prefill_suffixes(blk(3, 4), [4, 1, 2], 30); sync()
    assert e.kv_lengths(3) == [34, 31, 32] and torch.isfinite(lg).all()
    tok = torch.tensor([4, 5, 6], dtype=torch.int32)
    e.sampling_off()
    e.decode_step(tok)
    for call in (lambda: e.decode_step(tok[:2]), lambda: e.decode_verify([4, 5, 6]), lambda: e.beam_begin(1, 2, eos=[1], max_new=4),
                 lambda: e.decode_step_masked(tok, torch.full((3,), 9), torch.ones(3, 40))):
        with pytest.raises((ValueError, _lib.OmchatError)):
            call()
    assert e.kv_lengths(3) == [35, 32, 33]
    e.kv_rewind(3, 3)                                                       # below the prompt: the shared step refuses, the lengths stay
    with pytest.raises((ValueError, _lib.OmchatError), match="none shorter than the prompt"):
        e.decode_step(tok)
    assert e.kv_lengths(3) == [32, 29, 30]
    # max_seq, the section-7 modes, a beam search, a left-padded state
    e.prefill(emb[None, :30], [30]); e.group_begin(1, 2, 30, False)
    e3 = e.kv_lengths(2)
    with pytest.raises((ValueError, _lib.OmchatError), match="max_prefill_rows|max_seq"):
        e.prefill_suffixes(torch.zeros(2, 99, emb.shape[1], dtype=torch.bfloat16, device="cuda"), [99, 99], 30)
    assert e.kv_lengths(2) == e3
    e.enable_fp8_prefill(True)
    refused("fp8 x fp8 prefill", 2, 4, [4, 2], 30, rows=2)
    e.enable_fp8_prefill(False)
    e.prefill(emb[None, :30], [30])
    e.beam_begin(1, 2, max_new=4)
    refused("beam search", 1, 4, [4], 30, rows=2)
    e.prefill(torch.stack([emb[:30], emb[30:60]]), [30, 20], padding_side="left")
    refused("left-padded", 2, 4, [4, 2], 30, rows=2)
    e.enable_fp8_kv(True)
    e.prefill(emb[None, :30], [30])
    refused("e4m3 KV cache", 1, 4, [4], 30, rows=2)
    e.enable_fp8_kv(False)
    e.close()


# ---------------------------------------------------------------------------------------------------------------- generate / score
import constraints_ref as cr
import logprob_ref as lr
import sampling_ref as sr
from omchat_amd import suffix as sx

SEED = 1          # synthetic weights for which the ORACLE's greedy margins clear the guard at every position of every row: on the CPU, f16-rounded
                  # weights, margin / rms per position -- row 0: 0.0363 0.3473 0.4290 0.4254 0.3936 0.3326 0.2709 0.2090; row 1: 0.1596 0.3618
                  # 0.3612 0.3661 0.3178 0.2574 0.1910 0.1211; row 2: 0.1607 0.3152 0.2787 0.2324 0.1848 0.1340 0.0808 0.0269 -- all above
                  # 6 x 1.5e-3 (the guard of test_generate_reuse_second_turn with the f16 seam's error rounded up)
IDS1 = [3, -200, 17, 18, -200, 19, 20, 21]
SUF = [[40, 41, 42, 43, 44], [50, 51], [60, 61, 62, 63, 64, 65, 66, 67, 68]]
NEW = 8


def _chat_model(dt="f16", seed=SEED, max_batch=3):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    cfg = tiny()
    sd = synth.state_dict(cfg, seed)
    e = Engine(cfg, dtype=dt, max_seq=256, max_batch=max_batch, max_tiles=2)
    e.load_state_dict(sd)
    sdt = {k_: torch.from_numpy(v_).to(DT[dt]).float() for k_, v_ in sd.items()}
    img = torch.from_numpy(synth.pixels(2, 56, 3)).to(DT[dt])
    return cfg, e, OmChatQwen2ForCausalLM(cfg.clone(), e), sdt, img


def _oracle_greedy(cfg, sdt, ids, img, n):
    """the oracle's greedy continuation of ids: first-position logits, ids, and per position (margin, rms of the logits)"""
    logits, cache, _ = oracle.prefill(torch.tensor([ids]), img.float(), sdt, cfg.vision, cfg.text)
    first = logits[0, -1].float()
    out, info, last = [], [], first
    for _ in range(n):
        top2 = torch.topk(last, 2).values
        out.append(int(torch.argmax(last)))
        info.append((float(top2[0] - top2[1]), float(last.pow(2).mean().sqrt())))
        last = oracle.decode_step(torch.tensor([[out[-1]]]), sdt, cfg.text, cache)[0, -1].float()
    return first, out, info


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_generate_suffixes_greedy_image_prompt(gpu_lib, dt):
    cfg, e, m, sdt, img = _chat_model(dt)
    ids = torch.tensor([IDS1])
    N, P = len(SUF), len(IDS1) - 2 + 2 * e.ntok
    refs = [_oracle_greedy(cfg, sdt, IDS1 + s, img, NEW) for s in SUF]
    alone = [m.generate(torch.tensor([IDS1 + s]), images=img.cuda(), max_new_tokens=NEW)[0, len(IDS1) + len(s):].tolist() for s in SUF]
    plain = m.generate(ids, images=img.cuda(), max_new_tokens=NEW)
    for share in (False, True):
        e.encode_stats(reset=True)
        out = m.generate(ids, images=img.cuda(), suffixes=SUF, max_new_tokens=NEW, share_prompt=share)
        assert tuple(out.shape) == (N, NEW) and out.dtype == torch.int64          # the generated ids only
        assert e.suffix_stats() == dict(tiles_encoded=2, prompt_rows=P, suffix_rows=sum(map(len, SUF)), shared=share)
        assert e.encode_stats() == dict(calls=1, tiles=2)                         # the tower ran once, over the two tiles
        assert e.kv_lengths(N) == [P + len(s) + NEW - 1 for s in SUF]             # no pads in the cache: every row at its own length
        # the suffix pass's first-token logits against the oracle's full forward over each concatenated prompt
        rows, sh = m._suffix_params(ids, img.cuda(), None, SUF, 1, 1, share, False, {}, None)
        lg = m._forward_suffixes(ids, img.cuda(), None, rows, sh).local_logits; sync()
        for j in range(N):
            first, o_ids, info = refs[j]
            err = rel(lg[j], first)
            assert err < TOL_DEEP[dt], (j, err)
            compared, got = 0, out[j].tolist()
            for i in range(NEW):
                margin, rms = info[i]
                if margin > 6.0 * err * rms:
                    compared += 1
                    assert got[i] == alone[j][i] == o_ids[i], (share, j, i, margin, rms, got, alone[j], o_ids)
                elif not (got[i] == alone[j][i] == o_ids[i]):
                    break                                                        # a legitimate near-tie swap: the chains part from here
            print(f"\n{dt} share {share} row {j}: first-token logits rel err {err:.3e}; ids compared at {compared} / {NEW}; {got} alone {alone[j]} oracle {o_ids}")
            if dt == "f16":
                assert compared >= (3 * NEW + 3) // 4
        # a row that hits EOS early pads only itself
        free = out.tolist()
        cand = [t for t in free[0] if any(t not in r for r in free[1:])]
        assert cand, free
        eos, pad = cand[0], 0
        got = m.generate(ids, images=img.cuda(), suffixes=SUF, max_new_tokens=NEW, share_prompt=share, eos_token_id=eos, pad_token_id=pad).tolist()
        firsts = [r.index(eos) if eos in r else None for r in free]
        width = max(NEW if f is None else f + 1 for f in firsts)
        want = [(r if f is None else r[:f + 1] + [pad] * NEW)[:width] for r, f in zip(free, firsts)]
        assert got == want and firsts[0] is not None, (eos, got, want)
        # return_dict_in_generate: .sequences is the same tensor, the log-prob fields are [N, new]
        res = m.generate(ids, images=img.cuda(), suffixes=SUF, max_new_tokens=NEW, share_prompt=share, return_dict_in_generate=True, output_logprobs=True,
                         top_logprobs=3, score_token_ids=[5, 110])
        assert torch.equal(res.sequences, out) and tuple(res.logprobs.shape) == (N, NEW) == tuple(res.processed_logprobs.shape)
        assert tuple(res.top_logprobs.shape) == (N, NEW, 3) == tuple(res.top_token_ids.shape) and tuple(res.scored_logprobs.shape) == (N, NEW, 2)
        assert torch.equal(res.top_token_ids[:, :, 0], out)                       # greedy: the pick is the most likely id
        # one suffix: the same row, a streamer is allowed, the group is not begun
        one = m.generate(ids, images=img.cuda(), suffixes=[SUF[2]], max_new_tokens=NEW, share_prompt=share)
        assert one.tolist() == [alone[2]] or dt == "bf16"
        assert e.suffix_stats()["shared"] is False
        # the mode ended: a plain call returns what it returned before
        assert torch.equal(m.generate(ids, images=img.cuda(), max_new_tokens=NEW), plain)
    e.close()


PROMPT = [3, 17, 18, 19, 20, 21, 7, 9]
TSUF = [[40, 41, 42], [5], [60, 61, 62, 63, 64, 65, 66]]
SMP = dict(temperature=0.9, top_k=50, top_p=0.9, repetition_penalty=1.3)
V_TINY = tiny().text["vocab_size"]


def _tiny_model(max_batch=4, seed=21, dt="bf16", max_seq=128):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    cfg = tiny()
    sd = synth.state_dict(cfg, seed)
    e = Engine(cfg, dtype=dt, max_seq=max_seq, max_batch=max_batch, max_tiles=1, vision=False)
    e.load_state_dict(sd, strict=False)
    return cfg, e, OmChatQwen2ForCausalLM(cfg.clone(), e), {k_: torch.from_numpy(v_).to(DT[dt]).float() for k_, v_ in sd.items()}


def _host_loop(e, m, n, p, share, seed, graph=False):
    """what generate(suffixes=, do_sample=True, ...) does, one step at a time: every pick against the CPU restatement (the ban, then the
    sampler with row j's key and row j's history prompt + suffix_j) applied to that step's own device logits, and its recorded
    log-probabilities against logprob_ref.  -> ids [N, n]"""
    e.enable_decode_graph(graph)
    ids = torch.tensor([PROMPT])
    rows, sh = m._suffix_params(ids, None, None, TSUF, 1, 1, bool(share), False, {}, None)
    out = m._forward_suffixes(ids, None, None, rows, sh)
    N = len(TSUF)
    hist = sx.histories(PROMPT, TSUF)
    assert e.kv_lengths(N) == [len(h) for h in hist]
    e.set_constraints(N, hist, n, no_repeat_ngram_size=p["ngram"], suppress_tokens=p["suppress"])
    e.set_logprobs(N, n)
    e.set_sampling(N, seed=seed, seen=sx.seen_sets(PROMPT, TSUF), **SMP)
    lg = out.local_logits
    tok = e.sample(lg)
    got, lgs = [], []
    for step in range(n):
        raw = lg.cpu().numpy()
        ref = []
        for r in range(N):
            l = cr.apply(raw[r], cr.banned_ids(hist[r], p, step))
            ref.append(sr.sample_row(l, r, step, seed, SMP["temperature"], SMP["top_k"], SMP["top_p"], [i for i in hist[r] if i >= 0], SMP["repetition_penalty"]))
        assert tok.tolist() == ref, (step, tok.tolist(), ref)
        got.append(ref); lgs.append(raw)
        if step < n - 1:
            tok, lg = e.decode_step(tok, want_logits=True)
        for r in range(N):
            hist[r].append(ref[r])
    rawlp, proc, counts = e.read_logprobs(N)
    assert counts == [n] * N
    hist = sx.histories(PROMPT, TSUF)
    for step in range(n):
        for r in range(N):
            i, row = got[step][r], lgs[step][r]
            l_ = lr.lse(row)
            assert abs(float(rawlp[r, step]) - (float(row[i]) - l_)) <= lr.tolerance(row[i], l_), (step, r)
            sc = lr.scores(row, banned=cr.banned_ids(hist[r], p, step), temperature=SMP["temperature"], top_k=SMP["top_k"], top_p=SMP["top_p"],
                           penalty=SMP["repetition_penalty"], seen=[x for x in hist[r] if x >= 0])
            ls = lr.lse(sc)
            assert np.isfinite(sc[i]) and abs(float(proc[r, step]) - (float(sc[i]) - ls)) <= lr.tolerance(sc[i], ls), (step, r)
        for r in range(N):
            hist[r].append(got[step][r])
    e.enable_decode_graph(False)
    e.constraints_off(); e.sampling_off(); e.logprobs_off()
    return np.array(got).T


@pytest.mark.parametrize("share", [0, 1])
def test_generate_suffixes_sampled_with_bans_and_logprobs(gpu_lib, share):
    _, e, m, _ = _tiny_model()
    p = cr.params(V_TINY, ngram=2, suppress=[7, 9, 17])
    n = 10
    eager = _host_loop(e, m, n, p, share, 77)
    assert np.array_equal(_host_loop(e, m, n, p, share, 77, graph=True), eager)
    kw = dict(suffixes=TSUF, do_sample=True, seed=77, max_new_tokens=n, share_prompt=bool(share), no_repeat_ngram_size=2, suppress_tokens=[7, 9, 17], **SMP)
    out = m.generate(torch.tensor([PROMPT]), **kw)
    assert tuple(out.shape) == (len(TSUF), n) and np.array_equal(out.numpy(), eager)
    res = m.generate(torch.tensor([PROMPT]), return_dict_in_generate=True, output_logprobs=True, top_logprobs=4, score_token_ids=[5, 6, 7], **kw)
    assert torch.equal(res.sequences, out)
    assert tuple(res.logprobs.shape) == (3, n) == tuple(res.processed_logprobs.shape) and bool((res.logprobs <= 0).all())
    assert tuple(res.top_logprobs.shape) == (3, n, 4) == tuple(res.top_token_ids.shape) and tuple(res.scored_logprobs.shape) == (3, n, 3)
    # stopping criteria see the per-row full sequences, right-padded with the pad id
    seen_shapes = []

    def crit(seqs, scores):
        seen_shapes.append(seqs.clone())
        return seqs.shape[1] >= len(PROMPT) + 7 + 3
    short = m.generate(torch.tensor([PROMPT]), stopping_criteria=[crit], pad_token_id=2, **kw)
    assert short.shape[1] == 3 and np.array_equal(short.numpy(), eager[:, :3])
    last = seen_shapes[-1].tolist()
    assert last == sx.padded_sequences(PROMPT, TSUF, eager[:, :3].tolist(), 2) and last[1][-6:] == [2] * 6
    e.close()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("share", [False, True])
def test_score_suffixes_vs_oracle(gpu_lib, dt, share):
    """per-token log-probabilities of every suffix, held to the bounds of tests/test_gpu_score.py: against the existing path (Engine.lm_head
    on the same hidden rows, log-softmax in fp64) within the op tolerance 2 H 2^-24 max_n sum_k |h_k w_nk| + logprob_ref.tolerance, and
    against the oracle's log-softmax over the concatenated sequence within that path's own distance to the oracle + the op tolerance;
    sequence_logprobs rank the rows as the oracle does whenever the oracle's gap exceeds the summed bound"""
    cfg, e, m, sdt = _tiny_model(dt=dt)
    ids = torch.tensor([PROMPT])
    P, N, S = len(PROMPT), len(TSUF), max(map(len, TSUF))
    full = []
    for s in TSUF:
        cache = oracle.decoder.KVCache(cfg.text["num_hidden_layers"])
        h = oracle.qwen2_model(sdt["model.embed_tokens.weight"][torch.as_tensor(PROMPT + s)].float()[None], sdt, cfg.text, cache)
        full.append(oracle.lm_head(h, sdt)[0])
    want, want_seq, want_n = sfr.score_from_logits(full, P, TSUF)
    res = m.score(ids, suffixes=TSUF, share_prompt=share)
    st = e.suffix_stats()
    assert st["prompt_rows"] == P and st["suffix_rows"] == 11 and st["shared"] == share and st["tiles_encoded"] == 0
    tl = res["token_logprobs"].cpu().double()
    assert tuple(tl.shape) == (N, S) and res["num_tokens"].tolist() == want_n.tolist() == [3, 1, 7]
    # the existing path on the very same hidden rows (the second run issues the same launches: the same bits)
    rows, sh = m._suffix_params(ids, None, None, TSUF, 1, 1, share, False, {}, None)
    o = m._forward_suffixes(ids, None, None, rows, sh, want_hidden=True)
    e.group_end()
    hid = torch.cat([o.prompt_hidden[:, -1:].expand(N, 1, -1), o.suffix_hidden[:, :S - 1]], dim=1).contiguous()      # row t predicts suffix token t
    L = e.lm_head(hid).cpu().double()
    w64 = sdt.get("lm_head.weight", sdt["model.embed_tokens.weight"]).double()
    worst = (hid.float().cpu().double().abs().reshape(N * S, -1) @ w64.abs().T).max(dim=1).values.reshape(N, S)
    H = hid.shape[-1]
    d_new = d_ref = 0.0
    tol_min, bound = 1e9, torch.zeros(N)
    for j, s in enumerate(TSUF):
        for t, tok in enumerate(s):
            z = L[j, t].numpy()
            exist = float(z[tok]) - lr.lse(z)
            tol = 2.0 * H * 2.0 ** -24 * float(worst[j, t]) + lr.tolerance(z[tok], lr.lse(z))
            d_new, tol_min = max(d_new, abs(float(tl[j, t]) - exist)), min(tol_min, tol)
            assert abs(float(tl[j, t]) - exist) <= tol, (j, t, float(tl[j, t]), exist, tol)
            d_ref = max(d_ref, abs(exist - float(want[j, t])))
            bound[j] += tol
        assert bool((tl[j, len(s):] == 0).all())
    print(f"\n{dt} share {share}: token log-probs new-vs-existing {d_new:.3e} (tol >= {tol_min:.3e}); max|existing - oracle| {d_ref:.3e}; "
          f"max|new - oracle| {float((tl - want).abs().max()):.3e}")
    assert float((tl - want).abs().max()) <= d_ref + float(bound.max())
    seq = res["sequence_logprobs"].cpu().double()
    assert torch.allclose(seq, tl.sum(1), atol=1e-5)
    assert torch.allclose(res["perplexity"].cpu().double(), torch.exp(-seq / want_n), rtol=1e-4)
    for a in range(N):
        for b in range(N):
            if float(want_seq[a] - want_seq[b]) > d_ref * (len(TSUF[a]) + len(TSUF[b])) + float(bound[a] + bound[b]):
                assert float(seq[a]) > float(seq[b]), (a, b, seq.tolist(), want_seq.tolist())
    # against score() of each concatenated prompt on the same build, restricted to the suffix: two paths to the same numbers, each within
    # its distance to the oracle
    for j, s in enumerate(TSUF):
        one = m.score(torch.tensor([PROMPT + s]))["token_logprobs"][0, P:].cpu().double()
        d_one = float((one - want[j, :len(s)]).abs().max())
        assert float((one - tl[j, :len(s)]).abs().max()) <= d_one + d_ref + float(bound[j]), j
    # the group ended: a plain generate runs
    assert m.generate(ids, max_new_tokens=4).shape == (1, P + 4)
    e.close()


def test_generate_refusals_leave_the_model_alone_and_modes_compose(gpu_lib):
    _, e, m, _ = _tiny_model(max_batch=4, max_seq=64)
    ids = torch.tensor([PROMPT])
    plain = m.generate(ids, max_new_tokens=6)
    base = m.generate(ids, suffixes=TSUF, max_new_tokens=6, share_prompt=True)
    kv = e.kv_lengths(4)
    st = e.suffix_stats()
    for exc, kw in ((ValueError, dict(suffixes=[])), (ValueError, dict(suffixes=[[5], []])), (ValueError, dict(suffixes=[[5, -200]])),
                    (ValueError, dict(suffixes=[[V_TINY]])), (ValueError, dict(suffixes=[[5]] * 5)), (NotImplementedError, dict(suffixes=TSUF, num_beams=2)),
                    (NotImplementedError, dict(suffixes=TSUF, num_return_sequences=2, do_sample=True, seed=1)),
                    (NotImplementedError, dict(suffixes=TSUF, prompt_lookup_num_tokens=3)), (NotImplementedError, dict(suffixes=TSUF, reuse_cache=True)),
                    (NotImplementedError, dict(suffixes=TSUF, attention_mask=torch.tensor([[1] * 7 + [0]]))),
                    (ValueError, dict(suffixes=[[5] * 56]))):                   # 8 + 56 + 1 > max_seq = 64: refused on the splice plan
        with pytest.raises(exc):
            m.generate(ids, max_new_tokens=6, **kw)
        assert e.kv_lengths(4) == kv and e.suffix_stats() == st, kw
    with pytest.raises(ValueError):
        m.generate(torch.tensor([PROMPT, PROMPT]), suffixes=TSUF, max_new_tokens=6)
    # the shared group of the last successful call is still on and intact: a ragged step runs
    e.decode_step(torch.tensor([4, 5, 6], dtype=torch.int32))
    assert e.kv_lengths(3) == [x + 1 for x in kv[:3]]
    assert torch.equal(m.generate(ids, max_new_tokens=6), plain)                  # a plain call returns what it returned before
    # the decode graph and MXFP4 decode (both modes) compose with the suffix rows
    bases = {}
    for share in (False, True):
        eager = bases[share] = m.generate(ids, suffixes=TSUF, max_new_tokens=6, share_prompt=share)
        assert tuple(eager.shape) == (3, 6) and (not share or torch.equal(eager, base))
        e.enable_decode_graph(True)
        r0 = e.decode_graph_stats()["replays"]
        assert torch.equal(m.generate(ids, suffixes=TSUF, max_new_tokens=6, share_prompt=share), eager)
        assert e.decode_graph_stats()["replays"] > r0
        e.enable_decode_graph(False)
    for batched in (False, True):
        m.enable_mxfp4_decode(True, batched=batched)
        for share in (False, True):
            a = m.generate(ids, suffixes=TSUF, max_new_tokens=6, share_prompt=share)
            assert tuple(a.shape) == (3, 6) and torch.equal(a, m.generate(ids, suffixes=TSUF, max_new_tokens=6, share_prompt=share))
            if not batched:
                assert torch.equal(a, bases[share])                               # mode 1: batched steps keep the 16-bit weights
    m.enable_mxfp4_decode(False)
    assert torch.equal(m.generate(ids, max_new_tokens=6), plain)
    e.close()
