"""tests/vit_stats_ref.py checks itself here, without a GPU: that every operand survives its storage type, that the sums the kernels form are
exact in fp32 in any order, that the normalised scaled rows do not depend on the last bits of rsqrtf, the LDS-DMA / global source rule of the
in-launch row scale, and that the restatement tells each named mistake apart -- by a changed bit where tests/test_gpu_vit_stats.py compares
bits, by more than ten times the bound where it compares within a tolerance (printed; run with -s to read the figures)."""
import pytest
import torch

import gemm_exact_ref as X
import vit_stats_ref as V
from attn_prefill_ref import attend, row_rel
from gpu_util import TOL

DTS = ["bf16", "f16"]
N_CU = 256


def _orders(n, g):
    """index orders in which a sum of n terms is formed below: forward, backward, shuffled, interleaved halves"""
    idx = torch.arange(n)
    return [idx, idx.flip(0), torch.randperm(n, generator=g), torch.cat((idx[0::2], idx[1::2]))]


def _sum32(v, order):
    """the fp32 sum of v[order] formed one term at a time, and as a pairwise tree: both must give the same bits"""
    v = v.float()[order]
    seq = torch.zeros((), dtype=torch.float32)
    for t in v:
        seq = seq + t
    tree = v.clone()
    while tree.numel() > 1:
        if tree.numel() % 2:
            tree = torch.cat((tree, torch.zeros(1)))
        tree = tree[0::2] + tree[1::2]
    assert torch.equal(seq, tree[0]), "the sum depends on its order"
    return seq


def _used_rows():
    """(B, S, C) of every scaled-row operand the GPU tests build"""
    shapes = {(1, r, h) for r, h in V.SUMSQ_CASES} | {(1, r, c) for r, c, _, _ in V.KNORM_CASES} | {(1, r, c) for r, c in V.QKNORM_CASES}
    return sorted(shapes | {(b, s, h * 128) for b, s, h, _, _ in V.MHA_CASES})


# ------------------------------------------------------------------------------------------------------------------- scaled rows
def test_row_exponents_separate_every_neighbour():
    for B, S in sorted({(b, s) for b, s, _ in _used_rows()}):
        e = V.row_exponents(B, S)
        q = V.q_exponents(e)
        for x in (e, q):
            flat = x.reshape(-1)
            assert int(flat.min()) >= -4 and int(flat.max()) <= 5
            assert bool((flat[1:] != flat[:-1]).all()), "adjacent rows must differ"
            if B * S >= 5:
                assert len(flat.unique()) >= 5
            if B > 1:
                assert bool((x != torch.roll(x, 1, 0)).all()), "the same row of the other batch element must differ"
            if B * S > 2:
                for b in range(B):          # the first row of a batch element and the last row: a value neither neighbour has
                    i = b * S
                    assert all(int(flat[i]) != int(flat[j]) for j in (i - 1, i + 1) if 0 <= j < B * S)
                assert int(flat[-1]) != int(flat[-2])
        assert bool((e != q).all()), "q totals must differ from k totals on the same row"
        assert bool(((e - q).abs() >= 1).all())          # a factor of at least 4 between the sums of squares


@pytest.mark.parametrize("dt", DTS)
def test_scaled_rows_round_trip_and_sum_exactly_in_any_order(dt):
    g = torch.Generator().manual_seed(0)
    for B, S, C in _used_rows():
        e = V.row_exponents(B, S)
        for ee in (e, V.q_exponents(e)):
            x = V.scaled_rows(V.groups(3, B * S, C), ee)
            assert bool(X.representable(x, dt).all()), (B, S, C)
            want = V.sumsq_of(ee, C)
            assert torch.equal(X.f32(want), want) and float(want.max()) < 2 ** 24 * 4.0 ** int(ee.max())
            assert torch.equal((x * x).sum(1), want)
            for r in {0, B * S // 2, B * S - 1}:          # the fp32 sums a kernel forms, in four orders and two tree shapes each
                sq = (x[r].float() * x[r].float())
                for order in _orders(C, g):
                    assert float(_sum32(sq, order)) == float(want[r]), (B, S, C, r)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("eps", [1e-6, 0.0])
def test_normalised_rows_do_not_depend_on_the_last_bits_of_rsqrt(dt, eps):
    """+-8 ulp around torch's rsqrt, every exponent in [-4, 5], every channel count in use, C_total in {C, 2 C}: T(x * rstd) == group / 2,
    T(w * .) == w * group / 2, and the Q half's last product is one fp32 product"""
    dev = 0
    for C in sorted({c for _, _, c in _used_rows()}):
        e = torch.arange(-4, 6)
        grp = V.groups(5, len(e), C)
        x = V.scaled_rows(grp, e)
        w = V.norm_weights(6, C)
        want_k = V.exact_knorm(grp, w, dt)
        want_q = (want_k.float() * torch.tensor(V.Q_SCALE, dtype=torch.float32)).to(V.DT[dt])
        for mult in (1, 2):
            inv = V.rstd32(V.sumsq_of(e, mult * C), mult * C, eps)
            for d in range(-8, 9):
                inv_d = (inv.view(torch.int32) + d).view(torch.float32)
                dev += int((V.knorm(x, w, inv_d, dt) != want_k).sum()) + int((V.qnorm(x, w, inv_d, dt) != want_q).sum())
    assert dev == 0


# ------------------------------------------------------------------------------------------------------------------- hand-made slots
def test_slots_sum_exactly_in_any_order_and_differ_per_row_and_slot():
    g = torch.Generator().manual_seed(1)
    rows = 19
    e = V.row_exponents(1, rows)
    for C_total in (128, 384, 768, 3200, 6400):
        total = V.sumsq_of(e, C_total)
        for n in sorted(set(V.RS_NSLOTS) | {c[2] for c in V.KNORM_CASES} | set(V.FINISH_NSLOTS)):
            sl = V.split_slots(total, n)
            assert torch.equal(sl.sum(0), total) and bool((sl > 0).all())
            if n > 1:
                assert bool((sl[:, 1:] != sl[:, :-1]).any(0).all()) and bool((sl[1:] != sl[:-1]).any(1).all())
                assert float((sl / total).min()) > 0.01
            for r in (0, rows - 1):
                for order in _orders(n, g):
                    assert float(_sum32(sl[:, r], order)) == float(total[r])
                h = (n + 1) // 2                          # tile_row_scale's two half-sums, vit_knorm_slots' shuffle tree: covered by any-order
                assert float(sl[:h, r].float().sum() + sl[h:, r].float().sum()) == float(total[r])


def test_row_scale_slots_give_the_exact_factor():
    """rsqrt(sum / dim + 0) of a power of four: 4, 2, 1, 1/2 to the bit, +-0 ulp -- the sum is exact, 1 / dim is a power of two"""
    M = 258
    for n in V.RS_NSLOTS:
        s, sl = V.rs_slots(M, n)
        t = sl.float().sum(0) * torch.tensor(1.0 / V.RS_DIM, dtype=torch.float32)
        assert torch.equal(torch.rsqrt(t).double(), s) and len(s.unique()) >= 4
        assert bool((s[1:] / s[:-1] != 1).all())
        buf = V.slot_buffer(sl, M + 3)
        assert bool(torch.isnan(buf[n:]).all()) and bool(torch.isnan(buf[:, M:]).all()) and not bool(torch.isnan(buf[:n, :M]).any())


def test_row_scale_source_rule_reaches_both_sources_on_every_tile():
    """launch_cfg8 / launch_cfg restated from the tile's LDS bytes; the slot counts of the table reach LDS-DMA and global reads on every tile
    (both are reachable on each), the loop past 16 slots, and an odd count under the two-threads-per-row split"""
    for tile in V.RS_TILES:
        src = {n: V.rs_source(tile, n) for n in V.RS_NSLOTS}
        assert set(src.values()) == {"dma", "global"}, (tile, src)
        assert src[1] == src[2] == src[29] == src[32] == "dma" and src[67] == "global"
        bm = X.TILES[tile][0]
        if V.threads_per_row(tile) == 2:
            assert any(n % 2 == 1 and n > 32 for n in V.RS_NSLOTS)          # halves of unequal length, one of them past 16
        print("tile", tile, "BM", bm, "threads per row", V.threads_per_row(tile), {n: src[n] for n in V.RS_NSLOTS})
    # the production counts: 29 and 50 slots on the 256^2 kernel (32 KiB behind 128 KiB of stages), 67 everywhere
    assert V.rs_source(2, 32) == "dma" and V.rs_source(2, 33) == "global" and V.rs_source(2, 50) == "global"
    assert V.rs_source(1, 64) == "dma" and V.rs_source(1, 65) == "global"
    assert V.rs_source(9, 42) == "dma" and V.rs_source(9, 43) == "global" and V.rs_source(10, 42) == "dma" and V.rs_source(10, 43) == "global"
    assert V.rs_source(7, 32) == "dma" and V.rs_source(7, 33) == "global" and V.rs_source(8, 32) == "dma" and V.rs_source(8, 33) == "global"
    assert {V.threads_per_row(t) for t in V.RS_TILES} == {2}          # every tile kernel of the table has two threads per row
    # tile_row_scale_prefetch's last partial 64-row group: only a tile whose BM is no multiple of 64 has one -- tile 4 (224 rows), which
    # gemm_exact_ref.ROW_SCALE_TILES does not hold; RS_TILES adds it (and tile 5, the 8-wave 192-row tile)
    assert set(X.ROW_SCALE_TILES) < set(V.RS_TILES) and [t for t in V.RS_TILES if X.TILES[t][0] % 64] == [4]
    assert V.rs_source(4, 32) == "dma" and V.rs_source(4, 33) == "global" and V.rs_source(5, 42) == "dma" and V.rs_source(5, 43) == "global"


# ------------------------------------------------------------------------------------------------------------------- statistics epilogues
def _stats_cases():
    out = []
    for epi, tiles in ((V.EPI_LS_RESID_STATS, sorted(X.TILES)), (V.EPI_NONE_STATS, V.NONE_STATS_TILES + (10,))):
        for tile in tiles:
            out += [(epi, tile, m, n, k) for m, n, k in V.stats_shapes(tile, epi)]
    for tile in (12, 13):
        out.append((V.EPI_LS_RESID_STATS, tile) + X.split_shape(N_CU))
    out.append((V.EPI_LS_RESID_STATS, 2) + X.persistent_shape(N_CU))
    return out


@pytest.mark.parametrize("dt", DTS)
def test_statistics_operands_meet_the_granule_precondition(dt):
    """integer outputs |c| <= 63 for both epilogues of every case, every slot total below 2^24, expected slots fp32 values; and the shapes hold
    two whole slots and a partial one of 4 or 24 columns"""
    seen = set()
    for epi, tile, M, N, K in _stats_cases():
        edges = V.slot_edges(tile, epi, M, N, N_CU)
        if (M, N, K) not in (X.split_shape(N_CU), X.persistent_shape(N_CU)):
            w = V.slot_width(V.stats_tile(tile, epi))
            assert len(edges) == 3 == V.cdiv(N, w) and N % w in (4, 24) and M in (1, X.TILES[V.stats_tile(tile, epi)][0] + 1) and K in V.STATS_K
        elif tile in (12, 13):
            n_main, n_tail = X.split_rule(M, N, N_CU)
            assert len(edges) == n_main // 64 + V.cdiv(n_tail, 112) and edges[n_main // 64] == (n_main, n_main + 112)
        assert edges[0][0] == 0 and edges[-1][1] == N and all(a[1] == b[0] for a, b in zip(edges, edges[1:]))
        if (M, N, K) in seen:
            continue
        seen.add((M, N, K))
        ops = V.stats_operands(1, M, N, K, dt)
        for base in (X.EPI_NONE, X.EPI_LS_RESID):
            out = X.reference(ops, base, dt, bias=True)
            assert V.stats_precondition(out, edges), (tile, M, N, K, base)
            want = V.expected_stats(out, edges)
            assert torch.equal(X.f32(want), want)
            assert float(out.abs().max()) >= 8           # not a degenerate problem
            dropped = V.expected_stats(out, V.stats_mutant_edges(edges, N, "drop_last_column"))
            assert bool((dropped != want).any()), "a slot's last column dropped"


@pytest.mark.parametrize("dt", DTS)
def test_a_counted_column_beyond_n_changes_the_slot(dt):
    """a statistics epilogue that counts a column >= N adds that column's stored value squared to the last slot.  Every stored value of these
    operands is an integer and every slot total stays below 2^24, so ANY non-zero value there -- the smallest is 1; W's guard rows behind row N
    are NaN in the strided layout -- changes the fp32 slot: no value is absorbed by rounding.  (A zero there adds nothing and is no error.)"""
    for epi, tile in ((V.EPI_NONE_STATS, 2), (V.EPI_LS_RESID_STATS, 3), (V.EPI_LS_RESID_STATS, 10)):
        for M, N, K in V.stats_shapes(tile, epi):
            ops = V.stats_operands(1, M, N, K, dt)
            out = X.reference(ops, X.EPI_NONE if epi == V.EPI_NONE_STATS else X.EPI_LS_RESID, dt, bias=True)
            edges = V.slot_edges(tile, epi, M, N, N_CU)
            want = V.expected_stats(out, edges).float()
            for v in (1.0, -3.0, V.NAN):
                wider = torch.cat((out, torch.full((M, 1), v, dtype=torch.float64)), 1)
                bad = V.expected_stats(wider, V.stats_mutant_edges(edges, N, "count_beyond_n")).float()
                assert bool((bad[-1] != want[-1]).all()) and torch.equal(bad[:-1], want[:-1]), (tile, M, N, K, v)


def test_persistent_form_takes_the_statistics_epilogue():
    """launch_cfg8's dispatch restated (vit_stats_ref.persistent_dispatch): under tuning key 13 the persistent kernel runs when there are more
    256^2 tiles than workgroups and the launch has no in-launch row scale; a statistics epilogue is not part of the condition, so the GPU test
    runs EPI_LS_RESID_STATS on gemm_exact_ref.persistent_shape under key 13 -- and an rs_stats launch of that shape stays on the plain kernel"""
    M, N, K = X.persistent_shape(N_CU)
    assert V.persistent_dispatch(M, N, N_CU, persist=1, rs_stats=False)
    assert not V.persistent_dispatch(M, N, N_CU, persist=1, rs_stats=True)
    assert not V.persistent_dispatch(M, N, N_CU, persist=0, rs_stats=False)
    for tile in (2, 12, 13):          # the small shapes of the per-slot test never take it: one tile
        for m, n, _ in V.stats_shapes(tile, V.EPI_LS_RESID_STATS):
            assert not V.persistent_dispatch(m, n, N_CU, persist=1, rs_stats=False)


# ------------------------------------------------------------------------------------------------------------------- mutants, exact tests
@pytest.mark.parametrize("dt", DTS)
def test_slot_consumer_mutants_change_bits(dt):
    """vit_knorm_slots / stats_finish / the in-launch row scale on the hand-made slots: row r + 1, q and k groups swapped, the last slot
    dropped, a slot behind nslots read, C for C_total"""
    for rows, C, n, mult in V.KNORM_CASES:
        e = V.row_exponents(1, rows)
        grp = V.groups(11, rows, C)
        x = V.scaled_rows(grp, e)
        w = V.norm_weights(12, C)
        Ct = mult * C
        kq = torch.cat((V.split_slots(V.sumsq_of(V.q_exponents(e), Ct), n, 1), V.split_slots(V.sumsq_of(e, Ct), n, 2)), 0)
        buf = V.slot_buffer(kq, rows + 3)
        want = V.exact_knorm(grp, w, dt)
        live = want != 0
        tq, tk = V.slot_mutant_totals(buf, rows, 0, n, "ok")
        assert torch.equal(tq, V.sumsq_of(V.q_exponents(e), Ct)) and torch.equal(tk, V.sumsq_of(e, Ct))
        assert torch.equal(V.knorm(x, w, V.rstd32(tk, Ct, V.EPS), dt), want)
        for kind in ("swap_groups", "drop_last", "one_behind"):
            mq, mk = V.slot_mutant_totals(buf, rows, 0, n, kind)
            if kind == "drop_last" and n == 1:
                continue
            got = V.knorm(x, w, V.rstd32(mk, Ct, V.EPS), dt)
            assert bool(((got != want) | ~live).all()), (kind, rows, C, n)          # every non-zero output of every row
            assert bool((mq != tq).all())                 # (NaN != x: a slot behind the last one is NaN)
        if rows > 1:
            got = V.knorm(x, w, V.rstd32(V.mutant_row_plus_1(tk), Ct, V.EPS), dt)
            assert bool(((got != want) | ~live).all())
        if mult == 2:                                     # C used for C_total; the sums recomputed from the data
            for t, d in ((tk, C), ((x * x).sum(1), Ct)):
                got = V.knorm(x, w, V.rstd32(t, d, V.EPS), dt)
                assert bool(((got != want) | ~live).all())


@pytest.mark.parametrize("dt", DTS)
def test_row_scale_mutants_change_bits(dt):
    """the in-launch row scale: a factor from row r + 1, the last slot dropped -- every row's outputs change"""
    M, N, K = X.row_scale_shape(1)
    ops = X.cached_operands(1, M, N, K, dt)
    s, sl = V.rs_slots(M, 17)
    want = X.reference(ops, X.EPI_NONE, dt, bias=True, scale=s)
    for name, tot in (("row+1", V.mutant_row_plus_1(sl.sum(0))), ("drop_last", sl[:-1].sum(0))):
        bad = torch.rsqrt(tot.float() / V.RS_DIM).double()
        got = X.reference(ops, X.EPI_NONE, dt, bias=True, scale=bad)
        assert bool((got != want).any(1).all()), name


# ------------------------------------------------------------------------------------------------------------------- mutants, tolerance tests
@pytest.mark.parametrize("dt", DTS)
def test_q_norm_on_load_mutants_move_rows_by_ten_bounds(dt):
    """test 6 of the GPU file: the exact normed Q is what the restatement gives from the right statistics (6a compares bits of the attention
    on it), and each mutant of the statistic moves (sequence, row, head) outputs by more than 10 x gpu_util.TOL (6b)"""
    for B, S, H, stride, mult in V.MHA_CASES:
        inp = V.mha_inputs(B, S, H, mult, dt)
        assert torch.equal(V.mha_qn_from(inp, inp["sums"], inp["dim"], dt), inp["qn"])
        ref = attend(inp["qn"].float(), inp["k"], inp["v"], 1.0, 0, 0, None, None)
        buf = torch.full((B * S * stride,), V.NAN, dtype=torch.float64)
        buf[::stride] = inp["sums"]
        mutants = {"row+1": V.mutant_row_plus_1(inp["sums"]), "other batch": V.mutant_other_batch(inp["sums"], B, S)}
        if stride > 1:
            mutants["stride ignored"] = V.mutant_stride_ignored(buf, B * S, stride)
        for name, sums in mutants.items():
            qn = V.mha_qn_from(inp, sums, inp["dim"], dt)
            qn = torch.nan_to_num(qn.float(), nan=0.0)       # (a NaN statistic gives NaN outputs on the device: counted as moved)
            r = row_rel(attend(qn, inp["k"], inp["v"], 1.0, 0, 0, None, None), ref)
            moved = r > 10 * TOL[dt]
            if name == "stride ignored":
                moved |= torch.isnan(sums.reshape(B, S))[:, :, None]
            print(f"{dt} B{B} S{S} H{H} stride{stride} dim x{mult} {name}: rows moved > 10 TOL {float(moved.double().mean()):.3f}, "
                  f"median {float(r.median()):.3f}, max {float(r.max()):.3f}")
            assert float(r.max()) > 10 * TOL[dt] and float(moved.double().mean()) > 0.5, (name, B, S, H)
        for name, d in (("C for C_total", H * 128),) if mult == 2 else ():
            qn = V.mha_qn_from(inp, inp["sums"], d, dt)
            assert bool((qn != inp["qn"])[inp["qn"] != 0].all())          # bits (6a); sqrt(2) on the logits is not ten bounds on every row
            r = row_rel(attend(qn.float(), inp["k"], inp["v"], 1.0, 0, 0, None, None), ref)
            print(f"{dt} B{B} S{S} H{H} {name}: median {float(r.median()):.3f}, max {float(r.max()):.3f}")
            assert float(r.max()) > 10 * TOL[dt]


@pytest.mark.parametrize("dt", DTS)
def test_tower_row_statistic_mutants_move_rows(dt, monkeypatch):
    """test 7 of the GPU file: on the tower with scaled position rows, an RMSNorm that takes the statistic of row r + 1, or of the same row of
    the neighbouring tile, moves token rows of the oracle's output by more than ten times twice the per-row error of the oracle evaluated in
    the 16-bit type (the CPU's stand-in for the round-5 path; the GPU test measures the real one)"""
    import oracle
    import oracle.vit as ov
    from omchat_amd import synth
    from omchat_amd.config import tiny
    cfg = tiny(layers_v=2, heads_v=3)
    sd = synth.state_dict(cfg, 3, only_prefix=synth.TOWER)
    T = V.DT[dt]
    tower = {k[len(synth.TOWER):]: torch.from_numpy(v).to(T).float() for k, v in sd.items()}
    tower[V.POS_KEY] = V.scale_pos_rows(tower[V.POS_KEY]).to(T).float()
    px = V.scale_tiles(torch.from_numpy(synth.pixels(3, 56, 1)))
    ref = oracle.vision_tower_forward(px, tower, cfg.vision)
    low = oracle.vision_tower_forward(px, {k: v.to(T) for k, v in tower.items()}, cfg.vision).float()
    base = float(row_rel(low, ref).max())
    plain = ov.rms_norm

    def shifted(shift, dim):
        def f(x, weight, eps=1e-6):
            h = x.to(torch.float32)
            var = torch.roll(h.pow(2).mean(-1, keepdim=True), shift, dim)
            return weight * (h * torch.rsqrt(var + eps)).to(x.dtype)
        return f
    for name, f in (("row+1", shifted(-1, -2)), ("other tile", shifted(1, 0))):
        monkeypatch.setattr(ov, "rms_norm", f)
        got = oracle.vision_tower_forward(px, tower, cfg.vision)
        monkeypatch.setattr(ov, "rms_norm", plain)
        r = row_rel(got, ref)
        print(f"{dt} tower {name}: worst row {float(r.max()):.4f}, median {float(r.median()):.4f}; 16-bit oracle worst row {base:.5f}")
        assert float(r.max()) > 10 * 2 * base, name
