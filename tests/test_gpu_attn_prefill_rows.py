"""GPU: the prefill attention kernels (attention.hip launch_attn_prefill: attn_kernel, attn2_kernel, the seven GQA instantiations, head dim 64,
the head split, the one-XCD grid, the peeled last key, key groups) against the fp64 restatement (tests/attn_prefill_ref.py), ROW BY ROW:
    row_rel[b, i, h] = ||out - ref||_2 / ||ref||_2 over the D columns of one (sequence, row, head),   max over everything < gpu_util.TOL[dt]
-- the project's bound for one fused op, applied per row and head, never over a tensor.  A mask wrong by one key at the edge of a 32-query block
or a 64-key tile moves a whole-sequence Frobenius norm by less than that bound; it moves the row it concerns by ~1.  Every case runs three
input families (attn_prefill_ref: `plain`; `leak`, the first hidden key of every row tied to that row; `drop`, the last visible one), both types.
Every row i < Sq of every sequence is compared, except: rows at or beyond kv_len[b] of a sequence with a length (unspecified), and rows without a
visible key (the padded query rows of a left-padded causal sequence), which must be exactly 0.  `out` starts as NaN and one sentinel row behind
the last sequence must stay NaN.

What the bound has to cover and what it must catch, measured on the CPU on exactly these inputs (tests/test_attn_prefill_cpu.py, binding there):
    probabilities and output rounded to T, worst row over all cases     bf16: plain 3.22e-3  leak 3.22e-3  drop 3.17e-3     (bound 1.2e-2)
                                                                        f16:  plain 3.92e-4  leak 3.92e-4  drop 3.90e-4     (bound 2.5e-3)
    mask wrong by one key, smallest row_rel over all witnessing (row, kv head) pairs, either type:
        causal limit + 1   1.15  (leak)        kv_len + 1    1.3e3 (leak)        kv_start - 1   8.8e2 (leak)
        causal limit - 1   0.91  (drop)        kv_len - 1    0.94  (drop)        kv_start + 1   0.99  (drop)        peeled key lost  0.99 (drop)
i.e. rounding takes at most 0.27 of the bound, and every one-key mutant is at least 75 x (bf16) / 360 x (f16) outside it."""
import functools
import pytest
import torch

pytestmark = pytest.mark.gpu
from gpu_util import DT, CODE, TOL, ptr, sync
from omchat_amd import _lib
import attn_prefill_ref as apr

DTS = ["bf16", "f16"]
NAN = float("nan")
# generation, head split, one-XCD grid, key groups, peeled last key
KEY_DEFAULTS = {8: 1, 30: -1, 33: 1, 36: 0, 46: 1}


def i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device="cuda")


class tuning:
    """set tuning keys for a block, restore the defaults whatever happens"""
    def __init__(self, lib, **keys):
        self.lib, self.keys = lib, {int(k[1:]): v for k, v in keys.items()}

    def __enter__(self):
        for k, v in self.keys.items():
            _lib.check(self.lib.omchat_op_set_tuning(k, v))

    def __exit__(self, *exc):
        for k in self.keys:
            self.lib.omchat_op_set_tuning(k, KEY_DEFAULTS[k])


@functools.lru_cache(maxsize=None)
def _reference(name, family, dt):
    """(inputs, fp64 output): computed once per case, family and type, shared, never modified"""
    case = apr.CASES[name]
    inp = apr.case_inputs(name, family, DT[dt])
    ref = apr.attend(inp.q, inp.k, inp.v, apr.case_scale(case), case.causal, case.q_pos0, case.kv_len, case.kv_start)
    assert torch.isfinite(ref).all()
    return inp, ref


def launch(lib, dt, case, inp):
    """one call of the case's entry point on fresh device copies -> out [b * Sq + 1, Hq, D] (the last row is the sentinel)"""
    T, c = DT[dt], case
    out = torch.full((c.b * c.Sq + 1, c.Hq, c.D), NAN, dtype=T, device="cuda")
    dlen, dstart, scale = i32(c.kv_len), i32(c.kv_start), apr.case_scale(c)
    if c.api in ("mha_fwd", "mha_varlen"):
        qkv = apr.pack_qkv(inp.q, inp.k, inp.v).to("cuda", T)
        if c.api == "mha_fwd":
            _lib.check(lib.omchat_mha_fwd(ptr(qkv), c.b, c.Sq, c.Hq, scale, c.causal, ptr(out), CODE[dt], None))
        else:
            _lib.check(lib.omchat_mha_fwd_varlen(ptr(qkv), c.b, c.Sq, c.Hq, c.D, ptr(dlen), scale, c.causal, ptr(out), CODE[dt], None))
    else:
        dq, dk, dv = inp.q.to("cuda", T), inp.k.to("cuda", T), inp.v.to("cuda", T)
        if c.api == "prefill":
            _lib.check(lib.omchat_op_attn_prefill(CODE[dt], ptr(dq), ptr(dk), ptr(dv), ptr(out), c.b, c.Sq, c.Skv, c.Hq, c.Hkv, ptr(dlen), c.causal,
                                                  c.q_pos0, scale, None))
        elif c.api == "prefill_d":
            _lib.check(lib.omchat_op_attn_prefill_d(CODE[dt], ptr(dq), ptr(dk), ptr(dv), ptr(out), c.b, c.Sq, c.Skv, c.Hq, c.Hkv, c.D, ptr(dlen), c.causal,
                                                    c.q_pos0, scale, None))
        else:
            assert c.api == "left"
            _lib.check(lib.omchat_op_attn_prefill_left(CODE[dt], ptr(dq), ptr(dk), ptr(dv), ptr(out), c.b, c.Sq, c.Skv, c.Hq, c.Hkv, ptr(dlen), ptr(dstart),
                                                       c.causal, c.q_pos0, scale, 0, None))
    sync()
    return out


def check(lib, dt, name, family, tag=()):
    """one launch under whatever tuning keys are set, every compared row against the bound -> the output (for same-bits comparisons)"""
    case = apr.CASES[name]
    inp, ref = _reference(name, family, dt)
    out = launch(lib, dt, case, inp)
    where = (name, family, dt) + tuple(tag)
    assert bool(torch.isnan(out[-1].float()).all()), (where, "the row behind the last sequence was written")
    got = out[:-1].view(case.b, case.Sq, case.Hq, case.D).float().cpu()
    assert bool(torch.isfinite(got[inp.compared]).all()), (where, "unwritten or non-finite rows")
    assert bool((got[inp.zero] == 0).all()), (where, "a row without a visible key is not exactly 0")
    rr = apr.row_rel(got, ref)
    rr[~inp.compared] = 0
    b, i, h = (int(x) for x in (rr == rr.max()).nonzero()[0])
    print("attn prefill rows", where, f"worst row_rel {float(rr.max()):.3e} at (sequence, row, head) {(b, i, h)}, bound {TOL[dt]:.1e}")
    assert float(rr.max()) < TOL[dt], (where, "worst (sequence, row, head)", (b, i, h), float(rr.max()))
    return out


FAM = pytest.mark.parametrize("family", apr.FAMILIES)
DTP = pytest.mark.parametrize("dt", DTS)


# ------------------------------------------------------------------------------------------------ 1. GQA, second generation, causal
@DTP
@FAM
@pytest.mark.parametrize("name", ["gqa_7_1_s161", "gqa_4_2_suffix", "gqa_8_1_tile_edges", "gqa_4_2_qpos1", "gqa_4_2_qpos63", "gqa_4_2_qpos64"])
def test_gqa_second_generation(gpu_lib, dt, family, name):
    """attn2_kernel<GQA>: a one-row last query block and a 33-key last tile; the suffix form of omchat_prefill_suffixes (q_pos0 = keep, causal and
    length limits in one tile walk); every limit on a tile edge; q_pos0 just off, just below and on a tile edge"""
    with tuning(gpu_lib, k8=1, k30=-1):
        check(gpu_lib, dt, name, family)


# ------------------------------------------------------------------------------------------------ 2. every GQA instantiation
@DTP
@FAM
@pytest.mark.parametrize("n_rep", range(2, 10))
def test_every_gqa_group_size(gpu_lib, dt, family, n_rep):
    """attn2_kernel<T, NW = n_rep, GQA> for 2..8 query heads per kv head, and 9, which falls back to attn_kernel"""
    with tuning(gpu_lib, k8=1, k30=-1):
        check(gpu_lib, dt, f"nrep{n_rep}", family)


# ------------------------------------------------------------------------------------------------ 3. head split
@DTP
@FAM
def test_head_split_same_bits(gpu_lib, dt, family):
    """key 30: the heaviest causal block ranks issued as two head halves -- off, 4 ranks, 8 ranks (of 17): each per row, and the same bits"""
    outs = []
    for xs in (0, 4, 8):
        with tuning(gpu_lib, k8=1, k30=xs):
            outs.append(check(gpu_lib, dt, "hsplit_7_1_s513", family, ("key 30", xs)))
    for xs, o in zip((4, 8), outs[1:]):
        assert torch.equal(o[:-1].view(torch.int16), outs[0][:-1].view(torch.int16)), (dt, family, "key 30 =", xs, "changes the bits")


# ------------------------------------------------------------------------------------------------ 4. MHA, second generation, not causal
@DTP
@FAM
@pytest.mark.parametrize("name", ["mha_s129", "mha_s129_lens"])
def test_mha_peeled_key_and_grid_forms(gpu_lib, dt, family, name):
    """attn2_kernel<MHA>: 129 and 65 keys take the peeled-key path (key 46 = 1), 128 does not; the one-XCD grid (key 33 = 1) and the
    three-dimensional one.  The drop family ties key kv_len - 1: the peeled key is counted, and once.  Experiments build: two key groups."""
    for peel in (1, 0):
        for xcd in (1, 0):
            with tuning(gpu_lib, k8=1, k46=peel, k33=xcd):
                check(gpu_lib, dt, name, family, ("key 46", peel, "key 33", xcd))
    if gpu_lib.omchat_has_experiments():
        with tuning(gpu_lib, k8=1, k36=2):
            check(gpu_lib, dt, name, family, ("key 36", 2))


# ------------------------------------------------------------------------------------------------ 5. MHA causal
@DTP
@FAM
@pytest.mark.parametrize("name", ["mha_causal_qpos0", "mha_causal_qpos63"])
def test_mha_causal(gpu_lib, dt, family, name):
    """attn2_kernel<MHA> with the causal mask: 128-query blocks of four waves, each wave's own diagonal, q_pos0 off a tile edge"""
    with tuning(gpu_lib, k8=1):
        check(gpu_lib, dt, name, family)


# ------------------------------------------------------------------------------------------------ 6. head dim 64
@DTP
@FAM
@pytest.mark.parametrize("name", ["d64_mha", "d64_mha_causal", "d64_gqa_4_2_causal"])
def test_head_dim_64(gpu_lib, dt, family, name):
    """attn2_kernel<D = 64> (MHA) and attn_kernel<D = 64> (GQA) through omchat_op_attn_prefill_d"""
    with tuning(gpu_lib, k8=1):
        check(gpu_lib, dt, name, family)


# ------------------------------------------------------------------------------------------------ 7. first generation
@DTP
@FAM
@pytest.mark.parametrize("name", ["gqa_7_1_s161", "gqa_4_2_suffix", "mha_causal_qpos0", "mha_causal_qpos63"])
def test_first_generation(gpu_lib, dt, family, name):
    """key 8 = 0: attn_kernel (128-query blocks, 16 x 16 x 32 MFMA) on the shapes of 1 and 5"""
    with tuning(gpu_lib, k8=0):
        check(gpu_lib, dt, name, family, ("key 8", 0))


# ------------------------------------------------------------------------------------------------ 8. left-padded batches
@DTP
@FAM
@pytest.mark.parametrize("gen", [1, 0])
@pytest.mark.parametrize("heads", ["7_1", "3_3"])
def test_left_padded(gpu_lib, dt, family, gen, heads):
    """kv_start just before, on and just after a tile edge, causal and not, alone and with kv_len, both generations: the lower limit is witnessed
    by the key at kv_start - 1 (leak) and the key at kv_start (drop) in the first row that sees a key"""
    with tuning(gpu_lib, k8=gen):
        for mask in ("causal", "full"):
            for lens in ("", "_lens"):
                check(gpu_lib, dt, f"left_{heads}_{mask}{lens}", family, ("key 8", gen))


# ------------------------------------------------------------------------------------------------ 9. packed qkv
@DTP
@FAM
@pytest.mark.parametrize("name", ["packed_mha", "packed_mha_causal", "packed_varlen_d128", "packed_varlen_d128_causal", "packed_varlen_d64",
                                  "packed_varlen_d64_causal"])
def test_packed_qkv(gpu_lib, dt, family, name):
    """omchat_mha_fwd / omchat_mha_fwd_varlen: the same witnesses laid out as [B, S, 3, H, D] (row stride 3 H D for q, k and v alike)"""
    check(gpu_lib, dt, name, family)
