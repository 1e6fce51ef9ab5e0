"""GPU: the 16-bit decode attention WITH its fused RoPE + append live (launch_attn_decode, rope != null: the launch every decoder layer issues per
token), through the test hook omchat_op_attn_decode_append -- the one-tile kernel and its masked instantiation (attn_common.h attn_decode_tile),
attn_decode_multi_kernel<KLDS = false | true>, attn_decode_dma_kernel<NST = 2 | 3 | 4>, the merge's packed output.  Every case:
  1. the cache bytes after the call are omchat_op_rope_kv_pos's on a clone (same rows, same positions), every other slot untouched, NaN poison included;
  2. the output against the fp64 restatement (tests/decode_append_ref.py, itself checked by tests/test_decode_append_cpu.py), per (sequence, head);
  3. the output, bit for bit, against omchat_op_attn_decode under the same tuning keys on the cache and q that rope_kv_pos completed / rotated.
Every slot from the one being written on is NaN before the call, and so are `out` and the workspace.

The bound of (2) is gpu_util.TOL (one fused op) per HEAD, not over the tensor.  What rounding the operands alone costs on these inputs, measured
on the CPU (test_decode_append_cpu.py::test_operand_rounding_stays_under_half_the_bound), worst (sequence, head) over all cases below:
    probabilities rounded to T before the PV product:   bf16 2.08e-3   f16 2.71e-4
    ... and q / fresh k rotated with rope_chunk's 16-bit roundings:  bf16 5.67e-3   f16 8.95e-4
against TOL = 1.2e-2 / 2.5e-3: at most half of the bound in both types."""
import functools
import pytest
import torch

pytestmark = pytest.mark.gpu
from gpu_util import DT, CODE, TOL, ptr, sync
from omchat_amd import _lib
import decode_append_ref as dar

DTS = ["bf16", "f16"]
NAN = float("nan")
THETA = 1e6
SCALE = 128 ** -0.5
KEY_DEFAULTS = {10: 0, 12: 0, 25: 1, 26: 0}      # tiles per wave, K through LDS, ring form, ring slots | stages << 8


def i32(v):
    return torch.as_tensor(v, dtype=torch.int32).to("cuda")


def bits(t):
    return t.view(torch.int16)


@functools.lru_cache(maxsize=None)
def _reference(name, dt):
    """(inputs with the poison in place, mask, positions, fp64 output): computed once per case and type, shared, never modified"""
    T = DT[dt]
    b, Hq, Hkv, cap, L, _ = dar.SHAPES[name]
    qkv, k, v, lens = dar.case_inputs(name, T)
    mask, mpos = dar.masked_case_mask() if name == "masked" else (None, None)
    pos = mpos if mask is not None else torch.tensor(lens, dtype=torch.int32) - 1
    for i, n in enumerate(lens):      # the slot to be written and everything behind it; the keys a mask hides stay finite
        k[i, :, n - 1:] = NAN; v[i, :, n - 1:] = NAN
    ref, _, _, _ = dar.decode_append(qkv, k, v, Hq, Hkv, lens, pos, THETA, SCALE, T, mask)
    assert torch.isfinite(ref).all()
    return qkv.to(T), k.to(T), v.to(T), lens, mask, pos, ref


class Case:
    def __init__(self, lib, dt, name, uniform):
        self.lib, self.dt, self.name, self.T = lib, dt, name, DT[dt]
        self.b, self.Hq, self.Hkv, self.cap, self.L, shape_lens = dar.SHAPES[name]
        assert uniform == (shape_lens is None), name
        self.qkv, self.k, self.v, self.lens, self.mask, self.pos, self.ref = _reference(name, dt)
        self.dqkv = self.qkv.cuda()
        self.dlens = None if uniform else i32(self.lens)
        self.dpos = i32(self.pos)
        # visible keys are "!= 0", not "== 1"
        self.dmask = None if self.mask is None else (self.mask * torch.tensor([1, 2, 128, 255], dtype=torch.uint8).repeat(dar.MASK_SB // 4)).cuda()
        self.wsb = lib.omchat_op_attn_decode_ws(self.b, self.Hq, self.L)

    def workspace(self):
        return torch.full((self.wsb // 4 + 4,), NAN, dtype=torch.float32, device="cuda")

    def fused(self, pack_nb=0):
        """the hook on a fresh copy of the poisoned cache -> (out, k, v)"""
        dk, dv = self.k.cuda(), self.v.cuda()
        n_out = pack_nb * 16 * self.Hq * 128 if pack_nb else self.b * self.Hq * 128
        out = torch.full((n_out,), NAN, dtype=self.T, device="cuda")
        ws = self.workspace()
        _lib.check(self.lib.omchat_op_attn_decode_append(CODE[self.dt], ptr(self.dqkv), THETA, ptr(dk), ptr(dv), ptr(out), self.b, self.Hq, self.Hkv, self.cap,
                                                         self.L, ptr(self.dlens), ptr(self.dpos) if self.dmask is not None else None, ptr(self.dmask),
                                                         dar.MASK_SB if self.dmask is not None else 0, pack_nb, SCALE, ptr(ws), self.wsb, None))
        sync()
        assert torch.equal(bits(self.dqkv.cpu()), bits(self.qkv)), (self.name, "the raw projections were modified")
        return (out if pack_nb else out.view(self.b, self.Hq, 128)), dk, dv

    def unfused(self):
        """rope_kv_kernel on clones (positions = the fused launch's, slot0 = -1, masked: the slot L - 1) -> (rotated q [b, Hq, 128], k, v)"""
        dq, dk, dv = self.dqkv.clone(), self.k.cuda(), self.v.cuda()
        slot0 = self.L - 1 if self.dmask is not None else -1
        _lib.check(self.lib.omchat_op_rope_kv_pos(CODE[self.dt], ptr(dq), self.b, 1, self.Hq, self.Hkv, ptr(self.dpos), 0, slot0, self.L, THETA, ptr(dk),
                                                  ptr(dv), self.cap, None))
        sync()
        return dq.view(self.b, self.Hq + 2 * self.Hkv, 128)[:, :self.Hq].contiguous(), dk, dv

    def check(self, tag):
        out, dk, dv = self.fused()
        qr, kr, vr = self.unfused()
        # ---- 1. cache bytes
        assert torch.equal(bits(dk), bits(kr)), (tag, "k cache differs from rope_kv's bytes")
        assert torch.equal(bits(dv), bits(vr)), (tag, "v cache differs from rope_kv's bytes")
        want_k, want_v = self.k.clone(), self.v.clone()
        kc, vc = dk.cpu(), dv.cpu()
        for i, n in enumerate(self.lens):
            assert torch.isfinite(kc[i, :, n - 1].float()).all() and torch.isfinite(vc[i, :, n - 1].float()).all(), (tag, i, "the new rows were not written")
            want_k[i, :, n - 1] = kc[i, :, n - 1]; want_v[i, :, n - 1] = vc[i, :, n - 1]
        assert torch.equal(bits(kc), bits(want_k)) and torch.equal(bits(vc), bits(want_v)), (tag, "a slot other than the new one changed")
        # ---- 2. output against fp64, per (sequence, head)
        assert torch.isfinite(out.float()).all(), (tag, "unwritten or non-finite output")
        err = dar.rel_heads(out, self.ref)
        print("decode append", tag, "worst (sequence, head) rel", float(err.max()), "bound", TOL[self.dt])
        assert float(err.max()) < TOL[self.dt], (tag, err)
        # ---- 3. the unfused pair under the same tuning keys: the same operand bits, the same output bits
        if self.dmask is None:
            plain = torch.full((self.b, self.Hq, 128), NAN, dtype=self.T, device="cuda")
            ws = self.workspace()
            _lib.check(self.lib.omchat_op_attn_decode(CODE[self.dt], ptr(qr), ptr(kr), ptr(vr), ptr(plain), self.b, self.Hq, self.Hkv, self.cap, self.L,
                                                      ptr(self.dlens), SCALE, ptr(ws), self.wsb, None))
            sync()
            assert torch.equal(bits(out), bits(plain)), (tag, "fused and unfused outputs differ", float(dar.rel_heads(out, plain.float()).max()))
        return out


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


# ------------------------------------------------------------------------------------------------ one-tile kernel
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", ["one_tile_ragged_8_2", "one_tile_ragged_7_1", "one_tile_ragged_4_2", "one_tile_ragged_2_2"])
def test_one_tile_kernel_ragged(gpu_lib, dt, name):
    """attn_decode_tile with a kv_len array: the empty cache (pp == 0: every tile row is the fresh one, the cached-row read clamped to row 0), two
    keys, the new row last in a tile (63 / 127) and first in the next (64), rows beyond kv_len clamped onto the fresh row; GQA groups 4, 7, 2, 1"""
    with tuning(gpu_lib, k10=1, k25=0):
        Case(gpu_lib, dt, name, uniform=False).check((dt, name))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", ["one_tile_L1", "one_tile_L64", "one_tile_L65"])
def test_one_tile_kernel_uniform_length(gpu_lib, dt, name):
    """the same launch with kv_len = NULL (every sequence holds L keys)"""
    with tuning(gpu_lib, k10=1, k25=0):
        Case(gpu_lib, dt, name, uniform=True).check((dt, name))


# ------------------------------------------------------------------------------------------------ register multi-tile kernel
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("klds", [0, 1])
@pytest.mark.parametrize("name,tpw,uniform", [("multi4_ragged", 4, False), ("multi2_ragged", 2, False), ("multi4_uniform", 4, True)])
def test_multi_tile_kernel(gpu_lib, dt, klds, name, tpw, uniform):
    """attn_decode_multi_kernel, K in registers (key 12 = 0: partner fragment ds ^ 2) and through LDS (key 12 = 1: partner lane ^ 8): the owner in
    the first tile of a split, in its last tile, in the second split's first tile, in a split whose tile loop ends early"""
    with tuning(gpu_lib, k10=tpw, k12=klds, k25=0):
        Case(gpu_lib, dt, name, uniform).check((dt, name, "klds", klds))


# ------------------------------------------------------------------------------------------------ ring form
def ring_plan(b, Hkv, L, key26, cus):
    """(nsplit, 32-key tiles per split, ring stages) as launch_attn_decode plans the ring form with the slot count forced (key 26's low byte != 0)"""
    slots, st = (key26 & 255) * cus, (key26 >> 8) & 255
    tiles = -(-L // 32)
    tpw = max(2, -(-tiles // max(1, slots // (Hkv * b))))
    return -(-L // (32 * tpw)), tpw, min(max(st, 2), 4)


RING_KEYS = [4, 1, 64, (3 << 8) | 1, (4 << 8) | 1]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key26", RING_KEYS)
def test_ring_kernel_ragged(gpu_lib, dt, key26):
    """attn_decode_dma_kernel<2 | 3 | 4>: the new position on the last row of a 32-key tile (31, 511), on the first (32, 96), alone in the cache;
    the rotated key patched into the LDS image of stage 0 and of stage 1"""
    with tuning(gpu_lib, k10=4, k25=1, k26=key26):
        Case(gpu_lib, dt, "ring_ragged", uniform=False).check((dt, "ring_ragged", "key 26", key26))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("key26", [1, (3 << 8) | 1, (4 << 8) | 1])
def test_ring_kernel_after_the_ring_has_wrapped(gpu_lib, dt, key26):
    """one slot per CU: several 32-key tiles per split, so the owning tile (the last) arrives in a stage that was refilled, other than stage 0"""
    b, Hq, Hkv, cap, L, _ = dar.SHAPES["ring_wrap"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nsplit, tpw, stages = ring_plan(b, Hkv, L, key26, cus)
    last = -(-(L - (nsplit - 1) * 32 * tpw) // 32)      # tiles the owning (last) split walks
    print("ring plan", (dt, key26), "CUs", cus, "(nsplit, tiles per split)", (nsplit, tpw), "stages", stages, "owner tile", last - 1, "in stage", (last - 1) % stages)
    assert tpw > stages and last > stages and (last - 1) % stages != 0, "this device's plan does not wrap the ring: the case has to change"
    with tuning(gpu_lib, k10=4, k25=1, k26=key26):
        Case(gpu_lib, dt, "ring_wrap", uniform=True).check((dt, "ring_wrap", "key 26", key26))


# ------------------------------------------------------------------------------------------------ automatic plan
@pytest.mark.parametrize("dt", DTS)
def test_automatic_plan_batch_1(gpu_lib, dt):
    """every key at its default: 28 / 4 heads over 4161 keys = 66 one-tile splits, the owner is the last one (its tile holds the new key alone)
    and the merge takes its 65..256-split form"""
    for k, v in KEY_DEFAULTS.items():
        gpu_lib.omchat_op_set_tuning(k, v)
    Case(gpu_lib, dt, "auto_66_splits", uniform=True).check((dt, "auto_66_splits"))


# ------------------------------------------------------------------------------------------------ masked form
@pytest.mark.parametrize("dt", DTS)
def test_masked_form(gpu_lib, dt):
    """attn_decode_tile<MASKED>: left pads that hide part of a tile, one whole tile and two (their splits report m = NEG_BIG, l = 64, which the
    merge has to weight to zero), holes in the middle of a row, mask bytes of several non-zero values, the RoPE position pos[i] = sum(mask) - 1
    apart from the slot L - 1.  There is no unfused masked launch over the 16-bit cache: assertions 1 and 2."""
    Case(gpu_lib, dt, "masked", uniform=True).check((dt, "masked"))


# ------------------------------------------------------------------------------------------------ packed output
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name,nb", [("packed_nb1", 1), ("packed_nb2", 2)])
def test_packed_output(gpu_lib, dt, name, nb):
    """o_pack_nb: the merge writes the packed x layout the batched o_proj GEMV reads; unpacked it is the row-major output of the same call, bit
    for bit, and nothing else of the buffer is written"""
    with tuning(gpu_lib, k10=1, k25=0):
        c = Case(gpu_lib, dt, name, uniform=False)
        plain = c.check((dt, name))
        packed, dk, dv = c.fused(pack_nb=nb)
        _, kr, vr = c.unfused()
    assert torch.equal(bits(dk), bits(kr)) and torch.equal(bits(dv), bits(vr))
    got = dar.unpack_x(packed.cpu(), c.b, c.Hq * 128, nb).view(c.b, c.Hq, 128)
    assert torch.equal(bits(got), bits(plain.cpu())), (dt, name)
    assert int(torch.isfinite(packed.float()).sum()) == c.b * c.Hq * 128


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("dt", DTS)
def test_refusals_launch_nothing(gpu_lib, dt):
    c = Case(gpu_lib, dt, "masked", uniform=True)
    dk, dv = c.k.cuda(), c.v.cuda()
    out = torch.full((c.b, c.Hq, 128), NAN, dtype=c.T, device="cuda")
    ws = c.workspace()
    some_lens = i32(c.lens)
    good = dict(qkv=ptr(c.dqkv), k=ptr(dk), v=ptr(dv), out=ptr(out), ws=ptr(ws), cap=c.cap, L=c.L, kv_len=None, pos=None, mask=None)

    def call(**kw):
        a = dict(good, **kw)
        return gpu_lib.omchat_op_attn_decode_append(CODE[dt], a["qkv"], THETA, a["k"], a["v"], a["out"], c.b, c.Hq, c.Hkv, a["cap"], a["L"], a["kv_len"],
                                                    a["pos"], a["mask"], dar.MASK_SB, 0, SCALE, a["ws"], c.wsb, None)

    for kw in (dict(qkv=None), dict(k=None), dict(v=None), dict(out=None), dict(ws=None), dict(L=0), dict(L=c.cap + 1),
               dict(mask=ptr(c.dmask)), dict(mask=ptr(c.dmask), pos=ptr(c.dpos), kv_len=ptr(some_lens))):
        with pytest.raises(ValueError):
            _lib.check(call(**kw))
    sync()
    assert bool(torch.isnan(out.float()).all()) and bool(torch.isnan(ws).all())
    assert torch.equal(bits(dk.cpu()), bits(c.k)) and torch.equal(bits(dv.cpu()), bits(c.v))
