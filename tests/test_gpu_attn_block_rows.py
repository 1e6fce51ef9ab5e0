"""GPU: attn_verify_kernel in its four modes behind launch_attn_block (ATTN_VERIFY, ATTN_EXTEND, ATTN_SHARED, ATTN_SUFFIX) against the fp64
restatement of tests/attn_block_ref.py, per (query row, head): every defined (row, head) of every case x witness family x type is held to
gpu_util.TOL -- no whole-tensor ratio, no row norm over the heads.  The cases are the smallest that reach each branch (attn_block_ref.CASES:
both wave counts, loader-only waves, every L % 64 and P % 64 edge, splits of two tiles in all four modes and in the suffix walk); the plan hook
omchat_op_attn_block_plan reports that a case ran the branch it was chosen for.  In the drop family one dropped boundary key, in the leak family
one leaked hidden key misses its witness head by O(1) (tests/test_attn_block_cpu.py measures every one-slot mutant on these very inputs).

The two modes with a fused RoPE + append run in BOTH forms: fused through omchat_op_attn_verify_append / omchat_op_attn_shared_append (the
launch omchat_decode_step and omchat_decode_verify issue) and unfused on the caches that omchat_op_rope_kv / omchat_op_rope_kv_pos completed.
The fused launch must leave exactly those cache bytes and touch no other; both outputs are held to the bound against fp64 on those bytes.

What rounding the operands alone costs on these inputs (test_attn_block_cpu.py::test_operand_rounding_stays_under_half_the_bound), worst
(row, head) over all cases and families: bf16 3.11e-3, f16 3.89e-4 against bounds of 1.2e-2 and 2.5e-3."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
import attn_block_ref as abr
from gpu_util import CODE, DT, TOL, ptr, sync
from omchat_amd import _lib

DTS = ("bf16", "f16")
NAN = float("nan")


def _bits(t):
    return t.view(torch.int16)


def _nan(*shape, dt=torch.float32):
    return torch.full(shape, NAN, dtype=dt, device="cuda")


def _device_plan(lib, case):
    out = (C.c_int * 4)()
    _lib.check(lib.omchat_op_attn_block_plan(case.mode, case.G, case.N, case.S, case.Hq, case.Hkv, case.P, case.L, C.cast(out, C.c_void_p)))
    return dict(zip(("tpw", "nsp", "nss", "tps"), out))


def _check_plan(lib, case):
    """the branch the case was chosen for, as the launcher itself plans it on this device"""
    got = _device_plan(lib, case)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != abr.CUS:
        print(f"{case.name}: plan {got} on {cus} CUs; the table is derived for {abr.CUS} CUs -- branch assertion not made")
        return got
    assert got == abr.plan_of(case), (case.name, got, abr.plan_of(case))
    for field, least in case.want:
        assert got[field] >= least, (case.name, got)
    if case.want:
        print(f"{case.name}: ran the multi-tile branch, plan {got}")
    return got


def _hold(tag, out, ref, inp, dt):
    """every defined (row, head) under the bound; the others finite"""
    assert torch.isfinite(out.float()).all(), tag
    rr = abr.row_rel(out.float(), ref)
    worst = float(rr[inp.compared].max())
    r, h = divmod(int(rr.masked_fill(~inp.compared[:, None], -1.0).argmax()), rr.shape[1])
    print(f"{tag}: worst (row, head) = ({r}, {h}) row_rel {worst:.3e}  bound {TOL[dt]:.1e}")
    assert worst < TOL[dt], (tag, "row, head", (r, h), worst)


def _ws(nbytes):
    assert nbytes > 0
    return _nan(nbytes // 4 + 64)


# ---------------------------------------------------------------------------------------------------------------- the four modes
def _run_verify(lib, case, inp, dt):
    T, Hq, Hkv, L, cap = case.S, case.Hq, case.Hkv, case.L, abr.cap_of(case)
    code, up = CODE[dt], lambda x: x.to("cuda", DT[dt]).contiguous()
    qkv, k0, v0 = up(inp.qkv), up(inp.k0[0]), up(inp.v0[0])
    ws_b = lib.omchat_op_attn_decode_ws(T, Hq, L + T)
    # the bytes of the separate RoPE + append launch
    qkv_r, kr, vr = qkv.clone(), k0.clone(), v0.clone()
    _lib.check(lib.omchat_op_rope_kv(code, ptr(qkv_r), 1, T, Hq, Hkv, L, abr.THETA, ptr(kr), ptr(vr), cap, None))
    sync()
    q = qkv_r[:, :Hq * 128].reshape(T, Hq, 128).contiguous()
    new = torch.zeros(cap, dtype=torch.bool, device="cuda"); new[L:L + T] = True
    assert torch.equal(_bits(kr[:, ~new]), _bits(k0[:, ~new])) and torch.equal(_bits(vr[:, ~new]), _bits(v0[:, ~new]))
    assert torch.equal(_bits(q), _bits(up(inp.q))) and torch.equal(_bits(kr), _bits(up(inp.k[0]))), "the inputs are not the ones the CPU test calibrated"
    # fused
    kf, vf, out_f, ws = k0.clone(), v0.clone(), _nan(T, Hq, 128, dt=DT[dt]), _ws(ws_b)
    _lib.check(lib.omchat_op_attn_verify_append(code, ptr(qkv), abr.THETA, ptr(kf), ptr(vf), ptr(out_f), T, Hq, Hkv, cap, L, abr.SCALE, ptr(ws), ws_b, None))
    sync()
    assert torch.equal(_bits(kf), _bits(kr)) and torch.equal(_bits(vf), _bits(vr)), "appended bytes / untouched slots"
    assert torch.equal(_bits(qkv), _bits(up(inp.qkv))), "qkv is read-only"
    # unfused
    out_u, ws = _nan(T, Hq, 128, dt=DT[dt]), _ws(ws_b)
    _lib.check(lib.omchat_op_attn_verify(code, ptr(q), ptr(kr), ptr(vr), ptr(out_u), T, Hq, Hkv, cap, L, abr.SCALE, ptr(ws), ws_b, None))
    sync()
    ref = abr.attend(q.float(), kr[None].float(), vr[None].float(), inp.vis)
    return {"fused": out_f, "unfused": out_u}, ref


def _run_extend(lib, case, inp, dt):
    Sq, Hq, Hkv, L, cap = case.S, case.Hq, case.Hkv, case.L, abr.cap_of(case)
    up = lambda x: x.to("cuda", DT[dt]).contiguous()
    q, k, v = up(inp.q), up(inp.k[0]), up(inp.v[0])
    ws_b = lib.omchat_op_attn_extend_ws(Sq, Hq, Hkv, L)
    out, ws = _nan(Sq, Hq, 128, dt=DT[dt]), _ws(ws_b)
    _lib.check(lib.omchat_op_attn_extend(CODE[dt], ptr(q), ptr(k), ptr(v), ptr(out), Sq, Hq, Hkv, cap, L, abr.SCALE, ptr(ws), ws_b, None))
    sync()
    return {"extend": out}, abr.attend(q.float(), k[None].float(), v[None].float(), inp.vis)


def _run_suffix(lib, case, inp, dt):
    N, S, Hq, Hkv, P, cap = case.N, case.S, case.Hq, case.Hkv, case.P, abr.cap_of(case)
    up = lambda x: x.to("cuda", DT[dt]).contiguous()
    q, k, v = up(inp.q), up(inp.k), up(inp.v)
    ws_b = lib.omchat_op_attn_suffix_ws(N, S, Hq, Hkv, P)
    out, ws = _nan(N * S, Hq, 128, dt=DT[dt]), _ws(ws_b)
    lens = torch.tensor(case.lens, dtype=torch.int32)
    scratch = torch.zeros(N, dtype=torch.int32, device="cuda")
    _lib.check(lib.omchat_op_attn_suffix(CODE[dt], ptr(q), ptr(k), ptr(v), ptr(out), N, S, Hq, Hkv, cap, P, ptr(lens), ptr(scratch), abr.SCALE,
                                         ptr(ws), ws_b, None))
    sync()
    assert scratch.tolist() == [P + n for n in case.lens]
    return {"suffix": out}, abr.attend(q.float(), k.float(), v.float(), inp.vis)


def _run_shared(lib, case, inp, dt):
    G, N, Hq, Hkv, P, L, cap = case.G, case.N, case.Hq, case.Hkv, case.P, case.L, abr.cap_of(case)
    R = G * N
    code, up = CODE[dt], lambda x: x.to("cuda", DT[dt]).contiguous()
    qkv, k0, v0 = up(inp.qkv), up(inp.k0), up(inp.v0)
    lens = abr.row_lens(case)
    dlen = torch.tensor(lens, dtype=torch.int32, device="cuda")
    # the bytes of the separate RoPE + append launch: per-row position len - 1, slot = position
    qkv_r, kr, vr = qkv.clone(), k0.clone(), v0.clone()
    dpos = dlen - 1
    _lib.check(lib.omchat_op_rope_kv_pos(code, ptr(qkv_r), R, 1, Hq, Hkv, ptr(dpos), 0, -1, L, abr.THETA, ptr(kr), ptr(vr), cap, None))
    sync()
    q = qkv_r[:, :Hq * 128].reshape(R, Hq, 128).contiguous()
    new = torch.zeros(R, cap, dtype=torch.bool, device="cuda"); new[torch.arange(R, device="cuda"), dpos.long()] = True
    old = ~new[:, None, :].expand(R, Hkv, cap)
    assert torch.equal(_bits(kr)[old], _bits(k0)[old]) and torch.equal(_bits(vr)[old], _bits(v0)[old])
    assert torch.equal(_bits(q), _bits(up(inp.q))) and torch.equal(_bits(kr), _bits(up(inp.k))), "the inputs are not the ones the CPU test calibrated"

    def fused(Lg, kv_len):
        kf, vf, out, ws_b = k0.clone(), v0.clone(), _nan(R, Hq, 128, dt=DT[dt]), lib.omchat_op_attn_shared_ws(G, N, Hq, Hkv, P, Lg)
        ws = _ws(ws_b)
        _lib.check(lib.omchat_op_attn_shared_append(code, ptr(qkv), abr.THETA, ptr(kf), ptr(vf), ptr(out), G, N, Hq, Hkv, cap, P, Lg, ptr(kv_len),
                                                    abr.SCALE, ptr(ws), ws_b, None))
        sync()
        assert torch.equal(_bits(kf), _bits(kr)) and torch.equal(_bits(vf), _bits(vr)), ("appended bytes / untouched slots", Lg)
        return out

    def unfused(Lg, kv_len):
        out, ws_b = _nan(R, Hq, 128, dt=DT[dt]), lib.omchat_op_attn_shared_ws(G, N, Hq, Hkv, P, Lg)
        ws = _ws(ws_b)
        if kv_len is None:
            _lib.check(lib.omchat_op_attn_shared(code, ptr(q), ptr(kr), ptr(vr), ptr(out), G, N, Hq, Hkv, cap, P, Lg, abr.SCALE, ptr(ws), ws_b, None))
        else:
            _lib.check(lib.omchat_op_attn_shared_lens(code, ptr(q), ptr(kr), ptr(vr), ptr(out), G, N, Hq, Hkv, cap, P, Lg, ptr(kv_len), abr.SCALE,
                                                      ptr(ws), ws_b, None))
        sync()
        return out

    kv_len = None if case.lens is None else dlen
    outs = {"fused": fused(L, kv_len), "unfused": unfused(L, kv_len)}
    for form, run in (("fused", fused), ("unfused", unfused)):
        if case.lens is None:      # equal lengths give the bits of the no-lengths form
            assert torch.equal(_bits(run(L, dlen)), _bits(outs[form])), (form, "equal lengths")
        # a grid sized for a longer L: the extra suffix splits are neutral
        assert torch.equal(_bits(run(L + 70, dlen)), _bits(outs[form])), (form, "a grid sized for L + 70")
    assert torch.equal(_bits(qkv), _bits(up(inp.qkv))), "qkv is read-only"
    return outs, abr.attend(q.float(), kr.float(), vr.float(), inp.vis)


RUN = {abr.VERIFY: _run_verify, abr.EXTEND: _run_extend, abr.SHARED: _run_shared, abr.SUFFIX: _run_suffix}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family", abr.FAMILIES)
@pytest.mark.parametrize("name", list(abr.CASES))
def test_every_row_and_head_against_fp64(gpu_lib, name, family, dt):
    case = abr.CASES[name]
    _check_plan(gpu_lib, case)
    inp = abr.case_inputs(name, family, DT[dt])
    outs, ref = RUN[case.mode](gpu_lib, case, inp, dt)
    for form, out in outs.items():
        _hold(f"{name} {family} {dt} {form}", out, ref, inp, dt)


def test_plan_hook_is_pure_and_refuses_bad_arguments(gpu_lib):
    """every case's plan through the hook (the multi-tile ones report their branch), twice the same; a bad mode, no heads or no output are refused"""
    for case in abr.CASES.values():
        assert _check_plan(gpu_lib, case) == _device_plan(gpu_lib, case)
    out = (C.c_int * 4)()
    p = C.cast(out, C.c_void_p)
    assert gpu_lib.omchat_op_attn_block_plan(4, 1, 1, 1, 4, 2, 1, 2, p) != 0
    assert gpu_lib.omchat_op_attn_block_plan(-1, 1, 1, 1, 4, 2, 1, 2, p) != 0
    assert gpu_lib.omchat_op_attn_block_plan(0, 1, 1, 1, 4, 0, 1, 2, p) != 0
    assert gpu_lib.omchat_op_attn_block_plan(0, 1, 1, 1, 4, 2, 1, 2, None) != 0


def test_shared_append_refuses_bad_geometry(gpu_lib):
    qkv = torch.zeros(34, (28 + 8) * 128, dtype=torch.bfloat16, device="cuda")
    k = torch.zeros(34, 4, 16, 128, dtype=torch.bfloat16, device="cuda")
    v = torch.zeros_like(k)
    out = torch.zeros(34, 28, 128, dtype=torch.bfloat16, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    call = lambda G, N, P, L, ws_b=1 << 22, kp=k: gpu_lib.omchat_op_attn_shared_append(CODE["bf16"], ptr(qkv), 1e6, ptr(kp), ptr(v), ptr(out), G, N, 28, 4, 16,
                                                                                        P, L, None, 0.1, ptr(ws), ws_b, None)
    assert call(2, 17, 4, 8) != 0            # N > 16
    assert call(1, 2, 4, 4) != 0             # no own key
    assert call(1, 2, 0, 4) != 0             # no prompt
    assert call(1, 2, 4, 17) != 0            # beyond the capacity
    assert call(1, 2, 4, 8, ws_b=64) != 0    # workspace
    assert call(1, 2, 4, 8, kp=None) != 0    # null cache
    assert not k.any() and not v.any()       # a refused call writes nothing
    assert call(1, 2, 4, 8) == 0
    sync()
