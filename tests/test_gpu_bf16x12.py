"""bf16x12: the device encoder against the reference codec (tests/bf16x12_ref.py), each of the three batch-1 roles
bit-identical to its 16-bit launch, and the decode step with tuning key 50 on and off -- ids and fp32 logits bit-equal, eager and as the
captured graph, across a weight reload, over the patch cap, and next to the e4m3 / MXFP4 modes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from gpu_util import ptr, sync, randn, rnd, synth_state_dict
import bf16x12_ref as ref
from omchat_amd import synth, _lib
from omchat_amd.config import tiny, omchat13b
from omchat_amd.engine import Engine

BF16, EPI_NONE, EPI_RESID, EPI_SWIGLU = _lib.BF16, _lib.EPI_NONE, _lib.EPI_RESID, _lib.EPI_SWIGLU
KEY = 50
HOT = 2.0 ** 17      # what x (or the norm weight) holds at the planted positions: a miss there moves the output by about its own size


def bits_to_dev(w_bits):
    return torch.from_numpy(w_bits.view(np.int16)).cuda().view(torch.bfloat16)


def dev_encode(w_dev):
    lib = _lib.lib()
    N, K = w_dev.shape
    coded = torch.full((N, K * 3 // 2), 0xAA, dtype=torch.uint8, device="cuda")
    top = torch.full((N,), 0xAA, dtype=torch.uint8, device="cuda")
    cnt = torch.full((N,), 0xAA, dtype=torch.uint8, device="cuda")
    patch = torch.full((N, 32), -1, dtype=torch.int32, device="cuda")
    over = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.omchat_op_encode_bf16x12(ptr(w_dev), N, K, ptr(coded), ptr(top), ptr(cnt), ptr(patch), ptr(over), None))
    sync()
    return coded, top, cnt, patch, int(over.item())


PLANTED = 12      # rows 0..11 of planted()


def planted(N, K, seed):
    """random N(0, 0.02^2) rows + the planted rows of the CPU list (rows 0..11).  Returns the bf16 bit patterns, the `hot` positions and the
    (row, k) list of the finite misses.  A finite miss sits JUST below its row's window (e[7:1] = top - 7: 2^-13 .. 2^-12 of the row's
    largest binade) at a hot position, where every planted row is otherwise zero; the role tests put 2^17 at the hot positions of x (of the
    norm weight), so each such miss adds about 0.5 to a dot product of about 1 -- dropped, put into another lane, half-word or chunk, it changes
    output bits, also after the rounding to bf16 (test_role... checks that on the 16-bit launch itself)."""
    w = ref.bf16_bits((np.random.default_rng(seed).standard_normal((N, K)) * 0.02).astype(np.float32))
    filler = (0x3C00 | (np.arange(K) % 128)).astype(np.uint16)       # +2^-7 * [1, 2): top = 60
    w[0] = filler                                                     # no patch at all
    w[5] = filler
    w[6] = 0                                                          # zero row
    w[7] = ((np.arange(K) % 7).astype(np.uint16) << 7) | 0x8015      # top < 7
    w[8] = ref.bf16_bits((np.random.default_rng(seed + 1).standard_normal(K) * 3.0).astype(np.float32))      # another top
    w[9, ::2] = 0x8000                                                # signed zeros among random weights
    k32 = np.arange(32) * (K // 32) + 5                               # (k = 5 is one of them: a patch among the first eight weights)
    plan = {1: [0], 2: [K - 1], 3: [512 + 73, 512 + 78], 4: [167, 168, 175, 176], 5: list(k32)}
    # first k / last k / two in one lane's eight weights / ends of adjacent lanes (lanes 20|21 and 21|22 of chunk 0) / exactly 32 patches
    hot = np.unique(np.concatenate([np.asarray(v) for v in plan.values()]))
    w[:PLANTED, hot] = 0
    misses = []
    for r, ks in plan.items():
        top = int((((w[r] >> 7) & 0xFF) >> 1).max())
        assert top >= 8
        for j, k in enumerate(ks):
            w[r, k] = ((j & 1) << 15) | ((top - 7) << 8) | 0xC0 | (j % 64)      # e[7:1] = top - 7, e[0] = 1
            misses.append((r, int(k)))
    w[10, 171] = 0x7F80                                               # +inf in the middle of a row
    w[11, 5] = 0xFF80      # -inf among the first eight weights: in the long-K form the clamped chunks of the last pass read it in every lane
    #                        against zeros of x -- NaN only if they take the patch too (without it the result stays infinite)
    return w, hot, misses


def test_encoder_equals_reference(gpu_lib):
    w = planted(40, 3584, 1)[0]
    w = np.concatenate([w, planted(12, 3584, 2)[0][:6]])
    w[45, np.arange(33) * 100 + 3] = 0x9E2A                    # a row over the cap
    coded, top, cnt, patch, over = dev_encode(bits_to_dev(w))
    rc, rt, rn, rp, ok = ref.encode(w)
    assert over == 1 and not ok
    assert rn[0] == 0 and rn[5] == 32 and rn[6] == 0 and rn[4] >= 4 and rn[45] == 33      # (random rows carry a miss or two of their own)
    assert np.array_equal(top.cpu().numpy(), rt) and np.array_equal(cnt.cpu().numpy(), rn)
    assert np.array_equal(coded.cpu().numpy(), rc)
    assert np.array_equal(patch.cpu().numpy().view(np.uint32), rp)
    c2, t2, n2, p2, over2 = dev_encode(bits_to_dev(w[:40]))
    assert over2 == 0 and int(n2.max()) == 32
    assert np.array_equal(ref.decode(c2.cpu().numpy(), t2.cpu().numpy(), n2.cpu().numpy(), p2.cpu().numpy().view(np.uint32)), w[:40])


def _role(N, K, epi, seed):
    lib = _lib.lib()
    w, hot, misses = planted(N, K, seed)
    wd = bits_to_dev(w)
    coded, top, cnt, patch, over = dev_encode(wd)
    assert over == 0
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(K, generator=g) * 0.5)
    norm = epi != EPI_RESID
    nw = 1 + 0.1 * torch.randn(K, generator=g)
    sign = torch.from_numpy(np.where(np.arange(len(hot)) % 2 == 0, 1.0, -1.0)).float()
    if norm:
        x[hot] = 0.75 * sign; nw[hot] = HOT             # the normalised row holds about +-1.5 * 2^17 there
    else:
        x[hot] = 0.75 * HOT * sign
    x = x.bfloat16().cuda()
    nw = nw.bfloat16().cuda() if norm else None
    n_y = N // 2 if epi == EPI_SWIGLU else N
    f32 = epi == EPI_NONE
    res = (torch.randn(N, generator=g) * 0.5).bfloat16().cuda() if not norm else None
    it = torch.int32 if f32 else torch.int16

    def run16(wdev):
        y = torch.zeros(n_y, device="cuda", dtype=torch.float32 if f32 else torch.bfloat16)
        if norm:
            _lib.check(lib.omchat_op_gemv_norm(BF16, ptr(x), ptr(wdev), K, ptr(y), N, K, ptr(nw), 1e-6, None, epi, int(f32), None))
        else:
            _lib.check(lib.omchat_op_gemv(BF16, ptr(x), K, ptr(wdev), K, ptr(y), N, 1, N, K, None, ptr(res), N, epi, 0, None))
        sync()
        return y
    y16 = run16(wd)
    y12 = torch.ones_like(y16)
    _lib.check(lib.omchat_op_gemv_bf16x12(ptr(x), ptr(coded), ptr(top), ptr(cnt), ptr(patch), ptr(y12), N, K, ptr(nw), 1e-6, ptr(res), epi,
                                          int(f32), None))
    sync()
    assert torch.equal(y16.view(it), y12.view(it)), (y16.view(it) != y12.view(it)).nonzero().flatten().tolist()[:8]
    # the planted misses are visible: the 16-bit launch itself gives other bits in the row of EACH of them when that one element is dropped
    # (stored as +0, what the coded row holds) or moved by one element, one lane (8 elements) or one chunk
    for r, k in misses[:6] + misses[-2:]:
        for k2 in (None, k ^ 1, (k + 8) % K, (k + 512) % K):
            wv = w.copy()
            wv[r, k] = 0
            if k2 is not None:
                wv[r, k2] = w[r, k]
            yv = run16(bits_to_dev(wv))
            assert int(yv.view(it)[r]) != int(y16.view(it)[r]), (r, k, k2)
    return y16, w


@pytest.mark.parametrize("N,K,epi", [(64, 3584, EPI_SWIGLU), (1000, 3584, EPI_NONE), (48, 18944, EPI_RESID), (48, 8704, EPI_RESID)])
def test_role_bit_identical_to_16_bit(gpu_lib, N, K, epi):
    """gate|up (32 pairs), the lm_head form (N no multiple of the 16 rows of a workgroup), down_proj + residual at the real K and at 17
    chunks (a last pass whose clamped chunks read weights 0..7 in every lane against zeros of x); the outputs are compared as bits, and the
    planted misses are large enough to show in them (planted)"""
    y, w = _role(N, K, epi, 3)
    y = y.float()
    assert bool(torch.isfinite(y[:10]).all()) and bool(torch.isfinite(y[12:]).all())
    assert not bool(torch.isfinite(y[10])) and not bool(torch.isfinite(y[11]))      # the rows with an infinite weight
    if epi == EPI_RESID:
        assert K % 4096 != 0 and bool(torch.isnan(y[11]))      # -inf * x[5], then -inf * 0 in the clamped chunks: NaN, where a lost patch leaves inf


def test_refusals(gpu_lib):
    lib = _lib.lib()
    t = torch.zeros(64 * 1024, dtype=torch.uint8, device="cuda")
    args = lambda K, nw, res, epi: lib.omchat_op_gemv_bf16x12(ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), 4, K, nw, 1e-6, res, epi, 0, None)
    assert args(544, ptr(t), None, EPI_NONE) != 0            # K % 512
    assert args(1024, None, None, EPI_NONE) != 0            # no norm, short K: not one of the three roles
    assert args(1024, None, ptr(t), EPI_RESID) != 0         # the residual form is the long-K one
    assert lib.omchat_op_encode_bf16x12(ptr(t), 4, 544, ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), None) != 0


def _decoder_sd(cfg, seed):
    return {k: v for k, v in synth.state_dict(cfg, seed).items() if not k.startswith(synth.TOWER) and "mm_projector" not in k}


def _steps(e, x, first, n, graph):
    from test_gpu_graph import _run
    e.enable_decode_graph(graph)
    out = _run(e, x, [x.shape[1]], first, n, True)
    e.enable_decode_graph(False)
    return out


def _on_off(e, x, n=24):
    """n steps with the key on and off, eager and captured: ids and fp32 logits bit-equal"""
    lib = _lib.lib()
    first = torch.tensor([5], dtype=torch.int32)
    runs = []
    default = e.bf16x12_stats()["roles"]      # the library's own default: put back afterwards
    try:
        for key in (7, 0):
            lib.omchat_op_set_tuning(KEY, key)
            for graph in (False, True):
                runs.append(_steps(e, x, first, n, graph))
    finally:
        lib.omchat_op_set_tuning(KEY, default)
    for t, l in runs[1:]:
        assert torch.equal(t, runs[0][0]) and torch.equal(l.view(torch.int32), runs[0][1].view(torch.int32))
    return runs[0]


def test_model_tiny_geometry(gpu_lib):
    """hidden 256: no K of the tiny decoder is a multiple of 512, every role stays on 16 bits whatever the key says"""
    cfg = tiny()
    e = Engine(cfg, dtype="bf16", max_seq=256, max_batch=1, vision=False)
    e.load_state_dict(_decoder_sd(cfg, 3))
    _on_off(e, rnd(randn((1, 10, 256), 1, 0.5), "bf16"))
    e.close()


@pytest.fixture(scope="module")
def wide():
    """two decoder layers at the full widths, vocabulary 2048 (the lm_head form at K = 3584)"""
    cfg = omchat13b()
    cfg.text["num_hidden_layers"] = 2
    cfg.text["vocab_size"] = 2048
    sd = synth_state_dict(cfg, 0, lambda k: not k.startswith(synth.TOWER) and "mm_projector" not in k)
    e = Engine(cfg, dtype="bf16", max_seq=256, max_batch=1, vision=False)
    e.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    x = rnd(randn((1, 40, 3584), 1, 0.5), "bf16")
    yield e, sd, x
    e.close()


def test_model_full_width_on_off(gpu_lib, wide):
    e, sd, x = wide
    b0, s0 = e.device_bytes(), e.bf16x12_stats()
    assert s0["roles"] in (5, 7) and s0["launches"] == [0, 0, 0]
    _on_off(e, x)
    It, H, V = 18944, 3584, 2048
    coded = (2 * (2 * It * H + H * It) + V * H) * 3 // 2
    assert e.device_bytes() - b0 >= coded, "the coded copies were not built"
    s1 = e.bf16x12_stats()
    assert s1["coded"] == [2, 2, 1] and s1["roles"] == s0["roles"]
    # the key-on runs took the coded launches (24 eager steps + one capture, 2 layers), the key-off runs none: 16-bit launches count nothing
    assert s1["launches"] == [25 * 2, 25 * 2, 25]


def _one_step(e, x, key):
    """one eager step with tuning key 50 = key; returns the logits and the coded launches it enqueued per role"""
    lib = _lib.lib()
    default, n0 = e.bf16x12_stats()["roles"], e.bf16x12_stats()["launches"]
    try:
        lib.omchat_op_set_tuning(KEY, key)
        e.prefill(x)
        _, lg = e.decode_step(torch.tensor([5]), want_logits=True)
        sync()
    finally:
        lib.omchat_op_set_tuning(KEY, default)
    return lg[0].clone(), [a - b for a, b in zip(e.bf16x12_stats()["launches"], n0)]


def test_reload_and_patch_cap(gpu_lib, wide):
    e, sd, x = wide
    i32 = lambda t: t.view(torch.int32)
    before, n = _one_step(e, x, 7)
    assert n == [2, 2, 1]
    key = "model.layers.1.mlp.down_proj.weight"
    w2 = rnd(randn(tuple(sd[key].shape), 9, 0.05), "bf16")
    e.load_tensor(key, w2)                                    # stale: the next step re-encodes in place
    (a, na), (b, nb) = _one_step(e, x, 7), _one_step(e, x, 0)
    assert na == [2, 2, 1] and nb == [0, 0, 0]
    assert torch.equal(i32(a), i32(b)) and not torch.equal(a, before)
    w3 = w2.clone()
    w3[17, torch.arange(33) * 500 + 3] = 1e-30                # 33 misses in one row: this tensor is not coded ...
    e.load_tensor(key, w3)
    (a, na), (b, nb) = _one_step(e, x, 7), _one_step(e, x, 0)
    assert na == [2, 1, 1], na                                # ... its projection took the 16-bit launch, layer 0's the coded one
    assert e.bf16x12_stats()["coded"] == [2, 1, 1]
    assert torch.equal(i32(a), i32(b))
    e.load_tensor(key, torch.from_numpy(sd[key]))             # and back under the cap
    a, na = _one_step(e, x, 7)
    assert na == [2, 2, 1] and e.bf16x12_stats()["coded"] == [2, 2, 1]
    assert torch.equal(i32(a), i32(before))


def test_quantised_modes_take_their_own_launches(gpu_lib, wide):
    e, sd, x = wide
    l16, n = _one_step(e, x, 7)
    assert n == [2, 2, 1]
    for enable in (e.enable_fp8_decode, e.enable_mxfp4_decode):
        enable(True)
        (on, n_on), (off, _) = _one_step(e, x, 7), _one_step(e, x, 0)
        enable(False)
        assert n_on == [0, 0, 0]
        assert torch.equal(on.view(torch.int32), off.view(torch.int32)) and not torch.equal(on, l16)
    again, n = _one_step(e, x, 7)
    assert n == [2, 2, 1] and torch.equal(again.view(torch.int32), l16.view(torch.int32))
