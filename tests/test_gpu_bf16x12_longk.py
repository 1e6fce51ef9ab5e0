"""The long-K bf16x12 launch (down_proj + residual) against the 16-bit long-K launch, as bits: at the ends of the
accepted K range, where the two forms' pass lengths disagree about the clamped chunks, on the real grid of seven waves per workgroup,
and in a decode step with tuning key 50 = 7 against 0.  The coded form runs passes of another length than the 16-bit form's eight
chunks; its term set must still be the 16-bit form's ceil8(chunks), which is what the K = 6144 and K = 8192 cases look at."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from gpu_util import ptr, sync, randn, rnd, synth_state_dict
from omchat_amd import synth, _lib
from omchat_amd.config import tiny
from omchat_amd.engine import Engine

BF16, EPI_RESID = _lib.BF16, _lib.EPI_RESID
KEY = 50
HOT = 2.0 ** 17      # what x holds at the planted positions: a miss there moves the output by about its own size
PLANTED = 15         # rows 0..14 of planted()


def _top(row):
    return int(((row >> 8) & 0x7F).max())


def planted(N, K, seed):
    """random N(0, 0.02^2) rows on the device + the planted rows 0..14 (for N = 3584 also the first and the last row of the last
    workgroup).  Returns the bf16 bit patterns (int16, device), the `hot` positions and the (row, k) list of the planted misses.  A miss
    sits JUST below its row's window (e[7:1] = top - 7) at a hot position, where every planted row is otherwise zero; x holds 0.75 * 2^17
    there, so each miss adds about 0.5 to a dot product of about 1: dropped or put into another lane, half-word or chunk, it changes output
    bits (test_misses_are_visible checks that on the 16-bit launch itself)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).bfloat16().view(torch.int16)
    nch = K // 512
    first, mid, last = 0, (nch // 2) * 512, (nch - 1) * 512
    filler = (0x3C00 | (np.arange(K) % 128)).astype(np.uint16)       # +2^-7 * [1, 2): top = 60
    rows = {r: filler.copy() for r in (0, 1, 2, 3, 4, 5, 6, 7, 12)}  # rows 0 and 12: no patch at all
    rng = np.random.default_rng(seed + 1)
    rows[8] = (torch.from_numpy((rng.standard_normal(K) * 3.0).astype(np.float32)).bfloat16().view(torch.int16).numpy().view(np.uint16))   # another top
    rows[9] = w[9].cpu().numpy().view(np.uint16).copy()
    rows[9][::2] = 0x8000                                             # signed zeros among random weights
    rows[10] = w[10].cpu().numpy().view(np.uint16).copy()
    rows[11] = w[11].cpu().numpy().view(np.uint16).copy()
    rows[13] = np.zeros(K, np.uint16)                                 # zero row
    rows[14] = ((np.arange(K) % 7).astype(np.uint16) << 7) | 0x8015   # top < 7
    k32 = np.concatenate([first + 5 + 40 * np.arange(11), mid + 3 + 47 * np.arange(10), last + 9 + 45 * np.arange(11)])      # exactly 32, the cap
    plan = {1: [0], 2: [K - 1], 3: [512 + 73, 512 + 78], 4: [167, 168, 175, 176], 5: list(k32),
            6: [1024 + 5, 1024 + 300, 1536 + 9, 1536 + 500, 1536 + 511], 7: [3, last + 17, last + 400]}
    # first k / last k / two in one lane's eight weights / ends of adjacent lanes / 32 patches over the first, a middle and the last chunk /
    # five inside one decode group (chunks 2 and 3) / chunk 0 and the last real chunk
    assert len(k32) == 32 and k32.max() < K
    hot = np.unique(np.concatenate([np.asarray(v) for v in plan.values()]))
    misses = []
    for r in rows:
        rows[r][hot] = 0
    for r, ks in plan.items():
        top = _top(rows[r])
        assert top >= 8
        for j, k in enumerate(ks):
            rows[r][k] = ((j & 1) << 15) | ((top - 7) << 8) | 0xC0 | (j % 64)      # e[7:1] = top - 7, e[0] = 1
            misses.append((r, int(k)))
    rows[10][K // 2 + 171] = 0x7F80      # +inf in the middle of the row
    rows[11][5] = 0xFF80                 # -inf among the first eight weights: the clamped chunks (if the 16-bit form has any) read it against zeros
    if N > 64:                           # the real grid: seven rows per workgroup; rows 6 | 7 end and begin a workgroup, and so do these
        rows[N - 7], rows[N - 1] = rows[5].copy(), rows[7].copy()
    idx = torch.tensor(sorted(rows), device="cuda")
    w[idx] = torch.from_numpy(np.stack([rows[r] for r in sorted(rows)]).view(np.int16)).cuda()
    return w, hot, misses


def dev_encode(w_bits):
    lib = _lib.lib()
    N, K = w_bits.shape
    coded = torch.full((N, K * 3 // 2), 0xAA, dtype=torch.uint8, device="cuda")
    top = torch.full((N,), 0xAA, dtype=torch.uint8, device="cuda")
    cnt = torch.full((N,), 0xAA, dtype=torch.uint8, device="cuda")
    patch = torch.full((N, 32), -1, dtype=torch.int32, device="cuda")
    over = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.omchat_op_encode_bf16x12(ptr(w_bits), N, K, ptr(coded), ptr(top), ptr(cnt), ptr(patch), ptr(over), None))
    sync()
    assert int(over.item()) == 0
    return coded, top, cnt, patch


def _inputs(K, N, hot, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(K, generator=g) * 0.5
    x[hot] = 0.75 * HOT * torch.from_numpy(np.where(np.arange(len(hot)) % 2 == 0, 1.0, -1.0)).float()
    return x.bfloat16().cuda(), (torch.randn(N, generator=g) * 0.5).bfloat16().cuda()


def run16(w_bits, x, res):
    N, K = w_bits.shape
    y = torch.zeros(N, device="cuda", dtype=torch.bfloat16)
    _lib.check(_lib.lib().omchat_op_gemv(BF16, ptr(x), K, ptr(w_bits), K, ptr(y), N, 1, N, K, None, ptr(res), N, EPI_RESID, 0, None))
    sync()
    return y.view(torch.int16)


def run12(enc, x, res, N, K):
    coded, top, cnt, patch = enc
    y = torch.ones(N, device="cuda", dtype=torch.bfloat16)
    _lib.check(_lib.lib().omchat_op_gemv_bf16x12(ptr(x), ptr(coded), ptr(top), ptr(cnt), ptr(patch), ptr(y), N, K, None, 1e-6, ptr(res), EPI_RESID,
                                                 0, None))
    sync()
    return y.view(torch.int16)


CASES = [(48, 4608), (48, 6144), (48, 8192), (48, 9728), (48, 32768), (3584, 4608), (3584, 18944)]


@pytest.mark.parametrize("N,K", CASES)
def test_longk_bit_identical_to_16_bit(gpu_lib, N, K):
    """48 rows: one workgroup per row.  K = 4608 (9 chunks): fewer passes than buffers.  6144 (12): a 6- or 4-chunk pass has no chunk beyond
    the row while the 16-bit form has four clamped ones.  8192 (16): the 16-bit form has NO clamped chunk -- the row with -inf at weight 5
    stays infinite, any extra w * 0 term would turn it NaN.  9728 (19): a fourth and later pass goes round the buffers; patches in the last
    real chunk and in chunk 0.  32768 (64): the upper end of the range, the 64 KB of staged x.  3584 rows: seven waves per workgroup, two
    workgroups per CU, patched rows at both ends of a workgroup; at K = 18944 the shape of the real step."""
    w, hot, misses = planted(N, K, 3)
    x, res = _inputs(K, N, hot, 3)
    enc = dev_encode(w)
    cnt = enc[2].cpu().numpy()
    assert cnt[0] == 0 and cnt[12] == 0 and cnt[13] == 0 and cnt[5] == 32 and cnt[6] == 5 and cnt[7] == 3
    if N > 64:
        assert cnt[N - 7] == 32 and cnt[N - 1] == 3
    y16, y12 = run16(w, x, res), run12(enc, x, res, N, K)
    assert torch.equal(y16, y12), (y16 != y12).nonzero().flatten().tolist()[:8]
    y = y16.view(torch.bfloat16).float()
    keep = torch.ones(N, dtype=torch.bool, device="cuda")
    keep[10] = keep[11] = False
    assert bool(torch.isfinite(y[keep]).all())
    assert bool(torch.isinf(y[10]))                              # +inf mid-row: no clamped chunk reads it
    if K % 4096 == 0:
        assert bool(torch.isinf(y[11]))                          # no w * 0 term at all in the 16-bit form
    else:
        assert bool(torch.isnan(y[11]))                          # -inf * x[5], then -inf * 0 in the clamped chunks (which take the patch list too)


def test_misses_are_visible(gpu_lib):
    """the 16-bit launch itself gives other bits in the row of a planted miss when that one element is dropped (stored as +0, what the coded
    row holds) or moved by one element, one lane or one chunk: an equal output above means that every patch landed where it belongs"""
    N, K = 48, 9728
    w, hot, misses = planted(N, K, 3)
    x, res = _inputs(K, N, hot, 3)
    y16 = run16(w, x, res)
    for r, k in misses[:3] + misses[-10:]:
        for k2 in (None, k ^ 1, (k + 8) % K, (k + 512) % K):
            wv = w.clone()
            wv[r, k] = 0
            if k2 is not None:
                wv[r, k2] = w[r, k]
            assert int(run16(wv, x, res)[r]) != int(y16[r]), (r, k, k2)


def test_decode_step_down_proj_on_off(gpu_lib):
    """a decode step of the tiny text geometry with the MLP widened to 9 chunks (hidden 256: gate|up and lm_head stay on 16 bits, K = 256),
    key 50 = 7 against 0: ids and fp32 logits bit-equal, eager and captured, and the down_proj role's coded launches counted"""
    from test_gpu_graph import _run
    cfg = tiny(mlp_t=4608)
    K = cfg.text["intermediate_size"]
    if not (K % 512 == 0 and 4096 < K <= 32768):
        pytest.skip(f"down_proj K = {K} of this geometry is outside the long-K range (4096, 32768]")
    lib = _lib.lib()
    sd = synth_state_dict(cfg, 3, lambda k: not k.startswith(synth.TOWER) and "mm_projector" not in k)
    e = Engine(cfg, dtype="bf16", max_seq=256, max_batch=1, vision=False)
    e.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    x = rnd(randn((1, 10, cfg.text["hidden_size"]), 1, 0.5), "bf16")
    first = torch.tensor([5], dtype=torch.int32)
    default, n0 = e.bf16x12_stats()["roles"], e.bf16x12_stats()["launches"]
    runs, counts = [], []
    try:
        for key in (7, 0):
            lib.omchat_op_set_tuning(KEY, key)
            for graph in (False, True):
                e.enable_decode_graph(graph)
                runs.append(_run(e, x, [x.shape[1]], first, 8, True))
                e.enable_decode_graph(False)
            counts.append(e.bf16x12_stats()["launches"])
    finally:
        lib.omchat_op_set_tuning(KEY, default)
    for t, l in runs[1:]:
        assert torch.equal(t, runs[0][0]) and torch.equal(l.view(torch.int32), runs[0][1].view(torch.int32))
    L = cfg.text["num_hidden_layers"]
    assert e.bf16x12_stats()["coded"][1] == L
    assert counts[0][1] - n0[1] >= 8 * L and counts[0][0] == n0[0] and counts[0][2] == n0[2]      # key on: down_proj took the coded launch, eager (8 steps) + capture
    assert counts[1] == counts[0]                                                                  # key off: 16-bit launches count nothing
    e.close()
