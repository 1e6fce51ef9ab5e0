"""CPU restatement of the guidance stage (omchat_amd/csrc/guidance.hip) in fp64 numpy: logits [2b, V], rows [0, b)
conditional and rows [b, 2b) their twins over the negative prompt ->
    scores[r] = scale * (lc - lu) + lu,   lc = log_softmax(logits[r]), lu = log_softmax(logits[b + r])
-- HF's UnbatchedClassifierFreeGuidanceLogitsProcessor, which tests/test_guidance_cpu.py pins it to.  The -inf rule, where HF's formula has
NaN: the score of an id is -inf wherever the conditional or the twin logit is -inf; -inf entries add nothing to a row's sum.  `dtype`
float32 evaluates the same formula in fp32 numpy: the yardstick of the device's tolerance (tests/test_gpu_guidance.py)."""
import numpy as np


def log_softmax(x, dtype=np.float64):
    z = np.asarray(x, dtype=dtype)
    m = z.max(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(np.isfinite(m), np.exp(z - np.where(np.isfinite(m), m, 0)), 0).sum(axis=-1, keepdims=True, dtype=dtype)
        return (z - (m + np.log(s))).astype(dtype)


def guide(logits, b, scale, dtype=np.float64):
    """[2b, V] -> [b, V] in `dtype`"""
    z = np.asarray(logits, dtype=dtype)
    assert z.ndim == 2 and z.shape[0] == 2 * b
    zc, zu = z[:b], z[b:]
    with np.errstate(invalid="ignore"):
        lc, lu = log_softmax(zc, dtype), log_softmax(zu, dtype)
        out = dtype(scale) * (lc - lu) + lu
    return np.where(np.isneginf(zc) | np.isneginf(zu), dtype(-np.inf), out).astype(dtype)


def tolerance(logits, b, scale):
    """(the largest |fp32 numpy - fp64| over the finite scores of these inputs, 8 times that): what the device may deviate by -- its
    reduction order and expf differ from numpy's"""
    ref, f32 = guide(logits, b, scale), guide(logits, b, scale, np.float32)
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(f32))
    dev = float(np.abs(f32[fin].astype(np.float64) - ref[fin]).max()) if fin.any() else 0.0
    return dev, 8.0 * dev
