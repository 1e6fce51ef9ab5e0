#!/usr/bin/env python3
"""Beam-search golden vectors from the REAL reference (same recipe and rules as tools/make_golden.py: runs only in the build container,
the fixture is data only):

  beam_tiny.npz   the reference OmChatQwen2ForCausalLM (tiny geometry, synthetic weights, CPU) driven through tests/beam_ref.py -- HF 5.15's
                  generate() cannot drive it (omchat_arch.py:63 subscripts a DynamicCache) -- with a full forward of every running beam at
                  every step.  Two prompts: one single-tile image prompt (fp16: the tower casts pixels to fp16) and one text-only prompt (fp16
                  and fp32).  Recorded: the returned hypotheses, their scores and every step's smallest candidate margin.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_beam.py
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from make_golden import import_reference, T, save      # noqa: E402
import beam_ref as br                                   # noqa: E402

I = -200
N, MAX_NEW, NRET = 4, 8, 2
PROMPTS = {"img": [3, I, 17, 18, 19, 20, 21, 5, 9], "txt": [3, 17, 18, 19, 20, 21, 5, 9, 40, 41]}


def build_model(c, seed, dtype, enc_mod, InternVisionConfig, OmChatQwen2Config, OmChatQwen2ForCausalLM):
    from omchat_amd import synth
    orig = enc_mod.InternVisionConfig
    vcc = InternVisionConfig(**{**c.vision, "use_flash_attn": False})
    enc_mod.InternVisionConfig = lambda *a, **k: vcc
    try:
        qc = OmChatQwen2Config(
            hidden_size=c.text["hidden_size"], intermediate_size=c.text["intermediate_size"],
            num_hidden_layers=c.text["num_hidden_layers"], num_attention_heads=c.text["num_attention_heads"],
            num_key_value_heads=c.text["num_key_value_heads"], vocab_size=c.text["vocab_size"],
            head_dim=c.text["head_dim"], rms_norm_eps=1e-6, rope_theta=1e6, max_position_embeddings=4096,
            tie_word_embeddings=False, attn_implementation="eager",
            mm_vision_tower="internvit-6b-448px", mm_projector_type="mlp2x_gelu",
            mm_hidden_size=c.vision["hidden_size"], mm_vision_select_layer=-1, delay_load=False)
        try:
            qc.rope_parameters = {"rope_type": "default", "rope_theta": 1e6}
        except Exception:
            pass
        model = OmChatQwen2ForCausalLM(qc).eval()
    finally:
        enc_mod.InternVisionConfig = orig
    res = model.load_state_dict({k: T(v) for k, v in synth.state_dict(c, seed=seed).items()}, strict=False)
    assert not [k for k in res.missing_keys if "inv_freq" not in k] and not res.unexpected_keys
    model.config._attn_implementation = "eager"
    return model.to(dtype)


def run(mdl, ids, px, eos, dtype):
    """beam_ref driven by the reference: every running beam's whole sequence (prompt + its generated ids) through forward(images=...)"""
    seqs, margins = [], []

    def last_logits(row):
        o = mdl(input_ids=torch.tensor([row]), images=None if px is None else px.to(dtype), use_cache=False)
        return o.logits[0, -1].float().numpy()

    def fn(t, tokens, parents):
        nonlocal seqs
        if t == 0:
            rows = [list(ids)]
        else:
            prev = [list(ids)] * N if t == 1 else seqs
            rows = [prev[int(parents[r])] + [int(tokens[r])] for r in range(N)]
        seqs = rows
        lg = np.stack([last_logits(r) for r in rows]).astype(np.float32)
        # the step's smallest gap at a boundary that decides something: the KB kept candidates, the top N (which may finish), and
        # the N non-EOS candidates that run on
        run_sc = np.zeros(1, np.float32) if t == 0 else state["P"].run
        acc = np.concatenate([br.log_softmax(lg[j]) + run_sc[j] for j in range(len(rows))]).astype(np.float64)
        order = np.argsort(-acc, kind="stable")
        top = acc[order]
        KB = max(2, 1 + len(eos)) * N
        live = top[[k for k in range(4 * KB) if int(order[k] % lg.shape[1]) not in eos]]
        margins.append(float(min(top[KB - 1] - top[KB], top[N - 1] - top[N], live[N - 1] - live[N])))
        return lg

    state = {}
    orig_step = br.step

    def step(P, *a, **k):
        state["P"] = P
        return orig_step(P, *a, **k)
    br.step = step
    try:
        out, steps, Ps = br.search(fn, 1, N, MAX_NEW, eos=eos, num_return=NRET)
    finally:
        br.step = orig_step
    hyps = out[0]
    L = max(len(h) for h, _ in hyps)
    seq = np.full((NRET, L), -1, np.int64)
    for q, (h, _) in enumerate(hyps):
        seq[q, :len(h)] = h
    return seq, np.array([len(h) for h, _ in hyps]), np.array([s for _, s in hyps], np.float32), np.array(margins), steps


def main():
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    import_reference()
    from omchat_amd import synth
    from omchat_amd.config import tiny
    import omchat.model.multimodal_encoder.internVIT_encoder as enc_mod
    from omchat.model.multimodal_encoder.intern_vit_6b.configuration_intern_vit import InternVisionConfig
    from omchat.model.language_model.omchat_qwen2 import OmChatQwen2Config, OmChatQwen2ForCausalLM
    cfg = tiny()
    mk = lambda seed, dt: build_model(cfg, seed, dt, enc_mod, InternVisionConfig, OmChatQwen2Config, OmChatQwen2ForCausalLM)
    px = T(synth.pixels(1, cfg.vision["image_size"], seed=7))
    best = None
    for seed in range(60, 90):                       # a weight seed whose searches keep wide margins
        m16 = mk(seed, torch.float16)
        # EOS: the token the best image-prompt beam emits third, so that hypotheses end before MAX_NEW
        free = run(m16, PROMPTS["img"], px, [], torch.float16)
        eos = [int(free[0][0, 2])]
        rec = {"img": run(m16, PROMPTS["img"], px, eos, torch.float16), "txt": run(m16, PROMPTS["txt"], None, eos, torch.float16)}
        rec["txt32"] = run(mk(seed, torch.float32), PROMPTS["txt"], None, eos, torch.float32)
        score = min(float(r[3].min()) for r in rec.values())
        ended = any(int(l) < MAX_NEW for l in rec["img"][1])
        print(f"  seed {seed}: min margin {score:.4f}, early end {ended}")
        if ended and (best is None or score > best[0]):
            best = (score, seed, eos, rec)
        if ended and score >= 0.05:
            break
    score, seed, eos, rec = best
    arrs = dict(seed=seed, pixel_seed=7, n_tiles=1, num_beams=N, max_new=MAX_NEW, num_return=NRET, eos=np.array(eos),
                ids_img=np.array(PROMPTS["img"]), ids_txt=np.array(PROMPTS["txt"]))
    for name, (seq, lens, scores, margins, steps) in rec.items():
        arrs.update({f"{name}_seq": seq, f"{name}_len": lens, f"{name}_scores": scores, f"{name}_margins": margins, f"{name}_steps": steps})
    save("beam_tiny", **arrs)
    print(f"  beam_tiny: seed {seed}, eos {eos}, min margin {score:.4f}")


if __name__ == "__main__":
    main()
