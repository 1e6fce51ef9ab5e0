"""GPU: generate(num_beams=4) against the REFERENCE model's beam search (tests/golden/beam_tiny.npz, tools/make_golden_beam.py: the reference
OmChatQwen2ForCausalLM on CPU driven through tests/beam_ref.py, a full forward per beam per step).  One single-tile image prompt -- the
splice, the prefill of the spliced prompt and the fork of its cache row under beams -- and one text-only prompt, f16 and bf16.  Ids are
compared wherever every recorded margin so far exceeds the dtype's noise, as tests/test_gpu_round2.py guards its greedy ids."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from conftest import golden
from omchat_amd import synth
from omchat_amd.config import tiny
from omchat_amd.engine import Engine

NOISE = {"f16": 0.004, "bf16": 0.02}      # smallest margin (accumulated log-prob units) at which the dtype's logits cannot flip a decision


@pytest.fixture(scope="module")
def g():
    return golden("beam_tiny")


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("which", ["img", "txt"])
def test_beam_ids_equal_reference(gpu_lib, g, dtype, which):
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM
    cfg = tiny()
    N, nret, max_new = int(g["num_beams"]), int(g["num_return"]), int(g["max_new"])
    e = Engine(cfg, dtype=dtype, max_seq=128, max_batch=N, max_tiles=1)
    e.load_state_dict(synth.state_dict(cfg, int(g["seed"])))
    m = OmChatQwen2ForCausalLM(cfg.clone(), e)
    ids = torch.from_numpy(g["ids_" + which]).long()[None]
    images = None
    if which == "img":
        images = torch.from_numpy(synth.pixels(int(g["n_tiles"]), cfg.vision["image_size"], int(g["pixel_seed"]))).half().cuda()
    out = m.generate(ids, images=images, num_beams=N, num_return_sequences=nret, max_new_tokens=max_new, eos_token_id=[int(x) for x in g["eos"]],
                     return_dict_in_generate=True)
    # f16 against the fp16 reference run; bf16 against the fp32 one where it exists (the image prompt has only fp16: the tower casts to it)
    ref = which if (dtype == "f16" or which == "img") else "txt32"
    seq, lens, scores, margins = g[ref + "_seq"], g[ref + "_len"], g[ref + "_scores"], g[ref + "_margins"]
    T = ids.shape[1]
    got = [out.sequences[q, T:].tolist() for q in range(nret)]
    ok = int(np.argmax(np.append(margins <= NOISE[dtype], True)))          # leading steps whose every decision is above the noise
    if ok >= len(margins):
        # every decision of the search is clear: the whole result must be the reference's
        for q in range(nret):
            L = int(lens[q])
            assert got[q][:L] == seq[q, :L].tolist() and all(x == int(g["eos"][0]) for x in got[q][L:]), (q, got[q], seq[q])
        np.testing.assert_allclose(out.sequences_scores.numpy(), scores, atol=0.01 if dtype == "f16" else 0.05)
    else:
        # the best hypothesis up to the first decision inside the noise
        L = min(ok, int(lens[0]))
        assert got[0][:L] == seq[0, :L].tolist(), (ok, got[0], seq[0])
    e.close()


def test_golden_is_informative(g):
    """the fixture exercises what the GPU test relies on: an image prompt whose hypotheses end on EOS, clear f16 decisions for the text prompt"""
    assert int(g["img_len"].min()) < int(g["max_new"])
    assert float(g["txt_margins"].min()) > NOISE["f16"] and float(g["img_margins"][0]) > NOISE["f16"]
