"""CPU (no GPU): the C-ABI library loads and exports every symbol include/omchat_hip.h declares; host-side logic
(splice plan, prompt layout, key mapping, config parsing, error paths) against golden vectors."""
import ctypes as C
import json
import os
import re
import types
import numpy as np
import pytest
import torch
from conftest import golden, ROOT
from omchat_amd import _lib, synth
from omchat_amd.config import tiny, omchat13b


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "omchat_hip.h")).read()
    declared = set(re.findall(r"\b(omchat_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"omchat_ctx", "omchat_config"}
    l = C.CDLL(_lib.LIB_PATH)
    missing = [n for n in sorted(declared) if not hasattr(l, n)]
    assert not missing, missing
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert b"gfx950" in _lib.lib().omchat_version()


def test_no_gpu_means_loud_failure():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from omchat_amd.engine import Engine
    with pytest.raises(_lib.OmchatError):
        Engine(tiny())
    c = _lib.OmchatConfig(); c.dtype = _lib.BF16; c.v_hidden = 256
    h = C.c_void_p()
    rc = _lib.lib().omchat_ctx_create(C.byref(c), 0, 1, None, C.byref(h))
    assert rc != 0 and b"no HIP device" in _lib.lib().omchat_last_error()


def _plan(ids, mask, ntok, ntiles, side, maxlen):
    lib = _lib.lib()
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    b, T = ids.shape
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    S = C.c_int(0)
    lens = np.zeros(b, np.int32)
    pm = None if m is None else m.ctypes.data_as(C.c_void_p)
    _lib.check(lib.omchat_splice_plan(ids.ctypes.data_as(C.c_void_p), pm, b, T, ntok, ntiles, side, maxlen, None, lens.ctypes.data_as(C.c_void_p), C.byref(S), 0))
    idx = np.zeros((b, S.value), np.int32)
    _lib.check(lib.omchat_splice_plan(ids.ctypes.data_as(C.c_void_p), pm, b, T, ntok, ntiles, side, maxlen, idx.ctypes.data_as(C.c_void_p),
                                      lens.ctypes.data_as(C.c_void_p), C.byref(S), 0))
    return idx, lens


def test_splice_plan_rejects_ids_outside_the_embedding_table():
    """the reference's embed_tokens raises IndexError for an id >= vocab or a stray negative id (omchat_arch.py:139); the plan
    must refuse them before the device gather reads out of bounds.  Masked-out positions and -200 sentinels are fine."""
    lib = _lib.lib()
    S = C.c_int(0)
    lens = np.zeros(1, np.int32)
    call = lambda ids, mask, vocab: lib.omchat_splice_plan(np.ascontiguousarray(ids, np.int64).ctypes.data_as(C.c_void_p),
                                                           None if mask is None else np.ascontiguousarray(mask, np.uint8).ctypes.data_as(C.c_void_p),
                                                           1, len(ids[0]), 4, 1, 0, -1, None, lens.ctypes.data_as(C.c_void_p), C.byref(S), vocab)
    assert call([[1, -200, 319]], None, 320) == 0
    assert call([[1, -200, 320]], None, 320) == 4 and b"out of range" in lib.omchat_last_error()
    assert call([[1, -200, -100]], None, 320) == 4
    assert call([[1, -200, -100]], [[1, 1, 0]], 320) == 0          # padded positions are dropped first (:115)
    assert call([[1, -200, 10 ** 9]], None, 0) == 0                # vocab <= 0: unchecked
    with pytest.raises(IndexError):
        _lib.check(4)


@pytest.mark.parametrize("name", ["1x3", "2_uneven_right", "2_uneven_left", "noimage_row", "truncate"])
def test_splice_plan_reproduces_reference_embeds(name):
    """the integer plan + a numpy gather must give the reference's inputs_embeds bit for bit (omchat_arch.py:103-209)"""
    g = golden("splice_" + name)
    cfg = tiny()
    emb = synth.uniform("model.embed_tokens.weight", (cfg.text["vocab_size"], cfg.text["hidden_size"]), int(g["seed"]))
    feats = g["feats"].reshape(-1, g["feats"].shape[-1])
    mask = g["mask"] if bool(g["has_mask"]) else None
    idx, lens = _plan(g["ids"], mask, g["feats"].shape[1], g["feats"].shape[0], 1 if str(g["side"]) == "left" else 0, int(g["maxlen"]))
    out = np.zeros(idx.shape + (emb.shape[1],), np.float32)
    for i in range(idx.shape[0]):
        for s in range(idx.shape[1]):
            k = int(idx[i, s])
            if k == _lib.PAD_ROW:
                continue
            out[i, s] = emb[k] if k >= 0 else feats[-1 - k]
    assert np.array_equal(out, g["embeds"])
    if mask is not None:
        assert np.array_equal((idx != _lib.PAD_ROW).astype(np.int64), g["mask_out"])
    assert [int(x) for x in lens] == [int((idx[i] != _lib.PAD_ROW).sum()) for i in range(idx.shape[0])]


def test_splice_plan_errors_and_edges():
    with pytest.raises(ValueError):                         # more sentinels than tiles
        _plan([[1, -200, -200]], None, 4, 1, 0, -1)
    idx, lens = _plan([[7, 8, 9]], None, 4, 0, 0, -1)       # text only, zero tiles available
    assert idx.tolist() == [[7, 8, 9]] and lens.tolist() == [3]
    idx, lens = _plan([[1, -200, 2]], [[1, 1, 0]], 2, 1, 0, -1)   # padded token dropped before splicing (:115)
    assert idx.tolist() == [[1, -1, -2]]
    idx, lens = _plan([[-200]], None, 0, 1, 0, -1)          # zero-length features (ragged)
    assert idx.shape == (1, 0) and lens.tolist() == [0]


def test_decode_short_circuit_mask_matches_golden():
    """omchat_arch.py:61-70 through the mirror class, with a stub engine (pure torch integer logic)"""
    from omchat_amd.model.omchat_qwen2 import OmChatMetaForCausalLM
    g = golden("splice_decode_shortcircuit")
    m = OmChatMetaForCausalLM()
    m.vision_tower = object()
    probe = types.SimpleNamespace(shape=(2, 1, int(g["past_len"]), 4))
    past = ((probe, probe),)
    r = m.prepare_inputs_labels_for_multimodal(torch.zeros(2, 1, dtype=torch.long), None, torch.from_numpy(g["mask_in"]), past, None,
                                               torch.zeros(1, 3, 56, 56))
    assert r[4] is None and r[0] is not None
    assert np.array_equal(r[2].numpy(), g["mask_out"]) and np.array_equal(r[1].numpy(), g["position_ids"])


class _Tok:
    bos_token_id = None
    pad_token_id = 0
    def __call__(self, s):
        return types.SimpleNamespace(input_ids=[1000 + ord(ch) for ch in s])
    def encode(self, s):
        return [1000 + ord(ch) for ch in s]


def test_make_context_layout():
    """ChatML layout with hard-coded specials 151644/151645 (make_context.py:79-80) and one -200 per tile"""
    from omchat_amd.make_context import make_context
    raw, ids = make_context(_Tok(), "<image>\npatch:<image>\nhi", None, "sys")
    e = _Tok().encode
    expect = [151644] + e("system") + e("\n") + e("sys") + [151645] + e("\n") + [151644] + e("user") + e("\n") + \
        [-200] + e("\npatch:") + [-200] + e("\nhi") + [151645] + e("\n") + [151644] + e("assistant") + e("\n")
    assert ids == expect
    assert raw == "<|im_start|>system\nsys<|im_end|>\n<|im_start|>user\n<image>\npatch:<image>\nhi<|im_end|>\n<|im_start|>assistant\n"
    raw2, ids2 = make_context(_Tok(), "q2", [("q1", "a1")], "sys")
    assert ids2[:len(e("system")) + 1] == [151644] + e("system") and ids2.count(151644) == 5
    with pytest.raises(NotImplementedError):
        make_context(_Tok(), "x", chat_format="bogus")


def test_anyres_tile_counts():
    from omchat_amd.mm_utils import anyres_tile_count
    pin = [[448, 896], [896, 448], [896, 896], [1344, 448], [448, 1344], [1344, 1344]]
    assert [anyres_tile_count(s, pin) for s in [(448, 448), (570, 380), (1000, 667), (1344, 448)]] == [3, 3, 10, 4]


def test_anyres_tiles_for_reference_sample_image():
    """tile count/order/shape for a 570x380 picture (the size of the reference's images/extreme_ironing.jpg), PIL restatement;
    the product entry refuses a CPU processor (the pixels are produced on the device only)"""
    from PIL import Image
    from transformers import CLIPImageProcessor
    from oracle.preproc import pil_process_anyres_image
    from omchat_amd.mm_utils import process_anyres_image, process_dynamic_image
    proc = CLIPImageProcessor(crop_size=448, do_center_crop=True, do_normalize=True, do_resize=True,
                              image_mean=[0.485, 0.456, 0.406], image_std=[0.229, 0.224, 0.225], size=448)      # internVIT_encoder.py:25-29
    rng = np.random.default_rng(0)
    img = Image.fromarray(rng.integers(0, 255, (380, 570, 3), dtype=np.uint8))
    pin = [[448, 896], [896, 448], [896, 896], [1344, 448], [448, 1344], [1344, 1344]]
    tiles, best = pil_process_anyres_image(img, proc, pin, return_best_res=True)
    assert best == (896, 448) and tuple(tiles.shape) == (3, 3, 448, 448)
    with pytest.raises(TypeError):
        process_anyres_image(img, proc, pin)
    with pytest.raises(TypeError):
        process_dynamic_image(img, proc)


def test_key_layout_roundtrip():
    from omchat_amd.weights import to_hf_key, to_native_key, prepare_state_dict
    cfg = tiny()
    keys = [k for k, *_ in synth.tensor_specs(cfg)]
    hf = [to_hf_key(k) for k in keys]
    assert all(k.startswith(("vision_tower.", "multi_modal_projector.linear_", "language_model.")) for k in hf)
    assert [to_native_key(k) for k in hf] == keys
    sd = {to_hf_key(k): np.zeros(1) for k in keys}
    sd["language_model.model.layers.0.self_attn.rotary_emb.inv_freq"] = np.zeros(1)
    out = prepare_state_dict(sd, cfg)
    assert sorted(out) == sorted(keys)
    assert sorted(prepare_state_dict(sd, cfg, vision=False)) == sorted(k for k in keys if not k.startswith("model.vision_tower") and "mm_projector" not in k)


def test_pos_embed_resize_matches_reference_golden():
    """host-side pos-embed resize (folded constant, N9) == InternVisionEmbeddings._get_pos_embed via the golden embeddings"""
    from omchat_amd.weights import resize_pos_embed
    import oracle
    from oracle.pipeline import _sub, TOWER_PFX
    g = golden("vit_embed_resize")
    cfg = tiny(image_size=112)
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict(cfg, int(g["seed"]), synth.TOWER).items()}
    w = _sub(sd, TOWER_PFX)
    pos = resize_pos_embed(w["embeddings.position_embedding"], 8, 4)
    w2 = dict(w); w2["embeddings.position_embedding"] = pos
    emb = oracle.vit_embeddings(torch.from_numpy(g["pixels"]), w2, 14, 56)       # grid already 4x4: identity resize inside
    assert float((emb - torch.from_numpy(g["emb"])).abs().max()) < 1e-5


def test_checkpoint_config_parsing(tmp_path):
    from omchat_amd.model.builder import save_synthetic_checkpoint, config_from_json, iter_safetensors
    cfg = tiny()
    for layout in ("native", "hf"):
        d = save_synthetic_checkpoint(str(tmp_path / layout), cfg, 0, layout, with_tokenizer=False)
        c2 = config_from_json(d)
        assert c2.text == cfg.text and c2.vision["hidden_size"] == 256 and c2.image_grid_pinpoints == cfg.image_grid_pinpoints
        keys = [k for k, _ in iter_safetensors(d)]
        assert len(keys) == len(synth.tensor_specs(cfg))
        assert all(k.startswith(("vision_tower", "multi_modal", "language_model")) for k in keys) == (layout == "hf")


def test_projector_and_tower_builders_raise_like_reference():
    from omchat_amd.model import build_vision_projector, build_vision_tower
    with pytest.raises(ValueError):
        build_vision_projector(types.SimpleNamespace(mm_projector_type="nope"))
    with pytest.raises(ValueError):
        build_vision_tower(types.SimpleNamespace(mm_vision_tower="clip-vit", mm_vision_select_layer=-1))
    tw = build_vision_tower(types.SimpleNamespace(mm_vision_tower="InternViT-6B-448px", mm_vision_select_layer=-2), delay_load=True)
    assert tw.select_layer == -2 and tw.select_feature == "patch" and not tw.is_loaded
    with pytest.raises(RuntimeError):
        tw.forward(torch.zeros(1, 3, 448, 448))           # no engine attached -> loud failure, never a CPU fallback
    assert build_vision_projector(types.SimpleNamespace(mm_projector_type="identity")).forward(3) == 3


def test_local_dims_for_omchat13b():
    from omchat_amd import tp
    c = omchat13b()
    assert tp.local_dims(c, 0, 8) == dict(v_heads=4, v_mlp=1600, t_heads=4, t_kv_heads=1, t_mlp=2368, t_vocab=19008)
    heads = sorted(h for r in range(8) for h in tp.vit_head_map(c, r, 8) if h >= 0)
    assert heads == list(range(25))
    qs = sorted(q for r in range(8) for q in tp.decoder_head_map(c, r, 8)[0] if q >= 0)
    assert qs == list(range(28))
    for r in range(8):
        q, kv = tp.decoder_head_map(c, r, 8)
        assert all(x < 0 or x // 7 == kv[0] for x in q)          # a rank's q heads all belong to its kv head
    with pytest.raises(ValueError):
        tp.local_dims(c, 0, 3)


def test_keywords_stopping_criteria_semantics():
    """mm_utils.py:242-274: id-suffix match, decoded-tail substring match, bos stripping, all() over the batch"""
    import torch
    from omchat_amd.mm_utils import KeywordsStoppingCriteria

    class T:
        bos_token_id = 1
        def __call__(self, s):
            return types.SimpleNamespace(input_ids=[1] + [ord(c) for c in s])
        def batch_decode(self, x, skip_special_tokens=True):
            return ["".join(chr(int(v)) for v in row if 32 <= int(v) < 127) for row in x]
    prompt = torch.tensor([[9, 9, 9]])
    c = KeywordsStoppingCriteria(["###", "ab"], T(), prompt)
    assert c.max_keyword_len == 3 and [k.tolist() for k in c.keyword_ids] == [[35, 35, 35], [97, 98]]
    assert not c(torch.tensor([[9, 9, 9, 35, 35]]), None)
    assert c(torch.tensor([[9, 9, 9, 35, 35, 35]]), None)                       # id suffix
    assert c(torch.tensor([[9, 9, 9, 97, 98, 50]]), None)                       # substring of the decoded tail
    assert not c(torch.tensor([[9, 9, 9, 97, 50, 98]]), None)
    assert not c(torch.tensor([[9, 9, 9, 35, 35, 35], [9, 9, 9, 1, 2, 3]]), None)   # every row must hit


def test_fast_gelu_formula_accuracy():
    """csrc/common.h gelu_erf (erfc through t * exp(-z^2 + P9(t))) restated in numpy float32 against float64 erf GELU:
    far below the rounding of a 16-bit output, and the negative tail keeps its relative accuracy"""
    from scipy.special import erfc
    x = np.linspace(-6, 6, 400001).astype(np.float32)
    z = np.abs(x) * np.float32(0.70710678118654752440)
    t = np.float32(1) / (np.float32(1) + np.float32(0.5) * z)
    c = [-1.26551223, 1.00002368, 0.37409196, 0.09678418, -0.18628806, 0.27886807, -1.13520398, 1.48851587, -0.82215223, 0.17087277]
    p = np.float32(c[9])
    for k in range(8, -1, -1):
        p = (p * t + np.float32(c[k])).astype(np.float32)
    e = (np.float32(0.5) * t * np.exp((-z * z + p).astype(np.float32))).astype(np.float32)
    got = (x * np.where(x >= 0, np.float32(1) - e, e)).astype(np.float64)
    xd = x.astype(np.float64)
    ref = xd * 0.5 * erfc(-xd / np.sqrt(2))               # x * Phi(x) without cancellation in the tail
    nz = np.abs(ref) > 0
    assert np.abs(got - ref).max() < 5e-7
    assert (np.abs(got - ref)[nz] / np.abs(ref)[nz]).max() < 1e-5


def test_entry_scripts_parse_and_bench_cli():
    """bench.py / __graft_entry__.py / tools/*.py must at least compile (a stray edit once broke the bench line), and the bench CLI
    keeps the driver's contract flags"""
    import ast, glob, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for f in [os.path.join(root, "bench.py"), os.path.join(root, "__graft_entry__.py")] + glob.glob(os.path.join(root, "tools", "*.py")):
        ast.parse(open(f).read(), filename=f)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and all(flag in out.stdout for flag in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"))


def test_bench_dump_outputs_dtypes_fixed_sample_and_budget(tmp_path):
    """bench.py --dump-outputs: ids as float64 (exact), 16-bit / fp32 arrays as float32, an array above DUMP_SAMPLE elements as a sample at
    seeded indices -- the same ones in every run, so two builds compare element for element -- and the files stay within DUMP_BYTES"""
    import bench
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(96, 256, 3584 // 16, generator=g).to(torch.bfloat16)          # more than DUMP_SAMPLE elements
    logits = torch.randn(2, 152064, generator=g)
    ids = torch.tensor([[151642, 0, 17], [3, 4, 5]], dtype=torch.int32)
    assert feats.numel() > bench.DUMP_SAMPLE >= logits.numel()
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"image_features": feats, "prefill_logits": logits, "tokens": ids})
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(a) == ["image_features_sample.npy", "prefill_logits.npy", "tokens.npy"]
    assert a["tokens.npy"].dtype == np.float64 and np.array_equal(a["tokens.npy"], ids.numpy())
    assert a["prefill_logits.npy"].dtype == np.float32 and np.array_equal(a["prefill_logits.npy"], logits.numpy())
    s = a["image_features_sample.npy"]
    assert s.dtype == np.float32 and s.shape == (bench.DUMP_SAMPLE,)
    assert np.isin(s, feats.float().numpy()).all()                                        # values of the array, not a reduction of it
    for f, x in a.items():
        assert np.array_equal(np.load(tmp_path / "b" / f), x)                             # same sample in every run
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in a) <= bench.DUMP_BYTES
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "c"), {f"x{i}": torch.zeros(bench.DUMP_SAMPLE) for i in range(5)})


def test_public_header_is_plain_c(tmp_path):
    """include/omchat_hip.h is the drop-in boundary: it must compile as C99 (no torch / C++ types in the signatures)"""
    import os, shutil, subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "hdr.c"
    src.write_text('#include "omchat_hip.h"\nint main(void) { omchat_config c; (void)c; return omchat_version() == 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-c", str(src), "-o", str(tmp_path / "hdr.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_hf_auto_classes_dispatch_to_the_hip_library(tmp_path):
    """omchat_qwen2.py:113-114 / hf_example.py:7-8: the OmChat config / model / processor classes are registered with transformers'
    Auto classes; on a box without a GPU the dispatch still reaches this library, which fails loudly (no CPU fallback)."""
    import transformers
    from omchat_amd.model import hf as H
    from omchat_amd.model.builder import save_synthetic_checkpoint
    from omchat_amd.config import tiny
    assert type(transformers.AutoConfig.for_model("omchat")) is H.OmChatHFConfig
    assert type(transformers.AutoConfig.for_model("omchat_qwen2")) is H.OmChatQwen2HFConfig
    assert transformers.AutoModel._model_mapping[H.OmChatHFConfig] is H.OmChatForConditionalGeneration
    assert transformers.AutoModelForCausalLM._model_mapping[H.OmChatQwen2HFConfig] is H.OmChatQwen2ForCausalLMHF
    cfg = tiny(layers_v=1, layers_t=1)
    path = save_synthetic_checkpoint(str(tmp_path / "hf"), cfg, 1, "hf")
    assert type(transformers.AutoConfig.from_pretrained(path)) is H.OmChatHFConfig
    import torch
    if not torch.cuda.is_available():
        for auto in (transformers.AutoModel, H.AutoModel):
            with pytest.raises(_lib.OmchatError, match="HIP device"):
                auto.from_pretrained(path, trust_remote_code=True, torch_dtype=torch.float16)
    proc = H.AutoProcessor.from_pretrained(path, trust_remote_code=True)
    assert type(proc).__name__ == "OmChatProcessor" and proc.tokenizer is not None and proc.image_processor.crop_size["height"] == 56
    out = proc(text="w1 w2")                                  # text-only: no device work
    assert isinstance(out, transformers.BatchFeature) and out.input_ids.shape[0] == 1


def test_make_context_and_get_context_vs_ids_captured_from_the_reference():
    """omchat/make_context.py:14-43,66-148 run in the build container with a stub one-id-per-character tokenizer
    (tools/make_golden_r2.py): system prompt, image sentinels, the newest-first history window and the raw format must give the
    same raw_text and context_tokens here"""
    import json, os, types
    import torch
    from conftest import GOLDEN
    from omchat_amd.make_context import make_context, get_context
    import omchat_amd.make_context as mc

    class Tok:
        bos_token_id = None
        def encode(self, s): return [1000 + ord(ch) for ch in s]
        def __call__(self, s): return types.SimpleNamespace(input_ids=self.encode(s))

    cases = json.load(open(os.path.join(GOLDEN, "make_context.json")))
    assert len(cases) >= 10
    for c in cases:
        if c["name"].startswith("get_context"):
            n = c["n_tiles"]
            orig = mc.process_anyres_image
            mc.process_anyres_image = lambda image, ip, pins, flag, return_best_res=False, n=n: ([torch.zeros(3, 4, 4)] * n, (448, 896))
            try:
                inp, ids, image_tensor = get_context(c["text"], Tok(), image=object(), image_processor=None, image_grid_pinpoints=None, device="cpu")
            finally:
                mc.process_anyres_image = orig
            assert list(image_tensor.shape) == c["image_tensor_shape"] and str(image_tensor.dtype) == c["image_tensor_dtype"]
        else:
            hist = [tuple(h) for h in c["history"]] if c["history"] else None
            inp, ids = make_context(Tok(), c["query"], hist, c["system"], c["max_window_size"], c.get("chat_format", "chatml"))
        assert inp == c["raw_text"], c["name"]
        assert ids == c["context_tokens"], c["name"]
        assert ids.count(-200) == c["raw_text"].count("<image>") or c.get("chat_format") == "raw"


def test_decode_branch_of_the_splice_mirror_vs_reference_golden():
    """omchat_arch.py:61-70 (the decode short-circuit of prepare_inputs_labels_for_multimodal) in omchat_amd/model/omchat_qwen2.py against
    the mask / position_ids the reference's own code returned (tests/golden/leftpad_decode.npz, tools/make_golden_r3.py): integer work,
    bit-exact, for the right- AND the left-padded batch; no GPU involved (the cache is probed through the legacy [-1][-1].shape[-2])."""
    import types
    import torch
    from conftest import golden
    from omchat_amd.model.omchat_qwen2 import OmChatMetaForCausalLM

    class M(OmChatMetaForCausalLM):
        def get_vision_tower(self):
            return object()

    g = golden("leftpad_decode")
    m = M()
    for side in ("left", "right"):
        tok_mask = torch.from_numpy(g["mask"]).long()
        L = int(g[side + "_S"])
        for k in range(int(g["steps"])):
            tok_mask = torch.cat([tok_mask, torch.ones(2, 1, dtype=torch.long)], dim=1)
            probe = types.SimpleNamespace(shape=(2, 1, L + k, 128))
            cache = [(probe, probe)]
            ids, pos, mask, past, emb, labels = m.prepare_inputs_labels_for_multimodal(torch.zeros(2, 1, dtype=torch.long), None, tok_mask, cache,
                                                                                     None, torch.zeros(3, 3, 8, 8))
            assert emb is None and labels is None and past is cache and ids.shape == (2, 1)
            assert mask.dtype == torch.long and np.array_equal(mask.numpy(), g[f"{side}_dec_mask_{k}"])
            assert np.array_equal(pos.numpy(), g[f"{side}_dec_pos_{k}"])


def test_bench_parent_never_touches_hip_and_algorithmic_constants():
    """bench.py: (1) the process that spawns the N ranks counts GPUs from the KFD topology and must not reach torch / HIP (the
    children are started from it); (2) the algorithmic FLOPs / bytes the roofline fractions are priced with equal SURVEY.md 8(d)'s figures
    for OmChat-13B and follow the same formulas for OmChat-2.1-8B"""
    import importlib.util, inspect, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    src = inspect.getsource(bench.spawn_ranks) + inspect.getsource(bench.count_gpus_without_hip)
    assert "import torch" not in src and "torch." not in src and "ctypes" not in src and "_lib" not in src
    n = bench.count_gpus_without_hip()
    assert isinstance(n, int) and n >= 0
    from omchat_amd.config import omchat13b, omchat8b_21
    a = bench.algorithmic(omchat13b())
    assert abs(a["vit_tile"] / 1e12 - (11.945 + 0.0498)) < 2e-3            # ViT 11.945 TF + projector 0.0498 TF per tile
    assert abs(a["prefill"](3584) / 1e12 - 49.36) < 1e-2                    # 46.78 + 2.58 TF at S = 3584
    assert abs(a["decode_weight_bytes"] / 1e9 - 14.14) < 1e-2 and a["kv_bytes_per_pos"] == 57344.0
    b = bench.algorithmic(omchat8b_21())
    per_layer = 2 * 1025 * (4 * 1024 * 1024 + 2 * 1024 * 4096) + 4 * 1025 ** 2 * 1024
    assert abs(b["vit_tile"] - (24 * per_layer + 2 * 1024 * 588 * 1024 + 2 * 1024 * (1024 * 3584 + 3584 ** 2))) < 1.0
    assert b["decode_weight_bytes"] == a["decode_weight_bytes"]             # same Qwen2-7B decoder


def test_tp_projection_tool_reproduces_the_committed_curve():
    """tools/tp_projection.py on the committed shard lines: pure arithmetic on measured one-GPU inputs -- the table in
    DESIGN.md must be what the tool prints for the committed files (speed-ups of the closing code: configs1 2.04 x, configs2 2.85 x / 3.53 x
    with the data-parallel tower at N = 8)"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = [os.path.join(root, "profiles", f"r03_y_bench_{n}.json") for n in ("n1", "shard2", "shard4", "shard8")]
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "tp_projection.py")] + files, capture_output=True, text=True, check=True).stdout
    committed = open(os.path.join(root, "profiles", "r03_y_tp_projection.txt")).read()
    assert out.strip() == committed.strip()
    rows = {(l.split()[0], int(l.split()[1])): l for l in out.splitlines() if l.startswith("configs")}
    c1, c2 = rows[("configs1", 8)], rows[("configs2", 8)]
    assert abs(float(c1.split("|")[2].split()[1]) - 2.04) < 0.01
    assert abs(float(c2.split("|")[2].split()[1]) - 2.85) < 0.01 and "3.53" in c2
    log = open(os.path.join(root, "LOG.md")).read()          # (the round-3 table moved from DESIGN.md to LOG.md in round 6)
    assert "| 1 | 1.18 | 1.61 | **2.04** | 2.08 |" in log and "| 1 | 1.17 | 1.93 | **2.85** | **3.53** |" in log


def test_tp_projection_of_round_5_shard_lines():
    """the round-5 closing curve (profiles/r05_q_*: shard-width launch shapes of a tensor-parallel rank's decode GEMVs): configs[2] 3.12 x at N = 8
    (round 4: 2.79 x), 3.94 x with the data-parallel tower; the arithmetic is tools/tp_projection.py on the committed lines"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = [os.path.join(root, "profiles", f"r05_q_bench_{n}.json") for n in ("n1", "shard2", "shard4", "shard8")]
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "tp_projection.py")] + files, capture_output=True, text=True, check=True).stdout
    assert out.strip() == open(os.path.join(root, "profiles", "r05_q_tp_projection.txt")).read().strip()
    rows = {(l.split()[0], int(l.split()[1])): l for l in out.splitlines() if l.startswith("configs")}
    c2 = rows[("configs2", 8)]
    assert abs(float(c2.split("|")[2].split()[1]) - 3.12) < 0.01 and "3.94" in c2
    assert abs(float(rows[("configs2", 8)].split("|")[0].split()[4]) - 1.578) < 1e-3          # rank decode ms per step (round 4: 2.026)


def test_tp_projection_of_round_6_sequence_parallel_shard_lines():
    """round 6: per-rank shard lines with sequence-parallel norms (profiles/r06_e_*; comm_stats carry sp_reduce_scatters > 0, so every exchange is priced as
    reduce-scatter + all-gather) and the all-reduce form beside them; the figures DESIGN.md section 5 quotes are what the tool prints for the committed files"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    P = lambda f: os.path.join(root, "profiles", f)
    run = lambda files: subprocess.run([sys.executable, os.path.join(root, "tools", "tp_projection.py")] + files, capture_output=True, text=True, check=True).stdout
    sp = run([P("r06_h_bench_n1.json")] + [P(f"r06_e_bench_shard{n}.json") for n in (2, 4, 8)])
    ar = run([P("r06_h_bench_n1.json")] + [P(f"r06_e_bench_shard{n}_allreduce_form.json") for n in (2, 4, 8)])
    committed = open(P("r06_e_tp_projection.txt")).read()
    assert sp.strip() in committed and "\n".join(ar.strip().splitlines()[-5:]) in committed
    row = lambda out, wl, n: next(l for l in out.splitlines() if l.startswith(wl) and l.split()[1].rstrip("*") == str(n))
    up = lambda l: float(l.split("|")[2].split()[1])
    assert "*" in row(sp, "configs2", 8).split()[1] and "*" not in row(ar, "configs2", 8).split()[1]
    assert abs(up(row(sp, "configs2", 8)) - 3.18) < 0.01 and abs(up(row(ar, "configs2", 8)) - 3.10) < 0.01
    assert up(row(sp, "configs2", 8)) > up(row(ar, "configs2", 8)) and up(row(sp, "configs2", 4)) > up(row(ar, "configs2", 4))
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert "| 1.30 (1.17) | 2.08 (2.00) | **3.18 (3.10)** |" in design


def test_pmc_traffic_picks_the_manifest_file_and_refuses_a_renamed_kernel(tmp_path, capsys):
    """bench.py::pmc_traffic: the PMC pass behind `roofline.traffic` is the one profiles/MANIFEST.json names, not
    "the last file in lexicographic order" (which put r03_s after r03_ai); without a manifest the newest by (round, tag) order; and a
    file that no longer holds the kernel gives traffic None with the reason in the source string -- old counters never ride on new kernels."""
    import bench
    d = tmp_path
    mk = lambda name, kernels: (d / name).write_text(json.dumps({"note": "", "kernels": {k: {"traffic_bytes_per_launch": v} for k, v in kernels.items()}}))
    mk("r03_s_pmc_traffic.json", {"_Z_gemv_rows_norm_loop_kernelI_Li4ELi7ELb0E": 1.0})
    mk("r03_ai_pmc_traffic.json", {"_Z_gemv_rows_norm_loop_kernelI_Li4ELi7ELb0E": 2.0})
    mk("r04_b_pmc_traffic.json", {"_Z_some_other_kernel": 3.0})
    mk("r04_b_pmc_traffic_configs2.json", {"_Z_gemv_xs_kernelI_Li4ELi2E": 4.0})
    sub = ["gemv_rows_norm_loop_kernelI", "Li4ELi7ELb0E"]
    # no manifest: r04_b is the newest configs1 pass, and it does not hold the kernel -> None, reason given, warning on stderr
    tr, src = bench.pmc_traffic(sub, profiles_dir=str(d))
    assert tr is None and "r04_b_pmc_traffic.json" in src and "no kernel matching" in src
    assert "PMC traffic not reported" in capsys.readouterr().err
    assert bench.pmc_traffic(["gemv_xs_kernelI", "Li4ELi2E"], "pmc_traffic_configs2", profiles_dir=str(d)) == (4.0, "profiles/r04_b_pmc_traffic_configs2.json")
    (d / "r04_b_pmc_traffic.json").unlink()
    # (round, tag) order: 'ai' is newer than 's' (lexicographically it sorts first -- the bug)
    assert bench.pmc_traffic(sub, profiles_dir=str(d)) == (2.0, "profiles/r03_ai_pmc_traffic.json")
    # the manifest wins over any order
    (d / "MANIFEST.json").write_text(json.dumps({"pmc_traffic": "r03_s_pmc_traffic.json"}))
    assert bench.pmc_traffic(sub, profiles_dir=str(d)) == (1.0, "profiles/r03_s_pmc_traffic.json")
    (d / "MANIFEST.json").write_text(json.dumps({"pmc_traffic": "r09_z_pmc_traffic.json"}))
    tr, src = bench.pmc_traffic(sub, profiles_dir=str(d))
    assert tr is None and "missing" in src
    # the committed manifest names files that exist and hold the kernels the driver line quotes
    man = json.load(open(os.path.join(ROOT, "profiles", "MANIFEST.json")))
    for key in ("pmc_traffic", "pmc_traffic_configs2"):
        assert os.path.exists(os.path.join(ROOT, "profiles", man[key])), man[key]


def test_ragged_batch_decode_routing_follows_what_the_engine_can_run():
    """a ragged batch is routed to the masked decode step (omchat_arch.py:61-70 semantics) only where the engine has it
    (one GPU, 16-bit cache); under tensor parallelism a right-padded ragged batch keeps the per-sequence step and a left-padded one is
    refused BEFORE the prefill is enqueued.  Host logic only: a recording stand-in for the Engine, no GPU."""
    import types
    import pytest
    import torch
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM

    class FakeEngine:
        def __init__(self, can_mask):
            self.can_mask, self.calls, self.tp_size = can_mask, [], 1
            self.device, self.torch_dtype = "cpu", torch.float32
            self.c = types.SimpleNamespace(v_layers=0, max_seq=64, t_vocab=11)

        def masked_decode_supported(self):
            return self.can_mask

        def prefill(self, embeds, lengths, want_hidden=False, padding_side="right"):
            self.calls.append(("prefill", padding_side, list(lengths)))
            return torch.zeros(embeds.shape[0], 11), None

        def full_logits(self, x):
            return x

        def decode_step(self, tok, want_logits=False):
            self.calls.append(("decode_step",))
            return torch.zeros(tok.shape[0], dtype=torch.int32), torch.zeros(tok.shape[0], 11)

        def decode_step_masked(self, tok, pos, mask, want_logits=False):
            self.calls.append(("decode_step_masked",))
            return torch.zeros(tok.shape[0], dtype=torch.int32), torch.zeros(tok.shape[0], 11)

    cfg = types.SimpleNamespace(text={"vocab_size": 11}, mm={})
    emb = torch.zeros(2, 5, 8)
    right = torch.tensor([[1, 1, 1, 1, 1], [1, 1, 1, 0, 0]])
    left = torch.tensor([[1, 1, 1, 1, 1], [0, 0, 1, 1, 1]])
    for can_mask in (True, False):
        e = FakeEngine(can_mask)
        m = OmChatQwen2ForCausalLM(cfg, e)
        m.forward(inputs_embeds=emb, attention_mask=right)
        assert e.calls[-1] == ("prefill", "right", [5, 3]) and m._padded_batch == can_mask
    # left padding without the masked step: refused before anything is enqueued
    e = FakeEngine(False)
    m = OmChatQwen2ForCausalLM(cfg, e)
    with pytest.raises(NotImplementedError, match="left-padded ragged batch"):
        m.forward(inputs_embeds=emb, attention_mask=left)
    assert e.calls == []
    e = FakeEngine(True)
    m = OmChatQwen2ForCausalLM(cfg, e)
    m.forward(inputs_embeds=emb, attention_mask=left)
    assert e.calls == [("prefill", "left", [5, 3])] and m._padded_batch
    # equal lengths: never the masked step
    m.forward(inputs_embeds=emb, attention_mask=torch.ones(2, 5, dtype=torch.long))
    assert not m._padded_batch


def test_vit_fc1_roofline_prices_the_mean_tiles_per_launch():
    """VERDICT r04 #9a: a 32-tile clip through a context sized for 24 tiles runs every fc1 as two launches (24 + 8 tiles); the HIP-event
    average is over both, so the flops per launch are those of the MEAN launch.  Numbers of the round-4 line (profiles/r04_ai_bench_n1.json,
    configs4: 180 launches, 1188.9 us average, vit_mfma_frac 0.4259): the fc1 figure must stay within 15 % of the whole-tower fraction (fc1
    is the best-filled GEMM of a layer: 1.05-1.07 x the tower at configs[1] / configs[2]), not 1.6 x above it."""
    import bench
    blk = bench.roofline_vit_block(180 * 1188.9434774716697 / 1e3, 180, 32, 24, 1025, 12800, 3200)
    assert blk["tiles_per_launch"] == 16 and blk["launches"] == 180
    assert abs(blk["frac"] - 0.4520) < 2e-3
    assert blk["frac"] <= 1.15 * 0.42586780383442574
    # unchunked passes keep the old pricing: configs[1] (3 tiles, 135 launches of 262.29 us) and configs[2] (96 tiles = 4 x 24)
    one = bench.roofline_vit_block(135 * 262.2926079564624 / 1e3, 135, 3, 3, 1025, 12800, 3200)
    assert abs(one["frac"] - 0.38415722343469655) < 1e-6 and one["tiles_per_launch"] == 3
    four = bench.roofline_vit_block(540 * 1744.9176088527397 / 1e3, 540, 96, 24, 1025, 12800, 3200)
    assert abs(four["frac"] - 0.46196610998154536) < 1e-6 and four["tiles_per_launch"] == 24


def test_roofline_table_labels_dispatches_by_role():
    """tools/roofline_table.py: one kernel name serves several call sites (the plain 256x256 GEMM runs the ViT qkv, the prefill qkv and the
    projector), so dispatches are labelled from their neighbours in launch order; names as rocprofv3 prints them (profiles/r04_ai_kernel_stats*)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("roofline_table", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "roofline_table.py"))
    rt = importlib.util.module_from_spec(spec); spec.loader.exec_module(rt)
    N = "_ZN12_GLOBAL__N_1"
    norm = N + "14rmsnorm_kernelIDF16bEEvPKT_iS3_PS1_iifi"
    g0 = N + "12gemm8_kernelIDF16bLi0ELb0EEEvNS_5GemmPEi"
    g3 = N + "12gemm8_kernelIDF16bLi3ELb0EEEvNS_5GemmPEi"
    g4 = N + "12gemm8_kernelIDF16bLi4ELb0EEEvNS_5GemmPEi"
    fc1 = "void (anonymous namespace)::gemm8_kernel<bool _Accum, int, E, false>((anonymous namespace)::GemmP, int)"
    proj = N + "11gemm_kernelIDF16bLi192ELi256ELi3ELi4ELi2EEEvNS_5GemmPE"
    fc2 = N + "11gemm_kernelIDF16bLi256ELi192ELi4ELi3ELi2EEEvNS_5GemmPE"
    qkn = N + "17vit_qknorm_kernelIDF16bEEvPT_iPKS1_S4_iiffPKf"
    mha = N + "12attn2_kernelIDF16bLi4ELb0ELi128EEEvNS_5AttnPE"
    gqa = N + "12attn2_kernelIDF16bLi7ELb1ELi128EEEvNS_5AttnPE"
    rope = N + "14rope_kv_kernelIDF16bEEvPT_iiiiiPKiiPKfiS2_S2_llPhS7_PfS8_ll"
    dq = N + "21gemv_rows_norm_kernelIDF16bLi0ELi1ELi7ELb0ELi9EEEvNS_5GemvPE"
    da = N + "18attn_decode_kernelIDF16bLb0ELb0EEEvNS_5AttnPE"
    dm = N + "17attn_merge_kernelIDF16bEEvPKfiiPKiifPT_llii"
    do = "void (anonymous namespace)::gemv_rows_kernel<bool _Accum, int, ELi, E, 7, false>((anonymous namespace)::GemvP)"
    dg = N + "26gemv_rows_norm_loop_kernelIDF16bLi4ELi7ELb0EEEvNS_5GemvPEij"
    dd = N + "22gemv_rows_longk_kernelIDF16bLb0EEEvNS_5GemvPEi"
    lm = N + "21gemv_rows_norm_kernelIDF16bLi0ELi4ELi7ELb0ELi4EEEvNS_5GemvPE"
    am = "(anonymous namespace)::argmax_stage1_kernel(float const*, int, int, float*, int*)"
    vit = [norm, g0, qkn, mha, proj, norm, fc1, fc2]
    pre = [norm, g0, rope, gqa, g3, norm, g4, g3]
    dec = [dq, da, dm, do, dg, dd]
    seq = vit * 2 + pre * 2 + dec * 2 + [lm, am] + vit
    got = rt.label(seq)
    V = ["RMSNorm (ViT)", "ViT qkv GEMM", "ViT q/k norm", "ViT attention (MHA)", "ViT proj GEMM", "RMSNorm (ViT)", "ViT fc1 GEMM (GELU)", "ViT fc2 GEMM"]
    P = ["RMSNorm (prefill)", "prefill qkv GEMM", "prefill RoPE + KV write", "prefill attention (causal GQA)", "prefill o_proj GEMM", "RMSNorm (prefill)",
         "prefill gate|up GEMM (SwiGLU)", "prefill down_proj GEMM"]
    D = ["decode qkv GEMV (+RMSNorm)", "decode attention (split-KV)", "decode attention merge", "decode o_proj GEMV", "decode gate|up GEMV (+RMSNorm)",
         "decode down_proj GEMV"]
    assert got == V * 2 + P * 2 + D * 2 + ["lm_head GEMV (+final norm)", None] + V
    # the prices of the judge's own table: fc1 251.9 GF, ViT attention 40.3 GF, gate|up 271.58 MB, prefill attention 92.07 GF
    W = rt.work(3, 512, 32)
    assert abs(W["ViT fc1 GEMM (GELU)"][1] / 1e9 - 251.9) < 0.1 and abs(W["ViT attention (MHA)"][1] / 1e9 - 40.3) < 0.1
    assert abs(W["decode gate|up GEMV (+RMSNorm)"][1] / 1e6 - 271.58) < 0.01 and abs(W["prefill attention (causal GQA)"][1] / 1e9 - 92.07) < 0.01


def test_tuning_keys_are_refused_without_the_opt_in():
    """the ~35 tuning keys are process-global state shared by every context; they are test / measurement hooks and are refused
    unless the process opted in (OMCHAT_ALLOW_TUNING=1: conftest.py, bench.py --tuning, tools/gpu_job.sh).  No GPU needed: the call only sets globals."""
    from omchat_amd import _lib
    lib = _lib.lib()
    saved = os.environ.pop("OMCHAT_ALLOW_TUNING", None)
    try:
        assert lib.omchat_op_set_tuning(34, 15) != 0
        assert b"OMCHAT_ALLOW_TUNING" in lib.omchat_last_error()
        os.environ["OMCHAT_ALLOW_TUNING"] = "1"
        assert lib.omchat_op_set_tuning(34, 15) == 0
        assert lib.omchat_op_set_tuning(9999, 1) != 0          # unknown key
    finally:
        if saved is None:
            os.environ.pop("OMCHAT_ALLOW_TUNING", None)
        else:
            os.environ["OMCHAT_ALLOW_TUNING"] = saved
    # nothing in the product package sets a key
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hits = subprocess.run(["grep", "-rn", "omchat_op_set_tuning(", os.path.join(root, "omchat_amd"), "--include=*.py"], capture_output=True, text=True).stdout
    assert hits.strip() == "", hits


def test_roofline_table_merges_the_two_launches_of_a_split_gemm():
    """tile ids 12 / 13 run a GEMM as two launches over disjoint column ranges (the bf16 ViT fc1 in the committed table): the tail launch belongs to
    the same call, and the GEMM behind it is still fc2"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("roofline_table", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "roofline_table.py"))
    rt = importlib.util.module_from_spec(spec); spec.loader.exec_module(rt)
    N = "_ZN12_GLOBAL__N_1"
    norm = N + "14rmsnorm_kernelIDF16bEEvPKT_iS3_PS1_iifi"
    g0 = N + "12gemm8_kernelIDF16bLi0ELb0EEEvNS_5GemmPEi"
    qkn = N + "17vit_qknorm_kernelIDF16bEEvPT_iPKS1_S4_iiffPKf"
    mha = N + "12attn2_kernelIDF16bLi4ELb0ELi128ELi1EEEvNS_5AttnPE"
    proj = N + "11gemm_kernelIDF16bLi192ELi224ELi4ELi2ELi2EEEvNS_5GemmPE"
    fc1 = "void (anonymous namespace)::gemm8_kernel<bool _Accum, int, E, false>((anonymous namespace)::GemmP, int)"
    fc1_tail = N + "11gemm_kernelIDF16bLi192ELi224ELi4ELi2ELi1EEEvNS_5GemmPE"
    fc2 = N + "11gemm_kernelIDF16bLi192ELi224ELi4ELi2ELi2EEEvNS_5GemmPE"
    layer = [norm, g0, qkn, mha, proj, norm, fc1, fc1_tail, fc2]
    got = rt.label(layer * 2)
    want = ["RMSNorm (ViT)", "ViT qkv GEMM", "ViT q/k norm", "ViT attention (MHA)", "ViT proj GEMM", "RMSNorm (ViT)", "ViT fc1 GEMM (GELU)", "ViT fc1 GEMM (GELU)", "ViT fc2 GEMM"]
    assert got == want * 2


def test_pmc_symbol_patterns_match_the_built_library():
    """bench.py reads `roofline.traffic` out of a committed PMC summary by kernel SYMBOL; the patterns live in tools/kernel_roles.py (shared with
    tools/roofline_table.py) and every first-choice pattern must match a kernel of the library as built -- a renamed kernel or a changed template
    parameter list fails HERE, on the CPU, instead of nulling the traffic figure on the GPU box."""
    import subprocess
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools import kernel_roles
    from omchat_amd import _lib
    syms = subprocess.run(["nm", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    stubs = [l.split()[-1] for l in syms.splitlines() if "__device_stub__" in l]
    assert len(stubs) > 100
    for role, subs in kernel_roles.first_choice_patterns():
        # the host-side launch stub carries the kernel's mangled name with a __device_stub__ prefix inside the namespace part
        hits = [s for s in stubs if all(x in s.replace("__device_stub__", "") for x in subs)]
        assert hits, (role, subs)
    # and every kernel family the roofline table labels exists (or is an experiments-build / planned name explicitly listed as optional)
    optional = {"vit_qk_sumsq_kernel", "gemv_kernel", "attn_kernel", "gemm8p_kernel"}
    for fam in kernel_roles.FAMILIES:
        assert fam in optional or any(fam + "I" in s or fam + "E" in s or fam in s for s in stubs), fam


# (entry point omchat_op_attn_<name>, arguments, bytes -- or tiles per split) as a library built before the four block-attention launchers were
# folded into launch_attn_block answered, at the 256 compute units that the sizing falls back to without a device (the MI355X's own count).
# Each plan takes tiles-per-split 1 and > 1; the inputs that size nothing answer 0.
_ATTN_WS_TABLE = [
    ("decode_ws", (3, 28, 4000), 2794176),
    ("decode_ws", (1, 28, 1), 14784),
    ("decode_ws", (16, 40, 65), 675840),
    ("decode_ws", (0, 28, 100), 0),
    ("decode_ws", (2, 28, 0), 0),
    ("verify_tpw", (40000, 4), 5),
    ("verify_tpw", (3000, 4), 1),
    ("verify_tpw", (32769, 4), 5),
    ("verify_tpw", (1000000, 8), 8),
    ("verify_tpw", (0, 4), 1),
    ("extend_ws", (40, 28, 4, 9000), 21288960),
    ("extend_ws", (16, 28, 4, 1000), 3784704),
    ("extend_ws", (700, 28, 4, 100), 20697600),
    ("extend_ws", (1, 40, 8, 0), 21120),
    ("extend_ws", (0, 28, 4, 100), 0),
    ("extend_ws", (5, 28, 0, 300), 369600),
    ("shared_ws", (2, 4, 28, 4, 3000, 3300), 6150144),
    ("shared_ws", (8, 4, 28, 4, 20000, 20100), 8515584),
    ("shared_ws", (1, 16, 28, 4, 1, 2), 473088),
    ("shared_ws", (0, 4, 28, 4, 100, 200), 0),
    ("shared_ws", (2, 0, 28, 4, 100, 200), 0),
    ("shared_ws", (2, 4, 28, 4, 300, 300), 0),
    ("shared_ws", (2, 4, 28, 4, 0, 200), 0),
    ("shared_ws", (2, 4, 28, 0, 100, 200), 0),
    ("suffix_ws", (5, 70, 28, 4, 3000), 36220800),
    ("suffix_ws", (2, 5, 28, 4, 500), 1330560),
    ("suffix_ws", (3, 600, 28, 4, 1000), 133056000),
    ("suffix_ws", (0, 5, 28, 4, 500), 0),
    ("suffix_ws", (2, 0, 28, 4, 500), 0),
    ("suffix_ws", (2, 5, 28, 4, 0), 0),
    ("suffix_ws", (2, 5, 28, 0, 500), 0),
]


@pytest.mark.parametrize("name,args,want", _ATTN_WS_TABLE, ids=[f"{n}{a}".replace(" ", "") for n, a, _ in _ATTN_WS_TABLE])
def test_split_kv_workspace_sizing_is_pinned(name, args, want):
    """the workspace sizes and the verify plan that model.hip, the op hooks and the tests allocate by: one sizing function serves the four
    block-attention modes (attn_block_ws_bytes), and what it answers must stay what each mode's own function answered"""
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the table is recorded for 256 compute units")
    assert getattr(_lib.lib(), "omchat_op_attn_" + name)(*args) == want


# tests/golden/gemv_plan_table.json.  "traced": (omchat_op_gemv_plan arguments dtype, b, N, K, epi, ksplit, flags, wf; tuning keys set
# for the call; the plan's fields at 256 compute units, or the refusal text), one row per distinct call of a launch matrix that drove
# the ten omchat_op_gemv* hooks on an MI355X under a kernel trace with a PRODUCT library built BEFORE gemv_plan existed: both dtypes;
# the four decoder projections and the lm_head of the default config at b = 1, 2, 16, 17, 32, 33, at the TP = 1, 2, 4, 8 shard widths
# with the decode step's split-K counts; ragged shapes that reach the MFMA fallbacks; both sides of K = 4096 and 32768; tuning keys 1,
# 11, 16, 17, 28, 34, 38; every refusal the hooks can reach.  "unreached": the refusals no hook reaches (packed operands with a norm, a
# residual or N % 16 != 0), texts from the ladder's source.  "experiments": what only a -DOMCHAT_EXPERIMENTS=1 library answers (key 28
# below 256, key 39, the packed residual / norm forms), worked out by hand from the ladder's source; such a library answers the
# product rows too, except the ones that record the product build's own behaviour (its "need a -DOMCHAT_EXPERIMENTS=1 build" refusal
# and its ignoring key 28 below 256).  "split_k": (b, K, H, packed, down, key 34) -> the decode step's ksplit.
_GEMV_TUNING_DEFAULTS = {1: (0,), 11: (0,), 16: (0,), 17: (1,), 28: (0,), 34: (15,), 38: (1, 16), 39: (0,)}


@pytest.fixture(scope="module")
def gemv_table():
    with open(os.path.join(ROOT, "tests", "golden", "gemv_plan_table.json")) as f:
        return json.load(f)


def _with_tuning(l, pairs, fn):
    try:
        for k, v in pairs:
            assert l.omchat_op_set_tuning(k, v) == 0
        return fn()
    finally:
        for k, _ in pairs:
            for v in _GEMV_TUNING_DEFAULTS[k]:
                assert l.omchat_op_set_tuning(k, v) == 0


def _product_only(tune, want):
    return (isinstance(want, str) and "need a -DOMCHAT_EXPERIMENTS=1 build" in want) or any(k == 28 and 0 < v < 256 for k, v in tune)


@pytest.mark.parametrize("part", ["traced", "unreached", "experiments"])
def test_gemv_plan_is_pinned(part, gemv_table):
    """gemv_plan (what launch_gemv launches from) answers every row of the launch matrix as the launch ladder it replaced did.
    Family, weight form, packed flag, epilogue, NTILE, WAVES, UNROLL, NB, RR, NCH, NORM, grid x / y and block of every traced row are
    the traced kernel's name and dispatch.  The trace does not show the rest; those fields were CHECKED BY HAND against the ladder's
    formulas: dynamic LDS bytes and rows_per_wg of the long-K form ((cdiv(K, 512) + 7) / 8 * 8192; clamp(cdiv(N, 2 CUs), 1, 8)), per_wg
    and skew of the loop form (cdiv(n_out, 2 CUs); key 28 when >= 256 and n_out == per_wg * 2 CUs), n5 of the split form
    (K / 512 = 5 n5 + 2 (ksplit - n5)), xskew (0 outside the experiments build).  The "experiments" rows are by hand throughout."""
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the table is recorded for 256 compute units")
    l = _lib.lib()
    twin = bool(l.omchat_has_experiments())
    if part == "experiments" and not twin:
        pytest.skip("rows of the -DOMCHAT_EXPERIMENTS=1 build")
    out = (C.c_int * 20)()
    assert gemv_table["fields"][:4] == ["family", "wf", "wpack", "epi"] and len(gemv_table["fields"]) == 20
    assert len(gemv_table[part]) >= {"traced": 1000, "unreached": 9, "experiments": 10}[part]
    wrong = []
    for args, tune, want in gemv_table[part]:
        if twin and part != "experiments" and _product_only(tune, want):
            continue

        def plan():
            if l.omchat_op_gemv_plan(*args, 256, out):
                return l.omchat_last_error().decode()
            return list(out)
        got = _with_tuning(l, tune, plan)
        if got != want:
            wrong.append((args, tune, want, got))
    assert not wrong, f"{len(wrong)} rows differ, the first: {wrong[:3]}"


def test_gemv_split_k_is_pinned(gemv_table):
    """the K slices decode_body passes for o_proj and down_proj (gemv_split_k): b in {1, 2, 16, 32}, packed replica or not, at the TP = 1
    and TP = 8 widths, with key 34 at its default and at 0 -- the values the step computed inline before the function existed"""
    l = _lib.lib()
    wrong = []
    for b, K, H, packed, down, shard, want in gemv_table["split_k"]:
        got = _with_tuning(l, [(34, shard)], lambda: l.omchat_op_gemv_split_k(b, K, H, packed, down))
        if got != want:
            wrong.append((b, K, H, packed, down, shard, want, got))
    assert len(gemv_table["split_k"]) == 64
    assert not wrong, wrong


