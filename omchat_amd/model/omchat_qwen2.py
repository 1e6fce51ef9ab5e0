"""Counterpart of omchat/model/language_model/omchat_qwen2.py + omchat/model/omchat_arch.py on the HIP engine."""
import types
import torch

from ..constants import IMAGE_TOKEN_INDEX
from ..config import OmChatConfig
from .vision_tower import build_vision_tower
from .projector import build_vision_projector
from ..scoring import check_labels, shift_labels, splice_labels


class OmChatQwen2Config(OmChatConfig):
    model_type = "omchat_qwen2"


class KVHandle:
    """Opaque handle to the context-owned KV cache.  Quacks like the caches the reference probes:
    `get_seq_length()` (HF Cache) and the legacy `past_key_values[-1][-1].shape[-2]` (omchat_arch.py:63)."""

    def __init__(self, engine, batch):
        self.engine, self.batch = engine, batch

    def get_seq_length(self, layer_idx=0):
        return max(self.engine.kv_lengths(self.batch))

    def __bool__(self):
        return True

    def __getitem__(self, i):
        L = self.get_seq_length()
        kv = self.engine.local["t_kv_heads"]
        probe = types.SimpleNamespace(shape=(self.batch, kv, L, 128))
        return (probe, probe)

    def __len__(self):
        return self.engine.cfg.text["num_hidden_layers"]


class CausalLMOutputWithPast(dict):
    def __init__(self, logits, past_key_values):
        super().__init__(logits=logits, past_key_values=past_key_values, loss=None)
        self.logits, self.past_key_values, self.loss = logits, past_key_values, None

    def add(self, name, value):
        self[name] = value
        setattr(self, name, value)


class _GenerationConfig(types.SimpleNamespace):
    pass


class OmChatMetaForCausalLM:
    """omchat_arch.py:42-209."""

    def get_vision_tower(self):
        return self.vision_tower

    def encode_images(self, images):
        """omchat_arch.py:50-53 -- tower then projector, fused in one C ABI call."""
        t = self.get_vision_tower()
        if t.select_feature != "patch":
            return self.mm_projector(t(images))
        return self.engine.encode_images(images, t.select_layer).to(images.dtype)

    def prepare_inputs_labels_for_multimodal(self, input_ids, position_ids, attention_mask, past_key_values, labels, images):
        """omchat_arch.py:55-209.  Returns the reference's 6-tuple
        (input_ids|None, position_ids, attention_mask, past_key_values, inputs_embeds|None, labels).  Given labels come back as the
        reference's `new_labels` [b, S] (int64, CPU): filtered by the mask, image-token positions dropped, -100 on feature rows, padding
        (either side) and beyond tokenizer_model_max_length (:112-199; omchat_amd/scoring.py on top of the splice plan)."""
        vision_tower = self.get_vision_tower()
        if vision_tower is None or images is None or input_ids.shape[1] == 1:
            if past_key_values is not None and vision_tower is not None and images is not None and input_ids.shape[1] == 1:
                target = past_key_values[-1][-1].shape[-2] + 1                       # :63
                attention_mask = torch.cat((attention_mask, torch.ones((attention_mask.shape[0], target - attention_mask.shape[1]),
                                                                      dtype=attention_mask.dtype, device=attention_mask.device)), dim=1)
                position_ids = torch.sum(attention_mask, dim=1).unsqueeze(-1) - 1
            return input_ids, position_ids, attention_mask, past_key_values, None, labels
        if type(images) is list or images.ndim == 5:
            if type(images) is list:
                if any(im.ndim != 3 for im in images):
                    raise NotImplementedError("video inputs: the reference calls an undefined encode_videos (omchat_arch.py:87)")
                images = torch.stack(images)
            else:
                raise NotImplementedError("video inputs: the reference calls an undefined encode_videos (omchat_arch.py:87)")
        if getattr(self.config, "tune_mm_mlp_adapter", False) and getattr(self.config, "mm_use_im_start_end", False):
            raise NotImplementedError                                                  # :100-101
        feats = self.encode_images(images)
        side = getattr(self.config, "tokenizer_padding_side", "right")
        maxlen = getattr(self.config, "tokenizer_model_max_length", None)
        embeds, lengths, valid, plan = self.engine.splice(input_ids, attention_mask, feats, side, maxlen, return_plan=True)
        self._last_lengths = lengths
        new_mask = None if attention_mask is None else valid.to(dtype=attention_mask.dtype, device=attention_mask.device)   # :201-204
        new_pos = None                                                                 # :206-207 (None unless the caller passed one)
        if position_ids is not None:
            S = embeds.shape[1]
            new_pos = torch.zeros((embeds.shape[0], S), dtype=position_ids.dtype, device=position_ids.device)
            for i, n in enumerate(lengths):
                if side == "left":
                    new_pos[i, S - n:] = torch.arange(n, dtype=position_ids.dtype)
                else:
                    new_pos[i, :n] = torch.arange(n, dtype=position_ids.dtype)
        if labels is not None:
            labels = splice_labels(plan, input_ids, attention_mask, labels)
        return None, new_pos, new_mask, past_key_values, embeds, labels


class OmChatQwen2ForCausalLM(OmChatMetaForCausalLM):
    """OmChatQwen2ForCausalLM (omchat_qwen2.py:29-111): forward(images=...) + HF-style greedy generate()."""

    def __init__(self, config, engine):
        self.config = config
        self.engine = engine
        self.vocab_size = config.text["vocab_size"]
        args = types.SimpleNamespace(**config.mm)
        self.vision_tower = build_vision_tower(args, engine=engine) if engine.c.v_layers > 0 else None
        self.mm_projector = build_vision_projector(args, engine=engine) if engine.c.v_layers > 0 else None
        # sampling defaults as HF's GenerationConfig (temperature 1, top_k 50, top_p 1, no penalty); `seed` is this project's: the on-device
        # sampler draws from an explicit seed, never from torch's global RNG state
        self.generation_config = _GenerationConfig(pad_token_id=None, eos_token_id=None, max_new_tokens=None, do_sample=False, temperature=1.0,
                                                   top_k=50, top_p=1.0, repetition_penalty=1.0, seed=None, num_beams=1,
                                                   length_penalty=1.0, early_stopping=False, num_return_sequences=1, reuse_cache=False)
        self._last_lengths = None
        self.device = engine.device
        self.dtype = engine.torch_dtype

    def get_model(self):
        return self

    def reset_cache(self):
        """forget the conversation generate(reuse_cache=True) keeps in sequence 0's cache (record, tiles, feature rows): the next call
        prefills its whole prompt"""
        self.engine.drop_prefix()

    def eval(self):
        return self

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None, labels=None,
                use_cache=None, output_attentions=None, output_hidden_states=None, images=None, return_dict=None):
        """labels (int [b, T] beside input_ids, or [b, S] beside inputs_embeds; -100 = not scored) on a prefill call: teacher-forced scoring
        (DESIGN.md section 18).  The output then carries `loss` (fp32 device scalar: Qwen2's shifted cross-entropy over the spliced
        sequence, mean over the labels that are not ignored, NaN if there are none), `token_logprobs` fp32 [b, S] (column t >= 1:
        log p(labels[:, t] | slots < t) under the raw fp32 distribution; 0 where the label is ignored and in column 0) and `labels` (the
        spliced labels [b, S]).  The full [b, S, V] logits the reference returns are NOT materialised: `logits` stays [b, 1, V] of the
        last valid position, as without labels.  Text-only calls compact a row's unmasked tokens (Engine.splice), and so its labels:
        a label at a masked position is not scored.  labels on a decode call: ValueError; under tensor parallelism: NotImplementedError."""
        if output_attentions:
            raise NotImplementedError("attention maps are never materialised by the flash kernels")
        if labels is not None:
            if self.engine.tp_size > 1:      # before the tower runs
                raise NotImplementedError("forward(labels=...) under tensor parallelism: the lm_head is vocabulary-parallel and no exchange of "
                                          "the scoring partials is built")
            if inputs_embeds is None and (past_key_values is not None or input_ids is None):
                raise ValueError("forward(labels=...) scores a prefill call (inputs_embeds, or input_ids without a cache), not a decode step")
            # shape and range on the raw labels, before any work and before any state of an earlier prefill changes (the splice only moves
            # values and inserts -100; labels at image-token and masked positions drop out in it, so they are not looked at)
            want = tuple(input_ids.shape) if inputs_embeds is None else tuple(inputs_embeds.shape[:2])
            if tuple(labels.shape) != want:
                raise ValueError(f"labels {tuple(labels.shape)} must have the shape {want} of the call's {'input_ids' if inputs_embeds is None else 'inputs_embeds rows'}")
            host = labels.detach().to("cpu", torch.int64)
            if inputs_embeds is None:
                keep = input_ids.detach().to("cpu").ne(IMAGE_TOKEN_INDEX)
                if attention_mask is not None and tuple(attention_mask.shape) == want:
                    keep &= attention_mask.detach().to("cpu").ne(0)
                host = host[keep]
            check_labels(host, self.vocab_size)
        if inputs_embeds is None:
            (input_ids, position_ids, attention_mask, past_key_values, inputs_embeds, labels) = \
                self.prepare_inputs_labels_for_multimodal(input_ids, position_ids, attention_mask, past_key_values, labels, images)
        if inputs_embeds is None and past_key_values is None:
            # text-only prefill: embed_tokens through the same gather kernel
            inputs_embeds, lengths, _, plan = self.engine.splice(input_ids, attention_mask, None, return_plan=True)
            self._last_lengths = lengths
            if labels is not None:
                labels = splice_labels(plan, input_ids, attention_mask, labels)
        if inputs_embeds is not None:
            b, S, _ = inputs_embeds.shape
            lengths = self._last_lengths if self._last_lengths is not None and len(self._last_lengths) == b else [S] * b
            side = "right"
            if attention_mask is not None and attention_mask.shape[1] == S:
                lengths = [int(x) for x in attention_mask.ne(0).sum(dim=1)]
                right = all(int(attention_mask[i, :n].ne(0).sum()) == n for i, n in enumerate(lengths))
                left = all(int(attention_mask[i, S - n:].ne(0).sum()) == n for i, n in enumerate(lengths))
                if not right and not left:
                    raise NotImplementedError("attention masks with holes: pad on one side")
                # a left-padded batch (tokenizer_padding_side='left', omchat_arch.py:176-184) is prefilled exactly as the reference
                # does it (RoPE on arange(S), padded keys masked, logits of position S - 1); its decode steps go through the masked
                # step below (omchat_decode_step_masked), which positions and masks the rows as omchat_arch.py:61-70 does
                side = "right" if right else "left"
            self._last_lengths = None
            # a batch whose rows differ in (spliced) length, or any left-padded one, is decoded as the reference does it: common cache
            # slot, position_ids = sum(mask) - 1 and the padded token-level mask as the key mask (omchat_arch.py:61-70).  That step
            # exists on one GPU only (include/omchat_hip.h: omchat_decode_step_masked): under tensor parallelism a RIGHT-padded ragged
            # batch keeps the per-sequence step (every row at its own length: same tokens as the reference while no row has ended),
            # and a left-padded one is refused HERE, before any work is enqueued
            ragged = b > 1 and (side == "left" and min(lengths) < S or len(set(lengths)) > 1)
            can_mask = self.engine.masked_decode_supported()
            if ragged and side == "left" and not can_mask:
                raise NotImplementedError("left-padded ragged batch: the masked decode step runs at tp_size == 1 only; pad on the right")
            self._padded_batch = ragged and can_mask
            self._prefill_slots = S                                   # the common cache slot a padded batch's decode steps append at
            if labels is not None:
                new_labels = labels.detach().to("cpu", torch.int64)
            logits_last, hidden = self.engine.prefill(inputs_embeds, lengths, want_hidden=bool(output_hidden_states) or labels is not None,
                                                      padding_side=side)
            local = logits_last                                       # this rank's vocabulary shard (the whole vocabulary at TP = 1)
            logits_last = self.engine.full_logits(logits_last)        # vocab-parallel lm_head: gather the rank-local shards
            out = CausalLMOutputWithPast(logits_last.unsqueeze(1), KVHandle(self.engine, b))
            out.local_logits = local
            if output_hidden_states:
                out["hidden_states"] = (hidden,); out.hidden_states = (hidden,)
            if labels is not None:
                # slot t's row predicts the label of slot t + 1 (Qwen2ForCausalLM.forward: logits[..., :-1, :] against labels[..., 1:])
                lp, loss, seq_sum, seq_count = self.engine.score_hidden(hidden, shift_labels(new_labels))
                tl = torch.zeros_like(lp)
                tl[:, 1:] = lp[:, :-1]
                out.add("loss", loss); out.add("token_logprobs", tl); out.add("labels", new_labels)
                out.add("sequence_logprobs", seq_sum); out.add("num_tokens", seq_count)
            return out
        if input_ids.shape[1] != 1:
            raise ValueError("decode steps take exactly one token per sequence")
        if getattr(self, "_padded_batch", False):
            if attention_mask is None:
                raise ValueError("decode step of a padded batch: pass the token-level attention_mask (one more 1 per generated token) as HF "
                                 "generate does, so that omchat_arch.py:61-70 can position the rows")
            if position_ids is None:
                # text-only call (no `images`): the reference leaves position_ids to Qwen2Model, which takes cache_position -- the common
                # cache length -- for every row (modeling_qwen2.py:368-373), and the mask is the token-level one as passed
                L = past_key_values.get_seq_length() if past_key_values is not None else max(self.engine.kv_lengths(input_ids.shape[0]))
                position_ids = torch.full((input_ids.shape[0], 1), L, dtype=torch.long)
            nxt, logits = self.engine.decode_step_masked(input_ids[:, 0], position_ids, attention_mask, want_logits=True)
        else:
            nxt, logits = self.engine.decode_step(input_ids[:, 0], want_logits=True)
        out = CausalLMOutputWithPast(self.engine.full_logits(logits).unsqueeze(1), past_key_values)
        out.next_tokens = nxt
        return out

    __call__ = forward

    def score(self, input_ids, images=None, attention_mask=None, labels=None, suffixes=None, share_prompt=None):
        """Teacher-forced scoring of given text: forward(labels=...) with labels = input_ids by default -- the image
        placeholders drop out in the splice, so every text token but a row's first is scored.  -> dict: `loss` (fp32 scalar, mean negative
        log-probability of the scored tokens), `token_logprobs` fp32 [b, S] and `labels` int64 [b, S] as forward(labels=...) returns them,
        `sequence_logprobs` fp32 [b] (sum over a row's scored tokens), `num_tokens` int64 [b] and `perplexity` fp32 [b] =
        exp(-sequence_logprobs / num_tokens) (NaN for a row without scored tokens); all but `labels` on the device.  One host
        synchronisation, at the end.
        suffixes=[ids_0, ..., ids_{N-1}]: multiple-choice scoring of N candidate continuations of ONE prompt
        (input_ids [1, T]).  The tower and the prompt's prefill run once, the N suffixes go through the decoder in one pass.  -> dict over the
        SUFFIX tokens only: `token_logprobs` fp32 [N, S_max] (0 behind a row's end), `sequence_logprobs` fp32 [N], `num_tokens` int64 [N],
        `perplexity` fp32 [N]; row j's numbers are those of score() on input_ids[0] + suffixes[j] restricted to the suffix, to rounding.
        share_prompt and the refusals are generate(suffixes=)'s; `labels` cannot be combined with it."""
        if suffixes is not None:
            if labels is not None:
                raise ValueError("score(suffixes=...) scores the suffix tokens themselves: `labels` cannot be combined with it")
            return self._score_suffixes(input_ids, images, attention_mask, suffixes, share_prompt)
        out = self.forward(input_ids=input_ids, attention_mask=attention_mask, images=images, labels=input_ids if labels is None else labels)
        n = out.num_tokens
        res = dict(loss=out.loss, token_logprobs=out.token_logprobs, labels=out.labels, sequence_logprobs=out.sequence_logprobs,
                   num_tokens=n.to(torch.int64), perplexity=torch.exp(-out.sequence_logprobs / n))
        torch.cuda.current_stream().synchronize()
        return res

    def enable_mxfp4_decode(self, on=True, batched=False):
        """Engine.enable_mxfp4_decode: batch-1 decode steps of generate() stream the MXFP4 replica of the decoder weights (greedy, sampling,
        bans, logprobs, reuse_cache and the decode graph unchanged); batched steps and beam search keep the 16-bit weights, and
        prompt_lookup_num_tokens is refused while it is on.  batched=True: batched and padded batches (up to 32 rows), beam search and the
        prompt-lookup verify step stream the packed MXFP4 copy as well, and prompt_lookup_num_tokens is accepted."""
        self.engine.enable_mxfp4_decode(on, batched)

    def _stage_buffer(self, steps, b):
        """pinned staging rows for the generated ids + the event that guards them: allocated once and grown on demand (a hipHostMalloc per
        generate() call was measurable)"""
        cur = getattr(self, "_stage", None)
        if cur is None or cur.shape[0] < steps or cur.shape[1] != b:
            self._stage = torch.empty((max(steps, 64), b), dtype=torch.int32).pin_memory()
            self._stage_event = torch.cuda.Event()
        return self._stage

    def prepare_inputs_for_generation(self, input_ids, past_key_values=None, attention_mask=None, inputs_embeds=None, **kwargs):
        """omchat_qwen2.py:92-111."""
        if past_key_values:
            input_ids = input_ids[:, -1:]
        if inputs_embeds is not None and past_key_values is None:
            model_inputs = {"inputs_embeds": inputs_embeds}
        else:
            model_inputs = {"input_ids": input_ids}
        model_inputs.update({"past_key_values": past_key_values, "use_cache": kwargs.get("use_cache"),
                             "attention_mask": attention_mask, "images": kwargs.get("images", None)})
        return model_inputs

    def _sampling_params(self, temperature, top_k, top_p, repetition_penalty, seed, generator, kwargs=None):
        """HF's resolution of the sampling arguments (None -> generation_config), validated as HF's warpers validate them.  min_p,
        typical_p, epsilon_cutoff and eta_cutoff are popped from `kwargs`; they are on under the rules of HF's _get_logits_processor."""
        gc = self.generation_config
        pick = lambda v, name, d: v if v is not None else (getattr(gc, name, None) if getattr(gc, name, None) is not None else d)
        T = pick(temperature, "temperature", 1.0)
        k = pick(top_k, "top_k", 0)
        p = pick(top_p, "top_p", 1.0)
        rp = pick(repetition_penalty, "repetition_penalty", 1.0)
        if not float(T) > 0:
            raise ValueError(f"`temperature` (={T}) has to be a strictly positive float, otherwise your next token scores will be invalid. "
                             "If you're looking for greedy decoding strategies, set `do_sample=False`.")
        if not (isinstance(k, int) and k >= 0):
            raise ValueError(f"`top_k` has to be a non-negative integer, but is {k}")
        if not 0.0 < float(p) <= 1.0:
            raise ValueError(f"`top_p` has to be a float > 0 and <= 1, but is {p}")
        if not float(rp) > 0:
            raise ValueError(f"`penalty` has to be a strictly positive float, but is {rp}")
        kwargs = kwargs if kwargs is not None else {}
        flt = {name: pick(kwargs.pop(name, None), name, None) for name in ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")}
        if flt["min_p"] is not None and not 0 <= flt["min_p"] <= 1.0:
            raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {flt['min_p']}")
        if flt["typical_p"] is not None and flt["typical_p"] < 1.0:
            if not 0 < float(flt["typical_p"]) < 1:
                raise ValueError(f"`typical_p` has to be a float > 0 and < 1, but is {float(flt['typical_p'])}")
        else:
            flt["typical_p"] = None
        for name in ("epsilon_cutoff", "eta_cutoff"):      # HF switches them on inside (0, 1) only
            if flt[name] is None or not 0.0 < flt[name] < 1.0:
                flt[name] = None
        if seed is None and generator is not None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), generator=generator, dtype=torch.int64))
        if seed is None:
            seed = getattr(gc, "seed", None)
        if seed is None:
            raise NotImplementedError("do_sample=True draws on the device from an explicit seed: pass seed=<int> or generator=<torch.Generator> "
                                      "(or set generation_config.seed); sampling from torch's global RNG state is not implemented")
        return dict(seed=int(seed), temperature=float(T), top_k=int(k), top_p=float(p), repetition_penalty=float(rp),
                    **{name: None if v is None else float(v) for name, v in flt.items()})

    def _lookup_params(self, input_ids, kwargs, do_sample, num_beams):
        """(k, m, sample) of prompt-lookup decoding, or None when prompt_lookup_num_tokens is not set (argument or generation_config); every
        refusal is raised here, before any work is enqueued"""
        from ..lookup import MAX_LOOKUP_TOKENS
        gc = self.generation_config
        k = kwargs.pop("prompt_lookup_num_tokens", None)
        m = kwargs.pop("max_matching_ngram_size", None)
        smp = kwargs.pop("prompt_lookup_sample", None)
        k = k if k is not None else getattr(gc, "prompt_lookup_num_tokens", None)
        if k is None:
            return None
        m = m if m is not None else (getattr(gc, "max_matching_ngram_size", None) or 2)
        smp = bool(smp if smp is not None else getattr(gc, "prompt_lookup_sample", False))
        if input_ids.shape[0] > 1:
            raise ValueError("assisted generate is only supported for batch_size = 1")
        if num_beams > 1 and smp:
            raise NotImplementedError("prompt_lookup_sample=True with num_beams > 1 is not implemented: prompt-lookup decoding has no beams")
        if do_sample and not smp:
            raise NotImplementedError("prompt-lookup decoding with do_sample=True is not implemented without prompt_lookup_sample=True: it "
                                      "verifies greedy picks only unless that keyword asks for the sampled verify step")
        if num_beams > 1:
            raise NotImplementedError("prompt-lookup decoding with num_beams > 1 is not implemented")
        if getattr(self.engine, "_fp8_kv", False):
            raise NotImplementedError("prompt-lookup decoding over the e4m3 KV cache is not implemented: enable_fp8_kv(False)")
        if vars(self.engine).get("_mxfp4_decode", False) and not vars(self.engine).get("_mxfp4_batched", False):
            raise NotImplementedError("prompt-lookup decoding with MXFP4 decode weights is not implemented: a verify step runs on the 16-bit "
                                      "weights, so one generation would mix two weight sets: enable_mxfp4_decode(False)")
        if int(k) <= 0 or int(m) <= 0:
            raise ValueError("Invalid max_matching_ngram_size or num_output_tokens")
        if int(k) > MAX_LOOKUP_TOKENS:
            raise ValueError(f"prompt_lookup_num_tokens={k} exceeds the limit of {MAX_LOOKUP_TOKENS} draft tokens per verify step")
        return int(k), int(m), bool(do_sample and smp)

    def _guidance_params(self, input_ids, images, attention_mask, kwargs, nb, num_return_sequences, suffixes, reuse):
        """dict(scale, neg_ids int64 [b, Tn] on the CPU, neg_images) of generate(guidance_scale=...), or None when guidance is off -- no
        scale (argument or generation_config) or a scale of 1, where HF adds no processor either and the negative arguments are ignored.
        The four keywords are popped from `kwargs`.  Every refusal is raised here, from host data alone, before any work is enqueued."""
        import math
        import numbers
        gc = self.generation_config
        def take(name):
            v = kwargs.pop(name, None)
            return v if v is not None else getattr(gc, name, None)
        scale, neg, neg_mask, neg_images = (take(n) for n in ("guidance_scale", "negative_prompt_ids", "negative_prompt_attention_mask",
                                                              "negative_images"))
        if scale is None:
            return None
        if isinstance(scale, bool) or not isinstance(scale, numbers.Real):
            raise ValueError(f"`guidance_scale` has to be a finite number, but is {scale!r}")
        scale = float(scale)
        if not math.isfinite(scale):
            raise ValueError(f"`guidance_scale` has to be a finite number, but is {scale}")
        if scale == 1.0:
            return None
        e = self.engine
        nret = num_return_sequences if num_return_sequences is not None else (getattr(gc, "num_return_sequences", None) or 1)
        k = kwargs.get("prompt_lookup_num_tokens", None)
        k = k if k is not None else getattr(gc, "prompt_lookup_num_tokens", None)
        if nb > 1:
            raise NotImplementedError("guidance_scale with num_beams > 1 is not implemented: every beam row would need its twin")
        if isinstance(nret, int) and nret > 1:
            raise NotImplementedError("guidance_scale with num_return_sequences > 1 is not implemented: every sibling row would need its twin")
        if suffixes is not None:
            raise NotImplementedError("guidance_scale with suffixes= is not implemented: the suffix rows share one prompt, the twins would not")
        if k is not None:
            raise NotImplementedError("guidance_scale with prompt_lookup_num_tokens is not implemented: a verify step runs one sequence")
        if reuse:
            raise NotImplementedError("guidance_scale with reuse_cache=True is not implemented: the kept cache holds one conversation, not its twin")
        if e.tp_size > 1:
            raise NotImplementedError("guidance_scale under tensor parallelism is not implemented: the vocabulary-parallel exchange of the two "
                                      "log-sum-exps is not built (DESIGN.md section 7)")
        if vars(e).get("_fp8_kv", False) or vars(e).get("_fp8_prefill", False):
            raise NotImplementedError("guidance_scale with the e4m3 KV cache or fp8 x fp8 prefill GEMMs is not implemented (DESIGN.md section 7)")
        ids = input_ids.detach().to("cpu", torch.int64)
        b = ids.shape[0]
        if attention_mask is not None and bool((attention_mask == 0).any()):
            raise NotImplementedError("guidance_scale over a padded batch (attention_mask with zeros) is not implemented: pad the prompts to "
                                      "equal length or use b = 1")
        V = e.c.t_vocab_total
        if neg is None:
            neg = ids[:, -1:]                                         # HF: the unconditional context is the last prompt token alone
        neg = torch.as_tensor(neg).detach().to("cpu", torch.int64)
        neg = neg.view(1, -1) if neg.dim() == 1 else neg
        if neg.dim() != 2 or neg.shape[0] != b or neg.shape[1] < 1:
            raise ValueError(f"negative_prompt_ids {tuple(neg.shape)} must have one non-empty row per row of input_ids ({b})")
        if neg_mask is not None:
            neg_mask = torch.as_tensor(neg_mask).detach().to("cpu")
            if tuple(neg_mask.shape) != tuple(neg.shape):
                raise ValueError(f"negative_prompt_attention_mask {tuple(neg_mask.shape)} must have the shape {tuple(neg.shape)} of negative_prompt_ids")
            if bool((neg_mask == 0).any()):
                raise NotImplementedError("guidance_scale over padded negative prompts (negative_prompt_attention_mask with zeros) is not "
                                          "implemented: pad them to equal length or use b = 1")
        if bool(((neg != IMAGE_TOKEN_INDEX) & ((neg < 0) | (neg >= V))).any()):
            raise ValueError(f"negative_prompt_ids holds an id outside the vocabulary [0, {V}) that is not the image sentinel {IMAGE_TOKEN_INDEX}")
        n_sent = int((neg == IMAGE_TOKEN_INDEX).sum())
        if n_sent and neg_images is None:
            raise ValueError(f"negative_prompt_ids holds the image sentinel {IMAGE_TOKEN_INDEX} and negative_images is None: pass the tiles it "
                             "stands for, or a text-only negative prompt")
        if neg_images is not None and not n_sent:
            raise ValueError(f"negative_images without the image sentinel {IMAGE_TOKEN_INDEX} in negative_prompt_ids: nothing would see them")
        if 2 * b > e.c.max_batch:
            raise ValueError(f"guidance_scale needs 2 * b = {2 * b} cache rows (the prompts and their twins): create the model with max_batch >= "
                             f"{2 * b} (it has {e.c.max_batch})")
        tiles = (_n_tiles(images) if bool((ids == IMAGE_TOKEN_INDEX).any()) else 0) + (_n_tiles(neg_images) if n_sent else 0)
        if tiles > e.c.max_tiles:
            raise ValueError(f"guidance_scale: images and negative_images hold {tiles} tiles together, the model was created with max_tiles = {e.c.max_tiles}")
        len_c = self._spliced_lengths(ids, images)
        len_n = self._spliced_lengths(neg, neg_images)
        if len(set(len_c)) > 1:
            raise NotImplementedError("guidance_scale over rows of different spliced length is not implemented: pad the prompts to equal "
                                      "length or use b = 1")
        if len(set(len_n)) > 1:
            raise NotImplementedError("guidance_scale over negative prompts of different spliced length is not implemented: pad them to equal "
                                      "length or use b = 1")
        S = max(len_c[0], len_n[0])
        if S + 1 > e.c.max_seq or 2 * b * S > e.c.max_prefill_rows:
            raise ValueError(f"guidance_scale: 2 * b = {2 * b} rows of up to {S} slots do not fit max_seq = {e.c.max_seq} / max_prefill_rows = "
                             f"{e.c.max_prefill_rows}")
        return dict(scale=scale, neg_ids=neg, neg_images=neg_images)

    def _forward_guided(self, input_ids, images, gd):
        """The prefill of generate(guidance_scale=...) (the arguments went through _guidance_params): the b prompts and their b twins -- the
        negative prompts, spliced with negative_images or text-only -- as ONE right-padded ragged batch of 2b rows, every row at its own
        length; the tower runs once over the tiles of both.  -> forward()'s output with `local_logits` [2b, V], rows [b, 2b) the twins'."""
        e = self.engine
        ids = input_ids.detach().to("cpu", torch.int64)
        neg = gd["neg_ids"]
        b = ids.shape[0]

        def tiles(im, rows):
            if im is None or self.get_vision_tower() is None or not bool((rows == IMAGE_TOKEN_INDEX).any()):
                return None
            if type(im) is list:
                if any(t.ndim != 3 for t in im):
                    raise NotImplementedError("video inputs: the reference calls an undefined encode_videos (omchat_arch.py:87)")
                im = torch.stack(im)
            elif im.ndim == 5:
                raise NotImplementedError("video inputs: the reference calls an undefined encode_videos (omchat_arch.py:87)")
            return im
        px_c, px_n = tiles(images, ids), tiles(gd["neg_images"], neg)
        px = [p for p in (px_c, px_n) if p is not None]
        feats = self.encode_images(torch.cat([p.to(px[0].device, px[0].dtype) for p in px])) if px else None
        n_c = 0 if px_c is None else px_c.shape[0]
        maxlen = getattr(self.config, "tokenizer_model_max_length", None)
        emb_c, len_c, _ = e.splice(ids, None, None if px_c is None else feats[:n_c], "right", maxlen)
        emb_n, len_n, _ = e.splice(neg, None, None if px_n is None else feats[n_c:], "right", maxlen)
        S = max(emb_c.shape[1], emb_n.shape[1])
        embeds = torch.zeros(2 * b, S, emb_c.shape[2], dtype=emb_c.dtype, device=emb_c.device)
        embeds[:b, :emb_c.shape[1]] = emb_c
        embeds[b:, :emb_n.shape[1]] = emb_n
        logits, _ = e.prefill(embeds, list(len_c) + list(len_n))
        self._padded_batch = False
        self._last_lengths = None
        self._prefill_slots = S
        out = CausalLMOutputWithPast(e.full_logits(logits[:b]).unsqueeze(1), KVHandle(e, 2 * b))
        out.local_logits = logits
        return out

    @torch.no_grad()
    def generate(self, input_ids=None, images=None, do_sample=None, temperature=None, max_new_tokens=None, streamer=None, use_cache=True,
                 eos_token_id=None, pad_token_id=None, attention_mask=None, stopping_criteria=None, top_k=None, top_p=None,
                 repetition_penalty=None, seed=None, generator=None, num_beams=None, length_penalty=None, early_stopping=None,
                 num_return_sequences=None, return_dict_in_generate=False, reuse_cache=None, output_logprobs=None, share_prompt=None,
                 top_logprobs=None, score_token_ids=None, suffixes=None, token_fsm=None, fsm_start=None, **kwargs):
        """The loop HF GenerationMixin drives for single_inference.py:53-62, stop on EOS (kept in the output) or max_new_tokens; returns
        prompt + new ids [b, T + new].  Greedy: argmax of the last position (first index wins).  do_sample=True: the on-device sampler
        (omchat_set_sampling) with HF's order and defaults -- repetition penalty over the prompt's ids (the -200 image sentinel never counts)
        and the generated ones, temperature, top-k, top-p, then min_p, typical_p, epsilon_cutoff, eta_cutoff (HF's warpers of those names,
        taken from the call or generation_config) -- keyed by `seed` (or one drawn from `generator`); same ids for the same seed.
        prompt_lookup_num_tokens=k (max_matching_ngram_size=m, default 2; both also read from generation_config): HF's prompt-lookup
        decoding for b = 1, greedy (omchat_amd/lookup.py): drafts of up to k ids copied from the prompt + generated ids are verified in
        one verify step each.  With do_sample=True it needs prompt_lookup_sample=True (also read from generation_config; no effect when
        greedy): every verify row is then sampled on the device with the key and seen set the plain sampled loop would have at that
        position, so the call returns the ids of the same call without prompt_lookup_num_tokens ("Sampling").  Exactness: the verify rows go through the batched (MFMA-form) GEMVs and plain steps through the batch-1
        whole-row forms, so a position's logits can differ in the last bits and the ids can differ from greedy only at near-ties, as in
        HF's assisted decoding in fp16.
        reuse_cache=True (also read from generation_config; b = 1, num_beams = 1, no padding): multi-turn chat.  The
        call records what sequence 0's cache holds when it returns; the next reuse_cache=True call keeps the longest common prefix of that
        record and its own prompt -- tiles are compared bit for bit, equal ones reuse their feature rows -- and prefills only the rest
        (Engine.prefill_extend).  Kept slots written by decode steps came from the GEMV forms, so a position's logits can differ in the
        last bits from a fresh prefill's, and ids at near-ties only.  Default False: nothing is kept.
        no_repeat_ngram_size, bad_words_ids, min_new_tokens, min_length, suppress_tokens, begin_suppress_tokens (also read from
        generation_config): HF's processors of the same names as a ban stage on the device in front of the pick,
        greedy or sampled; refused with num_beams > 1 (unless beam_processors=True) and with prompt_lookup_num_tokens.
        beam_processors=True with num_beams > 1 (also read from generation_config; ignored with num_beams == 1): the
        beam search ranks processed scores as HF's _beam_search does -- per beam row log_softmax, then repetition_penalty (any value > 0)
        on the log-probabilities of the ids of the row's own history (prompt row + the ids along that beam's path), then the six token
        bans above, then + the running score.  The histories follow the beams on the device.  Without the keyword these arguments are
        refused under num_beams > 1, as before; with it and nothing set the call is the plain beam search, bit for bit.  Refused from host
        data, before any work: tensor parallelism (NotImplementedError); a penalty <= 0; lists and lengths that could leave a beam row
        fewer than max(2, 1 + n_eos) * num_beams finite scores -- vocabulary - (suppress_tokens + begin_suppress_tokens + bad words + EOS
        ids + prompt tokens + max_new_tokens) below that number (ValueError); and what the plain beam search refuses (do_sample, streamer,
        stopping_criteria, token_fsm, guidance_scale, dola_layers, padded or ragged rows).
        output_logprobs=True with return_dict_in_generate=True (also read from generation_config): returns a
        GenerateOutput whose .sequences is what the call returns otherwise, .logprobs [b, new] the log-probability of every generated id
        under the model's raw distribution and .processed_logprobs [b, new] under the distribution the pick was made from (bans, repetition
        penalty, temperature, top-k / top-p and the four filters behind them); recorded by the pick on the device, read back once at the end.  Positions behind a row's EOS,
        where the sequence holds pad, are 0.  Refused with num_beams > 1 (sequences_scores) and with prompt_lookup_num_tokens.
        top_logprobs=n (1..20) and score_token_ids=[...] (1..32 distinct ids of the vocabulary), each with output_logprobs=True (also read
        from generation_config): the output also carries .top_logprobs / .top_token_ids [b, new, n] -- the n most likely ids of every
        position under the raw distribution, by log-probability descending, then id ascending -- and .scored_logprobs [b, new, k], the raw
        log-probability of the listed ids at every position (multiple-choice scoring); selected and recorded on the device like the two
        numbers above.  Behind a row's EOS: 0.0 / -1 / 0.0.
        num_return_sequences=N with do_sample=True and num_beams == 1 (also read from generation_config): returns
        [b * N, T + new], prompt-major (rows i*N .. i*N+N-1 belong to prompt i, HF's _expand_inputs_for_generation order); log-prob fields
        [b * N, new].  Each prompt is prefilled ONCE -- every sibling sees its own prompt's tiles, as under beam search -- and row i*N + j
        samples with its own row key from the first token on.  share_prompt: False = the prompt's cache slots are forked into the N rows and
        the plain batched step runs; True = the rows of a prompt share its slots and the decode step's attention reads them once per prompt
        (16-bit KV cache, one GPU, N <= 16; NotImplementedError otherwise); None = the engine's rule (Engine.group_share_default).  Refused:
        padded or ragged batches, reuse_cache=True, prompt_lookup_num_tokens and a streamer when b * N > 1.
        suffixes=[ids_0, ..., ids_{N-1}] with input_ids [1, T]: one prompt, N >= 1 text-id suffixes of any lengths
        S_j >= 1 (lists or 1-D tensors).  Row j stands for the sequence input_ids[0] + suffixes[j], and its result is that of generate() on
        that concatenated prompt alone at b = 1 -- no pads in the cache, positions 0 .. P + S_j - 1, the image tiles seen by every row -- to
        rounding (ids can differ at near-ties only, as under reuse_cache).  This is NOT what HF computes for the same rows as a padded
        batch (pads in the cache, positions from the mask arithmetic): rows that only differ in their question want the b = 1 result.  The
        tower, the splice and the prompt's prefill run ONCE, the N suffixes are prefilled in one pass over the weights
        (Engine.prefill_suffixes), then the ordinary decode loop runs over N rows of different lengths.  Returns [N, new]: the generated
        ids only (the rows have no common prompt length), the pad id behind a row's EOS; with return_dict_in_generate=True that is
        .sequences and the log-prob fields keep their [N, new, ...] shapes.  Greedy and do_sample=True (row j samples with the key of row
        j; the repetition penalty's seen set and the ban history of row j are prompt + suffix_j), all sampling parameters and filters, the
        token-banning arguments, output_logprobs / top_logprobs / score_token_ids, the decode graph and MXFP4 decode.  stopping_criteria are
        handed the per-row full sequences prompt + suffix_j + generated_j, right-padded with the pad id (0 without one) to the longest row.
        share_prompt as for sampled groups: False = the prompt's slots are forked into the N rows, True = shared (16-bit cache, one GPU,
        N <= 16, N * n_rep <= 128; NotImplementedError otherwise), None = Engine.group_share_default.  Refused from host data, before
        anything is enqueued: input_ids of more than one row, an attention_mask with zeros, an empty list or suffix, an id < 0 or >= the
        vocabulary, N > max_batch, N * max S_j > max_prefill_rows, num_beams > 1, num_return_sequences > 1, prompt_lookup_num_tokens,
        reuse_cache=True, a streamer when N > 1, the e4m3 KV cache / fp8 prefill GEMMs / tensor parallelism (NotImplementedError); and
        P + max S_j + 1 > max_seq right after the splice plan, before the tower runs.
        token_fsm=TokenFSM (omchat_amd/fsm.py): a deterministic automaton over token ids -- the index a grammar or regex
        compiler builds -- constrains the form of the answer on the device: row r is in one state, only the ids that are edges of that
        state can be picked (greedy or sampled, in front of the warpers like HF's PrefixConstrainedLogitsProcessor, behind the token-banning
        arguments when both are given), and every decode step moves the state over the token it is fed.  fsm_start: the start state -- one
        int, or a list with one per prompt (repeated for the siblings of num_return_sequences / suffixes=) or one per row of the expanded
        batch; default 0.  A row that is fed a token without an edge (the pad behind its EOS) is no longer masked.  With
        return_dict_in_generate=True the output carries .fsm_states [rows]: omchat_amd.fsm.DEAD (-1) for a row that ended with an EOS, else
        the state the row stopped in (an answer cut by max_new_tokens).  Refused with num_beams > 1 and with prompt_lookup_num_tokens
        (NotImplementedError), and for a start state out of range or without an edge (ValueError).  HF's prefix_allowed_tokens_fn itself
        stays refused: TokenFSM.as_prefix_allowed_tokens_fn gives the callback that computes the same constraint there.
        guidance_scale=s with negative_prompt_ids [b, Tn] (negative_prompt_attention_mask, negative_images; all also read from
        generation_config): HF's UnbatchedClassifierFreeGuidanceLogitsProcessor on the device.  Prompt row r gets a
        twin cache row that holds the negative prompt -- negative_prompt_ids=None: the last prompt token alone, as HF does --, all 2b rows
        are prefilled as one ragged batch and decoded at their own lengths, and every pick of row r runs on
        s * (lc - lu) + lu, lc / lu the log-softmax of the row's and of the twin's logits, in front of the token-banning arguments, the
        automaton and the argmax or sampler; the id picked for row r is fed to its twin too.  negative_images (this project's extension):
        None = the twin is text-only, which is what HF's processor computes (it calls the model without `images`); otherwise the -200
        sentinels of negative_prompt_ids are spliced with those tiles -- the same question over a blank or another picture (visual
        contrastive decoding).  s of None or 1: nothing happens -- no twin rows, the launches and ids of a call without the keyword (HF
        adds the processor only when the scale is not 1).  Ban history, the penalty's seen set, automaton states, log-prob records,
        stopping criteria, the streamer and the returned sequences belong to the b prompt rows; .logprobs is the prompt row's raw
        log-softmax, .processed_logprobs that of the guided scores as the pick saw them.  Works greedy and with do_sample=True (all
        parameters and filters), with the decode graph and MXFP4 decode (a guided b = 1 step is a 2-row step: batched=True).  Refused from
        host data, before any work (_guidance_params): NotImplementedError for num_beams > 1, num_return_sequences > 1, suffixes=,
        prompt_lookup_num_tokens, reuse_cache=True, padded or ragged prompt rows or negative rows, tensor parallelism, the e4m3 KV cache
        and fp8 prefill GEMMs; ValueError for a scale that is no finite number, another row count than input_ids', ids outside the
        vocabulary other than -200, -200 without negative_images (or negative_images without -200), 2b > max_batch, more tiles than
        max_tiles, rows that do not fit max_seq / max_prefill_rows.
        dola_layers='low' | 'high' | [indices] with dola_relative_top (default 0.1) and dola_norm (all also read from generation_config;
        DESIGN.md section 22): HF's DoLa decoding (Chuang et al., "Decoding by Contrasting Layers") on the device.  The indices count HF's
        hidden_states -- 0 the embedding row, i the residual stream behind decoder layer i --; 'low' and 'high' resolve as HF's do
        (omchat_amd/dola.py).  At every pick each row's last-position hidden state at the k candidate layers goes through the head with the
        final row, in one pass over the head and without a second pass over the decoder; the candidate with the largest Jensen-Shannon
        divergence from the final row's distribution is contrasted with it: lm - lp on the ids with lm >= max lm + log(dola_relative_top),
        -inf elsewhere, in front of the token-banning arguments, the automaton and the argmax or sampler.  The candidate rows skip the
        final norm, as in HF; dola_norm=True (this project's extension) normalises them too.  Every row picks its own layer (HF averages
        the divergence over the batch: the same at b = 1; at b > 1 a row gets what it would get alone).  dola_layers=None: nothing happens
        -- the launches and ids of a call without the keyword.  .logprobs stays the final row's raw log-softmax, .processed_logprobs is what
        the pick saw; with return_dict_in_generate=True the output carries .dola_premature_layers [b, new]: the index of the layer every
        pick contrasted with, -1 behind a row's EOS.  Works greedy and with do_sample=True (all parameters and filters), with the ban
        arguments, token_fsm, output_logprobs and its extras, a streamer, stopping criteria and the decode graph.  Refused from host data,
        before any work (omchat_amd/dola.py): NotImplementedError for num_beams > 1, guidance_scale, num_return_sequences > 1, suffixes=,
        prompt_lookup_num_tokens, reuse_cache=True, padded or left-padded batches, tensor parallelism and the fp8 / MXFP4 decode modes;
        ValueError for a value that is none of the three forms, a negative or repeated index, no index below num_hidden_layers, more than
        16 layers, a dola_relative_top outside (0, 1], (k + 1) * b > min(max_batch, 32).  Not pinned against HF: transformers 5 moved DoLa
        out of the library; tests/dola_ref.py restates HF 4.4x's functions.
        penalty_alpha=a with top_k=k (both also read from generation_config): HF's contrastive search (Su et al., "A
        Contrastive Framework for Neural Text Generation") on the device, selected by HF's rule -- num_beams == 1, do_sample false,
        penalty_alpha > 0, top_k > 1; in every other case the call is the call without the keyword.  Per emitted id the k likeliest ids
        (ties to the lower id) run as the k rows of ONE decode step over the same cache -- the prompt row is forked into k rows once, or
        shared by them: share_prompt as for sampled groups -- and the id that maximises (1 - a) p_i - a max_j cos(h_i, H_j) is emitted
        (the first maximum), H the post-final-norm hidden rows of all earlier positions, image rows included; only the one new cache slot
        of the picked row is copied to the other rows.  Works with images, max_new_tokens, eos_token_id, stopping_criteria, a streamer, the
        decode graph and enable_mxfp4_decode(True, batched=True).  With return_dict_in_generate=True the output carries
        .contrastive_ranks [1, new] (the emitted id's rank among the candidates) and .degeneration_penalties [1, new] (its penalty).
        Refused from host data, before any work (omchat_amd/contrastive.py): NotImplementedError for b > 1, an attention_mask with zeros,
        num_return_sequences > 1, suffixes=, prompt_lookup_num_tokens, reuse_cache=True, guidance_scale, dola_layers, token_fsm, the
        token-banning arguments, repetition_penalty != 1, output_logprobs, tensor parallelism, the e4m3 KV cache, fp8 prefill GEMMs and
        batch-1-only MXFP4; ValueError for penalty_alpha > 1, top_k > min(16, max_batch) (generation_config.top_k defaults to 50: pass
        top_k), more than 8 distinct EOS ids (the device's done word knows 8) and prompt + max_new_tokens > max_seq.  The host reads every
        emitted id behind an event before it enqueues the next step (the search has no rewind), so the device idles for one host round
        trip per token.  Not pinned against HF: transformers 5 moved the strategy out of the library;
        tests/contrastive_ref.py restates HF 4.4x's loop."""
        if do_sample is None:
            do_sample = bool(getattr(self.generation_config, "do_sample", False))
        gc = self.generation_config
        nb = int(num_beams if num_beams is not None else (getattr(gc, "num_beams", None) or 1))
        reuse = bool(reuse_cache if reuse_cache is not None else getattr(gc, "reuse_cache", False))
        if reuse:      # every refusal before any work
            from ..prefix import check_reuse_args
            check_reuse_args(input_ids.shape[0], nb, None if attention_mask is None else attention_mask.tolist(),
                             getattr(self.config, "tokenizer_padding_side", "right"))
            if getattr(self.engine, "_fp8_kv", False) or getattr(self.engine, "_fp8_prefill", False) or self.engine.tp_size > 1:
                raise NotImplementedError("reuse_cache=True with the e4m3 KV cache, fp8 x fp8 prefill GEMMs or tensor parallelism is not "
                                          "implemented (DESIGN.md section 7)")
        # classifier-free guidance: resolved and refused from host data, before any work
        gd = self._guidance_params(input_ids, images, attention_mask, kwargs, nb, num_return_sequences, suffixes, reuse)
        # layer-contrastive decoding: resolved and refused from host data, before any work
        from .. import dola as _dola
        dl = _dola.resolve_dola(gc, kwargs, lambda: self.engine.c.t_layers, bool(getattr(self.config, "tie_word_embeddings", False)))
        if dl is not None:
            e = self.engine
            nret = num_return_sequences if num_return_sequences is not None else (getattr(gc, "num_return_sequences", None) or 1)
            plk = kwargs.get("prompt_lookup_num_tokens", None)
            plk = plk if plk is not None else getattr(gc, "prompt_lookup_num_tokens", None)
            ragged = input_ids.shape[0] > 1 and len(set(self._spliced_lengths(input_ids.detach().to("cpu", torch.int64), images))) > 1
            _dola.refuse(input_ids.shape[0], len(dl["layers"]), e.c.max_batch, nb, gd is not None, nret, suffixes is not None, plk is not None, reuse,
                         ragged or (attention_mask is not None and bool((attention_mask == 0).any())), e.tp_size,
                         vars(e).get("_fp8_decode", False), vars(e).get("_mxfp4_decode", False))
        # contrastive search: HF's mode rule; resolved and refused from host data, before any work
        from .. import contrastive as _cs
        cs = _cs.resolve_contrastive(gc, kwargs, top_k, do_sample, nb, lambda: self.engine.c.max_batch)
        if cs is not None:
            e = self.engine
            nret = num_return_sequences if num_return_sequences is not None else (getattr(gc, "num_return_sequences", None) or 1)
            plk = kwargs.get("prompt_lookup_num_tokens", None)
            plk = plk if plk is not None else getattr(gc, "prompt_lookup_num_tokens", None)
            rp = repetition_penalty if repetition_penalty is not None else getattr(gc, "repetition_penalty", None)
            olp_ = bool(output_logprobs if output_logprobs is not None else getattr(gc, "output_logprobs", False))
            _cs.refuse(input_ids.shape[0], attention_mask is not None and bool((attention_mask == 0).any()), nret, suffixes is not None,
                       plk is not None, reuse, gd is not None, dl is not None, token_fsm is not None, False, rp, olp_, e.tp_size,
                       vars(e).get("_fp8_kv", False), vars(e).get("_fp8_prefill", False), vars(e).get("_mxfp4_decode", False),
                       vars(e).get("_mxfp4_batched", False), share_prompt, e.group_share_refusal(cs["k"]))
            cs["max_new"] = int(max_new_tokens if max_new_tokens is not None else (gc.max_new_tokens or 20))
            if cs["max_new"] < 1:
                raise ValueError(f"`max_new_tokens` has to be a strictly positive integer, but is {cs['max_new']}")
            eos_cs = eos_token_id if eos_token_id is not None else gc.eos_token_id
            _cs.check_eos(list(eos_cs) if isinstance(eos_cs, (list, tuple)) else ([eos_cs] if eos_cs is not None else []))
            _cs.check_room(self._spliced_lengths(input_ids.detach().to("cpu", torch.int64), images)[0], cs["max_new"], e.c.max_seq)
        sfx = None
        if suffixes is not None:      # every refusal that host data decides, before any work (and before the other modes' own refusals)
            sfx = self._suffix_params(input_ids, images, attention_mask, suffixes, nb, num_return_sequences, share_prompt, reuse, kwargs, streamer)
        lookup = self._lookup_params(input_ids, kwargs, do_sample, nb)
        group = None if sfx is not None else self._group_params(input_ids, images, attention_mask, nb, do_sample, num_return_sequences, share_prompt, reuse, lookup, streamer)
        olp = bool(output_logprobs if output_logprobs is not None else getattr(gc, "output_logprobs", False))
        top_n, score_ids = resolve_logprob_extras(gc, olp, top_logprobs, score_token_ids, self.engine.c.t_vocab_total)
        if olp:      # every refusal before any work
            if not return_dict_in_generate:
                raise ValueError("output_logprobs=True needs return_dict_in_generate=True: the log-probabilities come back as fields of a "
                                 "GenerateOutput next to .sequences")
            if nb > 1:
                raise NotImplementedError("output_logprobs=True with num_beams > 1 is not implemented: beam search reports sequences_scores")
            if lookup is not None:
                raise NotImplementedError("output_logprobs=True with prompt_lookup_num_tokens is not implemented: a verify step's picks are "
                                          "not recorded")
        # HF's token-banning arguments (omchat_amd/constraints.py): resolved and refused here, before any work
        from ..constraints import resolve_constraints
        eos_ids = eos_token_id if eos_token_id is not None else gc.eos_token_id
        eos_ids = list(eos_ids) if isinstance(eos_ids, (list, tuple)) else ([eos_ids] if eos_ids is not None else [])
        bp = kwargs.pop("beam_processors", None)      # (ignored with num_beams == 1: the greedy and sampled paths have both stages already)
        bp = bool(bp if bp is not None else getattr(gc, "beam_processors", False)) and nb > 1
        con = resolve_constraints(gc, kwargs, eos_ids, self.engine.c.t_vocab_total, nb, lookup is not None, beam_processors=bp)
        if cs is not None and con is not None:
            _cs.refuse(banning=True)
        # the token automaton (omchat_amd/fsm.py): one start state per row of the expanded batch, refused here too
        from ..fsm import resolve_token_fsm
        n_prompts = input_ids.shape[0]
        n_rows = len(sfx[0]) if sfx is not None else n_prompts * (group[0] if group is not None else 1)
        fsm_rows = resolve_token_fsm(token_fsm, fsm_start, n_prompts, n_rows, self.engine.c.t_vocab_total, nb, lookup is not None)
        # the sampling arguments are resolved and refused here too, before the sticky state below is touched (beam search refuses do_sample itself)
        smp = self._sampling_params(temperature, top_k, top_p, repetition_penalty, seed, generator, kwargs) if do_sample and nb == 1 else None
        for name in ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff"):      # do_sample=False (or beam search): ignored, as HF ignores them
            kwargs.pop(name, None)
        if con is None or bp:                                         # sticky context state, like the sampler: off unless this call sets it
            self.engine.constraints_off()                             # (set below, after the prefill; equal parameters keep the decode graphs)
        if not olp and getattr(self.engine, "_logprobs_on", False):   # sticky too: a call without the keyword records nothing
            self.engine.logprobs_off()
        if fsm_rows is None and vars(self.engine).get("_fsm_on", False):      # sticky too: a call without the keyword is unconstrained
            self.engine.token_fsm_off()
        if gd is None and vars(self.engine).get("_guidance_on", False):      # sticky too: a call without the keyword (or with scale 1) is unguided
            self.engine.guidance_off()
        if dl is None and vars(self.engine).get("_dola", None) is not None:      # sticky too: a call without the keyword contrasts nothing
            self.engine.dola_off()
        if vars(self.engine).get("_cs", None) is not None:      # sticky too (a call that raised midway): a call starts with the mode off
            self.engine.group_end()
            self.engine.contrastive_off()
        if cs is not None:
            return self._contrastive_generate(input_ids, images, attention_mask, cs, streamer, eos_ids, stopping_criteria, share_prompt,
                                              return_dict_in_generate)
        if nb > 1:
            return self._beam_generate(input_ids, images, attention_mask, nb, do_sample, max_new_tokens, streamer, eos_token_id, pad_token_id,
                                       stopping_criteria, repetition_penalty, length_penalty, early_stopping, num_return_sequences,
                                       return_dict_in_generate, bp, con)
        if max_new_tokens is None:
            max_new_tokens = self.generation_config.max_new_tokens or 20
        eos = eos_token_id if eos_token_id is not None else self.generation_config.eos_token_id
        eos = set(eos) if isinstance(eos, (list, tuple)) else ({eos} if eos is not None else set())
        pad = pad_token_id if pad_token_id is not None else self.generation_config.pad_token_id
        b = input_ids.shape[0]
        hist = None      # generate(suffixes=): row j's history, prompt + suffix_j
        if sfx is not None:
            from ..suffix import histories, padded_sequences
            hist = histories(input_ids[0].tolist(), sfx[0])
        if streamer is not None:
            streamer.put(input_ids.cpu() if hist is None else torch.tensor(hist, dtype=torch.int64))      # (a streamer: N == 1)
        prompt_slots = None
        if sfx is not None:
            out = self._forward_suffixes(input_ids, images, attention_mask, sfx[0], sfx[1])
            b = len(sfx[0])
        elif reuse:
            out, prompt_slots = self._forward_reuse(input_ids, images)
        elif gd is not None:
            out = self._forward_guided(input_ids, images, gd)         # 2b rows: the prompts, then their twins over the negative prompts
        else:
            if dl is not None:                                        # before the prefill: the first id comes from its candidate rows
                self.engine.set_dola(b, dl["layers"], dl["relative_top"], dl["norm"])
            out = self.forward(input_ids=input_ids, attention_mask=attention_mask, images=images, use_cache=True)
        # ONE rule for the first token at every TP degree: omchat_greedy on this rank's vocabulary shard -- local first-index-wins argmax,
        # then the (max, index) exchange the decode step uses (pick.hip: greedy_pick); no torch re-statement on the gathered logits.
        # Sampling: the same seam with the sampler (omchat_sample); the decode steps below then sample too, the penalty's seen set growing
        # on the device.  HF drives the processors with input_ids (the prompt, pads included) + the generated ids.
        local_logits = out.local_logits
        if group is not None:
            # one prefill per prompt, then b * N rows, prompt-major: from here on the call is the sampled loop of the expanded batch
            N, share = group
            lens = self.engine.kv_lengths(b)
            if getattr(self, "_padded_batch", False) or len(set(lens)) > 1:
                raise NotImplementedError("num_return_sequences > 1 over rows of different spliced length is not implemented: pad the prompts "
                                          "to equal length or use b = 1")
            if share is None:
                share = self.engine.group_share_default(N, lens[0])
            self.engine.group_begin(b, N, lens[0], share)
            local_logits = local_logits.repeat_interleave(N, dim=0)
            input_ids = input_ids.repeat_interleave(N, dim=0)
            b = b * N
        if con is not None:
            # the history HF's processors see: the prompt rows as passed (-200 sentinels and pads included) + the ids every step is fed
            self.engine.set_constraints(b, input_ids.tolist() if hist is None else hist, max_new_tokens, **con)
        if fsm_rows is not None:
            self.engine.load_token_fsm(token_fsm)                     # (the same object as last time: the table and the graphs stay)
            self.engine.token_fsm_begin(b, fsm_rows, max_new_tokens)
        if olp:
            self.engine.set_logprobs(b, max_new_tokens, top_n, score_ids)      # the prefill's pick below is record 0
        # every stage above keeps b rows; under guidance the picks and steps below run 2b rows -- `tok` holds the b picked ids, then the
        # twins' copies of them -- and the host looks at the first b
        rows = b
        if gd is not None:
            self.engine.set_guidance(b, gd["scale"])
            rows = 2 * b
        if smp is not None:
            seen = [[int(i) for i in row if int(i) >= 0] for row in (input_ids.tolist() if hist is None else hist)]
            self.engine.set_sampling(b, seen=seen, **smp)
            tok = self.engine.sample(local_logits)
        else:
            self.engine.sampling_off()
            tok = self.engine.argmax(local_logits)
        padded = getattr(self, "_padded_batch", False)
        # The KV cache is context-owned with a fixed capacity (the reference's DynamicCache grows without bound): generate as
        # many tokens as fit and stop cleanly, returning what was produced, instead of failing mid-stream with 'KV cache full'.
        # A padded batch appends at the COMMON slot (omchat_arch.py:61-70: the cache length, pads included), so its room is counted from
        # there, not from the longest row's own length
        used = self._prefill_slots if padded else max(self.engine.kv_lengths(rows))      # (under guidance: the longest of the 2b rows)
        room = self.engine.c.max_seq - used + 1
        if max_new_tokens > room:
            import warnings
            warnings.warn(f"max_new_tokens={max_new_tokens} clamped to {room}: KV cache capacity max_seq={self.engine.c.max_seq}")
            max_new_tokens = max(room, 1)
        if lookup is not None:
            from ..lookup import lookup_loop
            gen = lookup_loop(self.engine, input_ids, int(tok.view(-1)[0]), max_new_tokens, eos, lookup[0], lookup[1],
                              self.engine.c.t_vocab_total, streamer, stopping_criteria, getattr(self, "_lookup_draft_hook", None),
                              self.engine.verify_max_tokens(), sample=lookup[2])
            if streamer is not None:
                streamer.end()
            self._record_prefix(prompt_slots, gen)
            return torch.cat([input_ids.cpu(), torch.tensor([gen], dtype=torch.int64)], dim=1)
        new, padded_out, padded_out_eos = [], [], []                  # (padded_out_eos: the rows already ended, whatever the pad id)
        done = torch.zeros(b, dtype=torch.bool)
        # padded batch (rows of different spliced length, or left padding): decoded as the reference does it (omchat_arch.py:61-70).  HF generate
        # passes the token-level mask grown by one 1 per generated token and `images` on every step; the decode branch pads it with ones to the
        # cache length and takes position_ids = sum(mask) - 1.  Over the cache slots that key mask is the same at every step -- [prompt mask |
        # ones] -- and the positions grow by one, so the branch is evaluated ONCE here (this class's mirror of it) and handed to the engine
        # (masked_decode_begin); the steps then need no host data and run ahead of the host exactly like the unpadded ones.
        if padded and max_new_tokens > 1:                             # (one token = the prefill's: no decode step is enqueued, nothing to begin)
            tok_mask = (attention_mask if attention_mask is not None else torch.ones_like(input_ids)).to("cpu", torch.long)
            m1 = torch.cat([tok_mask, torch.ones(b, 1, dtype=torch.long)], dim=1)
            _, pos1, mask1, _, _, _ = self.prepare_inputs_labels_for_multimodal(torch.zeros(b, 1, dtype=torch.long), None, m1, out.past_key_values,
                                                                                None, images)
            if pos1 is None:          # text-only: Qwen2Model positions every row at the common cache length (modeling_qwen2.py:368-373)
                pos1 = torch.full((b, 1), out.past_key_values.get_seq_length(), dtype=torch.long)
            self.engine.masked_decode_begin(pos1, mask1)
        step_fn = self.engine.decode_step_masked_next if padded else self.engine.decode_step
        # The host looks at every token (EOS, streamer, stopping criteria) as the reference's HF loop does -- but not with the GPU idle:
        # token k is copied to pinned host memory behind an event, step k + 1 is enqueued, and only then the host waits for the event.
        # When token k ends the generation the step that was already enqueued is taken back (omchat_kv_rewind).
        stage = self._stage_buffer(max_new_tokens, b)
        evt = self._stage_event
        for step in range(max_new_tokens):
            last = step == max_new_tokens - 1
            stage[step].copy_((tok if gd is None else tok[:b]).to(torch.int32), non_blocking=True)
            evt.record()
            ahead = None
            if not last:
                # rows that already ended are fed the pad id, as HF's loop does (their cache content then equals the reference's too)
                feed = tok if (pad is None or not bool(done.any())) else torch.where(done.repeat(rows // b).to(tok.device), torch.full_like(tok, pad), tok)      # (an ended row's twin is fed the pad too)
                ahead, _ = step_fn(feed)                              # runs while the host handles token `step`
            evt.synchronize()
            t_cpu = stage[step].to(torch.int64)
            if pad is not None:
                t_cpu = torch.where(done, torch.full_like(t_cpu, pad), t_cpu)
            new.append(t_cpu)
            padded_out.append(done if pad is not None else torch.zeros_like(done))
            padded_out_eos.append(done)
            if streamer is not None:
                streamer.put(t_cpu)
            done = done | torch.tensor([int(x) in eos for x in t_cpu])
            stop = bool(done.all()) or last
            if not stop and stopping_criteria:                        # HF StoppingCriteriaList semantics: any criterion stops the batch
                if hist is None:
                    so_far = torch.cat([input_ids.cpu(), torch.stack(new, dim=1)], dim=1)
                else:
                    so_far = torch.tensor(padded_sequences(input_ids[0].tolist(), sfx[0], torch.stack(new, dim=1).tolist(), pad), dtype=torch.int64)
                stop = any(bool(c(so_far, None)) for c in stopping_criteria)
            if stop:
                if ahead is not None:
                    self.engine.kv_rewind(rows, 1)
                break
            tok = ahead
        if streamer is not None:
            streamer.end()
        self._record_prefix(prompt_slots, [int(t[0]) for t in new])
        seqs = torch.cat([input_ids.cpu(), torch.stack(new, dim=1)], dim=1) if hist is None else torch.stack(new, dim=1)
        fsm_states = None
        if fsm_rows is not None and return_dict_in_generate:
            # the device holds the rows' states after every token that was fed: all but the last one emitted (the step enqueued ahead of an
            # EOS was taken back with its state).  A row that ended is DEAD by definition; the others take the last transition here
            from ..fsm import DEAD
            dev = self.engine.token_fsm_states(b)
            fsm_states = torch.tensor([DEAD if bool(done[r]) else token_fsm.next(dev[r], int(new[-1][r])) for r in range(b)], dtype=torch.int64)
        dola_rec = None
        if dl is not None and return_dict_in_generate:
            # one line per pick that was not taken back; behind a row's EOS the row was fed the pad and its picks count for nothing
            dola_rec = torch.where(torch.stack(padded_out_eos, dim=1), torch.full((), -1, dtype=torch.int64), self.engine.dola_record(b, len(new)))
        if not olp:
            if fsm_states is None and dola_rec is None:
                return seqs
            res = GenerateOutput(seqs, None, None)
            if fsm_states is not None:
                res.add("fsm_states", fsm_states)
            if dola_rec is not None:
                res.add("dola_premature_layers", dola_rec)
            return res
        # the step enqueued ahead was taken back with its record: exactly one record per generated token
        raw, proc, counts = self.engine.read_logprobs(b)
        if counts != [len(new)] * b:
            raise RuntimeError(f"log-probability record out of step with the generated tokens: {counts} records for {len(new)} tokens")
        keep = ~torch.stack(padded_out, dim=1)
        zero = torch.zeros((), dtype=torch.float32)
        res = GenerateOutput(seqs, torch.where(keep, raw, zero), torch.where(keep, proc, zero))
        if top_n or score_ids:
            tv, ti, sc, xcounts = self.engine.read_logprob_extras(b)
            if xcounts != counts:
                raise RuntimeError(f"log-probability extras out of step with the record: {xcounts} against {counts}")
            k3 = keep.unsqueeze(-1)
            if top_n:
                res.add("top_logprobs", torch.where(k3, tv, zero))
                res.add("top_token_ids", torch.where(k3, ti, torch.full((), -1, dtype=torch.int64)))
            if score_ids:
                res.add("scored_logprobs", torch.where(k3, sc, zero))
        if fsm_states is not None:
            res.add("fsm_states", fsm_states)
        if dola_rec is not None:
            res.add("dola_premature_layers", dola_rec)
        return res

    def _contrastive_generate(self, input_ids, images, attention_mask, cs, streamer, eos_ids, stopping_criteria, share_prompt,
                              return_dict_in_generate):
        """HF's _contrastive_search on the device (include/omchat_hip.h: omchat_set_contrastive).  The arguments went
        through omchat_amd/contrastive.py: every refusal was raised before any work.  Per emitted id: one k-row decode step over the
        candidates and one contrastive step (penalty, select and commit, one-slot KV gather, next top-k); the host reads the emitted id
        behind an event, as the greedy loop does, for EOS, the streamer and the stopping criteria."""
        e = self.engine
        k, alpha, max_new = cs["k"], cs["alpha"], cs["max_new"]
        eos = set(int(i) for i in eos_ids)
        P = self._spliced_lengths(input_ids.detach().to("cpu", torch.int64), images)[0]
        share = e.group_share_default(k, P) if share_prompt is None else bool(share_prompt)
        e.sampling_off()
        if streamer is not None:
            streamer.put(input_ids.cpu())
        e.set_contrastive(k, alpha, max_new, share, sorted(eos))
        new = []
        try:
            out = self.forward(input_ids=input_ids, attention_mask=attention_mask, images=images, use_cache=True)
            cand = e.contrastive_step(out.local_logits)               # top-k of the prefill's row, the fork / share of the prompt row
            stage = self._stage_buffer(max_new, 1)
            evt = self._stage_event
            for step in range(max_new):
                _, lg = e.decode_step(cand[:k], want_logits=True)
                cand = e.contrastive_step(lg)
                stage[step].copy_(cand[k:k + 1], non_blocking=True)
                evt.record()
                evt.synchronize()
                tok = int(stage[step][0])
                new.append(tok)
                if streamer is not None:
                    streamer.put(torch.tensor([tok], dtype=torch.int64))
                if tok in eos:
                    break
                if stopping_criteria and step + 1 < max_new:
                    so_far = torch.cat([input_ids.cpu(), torch.tensor([new], dtype=torch.int64)], dim=1)
                    if any(bool(c(so_far, None)) for c in stopping_criteria):
                        break
            rec = e.contrastive_record(len(new)) if return_dict_in_generate else None
        finally:
            e.group_end()
            e.contrastive_off()
        if streamer is not None:
            streamer.end()
        seqs = torch.cat([input_ids.cpu(), torch.tensor([new], dtype=torch.int64)], dim=1)
        if not return_dict_in_generate:
            return seqs
        res = GenerateOutput(seqs, None, None)
        n = len(new)
        res.add("contrastive_ranks", torch.from_numpy(rec["pick"].copy()).view(1, n))
        res.add("degeneration_penalties", torch.from_numpy(rec["penalties"][range(n), rec["pick"]].copy()).view(1, n))
        return res

    def _group_params(self, input_ids, images, attention_mask, nb, do_sample, num_return_sequences, share_prompt, reuse, lookup, streamer):
        """(N, share_prompt) of generate(do_sample=True, num_return_sequences=N > 1) with num_beams == 1, or None for N == 1 (and under beam
        search, which reads the argument itself); every refusal is raised here, from host data alone, before any work is enqueued"""
        gc = self.generation_config
        N = num_return_sequences if num_return_sequences is not None else (getattr(gc, "num_return_sequences", None) or 1)
        if nb > 1:
            return None
        if not (isinstance(N, int) and N >= 1):
            raise ValueError(f"`num_return_sequences` has to be a strictly positive integer, but is {N}")
        if N == 1:
            return None
        if not do_sample:
            raise ValueError(f"Greedy methods without beam search do not support `num_return_sequences` different than 1 (got {N}).")
        b = input_ids.shape[0]
        e = self.engine
        if b * N > e.c.max_batch:
            raise ValueError(f"num_return_sequences needs b * num_return_sequences = {b * N} cache rows: create the model with max_batch >= "
                             f"{b * N} (it has {e.c.max_batch})")
        if attention_mask is not None and bool((attention_mask == 0).any()):
            raise NotImplementedError("num_return_sequences > 1 over a padded batch (attention_mask with zeros) is not implemented: pad the "
                                      "prompts to equal length or use b = 1")
        ids_cpu = input_ids.detach().cpu()
        if b > 1 and bool((ids_cpu == IMAGE_TOKEN_INDEX).any()) and len(set(self._spliced_lengths(ids_cpu, images))) > 1:
            raise NotImplementedError("num_return_sequences > 1 over rows of different spliced length is not implemented: pad the prompts "
                                      "to equal length or use b = 1")
        if reuse:
            raise NotImplementedError("num_return_sequences > 1 with reuse_cache=True is not implemented: the cache rows end as siblings, "
                                      "not as one conversation")
        if lookup is not None:
            raise NotImplementedError("num_return_sequences > 1 with prompt_lookup_num_tokens is not implemented: a verify step runs one sequence")
        if streamer is not None:
            raise ValueError("`streamer` cannot be used with num_return_sequences > 1: it takes one sequence (b * num_return_sequences = "
                             f"{b * N})")
        if share_prompt:
            from ..engine import group_share_refusal
            why = group_share_refusal(getattr(e, "_fp8_kv", False), e.tp_size, e.c.t_heads, e.c.t_kv_heads, N)
            if why is not None:
                raise NotImplementedError(f"share_prompt=True is not available here ({why}): use share_prompt=False (DESIGN.md section 7)")
        return N, (None if share_prompt is None else bool(share_prompt))

    def _suffix_params(self, input_ids, images, attention_mask, suffixes, nb, num_return_sequences, share_prompt, reuse, kwargs, streamer):
        """(suffix id lists, share_prompt) of generate(suffixes=...); every refusal that host data decides is raised here, each with its own
        message, before any work is enqueued (omchat_amd/suffix.py: check_suffix_args); last the room in the cache, which needs the splice
        plan (host integers) for the prompt's slot count -- before the tower runs and before any sticky state of the engine changes"""
        from ..suffix import check_suffix_args, check_room
        gc = self.generation_config
        e = self.engine
        nret = num_return_sequences if num_return_sequences is not None else (getattr(gc, "num_return_sequences", None) or 1)
        k = kwargs.get("prompt_lookup_num_tokens", None)
        k = k if k is not None else getattr(gc, "prompt_lookup_num_tokens", None)
        rows = check_suffix_args(input_ids.shape[0], attention_mask is not None and bool((attention_mask == 0).any()), suffixes, e.c.t_vocab_total,
                                 e.c.max_batch, e.c.max_prefill_rows, nb, int(nret), k is not None, reuse, streamer is not None,
                                 vars(e).get("_fp8_kv", False), vars(e).get("_fp8_prefill", False), e.tp_size, e.c.t_heads, e.c.t_kv_heads, share_prompt)
        check_room(self._spliced_lengths(input_ids.detach().cpu(), images)[0], rows, e.c.max_seq)
        return rows, (None if share_prompt is None else bool(share_prompt))

    def _forward_suffixes(self, input_ids, images, attention_mask, rows, share, want_hidden=False):
        """The prefill of generate(suffixes=...) / score(suffixes=...) (the arguments went through _suffix_params): the prompt's forward at b = 1, the fork / share of its slots among the N rows and the suffix pass.  -> forward()'s output with the N rows' last
        logits (`local_logits` [N, V]); with want_hidden also `.prompt_hidden` [1, P, H] and `.suffix_hidden` [N, S_max, H]"""
        from .. import _lib
        from ..suffix import check_room, share_refusal, suffix_token_table
        e = self.engine
        N, lens = len(rows), [len(r) for r in rows]
        tiles0 = e.encode_stats()["tiles"]
        out = self.forward(input_ids=input_ids, attention_mask=attention_mask, images=images, use_cache=True, output_hidden_states=want_hidden)
        P = e.kv_lengths(1)[0]
        check_room(P, rows, e.c.max_seq)
        if share is None:
            share = N > 1 and e.group_share_default(N, P) and share_refusal(False, 1, e.c.t_heads, e.c.t_kv_heads, N) is None
        share = bool(share) and N > 1                 # one row shares with nobody: the b = 1 state is the state
        if N > 1:
            e.group_begin(1, N, P, share)
        idx = torch.tensor(suffix_token_table(rows, _lib.PAD_ROW), dtype=torch.int32).view(-1)
        emb = e.gather_rows(idx, None).view(N, max(lens), -1)
        logits, hidden = e.prefill_suffixes(emb, lens, P, want_hidden=want_hidden)
        e._sfx_st = dict(tiles_encoded=e.encode_stats()["tiles"] - tiles0, prompt_rows=P, suffix_rows=sum(lens), shared=share)
        self._padded_batch = False
        res = CausalLMOutputWithPast(e.full_logits(logits).unsqueeze(1), KVHandle(e, N))
        res.local_logits = logits
        if want_hidden:
            res.prompt_hidden, res.suffix_hidden = out.hidden_states[0], hidden
        return res

    def _score_suffixes(self, input_ids, images, attention_mask, suffixes, share_prompt):
        """score(suffixes=...): token 0 of every suffix from the prompt's last position, tokens 1 .. S_j - 1 from the suffix pass's hidden
        rows, both through omchat_score_hidden; no [N, S, V] tensor exists"""
        from ..suffix import score_labels
        e = self.engine
        rows, share = self._suffix_params(input_ids, images, attention_mask, suffixes, 1, 1, share_prompt, False, {}, None)
        out = self._forward_suffixes(input_ids, images, attention_mask, rows, share, want_hidden=True)
        N, S_max = len(rows), max(len(r) for r in rows)
        first, lab = score_labels(rows)
        last = out.prompt_hidden[:, -1:, :].expand(N, 1, -1).contiguous()
        lp0, _, _, _ = e.score_hidden(last, torch.tensor(first, dtype=torch.int64).view(N, 1))
        lp, _, _, _ = e.score_hidden(out.suffix_hidden, torch.tensor(lab, dtype=torch.int64))
        tl = torch.cat([lp0, lp[:, :S_max - 1]], dim=1)
        n = torch.tensor([len(r) for r in rows], dtype=torch.int64, device=tl.device)
        seq = tl.sum(dim=1)
        if N > 1:
            e.group_end()
        res = dict(token_logprobs=tl, sequence_logprobs=seq, num_tokens=n, perplexity=torch.exp(-seq / n))
        torch.cuda.current_stream().synchronize()
        return res

    def _forward_reuse(self, input_ids, images):
        """The prefill of generate(reuse_cache=True), b = 1: keeps the slots of sequence 0's cache that the new prompt shares with the
        recorded one and prefills the rest; the tower runs on tiles that differ from every kept tile only.  -> (forward()'s output for
        the last position, the prompt's slot list).  The engine's record is pending (dropped) until _record_prefix."""
        from ..prefix import slots_from_plan, keep_count
        e = self.engine
        px = None
        if images is not None and self.get_vision_tower() is not None:
            if type(images) is list:
                if any(im.ndim != 3 for im in images):
                    raise NotImplementedError("video inputs: the reference calls an undefined encode_videos (omchat_arch.py:87)")
                images = torch.stack(images)
            elif images.ndim == 5:
                raise NotImplementedError("video inputs: the reference calls an undefined encode_videos (omchat_arch.py:87)")
            px = e._px(images)
        n = 0 if px is None else px.shape[0]
        keys, src = e.tile_keys(px)
        idx = e.splice_plan(input_ids, n, getattr(self.config, "tokenizer_model_max_length", None))
        slots = slots_from_plan(idx.tolist(), e.ntok, keys)
        S = len(slots)
        kept = e._prefix
        P = keep_count(kept["record"], slots, e.kv_lengths(1)[0]) if kept is not None and kept.get("record") else 0
        feats = None
        fresh = [j for j in range(n) if src[j] < 0]
        if n:
            feats = torch.empty(n, e.ntok, e.cfg.text["hidden_size"], dtype=e.torch_dtype, device=e.device)
            for j in range(n):
                if src[j] >= 0:
                    feats[j].copy_(kept["feats"][src[j]])
            if fresh:
                feats[fresh] = self.encode_images(px[fresh]).to(e.torch_dtype)
        if P > 0:
            logits, _ = e.prefill_extend(e.gather_rows(idx[P:], feats), P)
        else:
            logits, _ = e.prefill(e.gather_rows(idx, feats).unsqueeze(0), [S])
        e._prefix = dict(record=None, px=px, feats=feats, keys=keys)
        e._ext_st = dict(kept_slots=P, prefilled_rows=S - P, tiles_encoded=len(fresh), tiles_reused=n - len(fresh))
        self._padded_batch = False
        self._prefill_slots = S
        self._last_lengths = None
        out = CausalLMOutputWithPast(e.full_logits(logits).unsqueeze(1), KVHandle(e, 1))
        out.local_logits = logits
        return out, slots

    def _record_prefix(self, prompt_slots, generated):
        """end of a reuse_cache=True call: the record = the prompt's slots + the generated ids that are cached (not the last emitted one)"""
        if prompt_slots is None:
            return
        from ..prefix import extend_record
        e = self.engine
        if e._prefix is not None:
            e._prefix["record"] = extend_record(prompt_slots, generated, e.kv_lengths(1)[0])

    def _spliced_lengths(self, ids, images):
        """the rows' lengths after the image-token splice, from the host-side plan alone (omchat_splice_plan: integers, nothing enqueued)"""
        from .. import _lib
        ids = ids.to(torch.int64).contiguous()
        b, T = ids.shape
        lens = torch.zeros(b, dtype=torch.int32)
        S = _lib.C.c_int(0)
        _lib.check(self.engine.lib.omchat_splice_plan(_lib.ptr(ids), None, b, T, self.engine.ntok, max(_n_tiles(images), int((ids == -200).sum())),
                                                      0, -1, None, _lib.ptr(lens), _lib.C.byref(S), 0))
        return [int(x) for x in lens]

    def _beam_generate(self, input_ids, images, attention_mask, N, do_sample, max_new_tokens, streamer, eos_token_id, pad_token_id,
                       stopping_criteria, repetition_penalty, length_penalty, early_stopping, num_return_sequences, return_dict_in_generate,
                       beam_processors=False, con=None):
        """HF's _beam_search on the device (include/omchat_hip.h: omchat_beam_begin) with the one-step-ahead loop of
        the greedy path: each prompt is prefilled once and its cache row forked into its N beam rows.  beam_processors: the repetition
        penalty and the token bans `con` (resolve_constraints) act on the beam rows' log-probabilities (omchat_beam_processors).  Every
        refusal is raised before any work is enqueued."""
        gc = self.generation_config
        pick = lambda v, name, d: v if v is not None else (getattr(gc, name, None) if getattr(gc, name, None) is not None else d)
        lp = float(pick(length_penalty, "length_penalty", 1.0))
        es = pick(early_stopping, "early_stopping", False)
        nret = int(pick(num_return_sequences, "num_return_sequences", 1))
        rp = pick(repetition_penalty, "repetition_penalty", 1.0)
        if do_sample:
            raise NotImplementedError("beam sampling (do_sample=True with num_beams > 1) is not implemented: use do_sample=False")
        if streamer is not None:
            raise ValueError("`streamer` cannot be used with beam search (yet!). Make sure that `num_beams` is set to 1.")
        if stopping_criteria:
            raise NotImplementedError("custom stopping_criteria are not implemented under beam search")
        if not beam_processors and float(rp) != 1.0:
            raise NotImplementedError("repetition_penalty is not implemented under beam search")
        if es not in (True, False, "never"):
            raise ValueError(f"`early_stopping` must be a boolean or 'never', but is {es}.")
        if nret > N:
            raise ValueError(f"`num_return_sequences` ({nret}) has to be smaller or equal to `num_beams` ({N}).")
        b = input_ids.shape[0]
        if b * N > self.engine.c.max_batch:
            raise ValueError(f"beam search needs b * num_beams = {b * N} cache rows: create the model with max_batch >= {b * N} "
                             f"(it has {self.engine.c.max_batch})")
        ids_cpu = input_ids.detach().cpu()
        if attention_mask is not None and bool((attention_mask == 0).any()):
            raise NotImplementedError("beam search over a padded batch (attention_mask with zeros) is not implemented: pad the prompts to "
                                      "equal length or use b = 1")
        if b > 1 and len(set(self._spliced_lengths(ids_cpu, images))) > 1:
            raise NotImplementedError("beam search over rows of different spliced length is not implemented: pad the prompts to equal "
                                      "length or use b = 1")
        if max_new_tokens is None:
            max_new_tokens = gc.max_new_tokens or 20
        eos = eos_token_id if eos_token_id is not None else gc.eos_token_id
        eos = [int(e) for e in (eos if isinstance(eos, (list, tuple)) else ([eos] if eos is not None else []))]
        pad = pad_token_id if pad_token_id is not None else gc.pad_token_id
        fill = (pad or eos[0]) if eos else -1                   # HF: `pad_token_id or eos_token_id[0] if eos_token_id is not None else -1`
        bpk = None
        if beam_processors:
            from ..constraints import resolve_beam_processors
            bpk = resolve_beam_processors(con, rp, N, eos, self.engine.c.t_vocab_total, input_ids.shape[1], max_new_tokens, self.engine.tp_size)
        out = self.forward(input_ids=input_ids, attention_mask=attention_mask, images=images, use_cache=True)
        lens = self.engine.kv_lengths(b)
        if getattr(self, "_padded_batch", False) or len(set(lens)) > 1:
            raise NotImplementedError("beam search over rows of different spliced length is not implemented: pad the prompts to equal "
                                      "length or use b = 1")
        P = lens[0]
        room = self.engine.c.max_seq - P + 1                    # as the greedy path clamps it
        if max_new_tokens > room:
            import warnings
            warnings.warn(f"max_new_tokens={max_new_tokens} clamped to {room}: KV cache capacity max_seq={self.engine.c.max_seq}")
            max_new_tokens = max(room, 1)
        e = self.engine
        e.sampling_off()
        e.beam_begin(b, N, lp, es, eos, max_new_tokens, P)
        if bpk is not None:
            e.beam_processors(ids_cpu.tolist(), **bpk)
        tok = e.beam_step(out.local_logits)
        stage = self._stage_buffer(1, 1)
        evt = self._stage_event
        # one step ahead: the done word of step t - 1 goes to pinned memory behind an event, step t is enqueued, and only then the host
        # waits; a prompt that is done is frozen, so the step enqueued after the last one changes nothing
        for t in range(1, max_new_tokens):
            stage[0].copy_(e.beam_done, non_blocking=True)
            evt.record()
            _, lg = e.decode_step(tok, want_logits=True)
            tok = e.beam_step(lg)
            evt.synchronize()
            if int(stage[0, 0]):
                break
        hyps, scores = e.beam_result(nret)
        gen = max(len(h) for h in hyps)
        rows = []
        for o, h in enumerate(hyps):
            rows.append(torch.cat([ids_cpu[o // nret], torch.tensor(h + [fill] * (gen - len(h)), dtype=ids_cpu.dtype)]))
        seqs = torch.stack(rows)
        if not return_dict_in_generate:
            return seqs
        return BeamSearchOutput(seqs, torch.from_numpy(scores.copy()))


def _n_tiles(images):
    if images is None:
        return 0
    if isinstance(images, (list, tuple)):
        return sum(_n_tiles(x) for x in images)
    return int(images.shape[0]) if images.dim() == 4 else 1


class BeamSearchOutput(dict):
    """generate(num_beams > 1, return_dict_in_generate=True): `.sequences` [b * num_return_sequences, T + new] and `.sequences_scores`
    (HF's GenerateBeamDecoderOnlyOutput fields of the same names; per-step `scores` are not kept)"""

    def __init__(self, sequences, sequences_scores):
        super().__init__(sequences=sequences, sequences_scores=sequences_scores)
        self.sequences, self.sequences_scores = sequences, sequences_scores


class GenerateOutput(dict):
    """generate(output_logprobs=True, return_dict_in_generate=True): `.sequences` [b, T + new] as the plain call returns them, `.logprobs`
    [b, new] = log_softmax(logits)[token] of every generated token (HF: compute_transition_scores on out.logits with normalize_logits=True)
    and `.processed_logprobs` [b, new] = the same under the processed scores the pick was made from (on out.scores); full-vocabulary
    `scores` / `logits` tuples are not kept.  Present only when asked for (top_logprobs=n / score_token_ids=[...]): `.top_logprobs`
    [b, new, n] fp32 with `.top_token_ids` [b, new, n] int64, and `.scored_logprobs` [b, new, k] fp32, all under the raw distribution"""

    def __init__(self, sequences, logprobs, processed_logprobs):
        super().__init__(sequences=sequences, logprobs=logprobs, processed_logprobs=processed_logprobs)
        self.sequences, self.logprobs, self.processed_logprobs = sequences, logprobs, processed_logprobs

    def add(self, name, value):
        self[name] = value
        setattr(self, name, value)


def resolve_logprob_extras(gc, olp, top_logprobs, score_token_ids, vocab):
    """generate()'s top_logprobs / score_token_ids (the call's, else generation_config's) -> (top_n, ids list), (0, []) when neither is
    given; every refusal is a ValueError raised from host data alone"""
    n = top_logprobs if top_logprobs is not None else getattr(gc, "top_logprobs", None)
    ids = score_token_ids if score_token_ids is not None else getattr(gc, "score_token_ids", None)
    if n is None and ids is None:
        return 0, []
    if not olp:
        raise ValueError("top_logprobs / score_token_ids need output_logprobs=True (and return_dict_in_generate=True): they are fields of "
                         "the same record")
    if n is not None and not (isinstance(n, int) and not isinstance(n, bool) and 1 <= n <= 20):
        raise ValueError(f"`top_logprobs` has to be an integer in 1..20, but is {n}")
    if n is not None and n > vocab:
        raise ValueError(f"`top_logprobs` ({n}) exceeds the vocabulary ({vocab})")
    if ids is not None:
        ids = [int(i) for i in (ids.tolist() if hasattr(ids, "tolist") else ids)]
        if not 1 <= len(ids) <= 32:
            raise ValueError(f"`score_token_ids` has to hold 1..32 ids, but holds {len(ids)}")
        if len(set(ids)) != len(ids):
            raise ValueError("`score_token_ids` has to hold distinct ids")
        bad = [i for i in ids if not 0 <= i < vocab]
        if bad:
            raise ValueError(f"`score_token_ids` outside the vocabulary [0, {vocab}): {bad}")
    return int(n or 0), list(ids or [])
