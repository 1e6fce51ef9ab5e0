"""Host side of generate(penalty_alpha=, top_k=): HF's mode rule for contrastive search, the validation of the two
parameters and every refusal that host data decides -- all before any work is enqueued.  The search itself runs on the device
(csrc/contrastive.hip)."""
import numbers

MAX_K = 16      # include/omchat_hip.h: OMCHAT_CS_MAX_K
REC_WORDS = 52      # include/omchat_hip.h: OMCHAT_CS_REC_WORDS


def selects(penalty_alpha, top_k, do_sample, num_beams):
    """HF's rule (GenerationConfig.get_generation_mode): contrastive search runs iff num_beams == 1, do_sample is false, penalty_alpha is
    not None and > 0, and top_k is not None and > 1"""
    return (num_beams == 1 and not do_sample and penalty_alpha is not None and not isinstance(penalty_alpha, bool)
            and isinstance(penalty_alpha, numbers.Real) and penalty_alpha > 0
            and top_k is not None and not isinstance(top_k, bool) and isinstance(top_k, numbers.Real) and top_k > 1)


def resolve_contrastive(generation_config, kwargs, top_k, do_sample, num_beams, max_batch):
    """Pops `penalty_alpha` from `kwargs` (None -> generation_config; top_k likewise).  -> None when the mode rule does not select
    contrastive search (the call then behaves as without the keyword), else dict(alpha, k).  ValueError: penalty_alpha > 1, a top_k that
    is no integer, top_k > min(MAX_K, max_batch).  max_batch: the number, or a callable that gives it."""
    pa = kwargs.pop("penalty_alpha", None)
    pa = pa if pa is not None else getattr(generation_config, "penalty_alpha", None)
    tk = top_k if top_k is not None else getattr(generation_config, "top_k", None)
    if not selects(pa, tk, do_sample, num_beams):
        return None
    if not float(pa) <= 1.0:
        raise ValueError(f"`penalty_alpha` has to be a float in (0, 1] for contrastive search, but is {pa!r}")
    if not isinstance(tk, numbers.Integral):
        raise ValueError(f"`top_k` has to be an integer, but is {tk!r}")
    max_batch = max_batch() if callable(max_batch) else max_batch      # (asked only when the mode is selected)
    cap = min(MAX_K, int(max_batch))
    if int(tk) > cap:
        raise ValueError(f"contrastive search (penalty_alpha={pa!r}) runs its top_k candidates as rows of one decode step: top_k={int(tk)} "
                         f"exceeds the cap min({MAX_K}, max_batch={int(max_batch)}) = {cap} (generation_config.top_k may default to 50: "
                         f"pass top_k, or create the model with a larger max_batch)")
    return dict(alpha=float(pa), k=int(tk))


def refuse(b=1, padded=False, num_return_sequences=1, suffixes=False, lookup=False, reuse=False, guidance=False, dola=False, token_fsm=False,
           banning=False, repetition_penalty=1.0, output_logprobs=False, tp_size=1, fp8_kv=False, fp8_prefill=False, mxfp4_decode=False,
           mxfp4_batched=False, share_prompt=None, share_refusal=None):
    """every combination generate(penalty_alpha=, top_k=) does not run, from host data alone (all NotImplementedError)"""
    def no(what, why):
        raise NotImplementedError(f"contrastive search (penalty_alpha, top_k) with {what} is not implemented: {why}")
    if b > 1:
        no("b > 1", "the candidates of one sequence fill the rows of the decode step (DESIGN.md section 7)")
    if padded:
        no("an attention mask with zeros", "the k-row step runs one unpadded sequence")
    if isinstance(num_return_sequences, int) and num_return_sequences > 1:
        no("num_return_sequences > 1", "it is a deterministic strategy: the rows would be equal")
    if suffixes:
        no("suffixes=", "the suffix pass keeps no history rows")
    if lookup:
        no("prompt_lookup_num_tokens", "a verify step runs one sequence, not its candidates")
    if reuse:
        no("reuse_cache=True", "the kept slots' hidden rows are gone")
    if guidance:
        no("guidance_scale", "every candidate row would need its twin")
    if dola:
        no("dola_layers", "every candidate row would need its layers' rows")
    if token_fsm:
        no("token_fsm", "logits processors do not run inside the loop (DESIGN.md section 7)")
    if banning:
        no("a token-banning argument", "logits processors do not run inside the loop (DESIGN.md section 7)")
    if repetition_penalty is not None and float(repetition_penalty) != 1.0:
        no("repetition_penalty != 1", "logits processors do not run inside the loop (DESIGN.md section 7)")
    if output_logprobs:
        no("output_logprobs", "the step's record holds the candidates' probabilities and penalties instead")
    if tp_size > 1:
        no("tensor parallelism", "the history and the top-k are not vocabulary- or row-parallel (DESIGN.md section 7)")
    if fp8_kv:
        no("the e4m3 KV cache", "the one-slot commit copies 16-bit slots only (DESIGN.md section 7)")
    if fp8_prefill:
        no("fp8 x fp8 prefill GEMMs", "not validated with the history rows")
    if mxfp4_decode and not mxfp4_batched:
        no("batch-1-only MXFP4 decode weights", "every step has top_k rows: enable_mxfp4_decode(True, batched=True) or enable_mxfp4_decode(False)")
    if share_prompt and share_refusal is not None:
        raise NotImplementedError(f"share_prompt=True is not available here ({share_refusal}): use share_prompt=False (DESIGN.md section 7)")


MAX_EOS = 8      # csrc/kernels.h: CS_EOS_MAX


def check_eos(eos_ids):
    """the select launch compares the emitted id with at most MAX_EOS ids"""
    n = len({int(i) for i in eos_ids})
    if n > MAX_EOS:
        raise ValueError(f"contrastive search takes at most {MAX_EOS} distinct eos_token_id values, got {n}")


def check_room(P, max_new, max_seq):
    """the history holds P + max_new rows and the cache one slot per emitted id"""
    if P + max_new > max_seq:
        raise ValueError(f"contrastive search: prompt ({P} positions) + max_new_tokens ({max_new}) exceed max_seq = {max_seq}")


def unpack_record(words, k):
    """words: int32 numpy [steps, REC_WORDS] (omchat_contrastive_read) -> dict(ids [steps, k] int64, probs / penalties [steps, k] fp32,
    pick [steps], token [steps], chunks [steps], rows [steps])"""
    import numpy as np
    w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1, REC_WORDS)
    f = w.view(np.float32)
    return dict(ids=w[:, :k].astype(np.int64), probs=f[:, 16:16 + k].copy(), penalties=f[:, 32:32 + k].copy(), pick=w[:, 48].astype(np.int64),
                token=w[:, 49].astype(np.int64), chunks=w[:, 50].astype(np.int64), rows=w[:, 51].astype(np.int64))
