"""Host side of generate(dola_layers=): the candidate layers of HF's `dola_layers` -- 'low', 'high' or a list of indices into
HF's hidden_states tuple (0 = the embedding row, i = the residual stream behind decoder layer i) -- resolved as HF 4.4x's _dola_decoding does,
the validation of dola_relative_top, and every refusal that host data decides -- all before any work is enqueued.  The contrast itself runs on
the device (csrc/dola.hip)."""
import numbers

MAX_LAYERS = 16      # include/omchat_hip.h: OMCHAT_DOLA_MAX_LAYERS
NAMES = ("dola_layers", "dola_relative_top", "dola_norm")


def resolve_layers(dola_layers, num_layers, tie_word_embeddings=False):
    """-> the list of candidate indices.  N = num_layers; 'low': range(start, N // 2, 2) (or [start] when start == N // 2), 'high':
    range(N // 2, N, 2); for N > 40 range(start, 20, 2) and range(N - 20, N, 2); start = 0, or with tied embeddings 2 if N > 2, 1 if
    N == 2, else 0; a list keeps its entries below N.  ValueError: anything else, an empty result, a negative entry, more than MAX_LAYERS."""
    N = int(num_layers)
    start = (2 if N > 2 else 1 if N == 2 else 0) if tie_word_embeddings else 0
    if isinstance(dola_layers, str):
        if dola_layers == "low":
            if N <= 40:
                cand = [start] if start == N // 2 else list(range(start, N // 2, 2))
            else:
                cand = list(range(start, 20, 2))
        elif dola_layers == "high":
            cand = list(range(N // 2, N, 2)) if N <= 40 else list(range(N - 20, N, 2))
        else:
            raise ValueError(f"`dola_layers` must be either 'low', 'high' or a list of integers, but is {dola_layers!r}")
    elif isinstance(dola_layers, (list, tuple)):
        if any(isinstance(i, bool) or not isinstance(i, numbers.Integral) for i in dola_layers):
            raise ValueError(f"`dola_layers` must be either 'low', 'high' or a list of integers, but is {dola_layers!r}")
        if any(i < 0 for i in dola_layers):
            raise ValueError(f"`dola_layers` holds a negative index: {list(dola_layers)!r} (indices count HF's hidden_states from the embeddings, 0)")
        cand = [int(i) for i in dola_layers if i < N]
        if len(set(cand)) != len(cand):
            raise ValueError(f"`dola_layers` holds an index twice: {list(dola_layers)!r}")
    else:
        raise ValueError(f"`dola_layers` must be either 'low', 'high' or a list of integers, but is {dola_layers!r}")
    if not cand:
        raise ValueError(f"`dola_layers`={dola_layers!r} leaves no candidate layer below num_hidden_layers = {N}")
    if len(cand) > MAX_LAYERS:
        raise ValueError(f"`dola_layers`={dola_layers!r} resolves to {len(cand)} candidate layers, more than the limit of {MAX_LAYERS}")
    return cand


def resolve_dola(generation_config, kwargs, num_layers, tie_word_embeddings=False):
    """Pops the three keywords from `kwargs` (None -> generation_config).  -> None when dola_layers is None (nothing happens), else
    dict(layers, relative_top, norm).  num_layers: the number, or a callable that gives it -- asked only when dola_layers is set."""
    got = {}
    for name in NAMES:
        v = kwargs.pop(name, None)
        got[name] = v if v is not None else getattr(generation_config, name, None)
    if got["dola_layers"] is None:
        return None
    layers = resolve_layers(got["dola_layers"], num_layers() if callable(num_layers) else num_layers, tie_word_embeddings)
    rt = got["dola_relative_top"]
    rt = 0.1 if rt is None else rt
    if isinstance(rt, bool) or not isinstance(rt, numbers.Real) or not (0.0 < float(rt) <= 1.0):
        raise ValueError(f"`dola_relative_top` has to be a float in (0, 1], but is {rt!r}")
    return dict(layers=layers, relative_top=float(rt), norm=bool(got["dola_norm"]))


def refuse(b, k, max_batch, num_beams=1, guidance=False, num_return_sequences=1, suffixes=False, lookup=False, reuse=False, padded=False,
           tp_size=1, fp8_decode=False, mxfp4_decode=False):
    """every combination generate(dola_layers=) does not run, from host data alone"""
    def no(what, why):
        raise NotImplementedError(f"dola_layers with {what} is not implemented: {why}")
    if num_beams > 1:
        no("num_beams > 1", "every beam row would need its candidate rows")
    if guidance:
        no("guidance_scale", "the two stages write the same copy of the logits")
    if isinstance(num_return_sequences, int) and num_return_sequences > 1:
        no("num_return_sequences > 1", "every sibling row would need its candidate rows")
    if suffixes:
        no("suffixes=", "the suffix pass keeps no candidate rows")
    if lookup:
        no("prompt_lookup_num_tokens", "every verify row would need its candidate rows")
    if reuse:
        no("reuse_cache=True", "the kept slots' candidate rows are gone, and the extending prefill keeps none")
    if padded:
        no("a padded or left-padded batch", "the masked step keeps no candidate rows; pad the prompts to equal length or use b = 1")
    if tp_size > 1:
        no("tensor parallelism", "the vocabulary-parallel exchange of the log-sum-exps and divergences is not built (DESIGN.md section 7)")
    if fp8_decode or mxfp4_decode:
        no("the fp8 or MXFP4 decode replicas", "the head pass over the candidate rows is 16-bit only in this version (DESIGN.md section 7)")
    if (k + 1) * b > min(max_batch, 32):
        raise ValueError(f"dola_layers: (k + 1) * b = {(k + 1) * b} rows go through the head in one pass, at most min(max_batch, 32) = "
                         f"{min(max_batch, 32)}: create the model with a larger max_batch or pass fewer layers")
