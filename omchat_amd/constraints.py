"""Host side of generate()'s HF logits constraints: resolution of no_repeat_ngram_size, bad_words_ids,
min_new_tokens / min_length, suppress_tokens and begin_suppress_tokens from the call or generation_config with HF's defaults and HF's
validation messages, and every refusal -- all before any work is enqueued.  The ban itself runs on the device (csrc/constrain.hip)."""
import numpy as np

# include/omchat_hip.h: OMCHAT_CON_MAX_*
MAX_NGRAM, MAX_EOS, MAX_SUPPRESS, MAX_BAD_WORDS, MAX_BAD_WORD_IDS = 64, 16, 1024, 1024, 8192

NAMES = ("no_repeat_ngram_size", "bad_words_ids", "min_new_tokens", "min_length", "suppress_tokens", "begin_suppress_tokens")
# HF generation arguments that change the logits and that this generate() has no kernel for: refused, never dropped
UNSUPPORTED = ("forced_eos_token_id", "sequence_bias", "prefix_allowed_tokens_fn", "logits_processor")


def _is_int(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


def _id_list(x):
    if x is None:
        return []
    if hasattr(x, "tolist"):
        x = x.tolist()
    return [int(i) for i in (x if isinstance(x, (list, tuple)) else [x])]


def resolve_constraints(generation_config, kwargs, eos, vocab_total, num_beams=1, lookup=False, *, beam_processors=False):
    """Pops the constraint arguments from `kwargs` (None -> generation_config).  -> None when no constraint is set, else the keyword
    arguments of Engine.set_constraints.  eos: the resolved EOS ids of the call.  beam_processors: generate(beam_processors=True) -- with
    num_beams > 1 the arguments are resolved for Engine.beam_processors (resolve_beam_processors) and not refused."""
    gc = generation_config
    for name in UNSUPPORTED:
        v = kwargs.pop(name, None)
        v = v if v is not None else getattr(gc, name, None)
        if v is not None and not (name == "logits_processor" and len(v) == 0):
            raise NotImplementedError(f"`{name}` is not implemented: it changes the logits of every step and this generate() picks on the "
                                      "device (DESIGN.md section 7); it was never applied, and is refused rather than dropped")
    got = {}
    for name in NAMES:
        v = kwargs.pop(name, None)
        got[name] = v if v is not None else getattr(gc, name, None)
    n = got["no_repeat_ngram_size"]
    if n is not None and (not _is_int(n) or n < 0):
        raise ValueError(f"`ngram_size` has to be a strictly positive integer, but is {n}")
    n = int(n or 0)
    words = got["bad_words_ids"]
    if words is not None:
        if not isinstance(words, list) or len(words) == 0:
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {words}.")
        if any(not isinstance(w, list) for w in words):
            raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {words}.")
        if any(any((not _is_int(t) or t < 0) for t in w) for w in words):
            raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {words}.")
        if any(len(w) == 0 for w in words):
            raise ValueError(f"Each list in `bad_words_ids` has to be a non-empty list, but is {words}.")
        invalid = [t for w in words for t in w if t >= vocab_total]
        if invalid:
            raise ValueError(f"The model vocabulary size is {vocab_total}, but the following tokens were being biased: {invalid}")
        words = [[int(t) for t in w] for w in words]
    min_len, min_new = got["min_length"], got["min_new_tokens"]
    if min_len is not None and (not _is_int(min_len) or min_len < 0):
        raise ValueError(f"`min_length` has to be a non-negative integer, but is {min_len}")
    if min_new is not None and (not _is_int(min_new) or min_new < 0):
        raise ValueError(f"`min_new_tokens` has to be a positive integer, but is {min_new}")
    # HF: min_new_tokens replaces min_length (generation_config.min_length = min_new_tokens + the prompt's length)
    min_new = int(min_new or 0)
    min_len = 0 if min_new else int(min_len or 0)
    eos = sorted({int(e) for e in eos})
    if not eos:      # HF adds the two length processors only when there is an EOS id
        min_new = min_len = 0
    sup, bsup = _id_list(got["suppress_tokens"]), _id_list(got["begin_suppress_tokens"])
    if not (n or words or min_new or min_len or sup or bsup):
        return None
    if num_beams > 1 and not beam_processors:
        raise NotImplementedError("no_repeat_ngram_size / bad_words_ids / min_new_tokens / min_length / suppress_tokens / begin_suppress_tokens "
                                  "with num_beams > 1 are not implemented: HF applies them to log-softmax scores inside the beam scorer")
    if lookup:
        raise NotImplementedError("logits constraints with prompt_lookup_num_tokens are not implemented: each verify row would need its own ban set")
    if n > MAX_NGRAM:
        raise ValueError(f"no_repeat_ngram_size={n} exceeds the limit of {MAX_NGRAM}")
    # the device reads the eos list for the length bounds and to drop bad words equal to [eos]; the other constraints never see it
    if not (min_new or min_len or words):
        eos = []
    if len(eos) > MAX_EOS:
        raise ValueError(f"{len(eos)} eos ids exceed the limit of {MAX_EOS} under min_new_tokens / min_length / bad_words_ids")
    if len(sup) > MAX_SUPPRESS or len(bsup) > MAX_SUPPRESS:
        raise ValueError(f"suppress_tokens / begin_suppress_tokens: at most {MAX_SUPPRESS} ids each")
    if words and (len(words) > MAX_BAD_WORDS or sum(len(w) for w in words) > MAX_BAD_WORD_IDS):
        raise ValueError(f"bad_words_ids: at most {MAX_BAD_WORDS} words and {MAX_BAD_WORD_IDS} ids in total")
    return dict(no_repeat_ngram_size=n, bad_words_ids=words or [], min_new_tokens=min_new, min_length=min_len, eos=eos, suppress_tokens=sup,
                begin_suppress_tokens=bsup)


def resolve_beam_processors(con, repetition_penalty, num_beams, eos, vocab_total, prompt_len, max_new, tp_size=1):
    """generate(num_beams > 1, beam_processors=True): `con` (resolve_constraints' result or None) and the repetition penalty -> the keyword
    arguments of Engine.beam_processors, or None when nothing changes the scores (the plain search).  eos: the search's EOS ids;
    prompt_len: the prompt row's length in tokens.  Every refusal is raised here, from host data, before any work is enqueued."""
    rp = 1.0 if repetition_penalty is None else repetition_penalty
    if isinstance(rp, bool) or not isinstance(rp, (int, float, np.integer, np.floating)) or not rp > 0:
        raise ValueError(f"`penalty` has to be a strictly positive float, but is {rp}")
    rp = float(np.float32(rp))
    if not np.isfinite(rp):
        raise ValueError(f"`penalty` has to be a finite float, but is {repetition_penalty}")
    if con is None and rp == 1.0:
        return None
    if tp_size != 1:
        raise NotImplementedError("beam_processors=True under tensor parallelism is not implemented (DESIGN.md section 7): the row's "
                                  "log-sum-exp would need an exchange of its own in front of the selection")
    con = con or dict(no_repeat_ngram_size=0, bad_words_ids=[], min_new_tokens=0, min_length=0, suppress_tokens=[], begin_suppress_tokens=[])
    eos = [int(e) for e in eos]      # as the search takes them: its candidates per step count the ids as passed
    words = [w for w in con["bad_words_ids"] if not (len(w) == 1 and w[0] in eos)]      # HF drops a bad word that is one EOS id
    KB = max(2, 1 + len(eos)) * int(num_beams)
    n_sup, n_bsup = len(con["suppress_tokens"]), len(con["begin_suppress_tokens"])
    left = int(vocab_total) - (n_sup + n_bsup + len(words) + len(eos) + int(prompt_len) + int(max_new))
    if left < KB:
        raise ValueError(f"beam_processors=True: the bans could leave a beam row fewer than {KB} finite scores (max(2, 1 + n_eos) * num_beams): "
                         f"vocabulary {vocab_total} - ({n_sup} suppress_tokens + {n_bsup} begin_suppress_tokens + {len(words)} bad words + "
                         f"{len(eos)} eos ids + {prompt_len} prompt tokens + {max_new} new tokens) = {left}")
    return dict(repetition_penalty=rp, no_repeat_ngram_size=con["no_repeat_ngram_size"], bad_words_ids=con["bad_words_ids"],
                min_new_tokens=con["min_new_tokens"], min_length=con["min_length"], suppress_tokens=con["suppress_tokens"],
                begin_suppress_tokens=con["begin_suppress_tokens"])
