"""Prompt-lookup decoding (generate(prompt_lookup_num_tokens=k)).

The drafter is HF's PromptLookupCandidateGenerator.get_candidates rule, kept incremental: an n-gram -> first-occurrence index per n-gram
size, updated once per emitted token, instead of a scan over the whole prompt per step.  The loop verifies each draft with one
Engine.decode_verify (all draft tokens plus the last emitted one through the decoder at once) and hands the emitted tokens to EOS
handling, the stopping criteria and the streamer one by one, as the greedy loop does.  Host-only code: the engine is duck-typed
(decode_step, decode_verify, kv_rewind), so tests drive the loop with a fake one."""
import torch

MAX_LOOKUP_TOKENS = 15      # a verify step runs at most 16 rows (the last emitted token + 15 drafts; launch_attn_block, ATTN_VERIFY)


class PromptLookupDrafter:
    """get_candidates of HF 5.15's PromptLookupCandidateGenerator over ids = prompt + generated ids, for batch 1:
    n-gram sizes from min(m, len - 1) down to 1; the first (leftmost) earlier occurrence of the trailing n-gram whose continuation is
    non-empty; at most k tokens of that continuation, cut before its first EOS.  An EOS cut that leaves nothing ends the search with no
    draft (as HF does).  This project's own rule on top: the draft is also cut before the first id outside [0, vocab) (the -200 image
    sentinel of the prompt), since such an id can never be a pick."""

    def __init__(self, ids, num_tokens, max_ngram=2, eos=(), vocab=None):
        if int(max_ngram) <= 0 or int(num_tokens) <= 0:
            raise ValueError("Invalid max_matching_ngram_size or num_output_tokens")
        self.k, self.m = int(num_tokens), int(max_ngram)
        self.eos = set(int(e) for e in eos)
        self.vocab = vocab
        self.ids = []
        self.first = [dict() for _ in range(self.m)]      # first[n - 1][n-gram] = index of its first occurrence
        for t in ids:
            self.append(t)

    def append(self, tok):
        ids = self.ids
        ids.append(int(tok))
        end = len(ids)
        for n in range(1, min(self.m, end) + 1):
            self.first[n - 1].setdefault(tuple(ids[end - n:end]), end - n)

    def candidates(self, max_length=None):
        """the draft for the next step (a list, possibly empty); max_length: HF's total-length bound (prompt + max_new_tokens)"""
        ids, L = self.ids, len(self.ids)
        if max_length is not None and max_length == L + 1:
            return []
        for n in range(min(self.m, L - 1), 0, -1):
            f = self.first[n - 1].get(tuple(ids[L - n:]))
            if f is None or f + n >= L:                    # only the trailing n-gram itself: no continuation
                continue
            end = min(f + n + self.k, L)
            if max_length is not None:
                end = min(end, max_length)
            out = []
            for t in ids[f + n:end]:
                if t in self.eos or (self.vocab is not None and not 0 <= t < self.vocab):
                    break
                out.append(t)
            return out
        return []


def lookup_loop(engine, input_ids, tok, max_new_tokens, eos, num_tokens, max_ngram, vocab, streamer=None, stopping_criteria=None,
                draft_hook=None, max_verify=MAX_LOOKUP_TOKENS + 1, sample=False):
    """Batch 1, after the prefill and the first pick `tok` (int): returns the generated ids (list of int), the same ids the greedy loop
    of generate() returns, EOS kept.  Each step drafts from the ids so far; a non-empty draft is verified in one Engine.decode_verify
    (the emitted tokens are the picks up to and including the first rejected position), an empty one takes a plain decode_step.  The
    emitted tokens go to EOS handling / stopping_criteria / streamer one by one; at the first stop the rest of the step is dropped and
    the cache trimmed to match (kv_rewind), as the greedy loop leaves it.  max_verify: the most tokens one verify step takes (the draft is
    cut to max_verify - 1; Engine.verify_max_tokens).  draft_hook(ids, k) -> list replaces the drafter (measurement).  sample=True (the
    engine's sampler is on and `tok` came from it): the verify steps take their sampled form, whose picks are the ids plain sampled steps
    would draw, so the loop returns the ids of the plain sampled loop with the same seed; nothing else changes."""
    prompt = input_ids.detach().cpu()
    drafter = PromptLookupDrafter(prompt[0].tolist(), num_tokens, max_ngram, eos, vocab)
    max_length = prompt.shape[1] + max_new_tokens
    new = []
    pending = [int(tok)]
    while True:
        stop = False
        for i, t in enumerate(pending):
            new.append(t)
            drafter.append(t)
            if streamer is not None:
                streamer.put(torch.tensor([t], dtype=torch.int64))
            stop = t in eos or len(new) >= max_new_tokens
            if not stop and stopping_criteria:                # HF StoppingCriteriaList semantics: any criterion stops
                so_far = torch.cat([prompt, torch.tensor([new], dtype=prompt.dtype)], dim=1)
                stop = any(bool(c(so_far, None)) for c in stopping_criteria)
            if stop:
                if len(pending) - 1 - i:
                    engine.kv_rewind(1, len(pending) - 1 - i)   # the slots of the dropped tokens' predecessors
                break
        if stop:
            return new
        budget = min(num_tokens, max_new_tokens - len(new) - 1, max_verify - 1)
        draft = []
        if budget > 0:
            draft = draft_hook(drafter.ids, budget) if draft_hook is not None else drafter.candidates(max_length)
            draft = draft[:budget]
        if draft:
            tokens = [new[-1]] + [int(d) for d in draft]
            picks, n = engine.decode_verify(tokens, sample=True) if sample else engine.decode_verify(tokens)
            pending = [int(x) for x in picks[:n + 1].tolist()]
        else:
            nxt, _ = engine.decode_step(torch.tensor([new[-1]], dtype=torch.int32))
            pending = [int(nxt.view(-1)[0])]
