"""References for prompt-lookup decoding (omchat_amd/lookup.py): HF's own PromptLookupCandidateGenerator as the drafter, and a fake engine
whose "model" is a deterministic function of the prefix, with the greedy loop of generate() restated over it."""
import zlib

import torch


def hf_candidates(ids, k, m, eos=(), max_length=None):
    """the draft HF 5.15's PromptLookupCandidateGenerator.get_candidates proposes after `ids` (list), or None without transformers"""
    try:
        from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    except ImportError:
        return None
    g = PromptLookupCandidateGenerator(eos_token_id=torch.tensor(list(eos)) if eos else None, num_output_tokens=k, max_matching_ngram_size=m,
                                       max_length=max_length if max_length is not None else len(ids) + 10 ** 6)
    cand, _ = g.get_candidates(torch.tensor([ids], dtype=torch.long))
    return cand[0, len(ids):].tolist()


class PrefixModel:
    """next id = a deterministic function of the whole prefix: mostly it continues the first earlier occurrence of the last id (so that
    prompt lookup has something to find), otherwise a hashed id in [0, V)"""

    def __init__(self, V=50, copy_every=4, seed=0):
        self.V, self.copy_every, self.seed = V, copy_every, seed

    def __call__(self, prefix):
        h = zlib.crc32(bytes(str((self.seed, tuple(prefix))), "ascii"))
        last = prefix[-1]
        if h % self.copy_every:
            for j, t in enumerate(prefix[:-1]):
                if t == last and 0 <= prefix[j + 1] < self.V:
                    return prefix[j + 1]
        return (h >> 8) % self.V


class FakeEngine:
    """the cache bookkeeping of omchat_decode_step / omchat_decode_verify / omchat_kv_rewind over PrefixModel"""

    def __init__(self, model, prompt):
        self.model, self.cache = model, list(prompt)
        self.verify_steps = self.plain_steps = self.accepted = 0

    def decode_step(self, tokens):
        self.cache.append(int(tokens.view(-1)[0]))
        self.plain_steps += 1
        return torch.tensor([self.model(self.cache)], dtype=torch.int32), None

    def decode_verify(self, tokens, keep_all=False):
        assert 2 <= len(tokens) <= 16
        picks = [self.model(self.cache + tokens[:j + 1]) for j in range(len(tokens))]
        n = 0
        while n < len(tokens) - 1 and tokens[n + 1] == picks[n]:
            n += 1
        self.cache += tokens if keep_all else tokens[:n + 1]
        self.verify_steps += 1
        self.accepted += n
        return torch.tensor(picks, dtype=torch.int32), n

    def kv_rewind(self, b, n):
        assert b == 1 and 0 < n <= len(self.cache)
        del self.cache[-n:]


def greedy_ref(model, prompt, max_new, eos, streamer=None, stopping_criteria=None):
    """generate()'s greedy loop at b = 1 over PrefixModel: EOS kept, stop on max_new_tokens or any stopping criterion"""
    ids = list(prompt)
    new = []
    tok = model(ids)
    while True:
        new.append(tok)
        ids.append(tok)
        if streamer is not None:
            streamer.put(torch.tensor([tok]))
        stop = tok in eos or len(new) >= max_new
        if not stop and stopping_criteria:
            so_far = torch.tensor([ids])
            stop = any(bool(c(so_far, None)) for c in stopping_criteria)
        if stop:
            return new
        tok = model(ids)
