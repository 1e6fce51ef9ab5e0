"""References for prompt-lookup decoding with do_sample=True ("Sampling"): the sampler's verify form restated on top of
sampling_ref / sampling_ref2, a fake engine that carries the sampler's step counter and seen set through decode_step, decode_verify(sample=True)
and kv_rewind as the library does, and the plain sampled loop of generate() over the same engine."""
import zlib

import numpy as np
import torch

import sampling_ref as sr
import sampling_ref2 as sr2

FILTER_KEYS = ("top_k", "top_p", "min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")


def split_params(params):
    """params as Engine.set_sampling takes them -> (temperature, penalty, the keyword arguments of sampling_ref2.interval)"""
    p = dict(params)
    T = float(p.pop("temperature", 1.0))
    pen = float(p.pop("repetition_penalty", p.pop("penalty", 1.0)))
    kw = {k: p.pop(k) for k in FILTER_KEYS if p.get(k) is not None}
    for k in FILTER_KEYS:             # (None = off, as Engine.set_sampling reads it)
        p.pop(k, None)
    kw.setdefault("top_k", 0)
    kw.setdefault("top_p", 1.0)
    assert not p, f"unknown sampling parameters {sorted(p)}"
    return T, pen, kw


def local_seen(seen, gbase, V, V_total):
    """global seen ids -> the local ids of the vocabulary slice [gbase, gbase + V); ids outside [0, V_total) or the slice are ignored"""
    return sorted({int(i) - gbase for i in seen if 0 <= int(i) < V_total and 0 <= int(i) - gbase < V})


def verify_sample_ref(logits, tokens, seed, step0, base_seen, params, gbase=0, V_total=None, want_interval=False):
    """the picks of a sampled verify step: logits [T, V] (rank-local slice at global offset gbase), tokens [T] = the last emitted id and the
    drafts.  Row j: row 0's key at step step0 + j, seen = base_seen + tokens[1..j] (global ids).  -> ids [T] (global), with want_interval
    also the two ends (lo, hi) of every row's kept key interval"""
    logits = np.asarray(logits, dtype=np.float32)
    T_rows, V = logits.shape
    V_total = V if V_total is None else V_total
    temp, pen, kw = split_params(params)
    ids, los, his = [], [], []
    for j in range(T_rows):
        seen = local_seen(list(base_seen) + [int(t) for t in tokens[1:j + 1]], gbase, V, V_total)
        ids.append(sr2.sample_row(logits[j], 0, step0 + j, seed, temp, seen, pen, gbase, **kw))
        if want_interval:
            lo, hi = sr2.interval(sr.processed(logits[j], temp, seen, pen), **kw)
            los.append(lo); his.append(hi)
    ids = np.array(ids, dtype=np.int64)
    return (ids, np.array(los, dtype=np.int64), np.array(his, dtype=np.int64)) if want_interval else ids


class PrefixLogits:
    """fp32 logits [V] as a deterministic function of the whole prefix: hashed normal values, and a large bonus on the id that continues the
    first earlier occurrence of the last id (so that sampling mostly copies and prompt lookup has something to find)"""

    def __init__(self, V=50, bonus=9.0, seed=0):
        self.V, self.bonus, self.seed = V, bonus, seed

    def __call__(self, prefix):
        h = zlib.crc32(bytes(str((self.seed, tuple(prefix))), "ascii"))
        x = np.random.default_rng(h).standard_normal(self.V).astype(np.float32)
        last = prefix[-1]
        for j, t in enumerate(prefix[:-1]):
            if t == last and 0 <= prefix[j + 1] < self.V:
                x[prefix[j + 1]] += np.float32(self.bonus)
                break
        return x


class FakeSampleEngine:
    """the cache, step-counter and seen-set bookkeeping of omchat_sample / omchat_decode_step / omchat_decode_verify(OMCHAT_VERIFY_SAMPLE) /
    omchat_kv_rewind for sequence 0 over PrefixLogits"""

    def __init__(self, model, prompt, seed, params):
        self.model, self.cache, self.seed, self.params = model, list(prompt), seed, dict(params)
        self.temp, self.pen, self.kw = split_params(params)
        self.step = 0
        # (as on the device, the seen set is kept only while the penalty is on)
        self.seen = set(int(i) for i in prompt if 0 <= int(i) < model.V) if self.pen != 1.0 else set()
        self.last = None            # the id whose bit the last plain pick newly set
        self.vlast = []             # per committed pick of the last verify step: the id it newly set, or None
        self.verify_steps = self.plain_steps = self.accepted = 0
        self.rewinds = []

    def _commit(self, tok):
        new = tok not in self.seen if self.pen != 1.0 else False
        if new:
            self.seen.add(tok)
        self.step += 1
        return tok if new else None

    def _pick(self):
        seen = sorted(self.seen) if self.pen != 1.0 else None
        return sr2.sample_row(self.model(self.cache), 0, self.step, self.seed, self.temp, seen, self.pen, **self.kw)

    def sample_first(self):
        tok = self._pick()
        self.last, self.vlast = self._commit(tok), []
        return tok

    def decode_step(self, tokens):
        self.cache.append(int(tokens.view(-1)[0]))
        self.plain_steps += 1
        tok = self._pick()
        self.last, self.vlast = self._commit(tok), []
        return torch.tensor([tok], dtype=torch.int32), None

    def decode_verify(self, tokens, keep_all=False, sample=False):
        assert sample and not keep_all and 2 <= len(tokens) <= 16
        logits = np.stack([self.model(self.cache + tokens[:j + 1]) for j in range(len(tokens))])
        base = sorted(self.seen) if self.pen != 1.0 else []
        picks = verify_sample_ref(logits, tokens, self.seed, self.step, base, self.params).tolist()
        n = 0
        while n < len(tokens) - 1 and tokens[n + 1] == picks[n]:
            n += 1
        self.vlast = [self._commit(p) for p in picks[:n + 1]]
        self.last = None
        self.cache += tokens[:n + 1]
        self.verify_steps += 1
        self.accepted += n
        return torch.tensor(picks, dtype=torch.int32), n

    def kv_rewind(self, b, n):
        assert b == 1 and 0 < n <= len(self.cache)
        if self.vlast and n <= len(self.vlast):
            for _ in range(n):
                t = self.vlast.pop()
                if t is not None:
                    self.seen.discard(t)
        else:
            assert n == 1 or self.pen == 1.0, "rewind of more than one step with the repetition penalty on"
            if self.last is not None:
                self.seen.discard(self.last)
            self.last, self.vlast = None, []
        self.step -= n
        del self.cache[-n:]
        self.rewinds.append(n)

    def sampling_state(self):
        return self.step, sorted(self.seen)


def sampled_ref(eng, prompt, max_new, eos, streamer=None, stopping_criteria=None):
    """generate()'s sampled loop at b = 1 over a FakeSampleEngine: EOS kept, stop on max_new_tokens or any stopping criterion; the step that
    generate() enqueues ahead of looking at a token and takes back at a stop is simply not taken"""
    ids = list(prompt)
    new = []
    tok = eng.sample_first()
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
        nxt, _ = eng.decode_step(torch.tensor([tok]))
        tok = int(nxt[0])
