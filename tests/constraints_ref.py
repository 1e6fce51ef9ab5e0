"""CPU restatement of the ban stage (omchat_amd/csrc/constrain.hip): the ids HF's NoRepeatNGram, NoBadWords, MinLength,
MinNewTokensLength, SuppressTokens and SuppressTokensAtBegin processors set to -inf for one row.  tests/test_constraints_cpu.py pins it to
the installed transformers, set for set."""
import numpy as np


def params(V, ngram=0, bad_words=(), eos=(), min_new=0, min_len=0, suppress=(), begin_suppress=()):
    return dict(V=int(V), ngram=int(ngram), bad_words=[list(w) for w in bad_words], eos=list(eos), min_new=int(min_new), min_len=int(min_len),
                suppress=list(suppress), begin_suppress=list(begin_suppress))


def banned_ids(history_row, params, step):
    """history_row: the ids HF's processors see (prompt row as passed + the ids appended so far, `step` of them generated) -> sorted banned
    ids.  Ids outside [0, V) are never banned."""
    h = [int(x) for x in history_row]
    L, P = len(h), len(h) - int(step)
    ban = set()
    n = params["ngram"]
    if n >= 1 and L + 1 >= n:
        tail = h[L - (n - 1):] if n > 1 else []
        for i in range(0, L - n + 1):
            if h[i:i + n - 1] == tail:
                ban.add(h[i + n - 1])
    eos = list(params["eos"])
    for w in params["bad_words"]:
        m = len(w)
        if m == 1 and w[0] in eos:        # NoBadWordsLogitsProcessor drops a word that is one EOS id
            continue
        if m > 1 and m > L:               # longer than the context: ignored
            continue
        if m == 1 or h[L - (m - 1):] == list(w[:-1]):
            ban.add(int(w[-1]))
    if L - P < params["min_new"] or L < params["min_len"]:
        ban.update(eos)
    ban.update(params["suppress"])
    if L == P:
        ban.update(params["begin_suppress"])
    return sorted(i for i in ban if 0 <= i < params["V"])


def apply(logits_row, ids, gbase=0):
    """fp32 logits (the slice starting at global id gbase) with the banned global ids at -inf"""
    l = np.asarray(logits_row, dtype=np.float32).copy()
    loc = [i - gbase for i in ids if 0 <= i - gbase < l.shape[0]]
    l[loc] = -np.inf
    return l
