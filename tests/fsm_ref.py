"""CPU restatement of the token-FSM stage (omchat_amd/csrc/fsm.hip) over the plain `{state: {token: next}}` dict:
the state after a row's fed tokens, the ids allowed there and the masked row.  tests/test_fsm_cpu.py pins `apply` to the installed
transformers' PrefixConstrainedLogitsProcessor."""
import numpy as np

DEAD = -1


def step(trans, state, token):
    """a token without an edge from the row's state kills the row; DEAD stays DEAD"""
    if state == DEAD:
        return DEAD
    return trans.get(state, {}).get(int(token), DEAD)


def walk(trans, ids, start=0):
    s = start
    for t in ids:
        s = step(trans, s, t)
    return s


def allowed(trans, state):
    """sorted global ids that stay finite in `state`; None in DEAD (the row passes through unmasked)"""
    return None if state == DEAD else sorted(trans.get(state, {}))


def apply(trans, logits_row, state, gbase=0):
    """fp32 logits (the slice starting at global id gbase) with every id that is no edge of `state` at -inf"""
    l = np.asarray(logits_row, dtype=np.float32)
    ids = allowed(trans, state)
    if ids is None:
        return l.copy()
    out = np.full_like(l, -np.inf)
    loc = [i - gbase for i in ids if 0 <= i - gbase < l.shape[0]]
    out[loc] = l[loc]
    return out
