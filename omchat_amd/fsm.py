"""Host side of generate(token_fsm=): the token automaton every grammar / regex compiler produces -- `state ->
{token id: next state}`, the keys of a state being the ids allowed there -- as CSR arrays, its validation, a trie builder for
multiple-choice answers, and the resolution of generate()'s arguments with every refusal before any work is enqueued.  The mask and the
transition run on the device (csrc/fsm.hip)."""

DEAD = -1      # the state of a row that was fed a token without an edge (the pad of an ended row, an EOS without an edge): nothing is masked there
MAX_STATES = 1 << 20      # include/omchat_hip.h: OMCHAT_FSM_MAX_STATES / OMCHAT_FSM_MAX_EDGES
MAX_EDGES = 1 << 26


class TokenFSM:
    """A deterministic automaton over token ids.  transitions: {state: {token: next state}} with states 0 .. n - 1 (a state that only occurs
    as a target counts, and then needs edges of its own); the keys of a state are the ids allowed there.  EOS ids are ordinary tokens: a
    state in which the answer may end has an EOS edge (its target does not matter; a self-loop on a final state is the usual choice).
    vocab_size: checked against the ids here when given, against the model's vocabulary in generate() in any case."""

    def __init__(self, transitions, vocab_size=None):
        if not isinstance(transitions, dict) or not transitions:
            raise ValueError("TokenFSM: transitions must be a non-empty dict {state: {token: next_state}}")
        n = 0
        for s, edges in transitions.items():
            if not isinstance(s, int) or isinstance(s, bool) or s < 0:
                raise ValueError(f"TokenFSM: state {s!r} is not a non-negative int")
            if not isinstance(edges, dict):
                raise ValueError(f"TokenFSM: the edges of state {s} must be a dict {{token: next_state}}")
            n = max([n, s + 1] + [int(t) + 1 for t in edges.values() if isinstance(t, int) and t >= 0])
        off, tok, nxt = [0], [], []
        for s in range(n):
            edges = transitions.get(s, {})
            for t in sorted(edges):
                if not isinstance(t, int) or isinstance(t, bool) or not isinstance(edges[t], int) or isinstance(edges[t], bool):
                    raise ValueError(f"TokenFSM: state {s} has an edge whose token or target is not an int")
                tok.append(t)
                nxt.append(edges[t])
            off.append(len(tok))
        self._init(off, tok, nxt, vocab_size)

    @classmethod
    def from_arrays(cls, off, tok, nxt, vocab_size=None):
        """CSR: the edges of state s are tok / nxt [off[s] : off[s + 1]], sorted by token"""
        self = cls.__new__(cls)
        self._init([int(x) for x in off], [int(x) for x in tok], [int(x) for x in nxt], vocab_size)
        return self

    @classmethod
    def from_choices(cls, choices, eos_token_id, vocab_size=None):
        """The trie whose language is exactly the given id sequences, each followed by EOS (one id or several: every one of them ends an
        answer).  A choice may be a prefix of another; an empty choice or an empty list is refused."""
        eos = [int(e) for e in (eos_token_id if isinstance(eos_token_id, (list, tuple)) else [eos_token_id])]
        if not eos or any(e < 0 for e in eos):
            raise ValueError("TokenFSM.from_choices: eos_token_id must be one or more non-negative ids")
        choices = [[int(t) for t in c] for c in choices]
        if not choices or any(not c for c in choices):
            raise ValueError("TokenFSM.from_choices: at least one choice, none of them empty")
        trans = {0: {}, 1: {e: 1 for e in eos}}      # 1 = the final state: EOS loops there
        for c in choices:
            s = 0
            for t in c:
                if t in eos:
                    raise ValueError("TokenFSM.from_choices: a choice contains an EOS id")
                if t not in trans[s]:
                    trans[s][t] = len(trans)
                    trans[len(trans)] = {}
                s = trans[s][t]
            for e in eos:
                trans[s][e] = 1
        return cls(trans, vocab_size)

    def _init(self, off, tok, nxt, vocab_size):
        n = len(off) - 1
        if n < 1 or off[0] != 0 or len(tok) != off[-1] or len(nxt) != len(tok):
            raise ValueError("TokenFSM: off must start at 0 and end at len(tok) == len(nxt), with at least one state")
        if n > MAX_STATES or len(tok) > MAX_EDGES:
            raise ValueError(f"TokenFSM: at most {MAX_STATES} states and {MAX_EDGES} edges")
        target = [False] * n
        for s in range(n):
            if off[s + 1] < off[s]:
                raise ValueError("TokenFSM: off must ascend")
            for e in range(off[s], off[s + 1]):
                if tok[e] < 0 or (vocab_size is not None and tok[e] >= vocab_size):
                    raise ValueError(f"TokenFSM: state {s} has an edge token outside the vocabulary ({tok[e]})")
                if e > off[s] and tok[e] <= tok[e - 1]:
                    raise ValueError(f"TokenFSM: the edges of state {s} must be sorted by token, without duplicates")
                if not 0 <= nxt[e] < n:
                    raise ValueError(f"TokenFSM: state {s} has an edge to state {nxt[e]}, outside the table")
                target[nxt[e]] = True
        # any state may be handed over as a start state, so every edge's source counts as reachable, and with it the edge's target
        for s in range(n):
            if target[s] and off[s + 1] == off[s]:
                raise ValueError(f"TokenFSM: state {s} can be reached and has no edge: every logit there would be -inf; add an EOS edge")
        self.n_states, self.off, self.tok, self.nxt, self.vocab_size = n, off, tok, nxt, vocab_size
        self._tok_max = None

    # ------------------------------------------------------------------ helpers
    def arrays(self):
        return self.off, self.tok, self.nxt

    def tok_max(self):
        """the largest edge token (-1 without edges)"""
        if self._tok_max is None:
            self._tok_max = max(self.tok) if self.tok else -1
        return self._tok_max

    def transitions(self):
        return {s: dict(zip(self.tok[self.off[s]:self.off[s + 1]], self.nxt[self.off[s]:self.off[s + 1]])) for s in range(self.n_states)}

    def allowed(self, state):
        """the ids allowed in `state`, ascending; None in DEAD (nothing is masked there)"""
        if state == DEAD:
            return None
        return self.tok[self.off[state]:self.off[state + 1]]

    def next(self, state, token):
        if state == DEAD:
            return DEAD
        import bisect
        lo, hi = self.off[state], self.off[state + 1]
        i = bisect.bisect_left(self.tok, int(token), lo, hi)
        return self.nxt[i] if i < hi and self.tok[i] == int(token) else DEAD

    def walk(self, ids, start=0):
        """the state after the ids, or DEAD"""
        s = start
        for t in ids:
            s = self.next(s, t)
        return s

    def check_start(self, state):
        if not (isinstance(state, int) and not isinstance(state, bool) and 0 <= state < self.n_states):
            raise ValueError(f"fsm_start: {state!r} is not a state of the token FSM (0 .. {self.n_states - 1})")
        if self.off[state + 1] == self.off[state]:
            raise ValueError(f"fsm_start: state {state} has no edge: every logit there would be -inf; add an EOS edge")

    def as_prefix_allowed_tokens_fn(self, prompt_len, start=0):
        """HF's callback computing the same constraint: generate(prefix_allowed_tokens_fn=...) there walks the ids behind the first
        prompt_len of the row; in DEAD everything is allowed.  start: one state, or one per batch row."""
        def fn(batch_id, input_ids):
            s0 = start[batch_id] if isinstance(start, (list, tuple)) else start
            ids = input_ids.tolist() if hasattr(input_ids, "tolist") else list(input_ids)
            s = self.walk(ids[prompt_len:], s0)
            if s == DEAD:
                return list(range(self.vocab_size))
            return list(self.allowed(s))
        if self.vocab_size is None:
            raise ValueError("TokenFSM.as_prefix_allowed_tokens_fn: a DEAD row allows every id; give the TokenFSM its vocab_size")
        return fn


def resolve_token_fsm(token_fsm, fsm_start, n_prompts, n_rows, vocab_total, num_beams=1, lookup=False):
    """generate()'s token_fsm / fsm_start -> None, or the start state of each of the n_rows rows of the expanded batch (n_prompts prompts,
    n_rows / n_prompts siblings each).  Every refusal is raised here, from host data, before anything is enqueued."""
    if token_fsm is None:
        if fsm_start is not None:
            raise ValueError("fsm_start without token_fsm")
        return None
    if not isinstance(token_fsm, TokenFSM):
        raise ValueError("token_fsm must be an omchat_amd.fsm.TokenFSM (TokenFSM(transitions) takes the index other libraries build)")
    if num_beams > 1:
        raise NotImplementedError("token_fsm with num_beams > 1 is not implemented: each beam row would need its parent's state")
    if lookup:
        raise NotImplementedError("token_fsm with prompt_lookup_num_tokens is not implemented: each verify row would need its own state")
    if token_fsm.tok and token_fsm.tok_max() >= vocab_total:
        raise ValueError(f"token_fsm has an edge token outside the model's vocabulary ({token_fsm.tok_max()} >= {vocab_total})")
    if fsm_start is None:
        fsm_start = 0
    if isinstance(fsm_start, int) and not isinstance(fsm_start, bool):
        starts = [fsm_start] * n_rows
    elif isinstance(fsm_start, (list, tuple)) and len(fsm_start) == n_rows:
        starts = list(fsm_start)
    elif isinstance(fsm_start, (list, tuple)) and len(fsm_start) == n_prompts and n_rows % n_prompts == 0:
        starts = [s for s in fsm_start for _ in range(n_rows // n_prompts)]      # prompt-major, as the rows are
    else:
        raise ValueError(f"fsm_start must be one state, or a list with one state per prompt ({n_prompts}) or per row ({n_rows})")
    for s in starts:
        token_fsm.check_start(s)
    return starts

