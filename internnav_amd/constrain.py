"""Token automata for constrained System-2 decoding (host side; numpy only, torch is imported by `to()` alone).

A System-2 answer is STOP, a run of arrow symbols or two pixel coordinates. A `TokenAutomaton` is a small deterministic automaton over token
CLASSES that says which tokens may come next; `ops.automaton_mask_rows` consults its tables on the device in front of every selection launch
(`s2_select.Selection._mask`), so a constrained answer is well formed by construction - what HF's prefix_allowed_tokens_fn
does, without a Python callback per row and step, and inside a captured decode graph.

Tables (limits: S <= 256 states, C <= 256 classes):
  token_class  uint8 [vocab]     the class of every token id
  allow        uint32 [S, 8]     per state a 256-bit class set: class c is allowed iff bit c & 31 of word c >> 5 is set
  next         uint8 [S, 256]    the successor of (state, class); only read for allowed pairs
  start, accepting bool [S], eos_ids
The host methods (`allowed_ids`, `step`, `accepts`) are the reference the device kernel is tested against.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Iterable, Sequence

import numpy as np

MAX_STATES = 256
MAX_CLASSES = 256


def _eos_tuple(eos_ids) -> tuple:
    return tuple(int(e) for e in (eos_ids if isinstance(eos_ids, (list, tuple, np.ndarray)) else [eos_ids]))


class TokenAutomaton:
    def __init__(self, token_class, allow, next, start: int, accepting, eos_ids, eos_absorbing: bool = True):
        """Validates the tables (ValueError naming what is wrong):
          * every allowed (state, class) pair has a successor inside [0, S);
          * every state allows at least one class that holds at least one token, so a logits row can never be masked completely;
          * EOS ids are allowed exactly in the accepting states and lead to an absorbing state that allows only EOS.
        eos_absorbing=False drops the last clause of the last rule: `universal`, whose one state allows everything, is the only user."""
        self.token_class = np.ascontiguousarray(token_class, dtype=np.uint8)
        self.allow = np.ascontiguousarray(allow, dtype=np.uint32)
        self.next = np.ascontiguousarray(next, dtype=np.uint8)
        self.accepting = np.ascontiguousarray(accepting, dtype=bool)
        self.start, self.eos_ids = int(start), _eos_tuple(eos_ids)
        if self.token_class.ndim != 1 or self.token_class.size == 0 or np.asarray(token_class).max() > 255 or np.asarray(token_class).min() < 0:
            raise ValueError("token_class must be a non-empty 1-d table of classes in [0, 256)")
        S = self.allow.shape[0] if self.allow.ndim == 2 else -1
        if not 1 <= S <= MAX_STATES or self.allow.shape != (S, 8):
            raise ValueError(f"allow must be uint32 [S, 8] with 1 <= S <= {MAX_STATES} states, got shape {self.allow.shape}")
        if self.next.shape != (S, 256) or np.asarray(next).max() > 255 or np.asarray(next).min() < 0:
            raise ValueError(f"next must be uint8 [{S}, 256], got shape {self.next.shape}")
        if self.accepting.shape != (S,):
            raise ValueError(f"accepting must be bool [{S}], got shape {self.accepting.shape}")
        if not 0 <= self.start < S:
            raise ValueError(f"start state {self.start} is outside [0, {S})")
        self.n_states, self.vocab = S, int(self.token_class.size)
        bad = [e for e in self.eos_ids if not 0 <= e < self.vocab]
        if bad:
            raise ValueError(f"eos ids {bad} are outside the vocabulary [0, {self.vocab})")
        # allowed[s, c]: the bit sets as booleans
        self._allowed = ((self.allow[:, np.arange(256) >> 5] >> (np.arange(256, dtype=np.uint32) & 31)) & 1).astype(bool)
        populated = np.bincount(self.token_class, minlength=256) > 0
        s_bad, c_bad = np.nonzero(self._allowed & (self.next >= S))
        if s_bad.size:
            raise ValueError(f"state {int(s_bad[0])} allows class {int(c_bad[0])} but next[{int(s_bad[0])}][{int(c_bad[0])}] = "
                             f"{int(self.next[s_bad[0], c_bad[0]])} is outside [0, {S})")
        empty = np.nonzero(~(self._allowed & populated[None, :]).any(axis=1))[0]
        if empty.size:
            raise ValueError(f"state {int(empty[0])} allows no class that holds a token: its logits row would be masked completely")
        for e in self.eos_ids:
            c = int(self.token_class[e])
            wrong = np.nonzero(self._allowed[:, c] != self.accepting)[0]
            if wrong.size:
                s = int(wrong[0])
                raise ValueError(f"eos id {e} is {'allowed' if self._allowed[s, c] else 'not allowed'} in state {s}, which is "
                                 f"{'accepting' if self.accepting[s] else 'not accepting'}: EOS must be allowed exactly in the accepting states")
            if not eos_absorbing:
                continue
            for s in np.nonzero(self.accepting)[0]:
                d = int(self.next[s, c])
                extra = np.setdiff1d(self.allowed_ids(d), np.asarray(self.eos_ids))
                if extra.size or any(int(self.next[d, self.token_class[e2]]) != d for e2 in self.eos_ids):
                    raise ValueError(f"eos id {e} leads from state {int(s)} to state {d}, which is not an absorbing state that allows only EOS"
                                     + (f" (it allows token {int(extra[0])})" if extra.size else ""))
        self._device = {}

    # ---- host reference
    def allowed_ids(self, state: int) -> np.ndarray:
        """the token ids allowed in `state`, ascending (int64)"""
        return np.nonzero(self._allowed[int(state)][self.token_class])[0]

    def step(self, state: int, tok: int) -> int:
        """the state after `tok` in `state`; -1 for a state outside the automaton, a token that is not allowed or an id outside [0, vocab)"""
        state, tok = int(state), int(tok)
        if not (0 <= state < self.n_states and 0 <= tok < self.vocab):
            return -1
        c = int(self.token_class[tok])
        return int(self.next[state, c]) if self._allowed[state, c] else -1

    def run(self, ids: Iterable[int], state=None) -> int:
        """the state after all of `ids` from `state` (default: start), -1 as soon as one is not allowed"""
        s = self.start if state is None else int(state)
        for t in ids:
            s = self.step(s, t)
            if s < 0:
                return -1
        return s

    def accepts(self, ids: Iterable[int]) -> bool:
        """every token allowed where it stands and the last state accepting (an answer may carry its EOS, and EOS fill behind it)"""
        s = self.run(ids)
        return s >= 0 and bool(self.accepting[s])

    def to(self, device):
        """the three tables on `device` (uploaded once per device, then cached): a namespace with token_class u8 [vocab], allow int32 [S, 8]
        (the uint32 words, bit for bit) and next u8 [S, 256]"""
        import torch

        key = str(torch.device(device))
        if key not in self._device:
            up = lambda a: torch.from_numpy(a).to(device)     # noqa: E731
            self._device[key] = SimpleNamespace(token_class=up(self.token_class), allow=up(self.allow.view(np.int32)), next=up(self.next))
        return self._device[key]

    # ---- builders
    @classmethod
    def universal(cls, vocab: int, eos_ids) -> "TokenAutomaton":
        """one accepting state that allows every token and is its own successor: the identity constraint (decoding under it equals
        unconstrained decoding bit for bit; EOS does not absorb)"""
        return cls(np.zeros(int(vocab), dtype=np.uint8), np.array([[1, 0, 0, 0, 0, 0, 0, 0]], dtype=np.uint32), np.zeros((1, 256), dtype=np.uint8), 0,
                   [True], eos_ids, eos_absorbing=False)

    @classmethod
    def _assemble(cls, token_class, trans, start, accepting, eos_ids):
        """trans int [S0, C0] (successor or -1) over S0 states and C0 non-EOS classes -> the automaton with the EOS class C0 (allowed in
        the accepting states) and the absorbing EOS state S0 appended"""
        S0, C0 = trans.shape
        if S0 + 1 > MAX_STATES:
            raise ValueError(f"{S0} states + the EOS state exceed {MAX_STATES}")
        if C0 + 1 > MAX_CLASSES:
            raise ValueError(f"{C0} token classes + the EOS class exceed {MAX_CLASSES}")
        accepting = np.append(np.asarray(accepting, dtype=bool), True)
        allowed = np.zeros((S0 + 1, 256), dtype=bool)
        allowed[:S0, :C0] = trans >= 0
        allowed[:, C0] = accepting
        nxt = np.zeros((S0 + 1, 256), dtype=np.uint8)
        nxt[:S0, :C0] = np.where(trans >= 0, trans, 0)
        nxt[:, C0] = S0
        allow = np.zeros((S0 + 1, 8), dtype=np.uint32)
        for c in range(C0 + 1):
            allow[:, c >> 5] |= allowed[:, c].astype(np.uint32) << np.uint32(c & 31)
        return cls(token_class, allow, nxt, start, accepting, eos_ids)

    @classmethod
    def from_token_sequences(cls, seqs: Sequence[Sequence[int]], eos_ids, vocab: int) -> "TokenAutomaton":
        """a trie over a closed set of answers (token id sequences without EOS): exactly these, each followed by EOS, are accepted.
        ValueError beyond 254 trie nodes (the root counts) or 255 distinct tokens."""
        eos, vocab = _eos_tuple(eos_ids), int(vocab)
        seqs = [[int(t) for t in s] for s in seqs]
        if not seqs:
            raise ValueError("from_token_sequences: no sequence")
        toks = sorted({t for s in seqs for t in s})
        if any(not 0 <= t < vocab for t in toks) or any(t in eos for t in toks):
            raise ValueError("from_token_sequences: the sequences hold ids outside the vocabulary or EOS ids (EOS is appended by the automaton)")
        if len(toks) > 255:
            raise ValueError(f"from_token_sequences: {len(toks)} distinct tokens exceed 255")
        col = {t: i for i, t in enumerate(toks)}
        children, accepting = [{}], [False]
        for s in seqs:
            node = 0
            for t in s:
                if t not in children[node]:
                    children[node][t] = len(children)
                    children.append({})
                    accepting.append(False)
                    if len(children) > 254:
                        raise ValueError("from_token_sequences: the trie of the sequences exceeds 254 nodes")
                node = children[node][t]
            accepting[node] = True
        others = vocab - len(toks) - len(set(eos))             # tokens in no sequence: one class more, never allowed
        trans = np.full((len(children), len(toks) + (1 if others else 0)), -1, dtype=np.int64)
        for node, ch in enumerate(children):
            for t, d in ch.items():
                trans[node, col[t]] = d
        token_class = np.full(vocab, len(toks), dtype=np.int64)
        token_class[toks] = np.arange(len(toks))
        token_class[list(eos)] = trans.shape[1]
        return cls._assemble(token_class, trans, 0, accepting, eos)

    @classmethod
    def from_byte_dfa(cls, token_bytes: Sequence[bytes], n_states: int, start: int, accepting, delta, eos_ids) -> "TokenAutomaton":
        """the usual lifting of a byte-level DFA to tokens (the tokenizer is byte-level BPE: token_bytes[i] = the bytes of token i; one
        symbol may be several tokens and one token several symbols). delta int [n_states, 256]: the successor of (state, byte), negative =
        dead. A token is allowed in state s iff its bytes run through delta from s without dying; its successor is where they end. Tokens
        with the same vector of successors share a class. Tokens without bytes (special tokens) are never allowed; the EOS ids get a class of
        their own, allowed in the accepting states. Byte states that no token sequence reaches from `start` are dropped (the others keep
        their order; with every state reachable the numbering is the caller's, the EOS state is n_states). ValueError beyond 256 states
        (the EOS state included) or 256 classes."""
        eos = _eos_tuple(eos_ids)
        delta = np.asarray(delta, dtype=np.int64)
        n_states = int(n_states)
        if delta.shape != (n_states, 256) or int(delta.max(initial=-1)) >= n_states:
            raise ValueError(f"from_byte_dfa: delta must be int [{n_states}, 256] with successors below {n_states}")
        vocab = len(token_bytes)
        dead = np.append(delta, np.full((1, 256), n_states, dtype=np.int64), axis=0)     # row n_states: the dead state, absorbing
        dead[dead < 0] = n_states
        vec = np.full((vocab, n_states), -1, dtype=np.int64)
        for i, bs in enumerate(token_bytes):
            if i in eos or len(bs) == 0:
                continue
            cur = np.arange(n_states)
            for b in bytes(bs):
                cur = dead[cur, b]
            vec[i] = np.where(cur == n_states, -1, cur)
        # byte states that no TOKEN sequence reaches from the start (the middle of a symbol this vocabulary never splits there) are dropped
        # and the kept ones renumbered in ascending order: such a state may allow no token at all, which the constructor refuses
        reach, todo = {int(start)}, [int(start)]
        while todo:
            for d in np.unique(vec[:, todo.pop()]):
                if d >= 0 and int(d) not in reach:
                    reach.add(int(d))
                    todo.append(int(d))
        keep = np.asarray(sorted(reach), dtype=np.int64)
        renum = np.full(n_states + 1, -1, dtype=np.int64)                 # (index -1 = the appended entry: dead stays dead)
        renum[keep] = np.arange(keep.size)
        vec, start, accepting, n_states = renum[vec[:, keep]], int(renum[int(start)]), np.asarray(accepting, dtype=bool)[keep], int(keep.size)
        rest = np.asarray([i for i in range(vocab) if i not in eos], dtype=np.int64)
        uniq, inv = np.unique(vec[rest], axis=0, return_inverse=True)
        token_class = np.full(vocab, uniq.shape[0], dtype=np.int64)
        token_class[rest] = inv.reshape(-1)
        if uniq.shape[0] + 1 > MAX_CLASSES:
            raise ValueError(f"from_byte_dfa: {uniq.shape[0]} distinct token transition vectors + the EOS class exceed {MAX_CLASSES} classes")
        return cls._assemble(token_class, uniq.T.copy(), int(start), accepting, eos)

    @classmethod
    def navigation_answers(cls, token_bytes: Sequence[bytes], eos_ids, actions=("↑", "←", "→", "↓"), stop: str = "STOP", max_actions: int = 8,
                           max_digits: int = 4, separators=(" ", ", ", ",")) -> "TokenAutomaton":
        """the System-2 answer language  stop | action{1..max_actions} | digits{1..max_digits} sep digits{1..max_digits}  as a byte DFA
        (UTF-8), lifted to the tokens of `token_bytes` with `from_byte_dfa`.
        NO real tokenizer or checkpoint has been seen: how the trained model spells a pixel goal (which separator, whether a space leads the
        second number) is an assumption, which is why the separator set - and every other piece - is a parameter. Build token_bytes from
        the checkpoint's tokenizer and check a few recorded answers with `accepts` before relying on it."""
        enc = lambda s: s.encode("utf-8") if isinstance(s, str) else bytes(s)     # noqa: E731
        acts, seps, stop_b = [enc(a) for a in actions], [enc(s) for s in separators], enc(stop)
        digits = b"0123456789"
        if not (acts and seps and stop_b and max_actions >= 1 and max_digits >= 1) or any(not a for a in acts) or any(not s for s in seps):
            raise ValueError("navigation_answers: actions, separators and stop must be non-empty, max_actions and max_digits >= 1")
        if any(b in digits for s in seps for b in s):
            raise ValueError("navigation_answers: a separator holds a digit")
        rows, accepting = [], []

        def new(acc=False):
            rows.append(np.full(256, -1, dtype=np.int64))
            accepting.append(acc)
            return len(rows) - 1

        def edge(s, b, make):
            """the successor of (s, b), created with make() when there is none yet"""
            if rows[s][b] < 0:
                rows[s][b] = make()
            return int(rows[s][b])

        words = [stop_b] + acts                                   # prefix-free and digit-free at the front: the tries below then never collide
        for i, a in enumerate(words):
            if a[0] in digits or any(j != i and o.startswith(a) for j, o in enumerate(words)):
                raise ValueError(f"navigation_answers: {a!r} starts with a digit, or is a prefix of (or equal to) another of stop / actions")
        start = new()
        done = [start] + [new(True) for _ in range(max_actions)]  # done[k]: k whole actions
        for k in range(max_actions):                              # behind done[k] a trie of the actions' bytes (at the start: and of stop's)
            for a in ([stop_b] if k == 0 else []) + acts:
                s = done[k]
                for b in a[:-1]:
                    s = edge(s, b, new)
                rows[s][a[-1]] = new(True) if (k == 0 and a is stop_b) else done[k + 1]
        first = [new() for _ in range(max_digits)]                # first[k]: k + 1 digits of the first coordinate
        second = [new(True) for _ in range(max_digits)]
        for d in digits:
            rows[start][d] = first[0]
            for k in range(max_digits - 1):
                rows[first[k]][d], rows[second[k]][d] = first[k + 1], second[k + 1]
        sep_root = new()                                          # a trie of the separators, shared by every first[k] (entered by its first byte)
        complete = set()
        for sp in seps:
            s = sep_root
            for b in sp:
                s = edge(s, b, new)
            complete.add(s)
        for s in complete:
            for d in digits:
                rows[s][d] = second[0]
        for k in range(max_digits):
            rows[first[k]] = np.where(rows[sep_root] >= 0, rows[sep_root], rows[first[k]])
        # sep_root itself is never entered: drop it (it is the last state but the trie's inner nodes, so renumber)
        keep = [i for i in range(len(rows)) if i != sep_root]
        remap = np.full(len(rows) + 1, -1, dtype=np.int64)
        remap[keep] = np.arange(len(keep))
        delta = np.stack([remap[rows[i]] for i in keep])          # (-1 indexes the appended -1)
        return cls.from_byte_dfa(token_bytes, len(keep), int(remap[start]), [accepting[i] for i in keep], delta, eos_ids)
