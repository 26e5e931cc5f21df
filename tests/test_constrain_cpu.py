"""CPU: the token automata of constrained System-2 decoding (internnav_amd/constrain.py) - the builders against brute force on a synthetic
300-token byte vocabulary, the trie builder and every validation error, and the numpy restatement of the device mask against transformers'
PrefixConstrainedLogitsProcessor."""
import itertools

import numpy as np
import pytest

import constrain_ref as R

from internnav_amd.constrain import TokenAutomaton

TOKS, EOS = R.byte_vocab(300)
IDX = {b: i for i, b in enumerate(TOKS) if b}


def _digit_dfa():
    """bytes: one or more digits, a comma, one digit (accepting)"""
    delta = np.full((4, 256), -1, dtype=np.int64)
    for d in b"0123456789":
        delta[0, d], delta[1, d], delta[2, d] = 1, 1, 3
    delta[1, ord(",")] = 2
    return delta, [False, False, False, True]


def _survive(delta, s, bs):
    for b in bs:
        if s < 0:
            return -1
        s = int(delta[s, b])
    return s


def test_from_byte_dfa_against_brute_force():
    delta, acc = _digit_dfa()
    a = TokenAutomaton.from_byte_dfa(TOKS, 4, 0, acc, delta, [EOS])
    assert a.vocab == 300 and a.n_states == 5 and a.start == 0 and a.eos_ids == (EOS,)
    assert a.token_class.dtype == np.uint8 and a.allow.dtype == np.uint32 and a.allow.shape == (5, 8) and a.next.dtype == np.uint8 and a.next.shape == (5, 256)
    for s in range(4):
        want = [i for i, bs in enumerate(TOKS) if bs and i != EOS and _survive(delta, s, bs) >= 0] + ([EOS] if acc[s] else [])
        assert a.allowed_ids(s).tolist() == sorted(want), s
        for i, bs in enumerate(TOKS):
            if i == EOS:
                assert a.step(s, i) == (4 if acc[s] else -1)
            else:
                assert a.step(s, i) == (_survive(delta, s, bs) if bs else -1), (s, i, bs)
    assert a.allowed_ids(4).tolist() == [EOS] and a.step(4, EOS) == 4 and a.step(4, 0) == -1
    for bad in (-1, 300, 10 ** 9):
        assert a.step(0, bad) == -1 and a.step(bad, 0) == -1
    # tokens with the same transition vector share a class, others do not
    assert a.token_class[IDX[b"3"]] == a.token_class[IDX[b"8"]] != a.token_class[IDX[b","]]
    assert a.token_class[IDX[b"the"]] == a.token_class[290]                                  # never allowed: one class with the byte-less tokens
    assert a.accepts([IDX[b"12"], IDX[b",1"]]) and a.accepts([IDX[b"1"], IDX[b","], IDX[b"7"], EOS, EOS]) and not a.accepts([IDX[b"1"], IDX[b","]])


def test_from_byte_dfa_limits():
    ring = np.full((256, 256), -1, dtype=np.int64)
    ring[np.arange(256), 1] = (np.arange(256) + 1) % 256
    with pytest.raises(ValueError, match="states"):                          # 256 reachable byte states + the EOS state
        TokenAutomaton.from_byte_dfa([b"eos", b"\x01"], 256, 0, [True] * 256, ring, [0])
    # byte states no token sequence reaches are dropped: of the 256 only 0 and 128 remain under a token of 128 bytes
    half = TokenAutomaton.from_byte_dfa([b"eos", b"\x01" * 128], 256, 0, [True] * 256, ring, [0])
    assert half.n_states == 3 and half.run([1, 1, 1]) == 1 and half.accepts([1, 0])
    # a ring of 254 states in which byte b is alive only in state b: 254 one-byte tokens with pairwise different transition vectors, the
    # byte-less token's all-dead vector and EOS are 256 classes; a two-byte token's vector is one too many
    n = 254
    delta = np.full((n, 256), -1, dtype=np.int64)
    for s in range(n):
        delta[s, s] = (s + 1) % n
    toks = [bytes([b]) for b in range(n)] + [b"", b"eos"]
    fits = TokenAutomaton.from_byte_dfa(toks, n, 0, [True] * n, delta, [n + 1])
    assert fits.n_states == 255 and int(fits.token_class.max()) == 255
    with pytest.raises(ValueError, match="classes"):
        TokenAutomaton.from_byte_dfa(toks + [bytes([0, 1])], n, 0, [True] * n, delta, [n + 1])
    with pytest.raises(ValueError, match="delta"):
        TokenAutomaton.from_byte_dfa(TOKS, 4, 0, [True] * 4, np.zeros((4, 255)), [EOS])


def _tokenisations(text: bytes):
    """every way to write `text` with the vocabulary's tokens"""
    if not text:
        yield []
        return
    for bs, i in IDX.items():
        if text.startswith(bs):
            for rest in _tokenisations(text[len(bs):]):
                yield [i] + rest


GOOD = ["STOP", "↑", "←→", "↑↑↑↑↑↑↑↑", "↓↓←", "1 2", "12,7", "640, 480", "0012 0007", "9999,9999", "5, 5"]
BAD = ["12", "1 2 3", "1,2,3", "12345 1", "1 12345", "", "↑1", "1↑", "↑ 1 2", "↑↑↑↑↑↑↑↑↑", "STOP↑", "STOPSTOP", "1  2", "1 ,2", "1,, 2", "1,", " 1 2", "STO",
       "↑STOP", "12 ", "the"]


@pytest.fixture(scope="module")
def nav():
    return TokenAutomaton.navigation_answers(TOKS, [EOS])


def test_navigation_answers_language(nav):
    assert nav.n_states <= 256 and int(nav.token_class.max()) < 256
    n_tok = 0
    for text in GOOD:
        ways = list(_tokenisations(text.encode("utf-8")))
        assert ways, text
        n_tok += len(ways)
        for ids in ways:
            assert nav.accepts(ids) and nav.accepts(ids + [EOS]) and nav.accepts(ids + [EOS, EOS]), (text, ids)
            assert not nav.accepts(ids + [EOS, ids[0]])
    assert n_tok > 100                                       # (split arrows, two-digit tokens, ' 2' tokens: many spellings per answer)
    for text in BAD:
        for ids in _tokenisations(text.encode("utf-8")):
            assert not nav.accepts(ids), (text, ids)
    assert not nav.accepts([]) and not nav.accepts([EOS])
    # parameters: another separator set, fewer actions / digits
    semi = TokenAutomaton.navigation_answers(TOKS, [EOS], separators=(",",), max_actions=2, max_digits=2)
    ok = lambda a, t: any(a.accepts(i) for i in _tokenisations(t.encode("utf-8")))     # noqa: E731
    assert ok(semi, "12,7") and not ok(semi, "12 7") and not ok(semi, "12, 7") and not ok(semi, "123,7") and ok(semi, "↑↑") and not ok(semi, "↑↑↑")
    with pytest.raises(ValueError, match="digit"):
        TokenAutomaton.navigation_answers(TOKS, [EOS], separators=(" 1",))
    with pytest.raises(ValueError, match="prefix"):
        TokenAutomaton.navigation_answers(TOKS, [EOS], actions=("↑", "↑↑"))


def test_navigation_answers_never_strands_a_row(nav):
    """from any reachable state an accepting state is reachable, over TOKENS: a constrained row can always finish"""
    succ = [sorted({nav.step(s, t) for t in nav.allowed_ids(s)}) for s in range(nav.n_states)]
    reach, todo = {nav.start}, [nav.start]
    while todo:
        for d in succ[todo.pop()]:
            if d not in reach:
                reach.add(d)
                todo.append(d)
    assert len(reach) > 30
    co = {s for s in range(nav.n_states) if nav.accepting[s]}
    grew = True
    while grew:
        grew = False
        for s in range(nav.n_states):
            if s not in co and any(d in co for d in succ[s]):
                co.add(s)
                grew = True
    assert reach <= co, sorted(reach - co)


def test_from_token_sequences_closed_set():
    seqs = [[5, 6, 7], [5, 6], [5, 9], [11]]
    a = TokenAutomaton.from_token_sequences(seqs, [2, 3], 40)
    for cand in itertools.chain.from_iterable(itertools.product([5, 6, 7, 9, 11, 2, 0], repeat=k) for k in range(0, 4)):
        body = list(cand)
        want = body in seqs or any(body[: len(s)] == s and len(body) > len(s) and all(t in (2, 3) for t in body[len(s):]) for s in seqs)
        assert a.accepts(body) == want, body
    assert a.allowed_ids(a.start).tolist() == [5, 11] and a.allowed_ids(a.run([5, 6])).tolist() == [2, 3, 7]
    assert a.run([5, 6, 2]) == a.run([11, 3, 2]) and a.allowed_ids(a.run([11, 3])).tolist() == [2, 3]
    # an empty answer is a member like any other
    e = TokenAutomaton.from_token_sequences([[], [4]], 1, 8)
    assert e.accepts([]) and e.accepts([1]) and e.accepts([4, 1]) and not e.accepts([4, 4])
    # limits: 254 nodes, 255 distinct tokens
    chain = list(range(1, 254))                                            # root + 253 nodes = 254
    assert TokenAutomaton.from_token_sequences([chain], 0, 300).accepts(chain + [0])
    with pytest.raises(ValueError, match="254 nodes"):
        TokenAutomaton.from_token_sequences([chain + [254]], 0, 300)
    with pytest.raises(ValueError, match="255"):
        TokenAutomaton.from_token_sequences([[t] for t in range(1, 257)], 0, 300)
    wide = TokenAutomaton.from_token_sequences([[t] for t in range(1, 254)], 0, 254)     # root + 253 leaves; tokens + EOS = the whole vocabulary
    assert wide.accepts([253, 0]) and len(wide.allowed_ids(wide.start)) == 253 and wide.n_states == 255 and int(wide.token_class.max()) == 253
    for bad in ([[41]], [[2]], []):
        with pytest.raises(ValueError):
            TokenAutomaton.from_token_sequences(bad, [2], 40)


def test_universal_is_the_identity():
    u = TokenAutomaton.universal(300, [EOS, 7])
    assert u.n_states == 1 and u.allowed_ids(0).size == 300 and u.step(0, EOS) == 0 and u.accepts([1, 2, 3]) and u.accepts([])
    x = np.random.default_rng(0).standard_normal((2, 300)).astype(np.float32)
    y, so = R.mask_rows(x, 300, u.token_class, u.allow, u.next, np.zeros(2, dtype=np.int32), np.array([5, EOS], dtype=np.int32))
    assert np.array_equal(x, y) and so.tolist() == [0, 0]


def test_validation_errors():
    cls = np.array([0, 0, 1, 2], dtype=np.uint8)                            # tokens 0, 1: class 0; token 2: class 1; token 3 (EOS): class 2
    allow = np.zeros((3, 8), dtype=np.uint32)
    nxt = np.zeros((3, 256), dtype=np.uint8)
    allow[0, 0], allow[1, 0], allow[2, 0] = 0b001, 0b110, 0b100             # 0: class 0 -> 1;  1 (accepting): class 1 -> 1, EOS -> 2;  2: EOS -> 2
    nxt[0, 0], nxt[1, 1], nxt[1, 2], nxt[2, 2] = 1, 1, 2, 2
    acc = [False, True, True]
    ok = TokenAutomaton(cls, allow, nxt, 0, acc, [3])
    assert ok.accepts([0, 2, 2, 3]) and not ok.accepts([0, 0])

    def broken(match, **kw):
        args = dict(token_class=cls, allow=allow.copy(), next=nxt.copy(), start=0, accepting=list(acc), eos_ids=[3])
        for k, v in kw.items():
            if callable(v):
                v(args[k])
            else:
                args[k] = v
        with pytest.raises(ValueError, match=match):
            TokenAutomaton(**args)

    broken("successor|outside", next=lambda n: n.__setitem__((0, 0), 3))                 # an allowed pair leaves the automaton
    broken("masked completely", allow=lambda a: a.__setitem__((0, 0), 0))                # a state that allows nothing
    broken("masked completely", allow=lambda a: a.__setitem__((0, 0), 1 << 9))           # ... or only a class without a token
    broken("accepting", accepting=[True, True, True])                                    # accepting without EOS
    broken("accepting", allow=lambda a: a.__setitem__((0, 0), 0b101), next=lambda n: n.__setitem__((0, 2), 2))    # EOS where it is not accepting
    broken("absorbing", next=lambda n: n.__setitem__((1, 2), 1))                         # EOS leads to a state that allows more than EOS
    broken("absorbing", next=lambda n: n.__setitem__((2, 2), 1))                         # the EOS state is left again
    broken("start", start=3)
    broken("eos", eos_ids=[4])
    broken("allow", allow=np.zeros((3, 7), dtype=np.uint32))
    broken("allow", allow=np.zeros((257, 8), dtype=np.uint32))
    broken("next", next=np.zeros((3, 255), dtype=np.uint8))
    broken("accepting", accepting=[True])
    broken("token_class", token_class=np.array([0, 300]))


def test_reference_mask_equals_transformers_prefix_constraint(nav):
    """HF's PrefixConstrainedLogitsProcessor with the function derived from allowed_ids gives exactly the restatement's processed scores"""
    torch = pytest.importorskip("torch")
    from transformers import PrefixConstrainedLogitsProcessor

    rng = np.random.default_rng(5)
    answers = [[IDX[b"12"], IDX[b", "], IDX[b"7"], EOS, EOS], [IDX["↑".encode()[:2]], IDX["↑".encode()[2:]], IDX["←→".encode()], EOS, EOS]]
    prompt = [[1, 2, 3], [4, 5, 6]]

    def fn(batch_id, input_ids):
        return nav.allowed_ids(nav.run(input_ids.tolist()[3:])).tolist()

    proc = PrefixConstrainedLogitsProcessor(fn, num_beams=1)
    state = np.full(2, nav.start, dtype=np.int32)
    for j in range(5):
        x = (rng.standard_normal((2, 300)) * 3).astype(np.float32)
        ids = torch.tensor([prompt[b] + answers[b][:j] for b in range(2)])
        want = proc(ids, torch.from_numpy(x.copy())).numpy()
        prev = None if j == 0 else np.array([answers[b][j - 1] for b in range(2)], dtype=np.int32)
        got, state = R.mask_rows(x, 300, nav.token_class, nav.allow, nav.next, state, prev)
        assert state.min() >= 0
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), j
        assert np.isfinite(got).sum() < 2 * 300
