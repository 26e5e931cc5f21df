"""numpy restatement of ops.automaton_mask_rows (internnav_amd/csrc/decode_constrain.hip): the advance and the mask of one launch, and the
small synthetic byte vocabulary the constraint tests share."""
import numpy as np


def allowed_bits(allow, s):
    """bool [256]: the class set of state s out of allow uint32 [S, 8]"""
    c = np.arange(256)
    return ((np.asarray(allow, dtype=np.uint32)[s, c >> 5] >> (c & 31).astype(np.uint32)) & 1).astype(bool)


def advance(n, token_class, allow, nxt, state_in, prev_tok):
    """state_out int32 [rows]; prev_tok None = no advance. Nothing is indexed before it is range-checked."""
    S = allow.shape[0]
    out = np.empty(len(state_in), dtype=np.int32)
    for r, s0 in enumerate(state_in):
        if prev_tok is None:
            out[r] = s0
            continue
        t, s = int(prev_tok[r]), -1
        if 0 <= s0 < S and 0 <= t < n:
            c = int(token_class[t])
            if allowed_bits(allow, int(s0))[c]:
                s = int(nxt[s0, c])
        out[r] = s
    return out


def mask_rows(X, n, token_class, allow, nxt, state_in, prev_tok):
    """-> (X' , state_out): X f32 [rows, ldx] (a copy is returned), the first n columns live. Banned entries become -inf, everything else - allowed
    entries (NaN included), rows whose state is outside [0, S), columns >= n - keeps its bits."""
    X = np.array(X, dtype=np.float32, copy=True)
    S = allow.shape[0]
    so = advance(n, token_class, allow, nxt, state_in, prev_tok)
    for r, s in enumerate(so):
        if 0 <= s < S:
            ban = ~allowed_bits(allow, int(s))[np.asarray(token_class[:n], dtype=np.int64)]
            X[r, :n][ban] = -np.inf
    return X, so


def byte_vocab(size=300):
    """a synthetic byte-level vocabulary of `size` tokens: single digits, two-digit tokens, ' 2'-style tokens, separators, whole and split UTF-8 arrows,
    STOP split as ST | OP (and whole), filler words; the rest are tokens without bytes (special tokens). -> (token_bytes, eos_id)"""
    toks = [bytes([48 + d]) for d in range(10)]                                 # 0 .. 9
    toks += [f"{d:02d}".encode() for d in (10, 12, 25, 37, 40, 64, 99, 0, 7)]    # two digits ('00', '07' included)
    toks += [f" {d}".encode() for d in range(10)]                               # ' 2'
    toks += [b" ", b",", b", ", b",1", b" 12"]
    arrows = [a.encode("utf-8") for a in "↑←→↓"]
    toks += arrows                                                              # whole arrows
    toks += [arrows[0][:2], arrows[0][:1]] + [a[2:] for a in arrows] + [a[1:] for a in arrows[:2]]     # E2 86 | E2 | last byte | last two
    toks += ["↑↑".encode(), "←→".encode(), "↓".encode() + b"1"]
    toks += [b"ST", b"OP", b"STOP", b"S", b"TOP", b"STO", b"P", b"STOP "]
    toks += [b"the", b" go", b"a", b"\n", b".", b"x1", b"1x"]
    assert len(set(toks)) == len(toks) and len(toks) < size - 1
    toks += [b""] * (size - len(toks))
    return toks, size - 1
