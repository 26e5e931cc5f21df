"""numpy restatement of the logits-processor rules of internnav_amd/logit_rules.py, working from the KEY VALUES (what transformers' processors
take), plus a few-line interpreter of the COMPILED tables and a generator of random cases that bind. No torch, no package import.

`apply_rules` is the table of the rules in transformers' order: sequence_bias -> [repetition penalty, applied by the selection kernels] ->
no_repeat_ngram_size -> bad_words_ids -> min_length -> min_new_tokens -> forced_eos_token_id -> suppress_tokens -> begin_suppress_tokens.
Bans are STORES of -inf (HF adds -inf for a bad word, which differs only at NaN / +inf scores)."""
import numpy as np

NEG = np.float32(-np.inf)
KEYS = ("sequence_bias", "no_repeat_ngram_size", "bad_words_ids", "min_length", "min_new_tokens", "forced_eos_token_id", "suppress_tokens",
        "begin_suppress_tokens")


def _items(sb):
    return list(sb.items()) if isinstance(sb, dict) else list({tuple(ids): b for ids, b in sb}.items())


def apply_rules(x, history, col, spec, eos_ids, prompt_len, max_new_tokens):
    """the processed scores of one row: x f32 [n] raw scores at answer column col, history = the row's prompt_len prompt tokens + col answer
    tokens (ids outside [0, n) allowed: they only ever compare), spec = a dict of KEYS"""
    x = np.array(x, dtype=np.float32, copy=True)
    n, h, H = x.size, [int(t) for t in history], len(history)
    assert H == prompt_len + col
    eos = [int(e) for e in eos_ids]
    ban = lambda t: x.__setitem__(t, NEG) if 0 <= t < n else None      # noqa: E731
    if spec.get("sequence_bias"):
        bias = {}
        for ids, b in _items(spec["sequence_bias"]):
            if len(ids) == 1:
                bias[ids[0]] = np.float32(b)
        for ids, b in _items(spec["sequence_bias"]):
            if len(ids) == 1 or len(ids) > H:
                continue
            hit = h[H - (len(ids) - 1):] == [int(t) for t in ids[:-1]]
            bias[ids[-1]] = np.float32(bias.get(ids[-1], np.float32(0.0)) + (np.float32(b) if hit else np.float32(0.0)))
        for t, b in bias.items():
            x[t] = x[t] + b
    k = spec.get("no_repeat_ngram_size") or 0
    if k > 0 and H >= k:
        prefix = h[H - (k - 1):] if k > 1 else []
        for i in range(H - k + 1):
            if h[i:i + k - 1] == prefix:
                ban(h[i + k - 1])
    for w in spec.get("bad_words_ids") or ():
        w = [int(t) for t in w]
        if (len(w) == 1 and w[0] in eos) or len(w) > max(H, 1):
            continue
        if len(w) == 1 or h[H - (len(w) - 1):] == w[:-1]:
            ban(w[-1])
    if spec.get("min_new_tokens"):
        short = col < spec["min_new_tokens"]                 # takes precedence: min_length := prompt_len + min_new_tokens
    else:
        short = H < (spec.get("min_length") or 0)
    if short:
        for e in eos:
            ban(e)
    forced = spec.get("forced_eos_token_id")
    if forced is not None and col == max_new_tokens - 1:
        x[:] = NEG
        x[[int(t) for t in (forced if isinstance(forced, (list, tuple)) else [forced])]] = np.float32(0.0)
    for t in spec.get("suppress_tokens") or ():
        ban(int(t))
    if col == 0:
        for t in spec.get("begin_suppress_tokens") or ():
            ban(int(t))
    return x


def interpret(tb, b, x, history, col):
    """the same row from the COMPILED tables of prompt b (a logit_rules.CompiledRules): what the kernel does, in numpy"""
    x = np.array(x, dtype=np.float32, copy=True)
    n, h, H = x.size, [int(t) for t in history], len(history)
    assert H == int(tb.len0[b]) + col

    def match(s):
        p = [int(t) for t in tb.seq_ids[tb.seq_ptr[s]:tb.seq_ptr[s + 1]]]
        return len(p) + 1 <= H and h[H - len(p):] == p

    for g in range(tb.grp_tok.size):
        t, ss = int(tb.grp_tok[g]), range(int(tb.grp_ptr[g]), int(tb.grp_ptr[g + 1]))
        if g < tb.n_bias:
            acc = np.float32(tb.grp_base[g])
            for s in ss:
                if match(s):
                    acc = np.float32(acc + tb.seq_bias[s])
            x[t] = x[t] + acc
    k = tb.ngram
    if k >= 1 and H >= k:
        for i in range(H - k + 1):
            if h[i:i + k - 1] == h[H - (k - 1):H] and 0 <= h[i + k - 1] < n:
                x[h[i + k - 1]] = NEG
    for g in range(tb.n_bias, tb.grp_tok.size):
        if any(match(s) for s in range(int(tb.grp_ptr[g]), int(tb.grp_ptr[g + 1]))):
            x[int(tb.grp_tok[g])] = NEG
    if col < int(tb.eos_first[b]):
        x[tb.eos_tok] = NEG
    if tb.forced_tok.size and col == tb.forced_col:
        x[:] = NEG
        x[tb.forced_tok] = np.float32(0.0)
    x[tb.ban_tok] = NEG
    if col == 0:
        x[tb.begin_tok] = NEG
    return x


def same(a, b) -> bool:
    """IEEE value equality: -0.0 equals 0.0, NaN positions must be equal"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all((a == b) | np.isnan(a)))


def random_case(g, n, keys, H=None, col=None, T=6, ngram=None, n_targets=None, max_seq=8, adversarial=False, finite=True):
    """one random case that BINDS for every key of `keys` it can bind for at (col, T): scores f32 [n], a history over a small alphabet (so that
    n-grams and sequences recur) whose tail completes an n-gram, a biased sequence and a bad word, EOS ids, and the spec. Token ids of the
    sequences are > 0 (transformers' list form of sequence_bias demands it). adversarial: a few history entries outside [0, n), placed in
    front of the tail. finite=False: NaN and +-inf among the scores."""
    keys = set(keys)
    if "forced_eos_token_id" in keys and col is None:
        col = T - 1
    if "begin_suppress_tokens" in keys and col is None:
        col = 0
    col = int(g.integers(0, T)) if col is None else int(col)
    H = int(g.integers(8, 40)) + col if H is None else int(H)
    assert H >= col and n >= 2
    alpha = np.unique(g.integers(1, n, 6))
    h = [int(t) for t in alpha[g.integers(0, alpha.size, H)]]
    tok = lambda: int(g.integers(1, n))     # noqa: E731
    eos = [int(alpha[0]), tok()]
    spec = {}
    if "no_repeat_ngram_size" in keys:
        k = int(g.integers(1, 5)) if ngram is None else int(ngram)
        spec["no_repeat_ngram_size"] = k
        if k > 1 and H >= 2 * (k - 1) + 1:                    # the tail repeats an earlier window, which then has a follower
            j = int(g.integers(0, H - 2 * (k - 1)))
            h[H - (k - 1):] = h[j:j + k - 1]
    if adversarial and H > 12:
        for i, v in zip(g.integers(0, H - 9, 4), (-1, -7, n, n + 5)):
            h[int(i)] = int(v)
    tail = lambda L: [t for t in h[H - (L - 1):]] if L > 1 else []     # noqa: E731  (the L - 1 tokens a sequence of L must end the history with)
    usable = lambda L: L <= H and all(0 < t < n for t in tail(L))      # noqa: E731
    if "sequence_bias" in keys:
        nt = int(g.integers(1, 4)) if n_targets is None else int(n_targets)
        targets = [int(t) for t in g.permutation(np.unique(np.concatenate([g.integers(1, n, 2 * nt + 4), np.arange(1, min(n, nt + 1))])))[:nt]]
        sb = []
        for i, t in enumerate(targets):
            if i == 0 or nt > 8 or g.random() < 0.5:              # (many targets: every one has an entry, so the group count is nt)
                sb.append([[t], float(np.float32(g.normal() * 3 + 0.5))])
            for _ in range(int(g.integers(0, 3)) if nt <= 8 else int(g.random() < 0.3)):      # duplicate targets: several sequences end in t
                L = int(g.integers(2, max_seq + 1))
                ids = tail(L) + [t] if g.random() < 0.6 and usable(L) else [tok() for _ in range(L - 1)] + [t]
                sb.append([ids, float(np.float32(g.normal() * 2))])
        if H + 1 <= 32:
            sb.append([[tok() for _ in range(H)] + [targets[0]], 1.25])      # longer than the history: ignored
        spec["sequence_bias"] = list({tuple(ids): [ids, b] for ids, b in sb}.values())
    if "bad_words_ids" in keys:
        bw = [[eos[0]], [int(alpha[-1])]]                     # [eos] is dropped; a single token is banned at every step
        for L in (2, 3, int(g.integers(2, max_seq + 1))):
            if usable(L):
                bw.append(tail(L) + [int(alpha[1 % alpha.size])])      # shared last token
            bw.append([tok() for _ in range(L - 1)] + [tok()])
        spec["bad_words_ids"] = bw
    if "min_new_tokens" in keys:
        spec["min_new_tokens"] = col + 1
    if "min_length" in keys:
        spec["min_length"] = H + 1 if "min_new_tokens" not in keys else int(g.integers(1, H + 3))
    if "forced_eos_token_id" in keys:
        spec["forced_eos_token_id"] = eos[0] if g.random() < 0.5 else [eos[0], tok()]
    if "suppress_tokens" in keys:
        spec["suppress_tokens"] = [tok() for _ in range(int(g.integers(1, 4)))]
    if "begin_suppress_tokens" in keys:
        spec["begin_suppress_tokens"] = [tok() for _ in range(int(g.integers(1, 4)))]
    x = (g.standard_normal(n) * 4).astype(np.float32)
    if not finite:
        for v in (np.nan, np.inf, -np.inf):
            x[g.random(n) < 0.03] = v
    return dict(x=x, history=h, col=col, prompt_len=H - col, T=T, eos=eos, spec=spec)
