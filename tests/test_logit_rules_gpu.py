"""GPU: ops.logit_rules_rows (csrc/decode_rules.hip) against the numpy restatement of tests/logit_rules_ref.py, which works from the key values.
Exact: the kernel stores -inf / 0.0 or adds one fp32 bias per target in HF's order, so entries no finite bias names are compared bit for bit
(NaN included, and the padding between and around the rows), biased entries as IEEE values. Every launch runs twice on equal inputs (same
bits), and the history rows, the other inputs and the tables are compared with what they must hold afterwards."""
import numpy as np
import pytest
import torch

import logit_rules_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.25
H_LENS = lambda k: [0, 1, max(k - 2, 0), max(k - 1, 0), k, 255, 256, 257, 1023]      # noqa: E731


@pytest.fixture(scope="module")
def ops(built_lib):
    from internnav_amd import ops as o

    return o


def _rows(g, n, rows, keys, lens, col, T, **kw):
    """`rows` cases that share one spec (made from row 0, whose history binds it): every other row has a history of its own over row 0's
    tokens, every second one ending in row 0's tail, so sequences and n-grams match in some rows and not in others"""
    c0 = R.random_case(g, n, keys, H=max(lens[0], col), col=col, T=T, **kw)
    pool = np.asarray(sorted({t for t in c0["history"] if 0 < t < n} | {1}))
    cases = [c0]
    for r in range(1, rows):
        H = max(lens[r % len(lens)], col)
        h = [int(t) for t in pool[g.integers(0, pool.size, H)]]
        if r % 2 and H >= 8 and len(c0["history"]) >= 8:
            h[-8:] = c0["history"][-8:]
        x = (g.standard_normal(n) * 4).astype(np.float32)
        for v in (np.nan, np.inf, -np.inf):
            x[g.random(n) < 0.03] = v
        cases.append(dict(c0, x=x, history=h, prompt_len=H - col))
    return cases


def _check(ops, cases, n, col, T, eos_first=None, stride=1):
    """launch on the rows `cases` (twice) and compare everything; stride > 1: the histories live in every stride-th row of the buffer"""
    from internnav_amd import logit_rules as LR

    rows, ldx, off, spec, eos = len(cases), n + 3, 1, cases[0]["spec"], cases[0]["eos"]
    host = LR.compile_rules(spec, n, eos, [c["prompt_len"] for c in cases], T)
    assert host is not None
    tb = host.to(DEV)
    first = host.eos_first if eos_first is None else np.asarray(eos_first, dtype=np.int32)
    cap = max(len(c["history"]) for c in cases) + 6
    hist0 = np.zeros((rows * stride + 1, cap), dtype=np.int32)
    for i in range(hist0.shape[0]):                               # poison everywhere: a cyclic repeat of a live tail, which would complete an
        h = cases[min(i // stride, rows - 1)]["history"]          # n-gram and a bad word if anything at or behind the live length were read
        t = h[-8:] if h else [1]
        hist0[i] = [t[j % len(t)] for j in range(cap)]
    want_hist = hist0.copy()
    prev = np.zeros(rows, dtype=np.int32)
    for r, c in enumerate(cases):
        h, H = c["history"], len(c["history"])
        live = H - 1 if col > 0 else H                            # what the buffer holds in front of the launch
        hist0[r * stride, :live] = want_hist[r * stride, :live] = h[:live]
        if col > 0:
            prev[r] = want_hist[r * stride, H - 1] = h[H - 1]
    x0 = np.full(rows * ldx + 12, SENTINEL, dtype=np.float32)
    want = x0.copy()
    biased = np.zeros(x0.size, dtype=bool)
    for r, c in enumerate(cases):
        s = spec
        if eos_first is not None:                                 # the row's own gate: EOS is banned while col < first[r]
            s = {k: v for k, v in spec.items() if k not in ("min_length", "min_new_tokens")}
            s["min_new_tokens"] = int(first[r])
        lo = off + r * ldx
        x0[lo:lo + n] = c["x"]
        want[lo:lo + n] = R.apply_rules(c["x"], c["history"], col, s, eos, c["prompt_len"], T)
        if not (host.forced_tok.size and col == host.forced_col):
            biased[lo + host.grp_tok[:host.n_bias]] = True
    len0 = torch.from_numpy(host.len0).to(DEV)
    outs = []
    for _ in range(2):
        buf, hist = torch.from_numpy(x0).to(DEV), torch.from_numpy(hist0).to(DEV)
        pt, ft = torch.from_numpy(prev).to(DEV), torch.from_numpy(first).to(DEV)
        v = buf[off: off + rows * ldx].view(rows, ldx)[:, :n]
        ops.logit_rules_rows(v, tb, col, hist[: rows * stride], len0, pt if col > 0 else None, ft, ld_hist=stride * cap)
        torch.cuda.synchronize()
        assert np.array_equal(pt.cpu().numpy(), prev) and np.array_equal(ft.cpu().numpy(), first) and np.array_equal(len0.cpu().numpy(), host.len0)
        outs.append((buf.cpu().numpy(), hist.cpu().numpy()))
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32)) and np.array_equal(outs[0][1], outs[1][1]), "two launches differ"
    got, got_hist = outs[0]
    assert np.array_equal(got_hist, want_hist), "history rows: prompt + appended token, nothing else touched"
    assert np.array_equal(got.view(np.uint32)[~biased], want.view(np.uint32)[~biased]), np.nonzero(got.view(np.uint32)[~biased] != want.view(np.uint32)[~biased])[0][:8]
    assert R.same(got[biased], want[biased])
    for k in ("grp_tok", "grp_base", "grp_ptr", "seq_ptr", "seq_ids", "seq_bias", "ban_tok", "begin_tok", "eos_tok", "forced_tok"):
        t = getattr(tb, k)
        assert t is None or np.array_equal(t.cpu().numpy(), getattr(host, k), equal_nan=True), k
    return got, want, x0


@pytest.mark.parametrize("step", ["col0", "col1", "forced"])
@pytest.mark.parametrize("rows", [1, 3, 64])
@pytest.mark.parametrize("n", [5, 4099, 152064])
def test_rows_columns_and_steps(ops, n, rows, step):
    g = np.random.default_rng(n * 7 + rows * 3 + len(step))
    T = 6
    col = {"col0": 0, "col1": 1, "forced": T - 1}[step]
    k = [1, 2, 3, 5][(rows + len(step)) % 4]
    keys = [key for key in R.KEYS if key != "min_length"]
    cases = _rows(g, n, rows, keys, [300] + H_LENS(k), col, T, ngram=k, adversarial=True, finite=False)
    if col > 0:
        cases[0]["history"][-1] = -1                              # prev_tok = -1: appended and compared, never an index
    first = [col + (r % 2) for r in range(rows)]                  # the per-row EOS gate on each side of this column
    got, want, x0 = _check(ops, cases, n, col, T, eos_first=first)
    assert not np.array_equal(got.view(np.uint32), x0.view(np.uint32)), "test data: no rule fired"


@pytest.mark.parametrize("k", [1, 2, 3, 5])
@pytest.mark.parametrize("col", [0, 1])
def test_history_lengths_around_the_ngram_size(ops, k, col):
    g = np.random.default_rng(100 + 10 * k + col)
    lens = H_LENS(k)
    for keys in (("no_repeat_ngram_size",), ("no_repeat_ngram_size", "bad_words_ids", "sequence_bias")):
        cases = _rows(g, 4099, len(lens) + 1, keys, [40] + lens, col, 6, ngram=k)
        _check(ops, cases, 4099, col, 6)


@pytest.mark.parametrize("G", [0, 1, 255, 256, 257])
def test_group_counts(ops, G):
    g = np.random.default_rng(500 + G)
    n, col, T = 4099, 1, 6
    cases = _rows(g, n, 3, ("sequence_bias", "bad_words_ids") if G else ("bad_words_ids",), [64, 257, 9], col, T, n_targets=max(G, 1))
    spec = cases[0]["spec"]
    tail = cases[0]["history"]
    lasts = g.permutation(np.arange(1, n))[:G]                    # G bad-word groups: distinct last tokens, lengths 2 .. 8, every third one matching
    words = [(tail[len(tail) - (2 + i % 7) + 1:] if i % 3 == 0 else [int(t) for t in g.integers(1, n, 1 + i % 7)]) + [int(t)] for i, t in enumerate(lasts)]
    spec["bad_words_ids"] = [[cases[0]["eos"][0]]] + ([[7]] if not G else []) + words
    from internnav_amd import logit_rules as LR

    host = LR.compile_rules(spec, n, cases[0]["eos"], [c["prompt_len"] for c in cases], T)
    assert host.grp_tok.size - host.n_bias == G and (host.n_bias == G or G == 0)
    _check(ops, cases, n, col, T)


def test_history_row_stride_and_refusals(ops):
    g = np.random.default_rng(9)
    cases = _rows(g, 257, 4, R.KEYS, [33, 12, 40, 8], 0, 1, ngram=2)
    _check(ops, cases, 257, 0, 1, stride=3)                       # K = 3 returned rows per prompt: the launch reads every third history
    from internnav_amd import logit_rules as LR

    tb = LR.compile_rules(dict(suppress_tokens=[3]), 64, [2], [5], 4).to(DEV)
    x, hist = torch.zeros(1, 64, device=DEV), torch.zeros(1, 16, dtype=torch.int32, device=DEV)
    l0 = torch.tensor([5], dtype=torch.int32, device=DEV)
    with pytest.raises(Exception, match="logit_rules_rows"):      # col beyond the history row: refused before any launch
        ops.logit_rules_rows(x, tb, 17, hist, l0, l0, None)
    ops.logit_rules_rows(x, tb, 12, hist, l0, l0, None)          # len0 + col > hist_cap: the row has no history, nothing is appended
    torch.cuda.synchronize()
    assert int(hist.abs().sum()) == 0 and float(x[0, 3]) == -np.inf and int(torch.isinf(x).sum()) == 1
