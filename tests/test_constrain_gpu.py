"""GPU: ops.automaton_mask_rows (csrc/decode_constrain.hip) against the numpy restatement of tests/constrain_ref.py, bit for bit - the live
columns, the padding behind them, the bytes around the buffer, the state output and the tables. No tolerance anywhere: the kernel stores -inf
or nothing. Then the four selection kernels on its output against the same selection on torch.where(allowed, x, -inf)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import constrain_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.25
NS = [1, 3, 31, 32, 33, 1023, 1024, 1025, 4099]
VOCAB = 152064


@pytest.fixture(scope="module")
def ops(built_lib):
    from internnav_amd import ops as o

    return o


def _bits(classes):
    w = np.zeros(8, dtype=np.uint32)
    for c in classes:
        w[c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    return w


def _tables(g, vocab, S, C, special=None):
    """random raw tables: token_class over C classes of which the LAST holds no token when C > 2; allow rows random, or `special`
    ('first' / 'last' / 'all' bits) in state 0"""
    used = C - 1 if C > 2 else C
    cls = g.integers(0, used, vocab).astype(np.uint8)
    if special == "last":
        cls[::3] = 255
    allow = np.stack([_bits([c for c in range(C) if g.random() < 0.5] or [0]) for _ in range(S)])
    if special:
        allow[0] = {"first": _bits([0]), "last": _bits([255]), "all": np.full(8, 0xFFFFFFFF, dtype=np.uint32)}[special]
    nxt = g.integers(0, S, (S, 256)).astype(np.uint8)
    return cls, allow, nxt


def _dev_tables(cls, allow, nxt):
    return SimpleNamespace(token_class=torch.from_numpy(cls).to(DEV), allow=torch.from_numpy(allow.view(np.int32)).to(DEV), next=torch.from_numpy(nxt).to(DEV))


def _logits(g, rows, n):
    x = (g.standard_normal((rows, n)) * 4).astype(np.float32)
    for v in (np.nan, np.inf, -np.inf):                               # at random places: allowed and banned positions alike
        x[g.random((rows, n)) < 0.05] = v
    return x


def _run(ops, x, ldx, off, tb, cls, allow, nxt, state_in, prev):
    """one launch on a strided view inside a sentinel-filled buffer -> (whole buffer as uint32, state_out); asserts a second launch on the
    same inputs gives the same bits and that the tables are untouched"""
    rows, n = x.shape
    outs = []
    for _ in range(2):
        buf = torch.full((rows * ldx + 12,), SENTINEL, dtype=torch.float32, device=DEV)
        v = buf[off: off + rows * ldx].view(rows, ldx)[:, :n]
        v.copy_(torch.from_numpy(x))
        si = torch.from_numpy(state_in).to(DEV)
        so = torch.full((rows + 1,), -77, dtype=torch.int32, device=DEV)
        ops.automaton_mask_rows(v, tb, si, None if prev is None else torch.from_numpy(prev).to(DEV), so[:rows])
        torch.cuda.synchronize()
        assert int(so[rows]) == -77 and np.array_equal(si.cpu().numpy(), state_in)
        outs.append((buf.view(torch.int32).cpu().numpy().view(np.uint32), so[:rows].cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), "two launches differ"
    assert np.array_equal(tb.token_class.cpu().numpy(), cls) and np.array_equal(tb.next.cpu().numpy(), nxt)
    assert np.array_equal(tb.allow.cpu().numpy().view(np.uint32), allow)
    return outs[0]


def _want(x, ldx, off, cls, allow, nxt, state_in, prev):
    rows, n = x.shape
    buf = np.full(rows * ldx + 12, SENTINEL, dtype=np.float32)
    v = buf[off: off + rows * ldx].reshape(rows, ldx)
    v[:, :n] = x
    y, so = R.mask_rows(v, n, cls, allow, nxt, state_in, prev)
    buf[off: off + rows * ldx] = y.reshape(-1)
    return buf.view(np.uint32), so


def _rows_case(g, n, cls, allow, nxt, S):
    """state_in / prev_tok of 8 rows: two regular rows, state -1, state S, token -1, token n, a token that is not allowed (when there is
    one), and a regular row again"""
    A = np.stack([R.allowed_bits(allow, s) for s in range(S)])
    s_in = g.integers(0, S, 8).astype(np.int32)
    s_in[0] = 0
    prev = np.zeros(8, dtype=np.int32)
    for r in range(8):
        ok = np.nonzero(A[s_in[r]][cls[:n]])[0]
        prev[r] = ok[g.integers(ok.size)] if ok.size else 0
    s_in[2], s_in[3] = -1, S
    prev[4], prev[5] = -1, n
    ban = np.nonzero(~A[s_in[6]][cls[:n]])[0]
    if ban.size:
        prev[6] = ban[0]
    return s_in, prev


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("n", NS)
def test_mask_and_advance_equal_the_restatement(ops, n, pad):
    g = np.random.default_rng(1000 * n + pad)
    ldx = n + pad
    cases = [(1, 1, None), (2, 2, None), (256, 256, None), (5, 40, "first"), (5, 256, "last"), (5, 256, "all")]
    seen_untouched = seen_unallowed = 0
    for S, C, special in cases:
        cls, allow, nxt = _tables(g, max(n, 8), S, C, special)
        tb = _dev_tables(cls, allow, nxt)
        x = _logits(g, 8, n)
        s_in, prev = _rows_case(g, n, cls, allow, nxt, S)
        for off in (0, 1):                                             # the first row 16-byte aligned, and not
            for p in (prev, None):
                got, so = _run(ops, x, ldx, off, tb, cls, allow, nxt, s_in, p)
                want, so_w = _want(x, ldx, off, cls, allow, nxt, s_in, p)
                assert np.array_equal(so, so_w), (S, C, special, off, so, so_w)
                assert np.array_equal(got, want), (S, C, special, off, np.nonzero(got != want)[0][:8])
                if p is not None:
                    assert so[2] == -1 and so[3] == -1 and so[4] == -1 and so[5] == -1
                    seen_unallowed += int(so[6] == -1)
                else:
                    assert np.array_equal(so, s_in)
                # rows outside the automaton are left exactly as they were
                rows_w = want[off: off + 8 * ldx].reshape(8, ldx)[:, :n]
                for r in np.nonzero((so < 0) | (so >= S))[0]:
                    assert np.array_equal(rows_w[r], x[r].view(np.uint32))
                    seen_untouched += 1
    assert seen_untouched > 0 and (seen_unallowed > 0 or n < 3)


@pytest.mark.parametrize("rows", [1, 7])
def test_full_vocabulary(ops, rows):
    g = np.random.default_rng(rows)
    cls, allow, nxt = _tables(g, VOCAB, 256, 256)
    allow[3] = _bits([17])                                             # a navigation-sized state: one class of 256, almost everything written
    tb = _dev_tables(cls, allow, nxt)
    x = _logits(g, rows, VOCAB)
    s_in = g.integers(0, 256, rows).astype(np.int32)
    s_in[0] = 3
    for ldx in (VOCAB, VOCAB + 5):
        got, so = _run(ops, x, ldx, 0, tb, cls, allow, nxt, s_in, None)
        want, so_w = _want(x, ldx, 0, cls, allow, nxt, s_in, None)
        assert np.array_equal(so, so_w) and np.array_equal(got, want)
    prev = g.integers(0, VOCAB, rows).astype(np.int32)
    got, so = _run(ops, x, VOCAB, 0, tb, cls, allow, nxt, s_in, prev)
    want, so_w = _want(x, VOCAB, 0, cls, allow, nxt, s_in, prev)
    assert np.array_equal(so, so_w) and np.array_equal(got, want)


@pytest.mark.parametrize("n", [4099, VOCAB])
def test_selection_kernels_on_the_masked_logits(ops, n):
    """argmax_rows, argmax_penalty_rows, logprob_rows and sample_rows read the kernel's output exactly as they read torch.where(allowed, x, -inf)"""
    g = np.random.default_rng(n)
    rows, S = 3, 6
    cls, allow, nxt = _tables(g, n, S, 30)
    only = 1234
    cls[only] = 29                                                     # class 29 (unpopulated by _tables) holds exactly one token
    allow[5] = _bits([29])
    tb = _dev_tables(cls, allow, nxt)
    x = (g.standard_normal((rows, n)) * 4).astype(np.float32)
    s_in = np.array([1, 2, 5], dtype=np.int32)
    xm = torch.from_numpy(x).to(DEV)
    so = torch.empty(rows, dtype=torch.int32, device=DEV)
    ops.automaton_mask_rows(xm, tb, torch.from_numpy(s_in).to(DEV), None, so)
    A = np.stack([R.allowed_bits(allow, int(s))[cls[:n]] for s in s_in])
    ref = torch.where(torch.from_numpy(A).to(DEV), torch.from_numpy(x).to(DEV), torch.full((), float("-inf"), device=DEV))
    assert torch.equal(xm.view(torch.int32), ref.view(torch.int32))
    ldw = ((n + 31) // 32 + 3) // 4 * 4
    ids = torch.from_numpy(g.integers(0, n, (rows, 50)).astype(np.int32)).to(DEV)
    lens = torch.full((rows,), 50, dtype=torch.int32, device=DEV)
    u = torch.from_numpy(g.random(rows).astype(np.float32)).to(DEV)

    def select(v):
        out = {}
        i32 = lambda: torch.empty(rows, dtype=torch.int32, device=DEV)       # noqa: E731
        f32 = lambda: torch.empty(rows, dtype=torch.float32, device=DEV)     # noqa: E731
        out["argmax"] = ops.argmax_rows(v, i32())
        seen = ops.token_seen_set(torch.zeros(rows, ldw, dtype=torch.uint32, device=DEV), ids, lens, n)
        out["argmax_pen"] = ops.argmax_penalty_rows(v, seen, 1.3, i32(), mark=False)
        t, lp, mg = i32(), f32(), f32()
        ops.logprob_rows(v, t, lp, mg)
        out["lp_tok"], out["lp"], out["lp_margin"] = t, lp, mg
        t2, lp2, nk, thr = i32(), f32(), i32(), f32()
        ops.sample_rows(v, u, t2, lp2, temperature=0.8, top_k=40, top_p=0.9, seen=seen, penalty=1.3, mark=False, n_kept=nk, thr=thr)
        out["smp_tok"], out["smp_lp"], out["smp_kept"], out["smp_thr"] = t2, lp2, nk, thr
        return {k: t_.view(torch.int32).cpu().numpy() for k, t_ in out.items()}

    a, b = select(xm), select(ref)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for k in ("argmax", "argmax_pen", "lp_tok", "smp_tok"):              # every choice is an allowed token
        assert all(A[r, a[k][r]] for r in range(rows)), k
    # the state that allows a single token: that token, with log-probability exactly 0.0
    assert a["argmax"][2] == only and a["lp_tok"][2] == only and a["smp_tok"][2] == only
    assert a["lp"].view(np.float32)[2] == 0.0 and a["smp_lp"].view(np.float32)[2] == 0.0 and a["smp_kept"][2] == 1


def test_refusals(ops):
    g = np.random.default_rng(0)
    cls, allow, nxt = _tables(g, 64, 4, 4)
    tb = _dev_tables(cls, allow, nxt)
    x = torch.zeros(2, 64, device=DEV)
    st = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(Exception, match="overlap"):
        ops.automaton_mask_rows(x, tb, st[:2], None, st[:2])
    with pytest.raises(Exception, match="overlap"):
        ops.automaton_mask_rows(x, tb, st[:2], None, st[1:3])
    with pytest.raises(Exception, match="token_class"):
        ops.automaton_mask_rows(torch.zeros(2, 65, device=DEV), tb, st[:2], None, st[2:])
    ops.automaton_mask_rows(x[:0], tb, st[:0], None, st[:0])          # no rows: nothing is launched
