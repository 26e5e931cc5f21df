"""GPU: ops.logprob_rows (csrc/decode_logprob.hip) against the float64 restatement and the bound model of tests/logprob_ref.py.

The token ids are compared bit for bit with ops.argmax_rows / ops.argmax_penalty_rows run on the SAME device buffers (that is what pins "the
switch changes no token"); logprob within the derived bound, margin within its one-ulp bound; X, the spare output row and every bitmap bit other
than the chosen one must keep their bits."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import decode_penalty_ref as R
import logprob_ref as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATTERN = 0xA5A5A5A5
NS = [1, 3, 4, 5, 31, 32, 33, 4097, 12288, 12400, 12547, 16384, 16389, 28675, 152064]
SENT_I, SENT_F = -7, 123.5


@pytest.fixture(scope="module")
def ops(built_lib):
    from internnav_amd import ops as o

    return o


def _u32(t: torch.Tensor) -> np.ndarray:
    return t.detach().view(torch.int32).cpu().numpy().view(np.uint32)


def _seen_dev(words: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(DEV).view(torch.uint32)


def _logits_dev(x: np.ndarray, ldx: int, off: int):
    """x f32 [rows, n] as a device view of row stride ldx that starts off floats behind a 16-byte aligned address, in a buffer with one spare
    row; -> (view, backing buffer)"""
    rows, n = x.shape
    buf = torch.full(((rows + 1) * ldx + 8,), 7.0, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off: off + rows * ldx].view(rows, ldx)[:, :n]
    v.copy_(torch.from_numpy(x))
    return v, buf


def _outs(rows):
    return (torch.full((rows + 1,), SENT_I, dtype=torch.int32, device=DEV), torch.full((rows + 1,), SENT_F, dtype=torch.float32, device=DEV),
            torch.full((rows + 1,), SENT_F, dtype=torch.float32, device=DEV))


def _run(ops, x, ldx, off, words=None, p=1.0, mark=False, target=None, with_margin=True):
    """launch on a fresh copy of x -> (tok, logprob, margin or None, seen words after); asserts what must stay untouched"""
    rows, n = x.shape
    xv, buf = _logits_dev(x, ldx, off)
    before = buf.clone()
    seen = None if words is None else _seen_dev(words)
    tok, lp, mg = _outs(rows)
    tgt = None if target is None else torch.from_numpy(np.asarray(target, dtype=np.int32)).to(DEV)
    ops.logprob_rows(xv, tok[:rows], lp[:rows], mg[:rows] if with_margin else None, seen=seen, penalty=p, mark=mark, target=tgt)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "X was modified"        # (bitwise: rows may hold NaN)
    assert int(tok[rows]) == SENT_I and float(lp[rows]) == SENT_F and float(mg[rows]) == SENT_F, "the spare output row was written"
    if not with_margin:
        assert bool((mg == SENT_F).all())
    return (xv, seen, tok[:rows].cpu().numpy(), lp[:rows].cpu().numpy(), mg[:rows].cpu().numpy() if with_margin else None,
            None if seen is None else _u32(seen))


def _check_values(x, words, p, toks, lp, mg, aligned, target=None, what=""):
    worst = 0.0
    for r in range(x.shape[0]):
        t, wl, wm, y = L.logprob_row(x[r], None if words is None else words[r], p, None if target is None else target[r])
        assert t == int(toks[r]), f"{what} row {r}: tok {int(toks[r])} want {t}"
        if target is not None and not 0 <= t < x.shape[1]:
            assert lp[r] == 0.0 and (mg is None or mg[r] == 0.0), f"{what} row {r}: ignored target gives {lp[r]}, {mg[r]}"
            continue
        ok, msg, err, b = L.check_row(float(lp[r]), None if mg is None else float(mg[r]), y, t, wl, wm, aligned)
        assert ok, f"{what} row {r}: {msg}"
        worst = max(worst, err / b if b else 0.0)
    return worst


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", NS)
def test_kernel_equals_restatement_and_the_argmax_kernels(ops, n, rows, off):
    g = np.random.default_rng(n * 16 + rows * 2 + off)
    x = (g.standard_normal((rows, n)) * 4.0).astype(np.float32)
    nw = (n + 31) // 32
    ids = g.integers(0, n, (rows + 1, min(n, 900)))
    words = np.full((rows + 1, nw + 2), PATTERN, dtype=np.uint32)          # ld_words larger than needed, one row more than the launch
    words[:, :nw] = R.seen_bitmap(ids, [ids.shape[1]] * (rows + 1), n)
    if n >= 33:
        # row 0: the raw maximum sits on a seen positive token, the runner-up is unseen and inside the factor -> the penalty moves the choice
        words[0, (n // 2) >> 5] &= ~np.uint32(1 << ((n // 2) & 31))
        mask = R.bitmap_mask(words[0, :nw], n)
        a, b = int(np.flatnonzero(mask)[-1]), int(np.flatnonzero(~mask)[0])
        x[0, b] = np.abs(x[0]).max() + 1.0
        x[0, a] = x[0, b] * np.float32(1.03)
    ldx = (n + 7) // 4 * 4                                                  # > n, a multiple of 4: every row has the alignment of the base
    aligned = off == 0
    o_ref = torch.empty(rows, dtype=torch.int32, device=DEV)
    worst = 0.0
    # ---- selection without a set: ids bit-equal to argmax_rows on the same buffer
    xv, _, tok, lp, mg, _ = _run(ops, x, ldx, off)
    ops.argmax_rows(xv, o_ref)
    assert np.array_equal(tok, o_ref.cpu().numpy()), "ids differ from argmax_rows"
    worst = max(worst, _check_values(x, None, 1.0, tok, lp, mg, aligned, what="plain"))
    assert bool((mg >= 0).all()) and bool((lp <= 0).all())
    # ---- selection over the penalised row, mark off and on: ids bit-equal to argmax_penalty_rows, the set changes by the chosen bit only
    for p, mark in ((1.05, False), (1.05, True), (2.0, True)):
        xv, seen, tok, lp, mg, after = _run(ops, x, ldx, off, words, p, mark)
        ops.argmax_penalty_rows(xv, _seen_dev(words), p, o_ref, mark=False)
        assert np.array_equal(tok, o_ref.cpu().numpy()), f"ids differ from argmax_penalty_rows (p={p})"
        worst = max(worst, _check_values(x, words, p, tok, lp, mg, aligned, what=f"penalty {p}"))
        exp = words.copy()
        if mark:
            for r in range(rows):
                exp[r, tok[r] >> 5] |= np.uint32(1 << (int(tok[r]) & 31))
        assert np.array_equal(after, exp), "the seen set changed by something other than the chosen token's bit"
        assert bool((mg >= 0).all())
        if n >= 33:
            assert tok[0] == b and int(np.argmax(x[0])) == a
    # ---- teacher forcing: in-range targets seen and unseen, ignored labels; with and without a set, with and without the margin pointer
    mask0 = R.bitmap_mask(words[:rows, :nw], n)
    tg = np.array([int(np.flatnonzero(mask0[r])[0]) if r % 2 == 0 and mask0[r].any() else int(g.integers(0, n)) for r in range(rows)])
    if rows == 3:
        tg[2] = -100 if off == 0 else n
    for w_, p in ((None, 1.0), (words, 1.05)):
        _, _, tok, lp, mg, after = _run(ops, x, ldx, off, w_, p, False, target=tg)
        worst = max(worst, _check_values(x, w_, p, tok, lp, mg, aligned, target=tg, what="target"))
        assert w_ is None or np.array_equal(after, words)
    _, _, tok2, lp2, _, _ = _run(ops, x, ldx, off, words, 1.05, False, target=tg, with_margin=False)
    assert np.array_equal(tok2, tok) and np.array_equal(lp2.view(np.int32), lp.view(np.int32))
    print(f"n={n} rows={rows} off={off}: worst |logprob - float64| / bound = {worst:.3f}")


def test_edge_rows(ops):
    """n = 4099 (vector body + one-by-one tail), one row per edge, aligned and not, plain and with a penalty"""
    n, g = 4099, np.random.default_rng(11)
    inf, nan = np.inf, np.nan
    nw = (n + 31) // 32
    xs, sets, names = [], [], []

    def row(name, x, seen=()):
        names.append(name)
        xs.append(np.asarray(x, dtype=np.float32))
        sets.append(list(seen))

    base = lambda: (g.standard_normal(n) * 3).astype(np.float32)          # noqa: E731
    t = base(); t[[70, 2000, 4098]] = 20.0
    row("tie", t)                                                          # three equal maxima: the first, margin 0
    t = base(); t[::3] = -inf
    row("-inf entries", t, [0, 3, 5])
    row("all -inf", np.full(n, -inf), [0, 7])
    t = base(); t[4097] = nan
    row("NaN in the tail", t, [4097])
    t = base(); t[10] = nan; t[11] = 50.0
    row("NaN in the body", t)
    t = base(); t[5], t[9] = 3e38, -3e38
    row("+-3e38", t, [9])
    t = base(); t[[6, 4096]] = 3e38; t[1::2] = -3e38
    row("+-3e38 tie", t)
    t = base(); t[1234] = 200.0
    row("dominant", t)
    t = -(np.abs(base()) + 0.5); s = [int(np.argmax(t)), 17, 4098]
    row("all negative, maximum seen", t, s)                                # multiplication: another token wins
    t = base(); t[40], t[50] = 30.0, 29.0
    row("seen positive maximum", t, [40, 50, 60])
    x = np.stack(xs)
    words = np.zeros((len(xs) + 1, nw), dtype=np.uint32)
    for r, s in enumerate(sets):
        if s:
            words[r] = R.seen_bitmap([s], [len(s)], n)[0]
    for off in (0, 1):
        ldx = n + 2 if off == 0 else n + 5                                 # n + 2 is odd: only rows 0, 4, 8 are 16-byte aligned - each row takes its own path
        for w_, p in ((None, 1.0), (words, 1.05), (words, 2.0)):
            xv, _, tok, lp, mg, _ = _run(ops, x, ldx, off, w_, p, False)
            for r in range(len(xs)):
                al = (off + r * ldx) % 4 == 0
                t_, wl, wm, y = L.logprob_row(x[r], None if w_ is None else w_[r], p)
                ok, msg, _, _ = L.check_row(float(lp[r]), float(mg[r]), y, t_, wl, wm, al)
                assert int(tok[r]) == t_ and ok, f"{names[r]} (off={off} p={p}): tok {tok[r]} want {t_}; {msg}"
            i = names.index
            assert tok[i("tie")] == 70 and mg[i("tie")] == 0.0
            assert tok[i("all -inf")] == 0 and math.isnan(lp[i("all -inf")])
            assert math.isnan(lp[i("NaN in the tail")]) and tok[i("NaN in the tail")] != 4097
            assert math.isnan(lp[i("NaN in the body")]) and tok[i("NaN in the body")] == 11
            assert tok[i("+-3e38")] == 5 and lp[i("+-3e38")] == 0.0 and np.isfinite(mg[i("+-3e38")])
            assert tok[i("+-3e38 tie")] == 6 and abs(lp[i("+-3e38 tie")] + math.log(2.0)) < 1e-6 and mg[i("+-3e38 tie")] == 0.0
            assert tok[i("dominant")] == 1234 and lp[i("dominant")] <= 0.0 and lp[i("dominant")] > -1e-30
            if w_ is not None:
                assert tok[i("all negative, maximum seen")] != sets[i("all negative, maximum seen")][0]
        # targets on the same rows: a NaN target, a -inf target, the tie's second index, ignored labels
        tg = np.array([2000, 0, 5, 4097, 11, 9, 4096, 0, 17, 50])
        tg[7] = -100
        for w_, p in ((None, 1.0), (words, 1.05)):
            _, _, tok, lp, mg, _ = _run(ops, x, ldx, off, w_, p, False, target=tg)
            for r in range(len(xs)):
                al = (off + r * ldx) % 4 == 0
                t_, wl, wm, y = L.logprob_row(x[r], None if w_ is None else w_[r], p, tg[r])
                assert int(tok[r]) == t_
                if t_ < 0:
                    assert lp[r] == 0.0 and mg[r] == 0.0
                    continue
                ok, msg, _, _ = L.check_row(float(lp[r]), float(mg[r]), y, t_, wl, wm, al)
                assert ok, f"target on {names[r]} (off={off} p={p}): {msg}"
            assert mg[0] == 0.0 and lp[1] == -inf                         # the tie's other index; a -inf target has probability 0


def test_marked_steps_chain_like_the_argmax_kernel(ops):
    """four steps back to back on one set, mark on: the same tokens and the same final set as argmax_penalty_rows"""
    n, rows, p = 4099, 4, 1.5
    g = np.random.default_rng(9)
    X = torch.from_numpy((g.standard_normal((4, rows, n)) * 3).astype(np.float32)).to(DEV)
    ids = torch.from_numpy(g.integers(0, n, (rows, 60)).astype(np.int32)).to(DEV)
    lens = torch.full((rows,), 60, dtype=torch.int32, device=DEV)
    sa = torch.zeros(rows, (n + 31) // 32, dtype=torch.uint32, device=DEV)
    ops.token_seen_set(sa, ids, lens, n)
    sb = sa.clone()
    ta, tb = torch.empty(4, rows, dtype=torch.int32, device=DEV), torch.empty(4, rows, dtype=torch.int32, device=DEV)
    lp, mg = torch.empty(4, rows, dtype=torch.float32, device=DEV), torch.empty(4, rows, dtype=torch.float32, device=DEV)
    for s in range(4):
        if s:
            X[s, torch.arange(rows), ta[s - 1].long()] = X[s].max() * 1.2   # raw maximum = the token just chosen: only a marked set moves it
        ops.argmax_penalty_rows(X[s], sa, p, ta[s], mark=True)
        ops.logprob_rows(X[s], tb[s], lp[s], mg[s], seen=sb, penalty=p, mark=True)
    assert torch.equal(ta, tb) and np.array_equal(_u32(sa), _u32(sb))
    assert all(len(set(ta[:, r].tolist())) > 1 for r in range(rows))


def test_abi_refusals(ops):
    from internnav_amd import _lib

    lib = _lib.lib()
    n, rows = 64, 2
    x = torch.randn(rows, n, device=DEV)
    seen = torch.zeros(rows, 2, dtype=torch.uint32, device=DEV)
    tgt = torch.zeros(rows, dtype=torch.int32, device=DEV)
    tok, lp, mg = _outs(rows)

    def call(X=x.data_ptr(), ldx=n, rows=rows, n=n, seen=seen.data_ptr(), ld_words=2, penalty=1.05, mark=0, target=None, tok=tok.data_ptr(),
             lp=lp.data_ptr(), mg=mg.data_ptr()):
        return lib.ina_logprob_rows(X, ldx, rows, n, seen, ld_words, C.c_float(penalty), mark, target, tok, lp, mg, None)

    nan = float("nan")
    for kw in L.abi_refusal_cases(n, tgt.data_ptr()):                      # the list tests/test_logprob_host_cpu.py runs without a GPU
        assert call(**kw) != 0, kw
        assert b"logprob_rows" in lib.ina_last_error(), kw
    torch.cuda.synchronize()
    assert bool((tok == SENT_I).all()) and bool((lp == SENT_F).all()) and bool((mg == SENT_F).all()), "a refused call launched something"
    assert call(rows=0) == 0                                               # nothing to do is not an error, and nothing is launched
    torch.cuda.synchronize()
    assert bool((tok == SENT_I).all()) and bool((lp == SENT_F).all())
    assert call(seen=None, ld_words=0, penalty=nan) == 0                   # without a set the penalty arguments are not looked at
    torch.cuda.synchronize()
    assert bool((tok[:rows] >= 0).all())
