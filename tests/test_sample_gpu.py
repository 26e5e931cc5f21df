"""GPU: ops.sample_rows (csrc/decode_sample.hip) against the float64 restatement, the acceptance check and the bound model of tests/sample_ref.py.

A token and a threshold pass by the acceptance check of sample_ref (the kernel's own thr, the float64 CDF, eps derived there); n_kept is exact;
logprob lies within its derived bound; top_k = 1 is bit-equal to the argmax kernels on the SAME buffers; two launches give the same bits; X, the
spare output row and every bitmap bit other than the drawn one keep their bits."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import decode_penalty_ref as R
import sample_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATTERN = 0xA5A5A5A5
NS = [1, 3, 4, 5, 31, 32, 33, 4097, 12288, 12400, 12547, 16384, 16389, 28675, 152064]
CONFIGS = [(1.0, 0, 1.0), (0.7, 50, 0.9), (1.0, 0, 0.9), (1.3, 1, 1.0), (1e-6, 0, 0.001)]      # (T, top_k, top_p)
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
    """x f32 [rows, n] as a device view of row stride ldx that starts off floats behind a 16-byte aligned address, in a buffer with one spare row"""
    rows, n = x.shape
    buf = torch.full(((rows + 1) * ldx + 8,), 7.0, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off: off + rows * ldx].view(rows, ldx)[:, :n]
    v.copy_(torch.from_numpy(x))
    return v, buf


class Out:
    def __init__(self, rows):
        self.rows = rows
        self.tok, self.nk = (torch.full((rows + 1,), SENT_I, dtype=torch.int32, device=DEV) for _ in range(2))
        self.lp, self.thr = (torch.full((rows + 1,), SENT_F, dtype=torch.float32, device=DEV) for _ in range(2))

    def spare_untouched(self):
        r = self.rows
        return int(self.tok[r]) == SENT_I and int(self.nk[r]) == SENT_I and float(self.lp[r]) == SENT_F and float(self.thr[r]) == SENT_F

    def host(self):
        r = self.rows
        return self.tok[:r].cpu().numpy(), self.lp[:r].cpu().numpy(), self.nk[:r].cpu().numpy(), self.thr[:r].cpu().numpy()


def _run(ops, x, u, cfg, ldx=None, off=0, words=None, p=1.0, mark=False, src=None, aux=True):
    """one launch on a fresh copy of x -> (logits view, seen tensor, tok, logprob, n_kept, thr, seen words after); asserts what must stay untouched"""
    T, k, tp = cfg
    n = x.shape[1]
    xv, buf = _logits_dev(x, ldx or n, off)
    before = buf.clone()
    seen = None if words is None else _seen_dev(words)
    rows = x.shape[0] if src is None else len(src)
    o = Out(rows)
    ud = torch.from_numpy(np.asarray(u, dtype=np.float32)).to(DEV)
    sd = None if src is None else torch.from_numpy(np.asarray(src, dtype=np.int32)).to(DEV)
    ops.sample_rows(xv, ud, o.tok[:rows], o.lp[:rows], temperature=T, top_k=k, top_p=tp, seen=seen, penalty=p, mark=mark, src=sd,
                    n_kept=o.nk[:rows] if aux else None, thr=o.thr[:rows] if aux else None)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "X was modified"
    assert o.spare_untouched(), "the spare output row was written"
    return (xv, seen) + o.host() + (None if seen is None else _u32(seen),)


def _check_row(z, cfg, u, tok, lp, nk, thr, what):
    """acceptance of one row -> (worst use of eps as a fraction, |logprob error| / bound, size of the acceptance set)"""
    T, k, tp = cfg
    n = z.shape[0]
    eps = S.eps_cdf(n)
    ok, msg, use_t = S.check_thr(z, k, tp, float(thr), eps)
    assert ok, f"{what}: {msg}"
    ok, msg, use_j = S.check_token(z, float(thr), float(u), int(tok), eps)
    assert ok, f"{what}: {msg}"
    assert int(nk) == int((z >= np.float32(thr)).sum()), f"{what}: n_kept {nk} want {int((z >= np.float32(thr)).sum())}"
    _, _, W = S.cdf_of(z, float(thr))
    want = S.logprob_of(z, int(tok), W)
    b = S.logprob_bound(z, int(tok), W, want)
    err = abs(float(lp) - want)
    assert err <= b, f"{what}: logprob {lp!r} want {want!r} err {err:.3e} bound {b:.3e}"
    return max(use_t, use_j), err / b, S.accepted_tokens(z, float(thr), float(u), eps).size


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", NS)
def test_kernel_passes_the_acceptance_check(ops, n, rows, off):
    g = np.random.default_rng(n * 16 + rows * 2 + off)
    x = (g.standard_normal((rows, n)) * 4.0).astype(np.float32)
    nw = (n + 31) // 32
    ids = g.integers(0, n, (rows + 1, min(n, 900)))
    words = np.full((rows + 1, nw + 2), PATTERN, dtype=np.uint32)          # ld_words larger than needed, one row more than the launch
    words[:, :nw] = R.seen_bitmap(ids, [ids.shape[1]] * (rows + 1), n)
    ldx = (n + 7) // 4 * 4                                                  # > n, a multiple of 4: every row has the alignment of the base
    o_ref = torch.empty(rows, dtype=torch.int32, device=DEV)
    worst_eps = worst_lp = 0.0
    for w_, p, mark in ((None, 1.0, False), (words, 1.05, True)):
        for ci, cfg in enumerate(CONFIGS):
            u = g.random(rows).astype(np.float32)
            xv, seen, tok, lp, nk, thr, after = _run(ops, x, u, cfg, ldx, off, w_, p, mark)
            assert bool(((tok >= 0) & (tok < n)).all())
            for r in range(rows):
                z = S.processed(x[r], None if w_ is None else w_[r], p, cfg[0])
                a, b, _ = _check_row(z, cfg, u[r], tok[r], lp[r], nk[r], thr[r], f"cfg {cfg} seen {w_ is not None} row {r}")
                worst_eps, worst_lp = max(worst_eps, a), max(worst_lp, b)
            if w_ is not None:
                exp = words.copy()
                for r in range(rows):
                    exp[r, tok[r] >> 5] |= np.uint32(1 << (int(tok[r]) & 31))
                assert np.array_equal(after, exp), "the seen set changed by something other than the drawn token's bit"
            # two launches: the same bits in every output
            _, _, tok2, lp2, nk2, thr2, _ = _run(ops, x, u, cfg, ldx, off, w_, p, mark)
            assert np.array_equal(tok, tok2) and np.array_equal(nk, nk2) and np.array_equal(lp.view(np.int32), lp2.view(np.int32))
            assert np.array_equal(thr.view(np.int32), thr2.view(np.int32))
            if cfg[1] == 1:
                # top_k = 1 on rows without a tie at the maximum: the argmax kernels' token on the same buffers for any u, logprob exactly 0
                if w_ is None:
                    ops.argmax_rows(xv, o_ref)
                else:
                    ops.argmax_penalty_rows(xv, _seen_dev(words), p, o_ref, mark=False)
                assert np.array_equal(tok, o_ref.cpu().numpy()), "top_k = 1 differs from the argmax kernel"
                assert bool((lp == 0.0).all()) and bool((nk == 1).all())
                _, _, tok3, lp3, _, _, _ = _run(ops, x, np.full(rows, 0.999999, dtype=np.float32), cfg, ldx, off, w_, p, mark, aux=False)
                assert np.array_equal(tok3, tok) and bool((lp3 == 0.0).all())
    print(f"n={n} rows={rows} off={off}: worst use of eps = {worst_eps:.3f}, worst |logprob - float64| / bound = {worst_lp:.3f}")


@pytest.mark.parametrize("n,rows", [(4097, 40), (152064, 12)])
def test_small_kept_sets_pin_a_single_token(ops, n, rows):
    """teeth: where at most 64 entries are kept the acceptance check must leave ONE token in >= 90 % of the rows"""
    g = np.random.default_rng(n + 1)
    x = (g.standard_normal((rows, n)) * 4.0).astype(np.float32)
    for cfg in (CONFIGS[1], CONFIGS[3], CONFIGS[4]):
        u = g.random(rows).astype(np.float32)
        _, _, tok, lp, nk, thr, _ = _run(ops, x, u, cfg)
        assert bool((nk <= 64).all())
        single, worst = 0, 0.0
        for r in range(rows):
            a, _, size = _check_row(S.processed(x[r], None, 1.0, cfg[0]), cfg, u[r], tok[r], lp[r], nk[r], thr[r], f"cfg {cfg} row {r}")
            single += int(size == 1)
            worst = max(worst, a)
        print(f"n={n} cfg={cfg}: one accepted token in {single} of {rows} rows, worst use of eps = {worst:.3f}")
        assert single >= 0.9 * rows


@pytest.mark.parametrize("n", [4097, 152064])
def test_top_k_takes_the_list_or_the_passes(ops, n):
    """behind a top-k the kernel works on a list of at most 1024 candidates when that list holds the kept set, else on passes over the row:
    k below and above the list's size, a k-th value with more than 1024 ties, and adjacent floats around the k-th value that the division
    by T merges across a 1024-key boundary (the tie in z then reaches below the list)"""
    g = np.random.default_rng(n + 7)
    rows = 4
    x = (g.standard_normal((rows, n)) * 4.0).astype(np.float32)
    x[1, g.choice(n, 1500, replace=False)] = 30.0                         # 1500 ties at the top
    bits = np.arange(-6, 6, dtype=np.int64) + 0x41F00000                  # twelve consecutive floats around 30.0 (a key boundary of 1024)
    x[2, g.choice(n, 12, replace=False)] = bits.astype(np.uint32).view(np.float32)
    x[3, : n // 2] = -np.inf
    worst = 0.0
    for cfg in ((1.0, 900, 0.9), (1.0, 1500, 1.0), (0.9, 3000, 0.95), (3.0, 8, 0.95), (7.0, 5, 1.0), (3.0, 11, 0.5), (1.0, n - 1, 1.0), (1.0, n // 2 + 9, 0.999)):
        u = g.random(rows).astype(np.float32)
        _, _, tok, lp, nk, thr, _ = _run(ops, x, u, cfg)
        for r in range(rows):
            a, _, _ = _check_row(S.processed(x[r], None, 1.0, cfg[0]), cfg, u[r], tok[r], lp[r], nk[r], thr[r], f"cfg {cfg} row {r}")
            worst = max(worst, a)
        if cfg[1] in (900, 1500) and cfg[0] == 1.0:
            assert nk[1] == 1500 and thr[1] == 30.0                        # the ties at v_k all stay, on either way
    print(f"n={n}: worst use of eps = {worst:.3f}")


def test_stratified_draws_follow_the_cdf(ops):
    """4096 output rows read ONE logits row through src with u_i = (i + 0.5) / 4096: every token's count is its float64 CDF interval's, +- 1 per edge"""
    m = 4096
    x = np.log(np.array([[0.1, 0.2, 0.3, 0.25, 0.15], [0.5, 0.1, 0.1, 0.1, 0.2]])).astype(np.float32)
    u = ((np.arange(m) + 0.5) / m).astype(np.float32)
    for row in (0, 1):
        _, _, tok, lp, nk, thr, _ = _run(ops, x, u, (1.0, 0, 1.0), src=np.full(m, row))
        z = S.processed(x[row])
        c, _, _ = S.cdf_of(z, -math.inf)
        edges = np.concatenate([[0.0], c])
        want = np.array([np.count_nonzero((u >= edges[j]) & (u < edges[j + 1])) for j in range(5)])
        got = np.bincount(tok, minlength=5)
        assert got.sum() == m and bool((np.diff(tok) >= 0).all()), "the draw is not monotone in u"
        assert np.abs(got - want).max() <= 2, (got, want)                  # an interval has two edges
        assert bool((nk == 5).all()) and bool((thr == z.min()).all())
        assert np.allclose(lp, np.log(np.diff(edges))[tok], atol=1e-6)


def test_src_maps_rows_and_refuses_entries_out_of_range(ops):
    n, g = 4097, np.random.default_rng(3)
    x = (g.standard_normal((3, n)) * 4.0).astype(np.float32)
    src = np.array([2, 0, 3, 1, -1, 2, 1 << 30])
    u = g.random(src.size).astype(np.float32)
    cfg = CONFIGS[1]
    _, _, tok, lp, nk, thr, _ = _run(ops, x, u, cfg, src=src)
    for r, s in enumerate(src):
        if 0 <= s < 3:
            _check_row(S.processed(x[s], None, 1.0, cfg[0]), cfg, u[r], tok[r], lp[r], nk[r], thr[r], f"row {r} <- {s}")
        else:
            assert tok[r] == 0 and math.isnan(lp[r]) and nk[r] == 0 and math.isnan(thr[r])


def test_ties_and_edge_rows(ops):
    n = 4099                                                               # quads + a tail of three
    inf, nan = np.inf, np.nan
    g = np.random.default_rng(11)
    base = lambda: (g.standard_normal(n) * 3).astype(np.float32)          # noqa: E731
    rows = {}
    t = base(); t[[70, 2000, 4098]] = 20.0; t[[5, 6, 7, 4097]] = 19.0
    rows["ties"] = t                                                       # three maxima, four runners-up
    t = base(); t[::3] = -inf
    rows["-inf entries"] = t
    rows["all -inf"] = np.full(n, -inf, dtype=np.float32)
    rows["all NaN"] = np.full(n, nan, dtype=np.float32)
    t = base(); t[4097] = nan; t[10] = nan; t[11] = 50.0
    rows["NaN entries"] = t
    t = base(); t[5], t[9] = 3e38, -3e38
    rows["+-3e38"] = t
    t = np.full(n, -inf, dtype=np.float32); t[[3, 4098]] = [0.0, -0.0]
    rows["two zeros"] = t
    t = base(); t[[8, 4096]] = inf
    rows["+inf"] = t
    names = list(rows)
    x = np.stack([rows[k] for k in names])
    i = names.index
    for off in (0, 1):
        for cfg in ((1.0, 0, 1.0), (1.0, 5, 1.0), (1.0, 0, 0.6), (0.7, 4, 0.9), (1.0, 2, 1.0)):
            u = g.random(len(names)).astype(np.float32)
            _, _, tok, lp, nk, thr, _ = _run(ops, x, u, cfg, ldx=n + 2 if off == 0 else n + 5, off=off)
            for r, name in enumerate(names):
                z = S.processed(x[r], None, 1.0, cfg[0])
                if name in ("all -inf", "all NaN"):
                    assert tok[r] == 0 and math.isnan(lp[r]) and nk[r] == 0 and math.isnan(thr[r]), name
                    continue
                _check_row(z, cfg, u[r], tok[r], lp[r], nk[r], thr[r], f"{name} cfg {cfg} off {off}")
                assert not np.isnan(z[tok[r]]) and z[tok[r]] > -inf, name
            T, k, tp = cfg
            if k == 5:
                assert nk[i("ties")] == 7 and thr[i("ties")] == 19.0      # 3 + 4 > 5: the ties at v_k all stay
            if k == 2:
                assert nk[i("ties")] == 3 and thr[i("ties")] == 20.0 and tok[i("ties")] in (70, 2000, 4098)
                assert abs(lp[i("ties")] + math.log(3.0)) < 1e-6
                assert nk[i("two zeros")] == 2 and thr[i("two zeros")] == 0.0 and tok[i("two zeros")] in (3, 4098)      # -0 == +0
                assert nk[i("+inf")] == 2 and tok[i("+inf")] in (8, 4096) and abs(lp[i("+inf")] + math.log(2.0)) < 1e-6
            if tp < 1.0 and k == 0:
                # top-p: the three maxima (mass ~ 0.52 with the runners-up at e^-1 each ... the value stays or goes as a whole)
                assert nk[i("ties")] in (3, 7) and thr[i("ties")] in (20.0, 19.0)
            assert tok[i("+-3e38")] == 5 and lp[i("+-3e38")] == 0.0
            assert tok[i("NaN entries")] not in (10, 4097)
            if k == 0 and tp == 1.0:
                assert nk[i("NaN entries")] == n - 2 and nk[i("-inf entries")] == n and thr[i("-inf entries")] == -inf


def test_abi_refusals(ops):
    from internnav_amd import _lib

    lib = _lib.lib()
    n, rows = 64, 2
    x = torch.randn(rows, n, device=DEV)
    seen = torch.zeros(rows, 2, dtype=torch.uint32, device=DEV)
    u = torch.full((rows,), 0.5, device=DEV)
    o = Out(rows)

    def call(X=x.data_ptr(), ldx=n, x_rows=rows, rows=rows, n=n, seen=seen.data_ptr(), ld_words=2, penalty=1.05, mark=0, T=1.0, top_k=0, top_p=1.0,
             u=u.data_ptr(), src=None, tok=o.tok.data_ptr(), lp=o.lp.data_ptr(), nk=o.nk.data_ptr(), thr=o.thr.data_ptr()):
        return lib.ina_sample_rows(X, ldx, x_rows, rows, n, seen, ld_words, C.c_float(penalty), mark, C.c_float(T), top_k, C.c_float(top_p), u, src,
                                   tok, lp, nk, thr, None)

    for kw in S.abi_refusal_cases(n, rows):                                # the list tests/test_sample_ref_cpu.py runs without a GPU
        assert call(**kw) != 0, kw
        assert b"sample_rows" in lib.ina_last_error(), kw
    torch.cuda.synchronize()
    untouched = lambda: bool((o.tok == SENT_I).all()) and bool((o.lp == SENT_F).all()) and bool((o.nk == SENT_I).all()) and bool((o.thr == SENT_F).all())      # noqa: E731
    assert untouched(), "a refused call launched something"
    assert call(rows=0) == 0
    torch.cuda.synchronize()
    assert untouched()
    assert call(seen=None, ld_words=0, penalty=float("nan"), nk=None, thr=None) == 0      # without a set the penalty arguments are not looked at
    torch.cuda.synchronize()
    assert bool(((o.tok[:rows] >= 0) & (o.tok[:rows] < n)).all()) and o.spare_untouched()
