"""GPU: the three beam-search kernels (csrc/decode_beam.hip) against tests/beam_ref.py.

beam_topm_rows: ids and order exact on inputs whose float64 reference has a gap of at least 2 x the derived bound at every rank boundary (asserted),
scores within the bound, exact ties and -inf entries in id order, two launches bit-equal, X and seen unchanged. beam_step: every output exact
against BeamPrompt.step (the same fp32 arithmetic) over tables that hit every branch (asserted). beam_reorder: bit-equal to torch indexing."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import beam_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops(built_lib):
    from internnav_amd import ops as o

    return o


def _u32(t):
    return t.detach().view(torch.int32).cpu().numpy().view(np.uint32)


def _seen_words(bits: np.ndarray) -> torch.Tensor:
    rows, n = bits.shape
    ld = (n + 31) // 32
    w = np.zeros((rows, ld), dtype=np.uint32)
    for r in range(rows):
        idx = np.nonzero(bits[r])[0]
        np.bitwise_or.at(w[r], idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return torch.from_numpy(w.view(np.int32)).to(DEV).view(torch.uint32)


def _planted_row(g, n, M, gap, sigma):
    """a row whose M + 1 best logits are planted `gap` apart above the noise: a run of neighbouring ids (one thread's 16-byte vector) and ids 1024
    apart (one thread of a row that is walked logit by logit) among them - a thread that owns three of the best takes the second walk"""
    x = (g.standard_normal(n) * sigma).astype(np.float32)
    top = float(x.max())
    want = min(M + 1, n)
    ids = []
    a = int(g.integers(0, max(1, (n - 8) // 4))) * 4
    ids += [a + q for q in range(min(5, want))]
    if n > 4096:
        b = int(g.integers(0, 1024))
        ids += [i for i in (b, b + 1024, b + 2048, b + 3072) if i not in ids]
    while len(ids) < want:
        c = int(g.integers(0, n))
        if c not in ids:
            ids.append(c)
    ids = np.asarray(ids[:want])
    g.shuffle(ids)
    x[ids] = (top + gap * (want + 1 - np.arange(want)) + g.uniform(0, gap / 8, want)).astype(np.float32)
    return x


def _reference(x, run, M, src, seen_bits, penalty):
    """the float64 reference of a case, per row its rank order, seen flags and bounds, and where the condition on the INPUTS is missed: every rank
    boundary has to be an exact tie of equal inputs (decided by the id) or a gap of at least 2 x the bound (nothing of the kernel is looked at)"""
    rows_x, n = x.shape
    want_s, want_t, full = R.topm_rows(x, np.asarray(run, dtype=np.float32), M, src=src, seen=seen_bits, penalty=penalty)
    rows, missed = {}, []
    for r in range(len(run)):
        s = r if src is None else int(src[r])
        if not 0 <= s < rows_x:
            continue
        order = R.topm_order(full[r], min(M + 1, n))
        sb = np.zeros(order.size, dtype=bool) if seen_bits is None else seen_bits[r, order]
        fin = np.isfinite(full[r, order])
        b = np.where(fin, R.cand_bound(x[s], order, float(np.float32(run[r])), sb, penalty), 0.0)
        for a in range(order.size - 1):
            i, k = order[a], order[a + 1]
            va, vb = full[r, i], full[r, k]
            same = (x[s, i] == x[s, k] or (np.isnan(x[s, i]) or np.isneginf(x[s, i])) and (np.isnan(x[s, k]) or np.isneginf(x[s, k]))) and sb[a] == sb[a + 1]
            tie = (va == vb) and (same or np.isneginf(va))
            if not (tie or va - vb >= 2 * max(b[a], b[a + 1])):
                missed.append(f"row {r} rank {a}: the reference's gap {va - vb:.3e} is below 2 x bound {max(b[a], b[a + 1]):.3e}")
        rows[r] = b
    return SimpleNamespace(want_s=want_s, want_t=want_t, bounds=rows, missed=missed)


def _check_rows(ops, x, run, M, src, seen_bits, penalty, ldx=None, ref=None):
    """launch twice, compare with the float64 reference under the gap condition; -> max error / bound"""
    rows_x, n = x.shape
    R_out = rows_x if src is None else len(src)
    ldx = n if ldx is None else ldx
    buf = torch.full((rows_x * ldx + 4,), 7.0, dtype=torch.float32, device=DEV)
    xv = buf[: rows_x * ldx].view(rows_x, ldx)[:, :n]
    xv.copy_(torch.from_numpy(x))
    before_x = buf.clone()
    seen = None if seen_bits is None else _seen_words(seen_bits)
    seen0 = None if seen is None else seen.clone()
    run_d = torch.from_numpy(np.asarray(run, dtype=np.float32)).to(DEV)
    src_d = None if src is None else torch.tensor(src, dtype=torch.int32, device=DEV)
    outs = []
    for _ in range(2):
        cs = torch.full((R_out + 1, M), 123.5, dtype=torch.float32, device=DEV)
        ct = torch.full((R_out + 1, M), -7, dtype=torch.int32, device=DEV)
        ops.beam_topm_rows(xv, run_d, cs[:R_out], ct[:R_out], seen=seen, penalty=penalty, src=src_d)
        torch.cuda.synchronize()
        outs.append((cs.cpu().numpy(), ct.cpu().numpy()))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes(), "two launches differ"
    assert torch.equal(buf.view(torch.int32), before_x.view(torch.int32)), "X was written"
    assert seen is None or torch.equal(seen.view(torch.int32), seen0.view(torch.int32)), "seen was written"
    cs, ct = outs[0]
    assert bool((cs[R_out] == 123.5).all()) and bool((ct[R_out] == -7).all()), "the spare output row was written"
    ref = _reference(x, run, M, src, seen_bits, penalty) if ref is None else ref
    assert not ref.missed, ref.missed[0]                         # the condition on the inputs holds in every case
    want_s, want_t = ref.want_s, ref.want_t
    worst = 0.0
    for r in range(R_out):
        s = r if src is None else int(src[r])
        if not 0 <= s < rows_x:
            assert ct[r].tolist() == list(range(M)) and bool(np.isneginf(cs[r]).all())
            continue
        b = ref.bounds[r]
        assert ct[r].tolist() == want_t[r].tolist(), (r, ct[r], want_t[r])
        for k in range(M):
            if np.isfinite(want_s[r, k]):
                e = abs(float(cs[r, k]) - want_s[r, k])
                assert e <= b[k], f"row {r} rank {k}: score {cs[r, k]!r} want {want_s[r, k]!r} err {e:.3e} bound {b[k]:.3e}"
                worst = max(worst, e / b[k])
            else:
                assert cs[r, k] == want_s[r, k], (r, k, cs[r, k], want_s[r, k])
    return worst


@pytest.mark.parametrize("n", [97, 4096, 4099, 12288, 12400, 12547, 16384, 16389, 28675, 152064])
@pytest.mark.parametrize("rows", [1, 3, 28])
@pytest.mark.parametrize("M", [2, 6, 24, 32])
@pytest.mark.parametrize("with_src", [False, True])
@pytest.mark.parametrize("with_seen", [False, True])
def test_topm_rows_against_float64(ops, n, rows, M, with_src, with_seen):
    """inputs: the first of a fixed sequence of draws whose float64 reference meets the condition of `_reference` (the kernel's output plays no
    part in the choice); the condition is asserted again in `_check_rows`"""
    for draw in range(6):
        g = np.random.default_rng([n, rows, M, int(with_src), int(with_seen), draw])
        rows_x = max(1, rows // 4) if with_src else rows
        x = np.stack([_planted_row(g, n, M, 0.37, 3.0) for _ in range(rows_x)])
        src = None
        if with_src:
            src = [int(v) for v in g.integers(0, rows_x, rows)]
            src[-1] = rows_x + 3 if rows > 1 else src[-1]         # outside the logits rows: never read
        run = (-g.uniform(0, 20, rows)).astype(np.float32)
        run[0] = 0.0
        bits = None
        if with_seen:
            bits = g.random((rows, n)) < 0.3
            for r in range(rows):                                  # some of the best are seen, some are not
                s = r if src is None else src[r]
                if 0 <= s < rows_x:
                    top = np.argsort(-x[s])[: M + 1]
                    bits[r, top] = g.random(top.size) < 0.5
        ref = _reference(x, run, M, src, bits, 1.3 if with_seen else 1.0)
        if not ref.missed:
            break
    worst = _check_rows(ops, x, run, M, src, bits, 1.3 if with_seen else 1.0, ref=ref)
    print(f"n={n} rows={rows} M={M} src={with_src} seen={with_seen} (draw {draw}): max error / bound = {worst:.3f}")


def test_topm_rows_ties_infinities_nan_and_sentinel_scores(ops):
    n, M = 4099, 6
    g = np.random.default_rng(5)
    x = np.stack([_planted_row(g, n, M, 300.0 if r in (4, 6) else 0.5, 2.0) for r in range(8)])   # (behind a -1e9 running score one fp32 step is 64)
    x[0, [4000, 17, 18, 19, 2100, 16]] = x[0].max() + 1.0          # exact ties: id order, three of them in one thread's vector
    x[1] = -np.inf
    x[1, [77, 3, 4098]] = [1.0, 2.0, 0.5]                          # fewer than M numbers: -inf entries fill up in id order
    x[2] = -np.inf                                                 # no number at all
    x[3, 124] = x[3].max() + 2.0
    x[3, 123] = np.nan                                             # a NaN beside the maximum: counts as -inf
    run = np.array([0.0, -2.5, -1.0, 0.0, -1e9, -np.inf, -1e9, -3.0], dtype=np.float32)
    _check_rows(ops, x, run, M, None, None, 1.0)
    bits = np.zeros((8, n), dtype=bool)
    bits[0, [17, 18, 4000]] = True                                 # the tie splits by the penalty, each half stays in id order
    bits[7, np.argsort(-x[7])[:3]] = True
    _check_rows(ops, x, run, M, None, bits, 1.3)


# ------------------------------------------------------------------------------------------------------------------------------ beam_step
def _state(B, K, T, eos):
    R_ = B * K
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=DEV)      # noqa: E731
    return SimpleNamespace(K=K, eos=torch.tensor(eos, dtype=torch.int32, device=DEV) if eos else None,
                           run_score=torch.full((R_,), 5.0, device=DEV), next_tok=z(R_), parent=z(R_), hist=z(2, R_, T), ts=z(2, R_, T, dt=torch.float32),
                           fin_tok=z(R_, T), fin_ts=z(R_, T, dt=torch.float32), fin_score=torch.full((R_,), 7.0, device=DEV), fin_len=z(R_) + 9,
                           fin_flag=z(R_) + 1, heur=z(B), done=z(B) + 1)


SCENARIOS = [  # K, eos, max_new, length_penalty, early_stopping, P(eos token), quantum of the scores
    (3, [5], 5, 1.0, False, 0.25, 0.125), (2, [5, 9], 4, 0.0, True, 0.5, 0.5), (4, [1, 2, 3], 6, 2.0, "never", 0.3, 0.25),
    (8, [7], 4, 1.0, True, 0.6, 1.0), (5, [], 3, 2.0, False, 0.0, 0.125), (3, [4], 6, 0.0, "never", 0.15, 0.25), (2, [3], 7, 1.0, False, 0.45, 2.0)]


def test_beam_step_equals_the_restatement_on_every_branch(ops):
    seen_branch = set()
    for si, (K, eos, T, lp, early, p_eos, q) in enumerate(SCENARIOS):
        for rep in range(4):
            g = np.random.default_rng(100 * si + rep)
            B = 3
            M = R.beams_to_keep(K, len(eos))
            st = _state(B, K, T + 1, eos)                          # (a history row wider than max_new_tokens)
            ref = [R.BeamPrompt(K, eos, T, lp, early) for _ in range(B)]
            for bp in ref:                                        # the reference keeps rows of width max_new_tokens
                assert bp.M == M
            for j in range(T + 1):
                if j == T:
                    assert all(bp.done for bp in ref)
                    break
                cs = np.zeros((B * K, M), dtype=np.float32)
                ct = np.zeros((B * K, M), dtype=np.int32)
                for b in range(B):
                    for k in range(K):
                        base = ref[b].run_score[k] if j else np.float32(0.0)
                        dec = np.sort(np.round(np.abs(g.standard_normal(M)) * 3 / q) * q).astype(np.float32)
                        cs[b * K + k] = (base - dec).astype(np.float32)
                        tok = g.integers(10, 60, M)
                        if eos:
                            hit = g.random(M) < p_eos
                            tok[hit] = g.choice(eos, int(hit.sum()))
                        ct[b * K + k] = tok
                        if rep == 3 and k == K - 1:
                            cs[b * K + k, M // 2:] = -np.inf      # a row that ran out of allowed tokens
                was_done = [bp.done for bp in ref]
                before = [(bp.fin_flag.copy(), bp.flag) for bp in ref]
                ops.beam_step(torch.from_numpy(cs).to(DEV), torch.from_numpy(ct).to(DEV), st, j, T, lp, early)
                torch.cuda.synchronize()
                for b, bp in enumerate(ref):
                    bp.step(cs[b * K:(b + 1) * K], ct[b * K:(b + 1) * K])
                    sl = slice(b * K, (b + 1) * K)
                    got = lambda t: t[sl].cpu().numpy()              # noqa: E731
                    assert got(st.run_score).tobytes() == bp.run_score.tobytes(), (si, rep, j, b, got(st.run_score), bp.run_score)
                    assert got(st.next_tok).tolist() == bp.next_tok.tolist() and (got(st.parent) - b * K).tolist() == bp.parent.tolist()
                    assert got(st.fin_score).tobytes() == bp.fin_score.tobytes(), (si, rep, j, b, got(st.fin_score), bp.fin_score)
                    assert got(st.fin_len).tolist() == bp.fin_len.tolist() and got(st.fin_flag).astype(bool).tolist() == bp.fin_flag.tolist()
                    assert bool(int(st.heur[b])) == bp.flag and bool(int(st.done[b])) == bp.done, (si, rep, j, b)
                    for k in range(K):
                        L = int(bp.fin_len[k])
                        assert got(st.fin_tok)[k, :L].tolist() == bp.fin_tok[k, :L].tolist()
                        assert got(st.fin_ts)[k, :L].tobytes() == bp.fin_ts[k, :L].tobytes()
                    if was_done[b]:
                        seen_branch.add("frozen")
                        continue
                    h, t = st.hist[1 - (j & 1)][sl].cpu().numpy(), st.ts[1 - (j & 1)][sl].cpu().numpy()
                    assert h[:, : j + 1].tolist() == bp.run_tok[:, : j + 1].tolist(), (si, rep, j, b)
                    assert t[:, : j + 1].tobytes() == np.ascontiguousarray(bp.run_ts[:, : j + 1]).tobytes()
                    # which branches this step took (from the reference's own state)
                    new_fin = bp.fin_flag & (bp.fin_len == j + 1)
                    if j == 0:
                        seen_branch.add("step0")
                    if j + 1 == T:
                        seen_branch.add("last")
                    if new_fin.any():
                        seen_branch.add("eos_in_first_K")
                    if new_fin.sum() == K and j + 1 < T:
                        seen_branch.add("all_first_K_hit")
                    if before[b][1] and not bp.flag:
                        seen_branch.add("heuristic_off")
                    if eos and j + 1 < T and any(int(v) in eos for v in ct[b * K:(b + 1) * K, K:].reshape(-1)):
                        seen_branch.add("eos_beyond_K")
                    if np.unique(cs[b * K:(b + 1) * K, :K]).size < cs[b * K:(b + 1) * K, :K].size:
                        seen_branch.add("ties")
                    seen_branch.add(f"lp{lp:g}")
    want = {"step0", "last", "eos_in_first_K", "all_first_K_hit", "heuristic_off", "frozen", "eos_beyond_K", "ties", "lp0", "lp2", "lp1"}
    assert want <= seen_branch, sorted(want - seen_branch)


def test_beam_step_early_stopping_true_with_a_full_set_freezes(ops):
    """K = 2, early_stopping True: both of the first K hit EOS in step 0 -> the set is full, the prompt is done; later tables change nothing"""
    K, eos, T = 2, [5], 4
    M = R.beams_to_keep(K, 1)
    st = _state(2, K, T, eos)
    ref = [R.BeamPrompt(K, eos, T, 1.0, True) for _ in range(2)]
    cs = np.array([[-0.5, -1.0, -2.0, -3.0]] * 4, dtype=np.float32)
    ct = np.array([[5, 5, 11, 12], [0, 0, 0, 0], [11, 5, 12, 13], [0, 0, 0, 0]], dtype=np.int32)
    for j in range(3):
        ops.beam_step(torch.from_numpy(cs).to(DEV), torch.from_numpy(ct).to(DEV), st, j, T, 1.0, True)
        torch.cuda.synchronize()
        for b in range(2):
            ref[b].step(cs[b * K:(b + 1) * K], ct[b * K:(b + 1) * K])
            assert st.fin_score[b * K:(b + 1) * K].cpu().numpy().tobytes() == ref[b].fin_score.tobytes()
            assert bool(int(st.done[b])) == ref[b].done
        cs = (cs - 1.0).astype(np.float32)
    assert ref[0].done and ref[0].step_idx == 1 and ref[0].fin_len.tolist() == [1, 1] and ref[1].step_idx == 3


# ---------------------------------------------------------------------------------------------------------------------------- beam_reorder
@pytest.mark.parametrize("t", [0, 1, 7])
@pytest.mark.parametrize("parents", ["perm", "dup", "identity", "bad"])
def test_beam_reorder_is_torch_indexing(ops, t, parents):
    rows, T, W, layers, n = 6, 8, 64, 2, 97
    g = np.random.default_rng(t * 10 + len(parents))
    par = {"perm": g.permutation(rows), "dup": np.array([0, 0, 3, 3, 3, 5]), "identity": np.arange(rows), "bad": np.array([2, -1, 0, rows, 1, 1 << 20])}[parents]
    ok = (par >= 0) & (par < rows)
    src = [torch.from_numpy(g.integers(-30000, 30000, (rows * T, W)).astype(np.int16)).to(DEV).view(torch.bfloat16) for _ in range(layers)]
    dst = [torch.full((rows * T, W), 3.0, dtype=torch.bfloat16, device=DEV) for _ in range(layers)]
    src0 = [s.clone() for s in src]
    base = lambda ts: torch.tensor([x.data_ptr() for x in ts], dtype=torch.int64, device=DEV)      # noqa: E731
    ld = (n + 31) // 32
    seen_s = torch.from_numpy(g.integers(0, 2 ** 31, (rows, ld)).astype(np.int32)).to(DEV).view(torch.uint32)
    seen_d = torch.full((rows, ld), 0x5A5A5A5A, dtype=torch.int32, device=DEV).view(torch.uint32)
    tok = torch.tensor([3, 96, 31, 32, n + 5, 64], dtype=torch.int32, device=DEV)                 # (row 4: a token outside the vocabulary marks nothing)
    st_s = torch.arange(10, 10 + rows, dtype=torch.int32, device=DEV)
    st_d = torch.full((rows,), -5, dtype=torch.int32, device=DEV)
    pd = torch.from_numpy(par.astype(np.int32)).to(DEV)
    ops.beam_reorder(pd, base(src), base(dst), T=T, t=t, row_bytes=W * 2, seen_src=seen_s, seen_dst=seen_d, next_tok=tok, n=n, state_src=st_s, state_dst=st_d)
    torch.cuda.synchronize()
    for l in range(layers):
        assert torch.equal(src[l].view(torch.int16), src0[l].view(torch.int16)), "the source set was written"
        want = torch.full((rows, T, W), 3.0, dtype=torch.bfloat16, device=DEV)
        s3 = src[l].view(rows, T, W)
        for r in range(rows):
            if ok[r]:
                want[r, :t] = s3[int(par[r]), :t]
        assert torch.equal(dst[l].view(torch.int16), want.view(rows * T, W).view(torch.int16))
    ws, wd, tk = _u32(seen_s), _u32(seen_d), tok.cpu().numpy()
    for r in range(rows):
        if not ok[r]:
            assert bool((wd[r] == 0x5A5A5A5A).all()) and int(st_d[r]) == -5
            continue
        w = ws[int(par[r])].copy()
        if 0 <= tk[r] < n:
            w[tk[r] >> 5] |= np.uint32(1) << np.uint32(tk[r] & 31)
        assert wd[r].tolist() == w.tolist() and int(st_d[r]) == 10 + int(par[r])


def test_entry_refusals_before_any_launch(ops):
    x = torch.zeros(2, 16, device=DEV)
    run = torch.zeros(2, device=DEV)
    for M in (1, 33, 17):
        with pytest.raises(RuntimeError):
            ops.beam_topm_rows(x, run, torch.zeros(2, M, device=DEV), torch.zeros(2, M, dtype=torch.int32, device=DEV))
    st = _state(1, 2, 4, [1])
    cs, ct = torch.zeros(2, 4, device=DEV), torch.zeros(2, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        ops.beam_step(cs, ct, st, 4, 4)                            # step beyond max_new_tokens
    with pytest.raises(RuntimeError):
        ops.beam_step(cs, ct, st, 0, 5)                            # max_new_tokens beyond the history rows
    with pytest.raises(RuntimeError):
        ops.beam_step(cs, ct, st, 0, 4, float("inf"))
