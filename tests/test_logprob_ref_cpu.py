"""CPU: the float64 restatement of ops.logprob_rows (tests/logprob_ref.py) against torch.log_softmax and against transformers'
RepetitionPenaltyLogitsProcessor + the normalisation of compute_transition_scores(normalize_logits=True); the bound model against fp32
evaluations (torch's, and an emulation of the kernel's own summation shape) so that it is neither violated by honest fp32 nor vacuous."""
import math

import numpy as np
import pytest
import torch

import decode_penalty_ref as R
import logprob_ref as L

NS = [1, 3, 4, 5, 31, 32, 33, 4097, 152064]


def _row(g, n, scale=4.0):
    return (g.standard_normal(n) * scale).astype(np.float32)


def _bitmap(g, n, k=900):
    ids = g.integers(0, n, (1, min(n, k)))
    return R.seen_bitmap(ids, [ids.shape[1]], n)[0]


@pytest.mark.parametrize("n", NS)
def test_restatement_equals_torch_log_softmax_in_float64(n):
    g = np.random.default_rng(n)
    x = _row(g, n)
    bm = _bitmap(g, n)
    for bitmap, p in ((None, 1.0), (bm, 1.05), (bm, 2.0)):
        y = L.penalised_row(x, bitmap, p)
        ls = torch.log_softmax(torch.from_numpy(y).double(), -1).numpy()
        tok, lp, mg, _ = L.logprob_row(x, bitmap, p)
        assert tok == int(np.argmax(y)) and abs(lp - ls[tok]) <= 1e-12 * max(1.0, abs(ls[tok]))
        srt = np.sort(y.astype(np.float64))
        assert mg == (srt[-1] - srt[-2] if n > 1 else math.inf) and mg >= 0
        for t in {0, n // 2, n - 1}:
            tk, lp, mg, _ = L.logprob_row(x, bitmap, p, target=t)
            assert tk == t and abs(lp - ls[t]) <= 1e-12 * max(1.0, abs(ls[t]))
            other = np.delete(y.astype(np.float64), t)
            assert mg == (y[t] - other.max() if n > 1 else math.inf)
        assert L.logprob_row(x, bitmap, p, target=-100)[:3] == (-100, 0.0, 0.0) and L.logprob_row(x, bitmap, p, target=n)[:3] == (n, 0.0, 0.0)


def test_restatement_conventions():
    inf, nan = math.inf, math.nan
    tok, lp, mg, _ = L.logprob_row([1.0, 3.0, 3.0, -inf])
    assert tok == 1 and mg == 0.0 and abs(lp - (-math.log(2 + math.exp(-2)))) < 1e-15          # tie: first index, margin 0; -inf adds 0
    tok, lp, mg, _ = L.logprob_row([-inf, -inf, -inf])
    assert tok == 0 and math.isnan(lp)
    tok, lp, mg, _ = L.logprob_row([0.0, nan, 5.0])
    assert tok == 2 and math.isnan(lp) and mg == 5.0                                          # NaN: never selected, skipped by the margin
    tok, lp, mg, _ = L.logprob_row([3e38, -3e38, 0.0])
    assert tok == 0 and lp == 0.0 and mg == float(np.float32(3e38))
    tok, lp, mg, _ = L.logprob_row([0.0, 200.0, 0.0])
    assert tok == 1 and -1e-80 < lp <= 0.0


def test_restatement_equals_transformers_processed_scores():
    tr = pytest.importorskip("transformers")
    n, g = 4097, torch.Generator().manual_seed(3)
    x = torch.randn(3, n, generator=g) * 6.0
    ids = torch.randint(0, n, (3, 300), generator=g)
    for p in (1.05, 1.5):
        scores = tr.RepetitionPenaltyLogitsProcessor(penalty=p)(ids, x.clone())               # the processed scores generate() returns
        ls = torch.log_softmax(scores.double(), -1)                                          # compute_transition_scores(normalize_logits=True) ...
        tok = scores.argmax(-1)                                                              # ... gathered at the greedy token
        want = ls.gather(1, tok[:, None])[:, 0].numpy()
        bm = R.seen_bitmap(ids.numpy(), [300] * 3, n)
        gt, lp, _ = L.logprob_rows(x.numpy(), bm, p)
        assert np.array_equal(gt, tok.numpy()) and np.abs(lp - want).max() <= 1e-12
        tgt = torch.tensor([5, 4096, int(ids[2, 0])])
        _, lp, _ = L.logprob_rows(x.numpy(), bm, p, target=tgt.numpy())
        assert np.abs(lp - ls.gather(1, tgt[:, None])[:, 0].numpy()).max() <= 1e-12


def test_summation_shape_mirrors_the_kernel_header():
    import re
    from pathlib import Path

    text = (Path(__file__).resolve().parent.parent / "internnav_amd" / "csrc" / "decode_logprob.hip").read_text()
    for name in ("LOGPROB_THREADS", "LOGPROB_VEC", "LOGPROB_WAVE", "LOGPROB_WAVES"):
        assert int(re.search(rf"//\s+{name} = (\d+)", text).group(1)) == getattr(L, name)
    assert L.summation_shape(152064, True) == (152, 38) and L.summation_shape(152064, False) == (149, 149)
    assert L.summation_shape(5, True) == (5, 2) and L.summation_shape(1, True) == (1, 1) and L.summation_shape(4096, True) == (4, 1)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("n", NS)
def test_fp32_evaluations_stay_inside_the_bound_and_the_bound_is_small(n, aligned):
    g = np.random.default_rng(1000 + n)
    rows = [_row(g, n), _row(g, n, 12.0), np.sort(_row(g, n)), np.sort(_row(g, n))[::-1].copy(), np.zeros(n, dtype=np.float32)]
    rows[0][n // 2] = 60.0                                     # one dominant logit
    rows.append(np.linspace(-90.0, 10.0, n, dtype=np.float32))  # ascending: the running maximum rises with every vector (most rescales)
    worst = 0.0
    for y in rows:
        for tok in {int(np.argmax(y)), 0, n - 1}:
            _, want, _, _ = L.logprob_row(y, target=tok)
            b = L.logprob_bound(y, tok, aligned)
            t32 = float(torch.log_softmax(torch.from_numpy(y), -1)[tok])
            emu = L.emulate_kernel_logprob(y, tok, aligned)
            assert abs(t32 - want) <= b and abs(emu - want) <= b, (n, tok, t32 - want, emu - want, b)
            worst = max(worst, abs(emu - want) / b)
            # not vacuous: a few 1e-5 at the full vocabulary (plus the relative part of a far-away target), nothing like a logit tolerance
            assert b <= 1.2e-4 * max(1.0, abs(want) / 50.0), (n, tok, b, want)
    print(f"n={n} aligned={aligned}: worst |emulation - float64| / bound = {worst:.3f}")
    assert L.logprob_bound(rows[1], 0, aligned) >= L.U                    # and never zero
