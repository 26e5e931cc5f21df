"""Reference of the beam-search path (csrc/decode_beam.hip, QwenVLEngine.decode on a beam state, generate(num_beams=K)).

Three pieces:
  topm_rows      float64 restatement of ops.beam_topm_rows: per output row the M best entries of run_score + processed log-softmax, ordered by
                 value descending, then token id ascending, with the kernel's conventions (a NaN logit counts as -inf; a row without a number
                 has every y = -inf; a src outside the logits rows gives -inf scores and ids 0 .. M-1)
  cand_bound     allowed |cand_score - float64| of one entry, derived from the kernel's summation shape (below)
  BeamPrompt     the bookkeeping of ONE prompt (ops.beam_step) in the fp32 sentinel arithmetic of transformers' _beam_search: the kernel does the
                 same operations on the same fp32 values, so its outputs are compared exactly
  beam_search    the whole search of one prompt over a `logits_fn` - the CPU test drives a transformers model with it, the GPU tests the engine

Rules (per prompt; K = num_beams, M = max(2, 1 + n_eos) * K, step j produces answer token j, L = j + 1):
  running rows start at scores [0, -1e9, ...]; step 0 reads row 0 only. Per running row y = log_softmax(x) (float64 here, fp32 on the device), the
  repetition penalty acts on y (seen ? (y < 0 ? y * p : y / p) : y), acc = y + running score. The M best of the K * V entries by (acc descending,
  beam * V + token ascending) are the candidates. Candidate i hits when its token is an EOS id or L == max_new_tokens. The next running set is
  the K best by acc + hit * -1e9 (ties by position). Finished set (K entries, start (-1e9, not finished)): a candidate is eligible when it hit
  and i < K; its score is acc / L ** length_penalty, plus -1e9 when the heuristic flag is off, plus -1e9 when early_stopping is True and
  the set was full, plus -1e9 when it is not eligible; old entries first, then the M candidates, the K best stay (ties by position). Heuristic:
  with H = max_new_tokens when early_stopping == "never" and length_penalty > 0, else L: flag &= any_k(running[0] / H ** lp >
  (finished_k ? min(all K finished scores) : -1e9)). Done: flag off, or early_stopping is True and all K finished, or all M candidates hit.
  A done prompt is frozen.

Summation shape of beam_topm_rows (the walk is vr_walk of csrc/vocab_row.h; change both together):
  BEAM_THREADS = 1024; the row maximum is exact; sum exp(x - max): aligned rows in 16-byte vectors - thread t takes vectors t, t + 1024, ... and
  adds their terms in ascending index; rows whose base is not 16-byte aligned, and the n % 4 tail, one logit per step. A wave's 64 sums are
  added in a 6-level butterfly, the 16 wave sums sequentially. expf / logf of the device library (2 ulp).
  y = (x - max) - logf(sum); penalty one multiplication or IEEE division; acc = y + run_score: one rounding each, no contraction.
"""
from __future__ import annotations

import math
from typing import Callable, Optional, Sequence

import numpy as np

U = 2.0 ** -24            # fp32 unit roundoff
ULP = 2.0 ** -23
BEAM_THREADS = 1024
BEAM_WAVES = 16
SENT = np.float32(-1.0e9)
f32 = np.float32


def beams_to_keep(K: int, n_eos: int) -> int:
    return max(2, 1 + n_eos) * K


def processed_logprobs(x, seen=None, penalty: float = 1.0) -> np.ndarray:
    """float64 y of one logits row: log-softmax with NaN as -inf (all -inf when the row has no number), then the penalty on the seen ids"""
    x = np.asarray(x, dtype=np.float64).copy()
    x[np.isnan(x)] = -np.inf
    M = x.max()
    if not M > -np.inf:
        return np.full_like(x, -np.inf)
    with np.errstate(all="ignore"):
        y = (x - M) - math.log(np.exp(x - M).sum())
        if seen is not None:
            s = np.asarray(seen, dtype=bool)
            y = np.where(s, np.where(y < 0, y * penalty, y / penalty), y)
    return y


def topm_order(acc: np.ndarray, M: int) -> np.ndarray:
    """the first M ids by (value descending, id ascending)"""
    ids = np.arange(acc.shape[0])
    return np.lexsort((ids, -acc))[:M]


def topm_rows(x, run_score, M: int, src=None, seen=None, penalty: float = 1.0):
    """-> cand_score f64 [R, M], cand_tok int64 [R, M], acc f64 [R, n] (the whole processed rows, for the gap checks)"""
    x = np.asarray(x)
    rows_x, n = x.shape
    R = len(run_score)
    cs, ct, full = np.full((R, M), -np.inf), np.tile(np.arange(M), (R, 1)), np.full((R, n), -np.inf)
    for r in range(R):
        s = r if src is None else int(src[r])
        if not 0 <= s < rows_x:
            continue
        y = processed_logprobs(x[s], None if seen is None else seen[r], penalty)
        with np.errstate(all="ignore"):
            acc = y + float(run_score[r])
        full[r] = acc
        o = topm_order(acc, min(M, n))
        cs[r, : o.size], ct[r, : o.size] = acc[o], o
    return cs, ct, full


def cand_bound(x_row, tok, run_score: float, seen_tok=False, penalty: float = 1.0):
    """allowed |cand_score - float64| for the entries tok (an index or an array of them; seen_tok likewise) of the fp32 logits row (finite or
    -inf entries) under the summation shape above. -inf scores are compared for equality, not through this bound."""
    x = np.asarray(x_row, dtype=np.float64).copy()
    x[np.isnan(x)] = -np.inf
    n = x.shape[0]
    M = x.max()
    with np.errstate(all="ignore"):
        d = x - M
        S = np.exp(d).sum()
        fin = d[np.isfinite(d)]
        D = min(float(np.abs(fin).max()) if fin.size else 0.0, 104.0)      # terms beyond exp(-104) are 0 in fp32 and in the sum
        terms = 4 * math.ceil(n / (4 * BEAM_THREADS)) + 3                   # one thread's sequential adds (vectors + the tail)
        rel_s = (2 * ULP + U * D) + (terms + 6 + BEAM_WAVES) * U              # one term's expf and x - max, then the adds
        tok, st = np.asarray(tok), np.asarray(seen_tok, dtype=bool)
        dk = np.abs(d[tok])
        y = d[tok] - math.log(S)
        scale = np.where(st, max(penalty, 1.0 / penalty), 1.0)
        yp = np.where(st, np.where(y < 0, y * penalty, y / penalty), y)
        b = (rel_s + 2 * ULP * abs(math.log(S)) + U * dk + U * np.abs(y)) * scale + np.where(st, U * np.abs(yp), 0.0) + U * np.abs(yp + run_score)
        b = b * (1.0 + 2.0 ** -6) + n * 2.0 ** -149
    return float(b) if b.ndim == 0 else b


def step_tolerance(cand_bounds, cand_scores) -> float:
    """what one step adds to the allowed |engine running score - this reference's|: the kernel's error on the step's candidates (`cand_bound`,
    its own rounding of y + running score included) plus THIS reference's rounding of its float64 candidates to fp32 (U |acc|), which
    `BeamPrompt.step` then carries on. Summed over the steps so far it is the tolerance on a hypothesis's accumulated score."""
    b, s = np.asarray(cand_bounds, dtype=np.float64), np.asarray(cand_scores, dtype=np.float64)
    live = np.isfinite(s)
    return float(np.max(np.where(live, b + U * np.abs(np.where(live, s, 0.0)), 0.0))) if live.any() else 0.0


def finished_tolerance(acc_tol: float, score: float, length: int, length_penalty: float) -> float:
    """allowed |engine finished score - this reference's|: the accumulated tolerance through the division by length ** length_penalty (the
    same fp32 divisor on both sides), plus one rounding of the quotient on each side"""
    return acc_tol / float(f32(float(length) ** length_penalty)) + 2 * U * abs(score)


class BeamPrompt:
    """bookkeeping of one prompt: what ops.beam_step does with the K * M candidates of a step, in the same fp32 operations"""

    def __init__(self, K: int, eos: Sequence[int], max_new_tokens: int, length_penalty: float = 1.0, early_stopping=False, M: Optional[int] = None):
        assert early_stopping in (False, True, "never")
        self.K, self.eos, self.T = K, tuple(int(e) for e in eos), int(max_new_tokens)
        self.M = beams_to_keep(K, len(self.eos)) if M is None else M
        self.lp, self.early = float(length_penalty), early_stopping
        T = self.T
        self.run_score = np.full(K, SENT, dtype=f32)
        self.run_score[0] = 0.0
        self.run_tok, self.run_ts = np.zeros((K, T), dtype=np.int64), np.zeros((K, T), dtype=f32)
        self.fin_tok, self.fin_ts = np.zeros((K, T), dtype=np.int64), np.zeros((K, T), dtype=f32)
        self.fin_score, self.fin_len, self.fin_flag = np.full(K, SENT, dtype=f32), np.zeros(K, dtype=np.int64), np.zeros(K, dtype=bool)
        self.flag, self.done, self.step_idx = True, False, 0
        self.next_tok, self.parent = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
        self.margin = math.inf        # the smallest gap a decision of this prompt rested on 

    # -- decisions' margins (only bookkeeping of the reference; no influence on the result). Counted: the order of the first K candidates and
    #    the gap behind the K-th (which of them are eligible for the finished set), the running selection (its K picks and the best entry left
    #    out), the gap behind the last candidate when that candidate runs on, the finished merge (its K picks and the best entry left out) and
    #    the heuristic's comparisons. Not counted: a comparison with a side that is not finite or at a -1e9 sentinel (empty, blocked and -inf
    #    entries: their order is HF's by construction, not by a margin), and the order among candidates K .. M - 1 where it reaches no
    #    selection (a swap there changes neither set).
    def _gap(self, a, b):
        a, b = float(a), float(b)
        if math.isfinite(a) and math.isfinite(b) and a > -1e8 and b > -1e8:
            self.margin = min(self.margin, abs(a - b))

    def merge(self, cand_score, cand_tok):
        """the prompt's M candidates of the K rows' lists (each sorted): (score, beam, token) by score descending, beam * V + token ascending"""
        K, M = self.K, self.M
        rows = 1 if (self.step_idx == 0 and M <= cand_score.shape[1]) else K     # (M beyond the vocabulary: the -1e9 rows fill up, as in HF)
        ptr, out = [0] * rows, []
        for _ in range(M):
            best = -1
            for k in range(rows):
                if ptr[k] < cand_score.shape[1] and (best < 0 or cand_score[k, ptr[k]] > cand_score[best, ptr[best]]):
                    best = k
            out.append((f32(cand_score[best, ptr[best]]), best, int(cand_tok[best, ptr[best]])))
            ptr[best] += 1
        nxt = [cand_score[k, ptr[k]] for k in range(rows) if ptr[k] < cand_score.shape[1]]
        for i in range(min(K, M - 1)):                       # the order of the first K (the finished set's eligibility) and its boundary
            self._gap(out[i][0], out[i + 1][0])
        self._behind = max(nxt) if nxt else None             # the best entry that is no candidate
        return out

    def step(self, cand_score, cand_tok):
        """cand_score f32 [K, M] / cand_tok [K, M]: the rows' sorted lists (ops.beam_topm_rows) -> advances the prompt by one step"""
        if self.done:
            return
        K, M, j = self.K, self.M, self.step_idx
        cand_score = np.asarray(cand_score, dtype=f32)
        L = j + 1
        last = L == self.T
        c = self.merge(cand_score, cand_tok)
        hit = [tok in self.eos or last for _, _, tok in c]
        with np.errstate(all="ignore"):
            rs = [f32(s + (SENT if h else f32(-0.0))) for (s, _, _), h in zip(c, hit)]
            lenpow = f32(float(L) ** self.lp)
            hyppow = f32(float(self.T if (self.early == "never" and self.lp > 0.0) else L) ** self.lp)
            full_early = bool(self.fin_flag.all()) and self.early is True
            fs = []
            for i, ((s, _, _), h) in enumerate(zip(c, hit)):
                v = f32(s / lenpow)
                v = f32(v + (SENT if full_early else f32(0.0)))
                v = f32(v + (SENT if not self.flag else f32(0.0)))
                v = f32(v + (SENT if not (h and i < K) else f32(0.0)))
                fs.append(v)
        # next running set: the K best by rs, ties by position
        taken, sel = [False] * M, []
        for _ in range(K):
            best = -1
            for i in range(M):
                if not taken[i] and (best < 0 or rs[i] > rs[best]):
                    best = i
            taken[best] = True
            sel.append(best)
        rest = [rs[i] for i in range(M) if not taken[i]]
        for a, b in zip(sel[:-1], sel[1:]):
            self._gap(rs[a], rs[b])
        if rest:
            self._gap(rs[sel[-1]], max(rest))
        if max(sel) == M - 1 and self._behind is not None:   # the last candidate runs on: which entry was the last candidate mattered
            self._gap(c[-1][0], self._behind)
        old_tok, old_ts, old_score = self.run_tok.copy(), self.run_ts.copy(), self.run_score.copy()

        def hist(i):
            s, beam, tok = c[i]
            t, ts = old_tok[beam].copy(), old_ts[beam].copy()
            t[j] = tok
            with np.errstate(all="ignore"):
                ts[j] = f32(-np.inf) if s == -np.inf else f32(s - old_score[beam])
            return t, ts

        for k, i in enumerate(sel):
            self.run_tok[k], self.run_ts[k] = hist(i)
            self.run_score[k], self.next_tok[k], self.parent[k] = rs[i], c[i][2], c[i][1]
        # finished set: old entries first, then the candidates; the K best stay
        ms = list(self.fin_score) + fs
        mtaken, msel = [False] * (K + M), []
        for _ in range(K):
            best = -1
            for i in range(K + M):
                if not mtaken[i] and (best < 0 or ms[i] > ms[best]):
                    best = i
            mtaken[best] = True
            msel.append(best)
        for a, b in zip(msel[:-1], msel[1:]):
            self._gap(ms[a], ms[b])
        mrest = [ms[i] for i in range(K + M) if not mtaken[i]]
        self._gap(ms[msel[-1]], max(mrest))
        o_tok, o_ts, o_len, o_flag = self.fin_tok.copy(), self.fin_ts.copy(), self.fin_len.copy(), self.fin_flag.copy()
        for k, i in enumerate(msel):
            if i < K:
                self.fin_tok[k], self.fin_ts[k], self.fin_len[k], self.fin_flag[k] = o_tok[i], o_ts[i], o_len[i], o_flag[i]
            else:
                self.fin_tok[k], self.fin_ts[k] = hist(i - K)
                self.fin_len[k], self.fin_flag[k] = L, bool(hit[i - K] and i - K < K)
            self.fin_score[k] = ms[i]
        # heuristic flag and done
        with np.errstate(all="ignore"):
            best = f32(self.run_score[0] / hyppow)
        worst_all = self.fin_score.min()
        better = False
        for k in range(K):
            w = worst_all if self.fin_flag[k] else SENT
            self._gap(best, w)
            better = better or bool(best > w)
        self.flag = self.flag and better
        self.done = (not self.flag) or (self.early is True and bool(self.fin_flag.all())) or all(hit)
        self.step_idx += 1

    def results(self, n: int):
        """the first n finished entries: (tokens of the answer, score, length, valid)"""
        out = []
        for k in range(n):
            L = int(self.fin_len[k])
            valid = bool(self.fin_flag[k]) and float(self.fin_score[k]) > -np.inf
            out.append((self.fin_tok[k, :L].copy(), float(self.fin_score[k]), L, valid, self.fin_ts[k, :L].copy()))
        return out


def beam_search(logits_fn: Callable, prompt_ids: Sequence[int], K: int, eos: Sequence[int], max_new_tokens: int, length_penalty: float = 1.0,
                early_stopping=False, penalty: float = 1.0, M: Optional[int] = None) -> BeamPrompt:
    """the whole search of one prompt. logits_fn(answers) -> [len(answers), V]: the next-token logits behind prompt + answers[k] (a list of K
    token lists; step 0 passes ONE empty answer). The log-softmax, the penalty and the top M run in float64 (`topm_rows`); the candidates are
    rounded to fp32 and handed to `BeamPrompt.step`, which keeps the smallest gap a decision rested on (`margin`): the order of the
    first K candidates, the running and the finished selections and the heuristic's comparison."""
    bp = BeamPrompt(K, eos, max_new_tokens, length_penalty, early_stopping, M)
    prompt_ids = [int(t) for t in prompt_ids]
    while not bp.done:
        j = bp.step_idx
        answers = [[]] if j == 0 else [list(bp.run_tok[k, :j]) for k in range(K)]
        x = np.asarray(logits_fn(answers), dtype=np.float64)
        V = x.shape[1]
        if j == 0 and bp.M > V:
            answers, x = [[]] * K, np.repeat(x, K, axis=0)
        seen = np.zeros((len(answers), V), dtype=bool)
        for k, a in enumerate(answers):
            seen[k, prompt_ids + [int(t) for t in a]] = True
        Mr = min(bp.M, V)
        cs, ct, _ = topm_rows(x, bp.run_score[: len(answers)], Mr, seen=seen if penalty != 1.0 else None, penalty=penalty)
        if len(answers) < K:
            cs = np.concatenate([cs, np.full((K - len(answers), Mr), -np.inf)])
            ct = np.concatenate([ct, np.zeros((K - len(answers), Mr), dtype=ct.dtype)])
        bp.step(cs.astype(f32), ct)
    return bp
