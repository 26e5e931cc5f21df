"""TEST INFRASTRUCTURE: float64 restatement of ops.sample_rows (internnav_amd/csrc/decode_sample.hip), its acceptance check and the error-bound
model of the kernel's arithmetic, shared by tests/test_sample_ref_cpu.py, tests/test_sample_gpu.py and tests/test_sample_decode_gpu.py. numpy.

Restatement, per row (x fp32 [n], bitmap = the row's seen set or None, p the penalty, T > 0, top_k (0 = off), top_p in (0, 1] (1 = off), u):
  1. y = logprob_ref.penalised_row(x, bitmap, p) (one IEEE fp32 operation, the kernel's bits); z = fp32(y / fp32(T)), one IEEE fp32 division -
     torch's scores / temperature. -0 counts as +0. HF's order: penalty, temperature, top-k, top-p.
  2. top-k: k = min(top_k, entries that are not NaN), v_k = the k-th largest z; keep z >= v_k (ties at v_k all stay). Pure fp32 comparisons: exact.
  3. top-p over what top-k kept, masses w_i = exp(z_i - max z) in float64, W = their sum: m(v) = sum of w_i / W over the kept entries with
     z_i <= v; the VALUE v stays iff m(v) > 1 - top_p. Entries of one value stay or go together; the maximum always stays. top_p == 1 is OFF:
     everything top-k kept stays, entries of mass 0 included. thr = the smallest kept value, n_kept = the number of entries with z >= thr.
  4. q_i = w_i / (kept mass); the token is the first kept index j in ascending id whose inclusive cumulative q exceeds u.
  5. logprob = log q_tok.
  NaN entries are never kept; -inf entries have mass 0; a row with nothing above -inf gives (0, NaN) with n_kept 0 and thr NaN; with a +inf
  maximum the +inf entries share the mass.

Acceptance (no row is ever excluded). The kernel reports its threshold, so the check follows the kernel's own kept set:
  * thr passes iff it is a value top-k kept and, with top_p < 1, m64(thr) > 1 - top_p - eps while the next kept value below it has
    m64 <= 1 - top_p + eps; with top_p == 1 iff it EQUALS v_k (the smallest entry when top-k is off);
  * a token j passes iff z_j >= thr (not NaN) and c[j-1] - eps <= u < c[j] + eps on the float64 inclusive CDF c of the set {z >= thr}.

eps, in CDF units, from the kernel's summation shape (header of decode_sample.hip, the walk of csrc/vocab_row.h; nothing in it comes from a
kernel's output). U = 2^-24 is the rounding of one fp32 operation, ULP = 2^-23, expf / logf are taken as 2-ulp functions as in logprob_ref.py. An entry's mass is
trunc(expf(fl(z - M)) * 2^44) as an integer and EVERY sum is an exact integer sum, so a sum adds no rounding at all:
  * a mass that does not vanish has z - M >= -44 ln 2, so the rounding of its argument is a relative U * D of the term with
    D = min(max |z - M|, 44 ln 2 + 1), next to the 2 ULP of expf: rel = 2 ULP + U * D per term, hence of any sum of terms;
  * the truncation loses < 2^-44 per entry (an entry whose mass vanishes loses all of its < 2^-44): n * 2^-44 absolute on a sum, in units of
    the maximum's own mass, which every kept set contains - so every normaliser is >= 1;
  * a CDF value or a mass fraction is a ratio num / den with num <= den: error <= 2 * (rel + n * 2^-44), with 2^-6 of head-room for products;
  * the thresholds floor(u * W) + 1 and ceil(top_p * W) are formed in double and move by at most one unit of 2^-44 each: 2^-43 in all.
  eps = 2 (2 ULP + U D)(1 + 2^-6) + 2 n 2^-44 + 2^-43 <= 4.3e-6 for n <= 262144; the file asserts eps <= 1e-5.
logprob = fl(fl(z_tok - M) - logf(fl(W))): U |z_tok - M| + (rel + n 2^-44 + U)(1 + 2^-6) [W as above, its conversion to fp32] + 2 ULP |log W|
+ U |logprob|.
"""
from __future__ import annotations

import math

import numpy as np

import logprob_ref as L

SAMPLE_THREADS = 1024
SAMPLE_MASS_BITS = 44
U = 2.0 ** -24
ULP = 2.0 ** -23
MASS_UNIT = 2.0 ** -SAMPLE_MASS_BITS
D_CAP = SAMPLE_MASS_BITS * math.log(2.0) + 1.0
EPS_LIMIT = 1e-5
MAX_VOCAB = 262144


def processed(x, bitmap=None, p: float = 1.0, T: float = 1.0) -> np.ndarray:
    """step 1: the fp32 row z the selection runs over"""
    y = L.penalised_row(x, bitmap, p)
    with np.errstate(all="ignore"):
        z = (y / np.float32(T)).astype(np.float32)
    z[z == 0] = np.float32(0.0)
    return z


def _masses(z: np.ndarray, M: float) -> np.ndarray:
    z64 = z.astype(np.float64)
    with np.errstate(all="ignore"):
        w = np.where(z64 == M, 1.0, np.exp(z64 - M))
    return np.where(np.isnan(z64), 0.0, w)


def topk_threshold(z: np.ndarray, top_k: int) -> float:
    """v_k of step 2 (the smallest entry that is not NaN when top-k is off or k covers them all); NaN for a row of NaN"""
    v = z[~np.isnan(z)]
    if v.size == 0:
        return math.nan
    k = min(int(top_k), v.size) if top_k > 0 else v.size
    return float(np.sort(v)[::-1][k - 1])


def value_masses(z: np.ndarray, vk: float):
    """over the set top-k kept: (distinct values ascending, m64 of each = the normalised mass of the kept entries at or below it)"""
    M = float(np.nanmax(z))
    keep = ~np.isnan(z) & (z >= np.float32(vk))
    w = _masses(z, M)
    vals, inv = np.unique(z[keep], return_inverse=True)
    per = np.zeros(vals.size)
    np.add.at(per, inv, w[keep])
    return vals, np.cumsum(per) / per.sum()


def kept_row(z: np.ndarray, top_k: int, top_p: float):
    """steps 2 and 3 -> (kept mask, thr, v_k); (all False, NaN, NaN) for a row with nothing above -inf"""
    valid = ~np.isnan(z)
    if not valid.any() or not float(np.max(z[valid])) > -math.inf:
        return np.zeros(z.shape, dtype=bool), math.nan, math.nan
    vk = topk_threshold(z, top_k)
    thr = vk
    tp = float(np.float32(top_p))
    if tp < 1.0:
        vals, m = value_masses(z, vk)
        ok = m > 1.0 - tp
        ok[-1] = True                                     # the maximum always stays
        thr = float(vals[np.argmax(ok)])                  # m rises with the value: the kept values are a suffix
    return valid & (z >= np.float32(thr)), thr, vk


def cdf_of(z: np.ndarray, thr: float):
    """float64 inclusive CDF in id order over {z >= thr} -> (c [n], kept mask, kept mass in units of the maximum's)"""
    keep = ~np.isnan(z) & (z >= np.float32(thr))
    w = np.where(keep, _masses(z, float(np.nanmax(z))), 0.0)
    W = w.sum()
    return np.cumsum(w) / W, keep, W


def draw_row(z: np.ndarray, top_k: int, top_p: float, u: float):
    """the whole restatement -> (tok, logprob float64, n_kept, thr)"""
    keep, thr, _ = kept_row(z, top_k, top_p)
    if not keep.any():
        return 0, math.nan, 0, math.nan
    c, keep, W = cdf_of(z, thr)
    hit = np.flatnonzero(keep & (c > float(u)))
    j = int(hit[0]) if hit.size else int(np.flatnonzero(keep & (np.diff(c, prepend=0.0) > 0))[-1])
    return j, logprob_of(z, j, W), int(keep.sum()), thr


def logprob_of(z: np.ndarray, j: int, W: float) -> float:
    M = float(np.nanmax(z))
    with np.errstate(all="ignore"):
        return (0.0 if float(z[j]) == M else float(z[j]) - M) - math.log(W)


def spread(z: np.ndarray) -> float:
    v = z[np.isfinite(z)].astype(np.float64)
    return min(float(v.max() - v.min()) if v.size else 0.0, D_CAP)


def eps_cdf(n: int, D: float = D_CAP) -> float:
    """allowed error of a CDF value / mass fraction of the kernel against float64 (module docstring)"""
    e = 2.0 * (2 * ULP + U * min(D, D_CAP)) * (1.0 + 2.0 ** -6) + 2.0 * n * MASS_UNIT + 2.0 * MASS_UNIT
    assert e <= EPS_LIMIT, e
    return e


assert eps_cdf(MAX_VOCAB) <= EPS_LIMIT


def logprob_bound(z: np.ndarray, j: int, W: float, lp: float) -> float:
    n = z.shape[0]
    M = float(np.nanmax(z))
    d = 0.0 if float(z[j]) == M else abs(float(z[j]) - M)
    rel = (2 * ULP + U * spread(z) + n * MASS_UNIT + U) * (1.0 + 2.0 ** -6)
    return U * d + rel + 2 * ULP * abs(math.log(W)) + U * abs(lp)


def check_thr(z: np.ndarray, top_k: int, top_p: float, thr: float, eps: float):
    """-> (ok, message, worst |m64 - (1 - top_p)| that needed the tolerance, as a fraction of eps)"""
    vk = topk_threshold(z, top_k)
    tp = float(np.float32(top_p))
    if tp >= 1.0:
        return thr == vk, f"thr {thr!r} want v_k {vk!r} (top-p off)", 0.0
    vals, m = value_masses(z, vk)
    i = np.flatnonzero(vals == np.float32(thr))
    if i.size == 0:
        return False, f"thr {thr!r} is not a value that top-k kept (v_k {vk!r})", 0.0
    i = int(i[0])
    cut = 1.0 - tp
    used = 0.0
    ok = True
    if i < vals.size - 1:                                 # (the maximum stays whatever its mass)
        ok = ok and m[i] > cut - eps
        used = max(used, (cut - m[i]) / eps)
    if i > 0:
        ok = ok and m[i - 1] <= cut + eps
        used = max(used, (m[i - 1] - cut) / eps)
    return bool(ok), f"thr {thr!r}: m64 {m[i]!r}, next below {m[i - 1] if i else None!r}, cut {cut!r}, eps {eps:.3e}", max(used, 0.0)


def accepted_tokens(z: np.ndarray, thr: float, u: float, eps: float) -> np.ndarray:
    """every token id the acceptance check lets pass for this (thr, u)"""
    c, keep, _ = cdf_of(z, thr)
    lo = np.concatenate([[0.0], c[:-1]])
    return np.flatnonzero(keep & (lo - eps <= float(u)) & (float(u) < c + eps))


def check_token(z: np.ndarray, thr: float, u: float, j: int, eps: float):
    """-> (ok, message, how far outside [c[j-1], c[j]) u lies, as a fraction of eps)"""
    n = z.shape[0]
    if not 0 <= j < n or np.isnan(z[j]) or not z[j] >= np.float32(thr):
        return False, f"token {j} is not in the kept set (thr {thr!r})", 0.0
    c, _, _ = cdf_of(z, thr)
    lo, hi = (float(c[j - 1]) if j else 0.0), float(c[j])
    used = max(lo - float(u), float(u) - hi, 0.0) / eps
    return (lo - eps <= float(u) < hi + eps), f"token {j}: u {float(u)!r} against [{lo!r}, {hi!r}) eps {eps:.3e}", used


# ---- HF's warpers on the CPU (transformers is a test dependency of the CPU test only)
def hf_kept(z_raw: np.ndarray, T: float, top_k: int, top_p: float) -> np.ndarray:
    """kept mask [rows, n] of TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper(min_tokens_to_keep=1) over fp32 rows"""
    import torch
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper

    s = torch.from_numpy(np.asarray(z_raw, dtype=np.float32)).clone()
    ids = torch.zeros(s.shape[0], 1, dtype=torch.long)
    s = TemperatureLogitsWarper(float(T))(ids, s)
    if top_k > 0:
        s = TopKLogitsWarper(int(top_k))(ids, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(float(top_p), min_tokens_to_keep=1)(ids, s)
    return (s > -math.inf).numpy()


# ---- the argument sets ina_sample_rows must refuse before any HIP call (defaults of the callers: rows rows of n logits, x_rows = rows, ldx = n,
#      a seen set of ceil(n / 32) words, penalty 1.05, mark 0, T 1, top_k 0, top_p 1, no src); keys name the argument that is replaced
def abi_refusal_cases(n: int, rows: int):
    nan, inf = float("nan"), float("inf")
    return [dict(X=None), dict(tok=None), dict(u=None), dict(lp=None), dict(rows=-1), dict(n=0), dict(n=-3), dict(ldx=n - 1), dict(x_rows=0),
            dict(x_rows=rows - 1), dict(T=0.0), dict(T=-1.0), dict(T=nan), dict(T=inf), dict(top_k=-1), dict(top_p=0.0), dict(top_p=-0.5),
            dict(top_p=1.5), dict(top_p=nan), dict(ld_words=(n + 31) // 32 - 1), dict(penalty=0.0), dict(penalty=-1.0), dict(penalty=nan),
            dict(penalty=inf), dict(mark=1, seen=None)]
