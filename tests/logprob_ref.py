"""TEST INFRASTRUCTURE: float64 restatement of ops.logprob_rows (internnav_amd/csrc/decode_logprob.hip) and the error-bound model of its fp32
arithmetic, shared by tests/test_logprob_ref_cpu.py, tests/test_logprob_gpu.py and tests/test_token_logprobs_gpu.py. numpy on the CPU.

Restatement, per row (x fp32 [n], bitmap = the row's seen set or None, p the penalty, target an index or None):
    y       = decode_penalty_ref.penalised(x, bitmap, p)        one IEEE fp32 operation, the same bits as the kernel; y = x without a bitmap
    tok     = target, or decode_penalty_ref.argmax_first(y)     first maximum, NaN never selected, nothing above -inf -> 0
    logprob = y[tok] - max(y) - log(sum(exp(y - max(y))))       in float64 on the fp32 y: NaN if any y is NaN or every y is -inf
    margin  = y[tok] - max(y at the other indices, NaN skipped) in float64; no other index (n == 1) -> +inf
    a target outside [0, n) is an ignored label: logprob 0, margin 0.

Bound on |logprob_kernel - logprob_float64| (derived from the number formats and the kernel's summation shape; nothing in it comes from a kernel's
output). u = 2^-24 is the rounding of one fp32 operation, ulp = 2^-23; expf and logf are taken as 2-ulp functions (the device library documents
1 ulp for both). The constants below mirror the header comment of decode_logprob.hip; the per-thread order of the walk (LOGPROB_THREADS,
LOGPROB_VEC) is that of vr_walk in csrc/vocab_row.h.
  * one term exp(y - c): 2 ulp of expf + the rounding of its argument, |fl(y - c) - (y - c)| <= u |y - c|, i.e. a relative u * D with
    D = max |y - max y|. A term with y - c < -104 is 0 in fp32 and below 2^-149 exactly, so D is capped at 104 and n * 2^-149 is added;
  * a thread adds T terms sequentially (T u) and rescales its sum at most R times, once per 16-byte vector (or per logit on the one-by-one
    path): R * (2 ulp + u) for expf and the product; the arguments of the rescales telescope (the running maximum only rises): + u * D in all;
  * the wave scales every lane's sum once to the wave's maximum and the workgroup every wave's sum once to the row's: 2 * (2 ulp + u + u * D);
  * the 6-level butterfly and the 16 sequential adds of thread 0: (6 + 16) u.
  All of these are relative errors of S = sum exp(y - max y) >= 1, i.e. absolute errors of log S; 2^-6 of head-room covers their products.
  * logf: 2 ulp * |log S|;  fl(y[tok] - max y): u * |y[tok] - max y|;  the final subtraction: u * |logprob|.
margin is ONE fp32 subtraction of two fp32 values: bound u * |margin| (its ulp), +inf where float64's value exceeds the fp32 range.
"""
from __future__ import annotations

import math

import numpy as np

import decode_penalty_ref as R

LOGPROB_THREADS = 1024
LOGPROB_VEC = 4
LOGPROB_WAVE = 64
LOGPROB_WAVES = 16
U = 2.0 ** -24
ULP = 2.0 ** -23
EXP_UNDERFLOW = 104.0
F32_MAX = float(np.finfo(np.float32).max)


def penalised_row(x, bitmap=None, p: float = 1.0) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    return x if bitmap is None else R.penalised(x, np.asarray(bitmap, dtype=np.uint32)[..., : (x.shape[-1] + 31) // 32], p)


def logprob_row(x, bitmap=None, p: float = 1.0, target=None):
    """-> (tok, logprob float64, margin float64, y fp32 [n]) of one row"""
    y = penalised_row(x, bitmap, p)
    n = y.shape[0]
    if target is not None and not 0 <= int(target) < n:
        return int(target), 0.0, 0.0, y
    tok = int(R.argmax_first(y)) if target is None else int(target)
    y64 = y.astype(np.float64)
    with np.errstate(all="ignore"):
        if np.isnan(y64).any():
            lp = math.nan
        else:
            M = y64.max()
            lp = float(y64[tok] - M - np.log(np.exp(y64 - M).sum()))       # all -inf: -inf - -inf = NaN
        others = np.delete(y64, tok)
        others = others[~np.isnan(others)]
        other = others.max() if others.size else -math.inf
        mg = float(y64[tok] - other)
    return tok, lp, mg, y


def logprob_rows(x, bitmap=None, p: float = 1.0, target=None):
    """rows of logprob_row -> (tok int64 [rows], logprob float64 [rows], margin float64 [rows])"""
    x = np.asarray(x, dtype=np.float32)
    out = [logprob_row(x[r], None if bitmap is None else bitmap[r], p, None if target is None else target[r]) for r in range(x.shape[0])]
    return np.array([o[0] for o in out], dtype=np.int64), np.array([o[1] for o in out]), np.array([o[2] for o in out])


def summation_shape(n: int, aligned: bool):
    """(terms a thread adds sequentially, rescales of a thread's sum) at most, for a row of n logits whose base is / is not 16-byte aligned"""
    n4 = n // LOGPROB_VEC if aligned else 0
    vecs = -(-n4 // LOGPROB_THREADS)
    tail = -(-(n - LOGPROB_VEC * n4) // LOGPROB_THREADS)
    return LOGPROB_VEC * vecs + tail, vecs + tail


def logprob_bound(y, tok: int, aligned: bool) -> float:
    """allowed |logprob - float64| for the penalised fp32 row y and the index tok (finite rows; see the module docstring)"""
    y64 = np.asarray(y, dtype=np.float64)
    n = y64.shape[0]
    with np.errstate(all="ignore"):
        M = y64.max()
        d = y64 - M
        S = np.exp(d).sum()
        fin = d[np.isfinite(d)]
        D = min(float(np.abs(fin).max()) if fin.size else 0.0, EXP_UNDERFLOW)
        dk = abs(float(y64[tok] - M))
        lp = float(y64[tok] - M - math.log(S))
    T, Rs = summation_shape(n, aligned)
    exp1 = 2 * ULP + U * D
    rel = exp1 + T * U + Rs * (2 * ULP + U) + U * D + 2 * (2 * ULP + U + U * D) + (6 + LOGPROB_WAVES) * U
    rel *= 1.0 + 2.0 ** -6
    return rel + n * 2.0 ** -149 + 2 * ULP * abs(math.log(S)) + U * dk + U * abs(lp)


def margin_bound(margin: float) -> float:
    return U * abs(margin)


def check_row(got_lp: float, got_margin, y, tok: int, want_lp: float, want_margin: float, aligned: bool):
    """-> (ok, message, |logprob error|, bound): NaN must be NaN, infinities equal, the rest inside the bounds"""
    err, b = 0.0, 0.0
    if math.isnan(want_lp):
        ok = math.isnan(got_lp)
    elif math.isinf(want_lp) or abs(want_lp) > F32_MAX:          # beyond the fp32 range (a -3e38 target under a 3e38 maximum): -inf
        ok = math.isinf(got_lp) and (got_lp > 0) == (want_lp > 0)
    else:
        b = logprob_bound(y, tok, aligned)
        err = abs(float(got_lp) - want_lp)
        ok = err <= b                                  # (False for a NaN result)
    msg = f"logprob {got_lp!r} want {want_lp!r} err {err:.3e} bound {b:.3e}"
    if got_margin is not None:
        if math.isnan(want_margin):
            okm = math.isnan(got_margin)
        elif abs(want_margin) > F32_MAX:
            okm = math.isinf(got_margin) and (got_margin > 0) == (want_margin > 0)
        else:
            okm = abs(float(got_margin) - want_margin) <= margin_bound(want_margin)
        msg += f"; margin {got_margin!r} want {want_margin!r}"
        ok = ok and okm
    return ok, msg, err, b


# ---- the argument sets ina_logprob_rows must refuse before any HIP call: ONE list for tests/test_logprob_host_cpu.py (dummy pointers, no GPU)
#      and tests/test_logprob_gpu.py (device pointers, outputs must stay untouched). Defaults of the callers: rows >= 1 rows of n logits, ldx = n,
#      a seen set of ld_words = ceil(n / 32) words, penalty 1.05, mark 0, no target; keys name the argument that is replaced.
def abi_refusal_cases(n: int, ptr):
    """ptr: any non-null pointer value (used where a case needs a target)"""
    nan, inf = float("nan"), float("inf")
    return [dict(X=None), dict(tok=None), dict(lp=None), dict(rows=-1), dict(n=0), dict(n=-3), dict(ldx=n - 1), dict(ld_words=(n + 31) // 32 - 1),
            dict(n=n + 1, ldx=n + 1), dict(penalty=0.0), dict(penalty=-1.0), dict(penalty=nan), dict(penalty=inf), dict(penalty=-inf),
            dict(mark=1, target=ptr), dict(mark=1, seen=None)]


# ---- host-side restatement of the generate() surface: masking after the first EOS and the sequence sum
def mask_after_eos(values, tokens, eos_ids):
    """values [B, n] of the emitted tokens [B, n] -> (values with 0.0 behind each row's first EOS, lengths up to and including it)"""
    values, tokens = np.asarray(values, dtype=np.float32).copy(), np.asarray(tokens)
    lens = np.full(tokens.shape[0], tokens.shape[1], dtype=np.int64)
    for b in range(tokens.shape[0]):
        hit = np.flatnonzero(np.isin(tokens[b], list(eos_ids)))
        if hit.size:
            lens[b] = hit[0] + 1
        values[b, lens[b]:] = 0.0
    return values, lens


# ---- fp32 emulation of the kernel's summation shape (numpy's fp32 exp / log in place of the device library's): shows on the CPU that the bound
#      model covers the shape it describes, adversarial rows (a maximum that rises with every vector) included
def emulate_kernel_logprob(y, tok: int, aligned: bool) -> float:
    y = np.asarray(y, dtype=np.float32)
    n, T, f = y.shape[0], LOGPROB_THREADS, np.float32
    best, s = np.full(T, -np.inf, dtype=f), np.zeros(T, dtype=f)

    def step(vals):                                   # vals fp32 [T, k] (NaN-free here; pad = -inf): one vector (k = 4) or one logit per thread
        nonlocal best, s
        nb = np.maximum(best, vals.max(axis=1))
        with np.errstate(all="ignore"):
            sc = np.where(nb > best, np.exp((best - nb).astype(f)), f(1)).astype(f)
            s = (s * sc).astype(f)
            c = np.where(nb > -np.inf, nb, f(0)).astype(f)
            for q in range(vals.shape[1]):
                s = (s + np.exp((vals[:, q] - c).astype(f)).astype(f)).astype(f)
        best = nb

    n4 = n // LOGPROB_VEC if aligned else 0
    for k in range(-(-n4 // T)):
        v = np.full((T, LOGPROB_VEC), -np.inf, dtype=f)
        m = min(T, n4 - k * T)
        v[:m] = y[4 * k * T: 4 * (k * T + m)].reshape(m, LOGPROB_VEC)
        step(v)
    for j0 in range(4 * n4, n, T):
        v = np.full((T, 1), -np.inf, dtype=f)
        v[: min(T, n - j0), 0] = y[j0: j0 + T]
        step(v)

    def scaled(s_, m_, M_):
        with np.errstate(all="ignore"):
            return (s_ * np.where(m_ == M_, f(1), np.exp((m_ - M_).astype(f))).astype(f)).astype(f)

    bw, sw = best.reshape(LOGPROB_WAVES, LOGPROB_WAVE), s.reshape(LOGPROB_WAVES, LOGPROB_WAVE)
    Mw = bw.max(axis=1)
    part = scaled(sw, bw, Mw[:, None])
    o = LOGPROB_WAVE // 2
    while o:                                          # butterfly: lane i adds lane i ^ o
        part = (part + part[:, np.arange(LOGPROB_WAVE) ^ o]).astype(f)
        o //= 2
    M = Mw.max()
    S = f(0)
    for w in range(LOGPROB_WAVES):
        S = f(S + scaled(part[w, 0], Mw[w], M))
    with np.errstate(all="ignore"):
        return float(f(f(y[tok] - M) - np.log(S).astype(f)))
