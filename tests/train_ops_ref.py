"""TEST INFRASTRUCTURE: float64 restatements of the SFT-step kernels (internnav_amd/csrc/train.hip), written from the formula comments of the
kernels and the docstrings of `internnav_amd.train_ops`, independent of tests/_cpu_kernels.py.

Every function takes the arguments of the train_ops wrapper of the same name, upcasts the (already bf16- / fp32-rounded) inputs to float64 and
returns `(ref, scale)` (tuples of them for ops with two results): `ref` is the exact result for those inputs, `scale` the float64 sum of the
|terms| that enter each output element - every fp32 rounding of a correct kernel is relative to a partial sum no larger than that, so
    |kernel - ref| <= k * 2^-24 * (sqrt(n) + 4) * scale          (n: reduction length, 1 for element-wise ops)
is the bound the tests build from it (`fp32_bound`). Derivatives are closed forms written by hand; tests/test_train_ops_ref_cpu.py checks them
against torch.autograd in float64. `accumulate=True` reads the prior content of `out`, so call the reference BEFORE the kernel.

Conditioning that is a property of the fp32 ARGUMENT of a function, not of the kernel, is part of `scale`:
  * exp(-x) evaluated from an fp32 product x * log2(e) carries a relative error ~ |x| * 2^-24: terms made of an exponential are weighted (1 + |arg|);
  * LayerNorm's d = x - mean carries an absolute error ~ 2^-24 * |x|max, i.e. 2^-24 * cond in xhat with cond = |x|max * rstd: the xhat-dependent
    terms and rstd itself (through the variance) are weighted with cond (measured on the CPU, fp32 torch against float64: without the term the
    model is missed by 48x at C = 8 with mean = 64 x spread, with it the worst ratio is below 2).
"""
from __future__ import annotations

import math

import numpy as np
import torch

U = 2.0 ** -24          # fp32 unit roundoff
BF = 2.0 ** -8          # bf16 relative spacing
TINY = 2.0 ** -126      # smallest normal fp32: results below it may be flushed
F64 = torch.float64
K0, K1 = 0.7978845608028654, 0.044715
ACTS = ("gelu_erf", "gelu_tanh", "relu", "silu", "tanh")


def f32(v: float) -> float:
    """a Python float as the kernel receives it (c_float argument)."""
    return float(np.float32(v))


def fp32_bound(scale, n=1, k=16.0):
    return k * U * (math.sqrt(n) + 4.0) * scale + TINY


def out_bound(ref, bound, dtype):
    """bound of a stored result: one more rounding to 8 mantissa bits for bf16 outputs."""
    return bound + (BF * ref.abs() if dtype == torch.bfloat16 else 0.0)


def _d(t):
    return None if t is None else t.detach().to(F64)


def _prior(out, accumulate, like):
    return _d(out) if (accumulate and out is not None) else torch.zeros_like(like)


# ---------------------------------------------------------------------------------------------------------------- element-wise
def _scale_fn(s, s_f):
    if s_f == "one_plus":
        return 1.0 + s, 1.0 + s.abs()
    if s_f == "tanh":
        return torch.tanh(s), torch.tanh(s).abs() * (1.0 + s.abs())
    return s, s.abs()


def affine(x, scale=None, s_div=1, s_f=None, base=None, tab=None, out=None, out_dtype=None, accumulate=False):
    """out (+)= x * f(scale[r // s_div]) + base + tab[r % len(tab)]"""
    y = _d(x)
    mag = y.abs()
    rows, C = y.shape
    r = torch.arange(rows, device=y.device)
    if scale is not None:
        f, fm = _scale_fn(_d(scale)[r // s_div], s_f)
        y, mag = y * f, mag * fm
    if base is not None:
        y, mag = y + _d(base), mag + _d(base).abs()
    if tab is not None:
        t = _d(tab).reshape(-1, C)[r % (tab.numel() // C)]
        y, mag = y + t, mag + t.abs()
    p = _prior(out, accumulate, y)
    return y + p, mag + p.abs()


def act_value(x, act):
    """(act(x), scale) in float64."""
    x = _d(x)
    ax = x.abs()
    if act == "gelu_erf":
        e = torch.erf(x * math.sqrt(0.5))
        return 0.5 * x * (1.0 + e), 0.5 * ax * (1.0 + e.abs())
    if act == "gelu_tanh":
        u = K0 * (x + K1 * x ** 3)
        t = torch.tanh(u)
        return 0.5 * x * (1.0 + t), 0.5 * ax * (1.0 + t.abs())
    if act == "relu":
        return x.clamp_min(0.0), x.clamp_min(0.0)
    if act == "silu":
        y = x * torch.sigmoid(x)
        return y, y.abs() * (1.0 + ax)
    if act == "tanh":
        t = torch.tanh(x)
        return t, t.abs() * (1.0 + ax)
    raise KeyError(act)


def act_slope(x, act):
    """(act'(x), scale) in float64, closed forms."""
    x = _d(x)
    ax = x.abs()
    if act == "gelu_erf":
        e = torch.erf(x * math.sqrt(0.5))
        phi = torch.exp(-0.5 * x * x) * 0.3989422804014327
        return 0.5 * (1.0 + e) + x * phi, 0.5 * (1.0 + e.abs()) + ax * phi * (1.0 + 0.5 * x * x)
    if act == "gelu_tanh":
        t = torch.tanh(K0 * (x + K1 * x ** 3))
        w = 0.5 * K0 * (1.0 + 3.0 * K1 * x * x)
        return 0.5 * (1.0 + t) + x * (1.0 - t * t) * w, 0.5 * (1.0 + t.abs()) + ax * (1.0 + t * t) * w
    if act == "relu":
        s = (x > 0).to(F64)
        return s, s
    if act == "silu":
        s = torch.sigmoid(x)
        return s * (1.0 + x * (1.0 - s)), s * (1.0 + ax * (1.0 + s)) * (1.0 + ax)
    if act == "tanh":
        t = torch.tanh(x)
        return 1.0 - t * t, 1.0 + t * t
    raise KeyError(act)


def act_fwd(x, act, out=None, out_dtype=None):
    return act_value(x, act)


def act_bwd(x, dy, act, out=None, out_dtype=None, accumulate=False):
    """out (+)= dy * act'(x)"""
    s, sm = act_slope(x, act)
    y, mag = _d(dy) * s, _d(dy).abs() * sm
    p = _prior(out, accumulate, y)
    return y + p, mag + p.abs()


def glu_fwd(a, b, out=None):
    y, ym = act_value(a, "silu")
    return y * _d(b), ym * _d(b).abs()


def glu_bwd(a, b, dy, da=None, db=None):
    """silu(a) * b backward -> ((da, scale), (db, scale))"""
    s, sm = act_slope(a, "silu")
    y, ym = act_value(a, "silu")
    dy, b = _d(dy), _d(b)
    return (dy * b * s, (dy * b).abs() * sm), (dy * y, dy.abs() * ym)


# ---------------------------------------------------------------------------------------------------------------- column sums
def colsum(x, x2=None, out=None, group_rows=0, accumulate=False, scale=1.0, x2_bcast=False, out_cs=1, x_bcast=False):
    """out[g, c] (+)= scale * sum_{rows of group g} x[r, c] * x2[r, c]; x2_bcast / x_bcast: that operand is one value per row; scale 0 means 1.
    Returned as [groups, C]."""
    v = _d(x)
    if x_bcast:
        v = v.reshape(-1, 1)
    if x2 is not None:
        w = _d(x2)
        v = v * (w.reshape(-1, 1) if x2_bcast else w)
    rows, C = v.shape
    gr = group_rows or rows
    sc = f32(scale) if scale != 0 else 1.0
    s = v.view(rows // gr, gr, C).sum(1) * sc
    m = v.abs().view(rows // gr, gr, C).sum(1) * abs(sc)
    if accumulate and out is not None:
        p = _d(out).reshape(s.shape)
        s, m = s + p, m + p.abs()
    return s, m


# ---------------------------------------------------------------------------------------------------------------- norm backward
def norm_bwd(x, dy, gamma=None, eps=1e-5, rms=False, dx=None, dx_dtype=None, accumulate=False, want_xhat=False):
    """g = dy * gamma; LN: dx = rstd * (g - mean(g) - xhat * mean(g * xhat)); RMS: dx = rstd * (g - xhat * mean(g * xhat)).
    -> ((dx, scale), (xhat, scale))"""
    x, g = _d(x), _d(dy)
    if gamma is not None:
        g = g * _d(gamma)
    mean = torch.zeros_like(x[:, :1]) if rms else x.mean(1, keepdim=True)
    d = x - mean
    rstd = torch.rsqrt((d * d).mean(1, keepdim=True) + f32(eps))
    xh = d * rstd
    s1 = torch.zeros_like(mean) if rms else g.mean(1, keepdim=True)
    s2 = (g * xh).mean(1, keepdim=True)
    ref = rstd * (g - s1 - xh * s2)
    a1 = torch.zeros_like(mean) if rms else g.abs().mean(1, keepdim=True)
    a2 = (g * xh).abs().mean(1, keepdim=True)
    base = rstd * (g.abs() + a1 + xh.abs() * a2)
    cond = torch.zeros_like(mean) if rms else x.abs().amax(1, keepdim=True) * rstd
    scale = base * (1.0 + cond) + cond * rstd * (a2 + xh.abs() * g.abs().mean(1, keepdim=True))
    p = _prior(dx, accumulate, ref)
    return (ref + p, scale + p.abs()), (xh, xh.abs() * (1.0 + cond) + cond)


def norm_fwd(x, gamma=None, eps=1e-5, rms=False):
    """the forward the closed form above differentiates (autograd check only)."""
    d = x if rms else x - x.mean(1, keepdim=True)
    y = d * torch.rsqrt((d * d).mean(1, keepdim=True) + eps)
    return y * gamma if gamma is not None else y


# ---------------------------------------------------------------------------------------------------------------- the small ones
def transpose(x, pad=8, out=None):
    """bf16 [cols, ceil(rows / pad) * pad], zero tail: exact (compare with torch.equal)."""
    rows, cols = x.shape
    y = torch.zeros(cols, (rows + pad - 1) // pad * pad, dtype=torch.bfloat16, device=x.device)
    y[:, :rows] = x.t().to(torch.bfloat16)
    return y


def sparse_rows(inp, idx, coef, out=None, accumulate=False):
    """out[t] (+)= sum_j coef[t, j] * inp[idx[t, j]], idx -1 = unused"""
    w = torch.where(idx >= 0, _d(coef), torch.zeros_like(_d(coef)))
    rows = _d(inp)[idx.clamp_min(0).long()]
    s, m = (rows * w.unsqueeze(-1)).sum(1), (rows.abs() * w.abs().unsqueeze(-1)).sum(1)
    p = _prior(out, accumulate, s)
    return s + p, m + p.abs()


def small_linear(x, w, bias=None, tab=None, out=None, out_dtype=torch.float32, w_transposed=False):
    """out[r, n] = sum_k x[r, k] * W[n, k] + bias[n] + tab[r % len(tab), n]"""
    W = _d(w).t() if w_transposed else _d(w)
    y, m = _d(x) @ W.t(), _d(x).abs() @ W.abs().t()
    if bias is not None:
        y, m = y + _d(bias), m + _d(bias).abs()
    if tab is not None:
        N = y.shape[1]
        t = _d(tab).reshape(-1, N)[torch.arange(y.shape[0], device=y.device) % (tab.numel() // N)]
        y, m = y + t, m + t.abs()
    return y, m


def mse_masked(pred, target, mask, T, loss_scale=1.0, want_grad=True):
    """loss = sum_s mask[s] * sum_{t,d} (pred - target)^2 / (sum_s mask[s] * T * D), dpred = loss_scale * d loss / d pred; a batch whose mask
    sums to 0 gives loss 0 and dpred 0. -> ((loss [1], scale), (dpred, scale))"""
    D = target.shape[1]
    p, t = _d(pred)[:, :D], _d(target)
    m = _d(mask).repeat_interleave(T)[:, None]
    denom = _d(mask).sum() * T * D
    inv = 1.0 / denom if denom > 0 else torch.zeros((), dtype=F64, device=p.device)
    e = p - t
    loss = ((m * e * e).sum() * inv).view(1)
    lmag = ((m.abs() * (p.abs() + t.abs()) ** 2).sum() * inv.abs()).view(1)
    ls = f32(loss_scale)
    amask = _d(mask).abs().sum() * T * D
    rel = amask * inv.abs() if denom > 0 else 0.0          # cancellation inside the mask sum (1 for non-negative weights)
    return (loss, lmag * rel), (2.0 * m * e * inv * ls, 2.0 * m.abs() * (p.abs() + t.abs()) * inv.abs() * abs(ls) * rel)


def gemm_nn(x, w, out=None, out_dtype=torch.float32, splits=None):
    """out[m, k] = sum_n x[m, n] * w[n, k]"""
    return _d(x) @ _d(w), _d(x).abs() @ _d(w).abs()


# ---------------------------------------------------------------------------------------------------------------- AdamW
def adamw(p, g, m, v, lr, beta1, beta2, eps, wd, step, sumsq=None, max_norm=0.0, grad_scale=1.0):
    """one torch.optim.AdamW step after clip_grad_norm_(max_norm) on grad_scale * g, from float64 copies of the state (not in place).
    `sumsq` is ||g||^2 of the whole (unscaled) gradient buffer, or None (no norm: no clipping). Hyper-parameters are taken as the fp32 values the
    kernel receives. Returns a dict: p, m, v, norm (float), clip (float) and per-element scales sp, sm, sv; cp, cm, cv are d(result) / d ln(clip),
    the sensitivity to the relative error of the fp32 norm (zero when the clip is inactive)."""
    lr, b1, b2, eps, wd, gsc, mx = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(wd), f32(grad_scale), f32(max_norm)
    bc1, bc2 = f32(1.0 - beta1 ** step), f32(1.0 - beta2 ** step)
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    total = math.sqrt(float(sumsq)) * gsc if sumsq is not None else 0.0
    clip = min(1.0, mx / (total + f32(1e-6))) if mx > 0 else 1.0
    gg = g * (gsc * clip)
    m1 = b1 * m + (1.0 - b1) * gg
    v1 = b2 * v + (1.0 - b2) * gg * gg
    den = v1.sqrt() / math.sqrt(bc2) + eps
    upd = (lr / bc1) * m1 / den
    p1 = p * (1.0 - lr * wd) - upd
    sm = b1 * m.abs() + (1.0 - b1) * gg.abs()
    sv = v1
    sp = p.abs() * (1.0 + lr * wd) + 2.0 * upd.abs()
    active = 1.0 if clip < 1.0 else 0.0
    cm = active * (1.0 - b1) * gg.abs()
    cv = active * 2.0 * (1.0 - b2) * gg * gg
    cp = (lr / bc1) * (cm / den + m1.abs() * (0.5 * cv / v1.sqrt().clamp_min(1e-300)) / math.sqrt(bc2) / (den * den))
    return dict(p=p1, m=m1, v=v1, norm=total, clip=clip, sp=sp, sm=sm, sv=sv, cp=cp, cm=cm, cv=cv)


def norm_rel_bound(n: int) -> float:
    """relative bound of the fp32 gradient norm: sum of squares in 1024 column partials of n / 1024 rows each, then 1024 partials, one sqrt."""
    return 16 * U * math.sqrt(1024 + n / 1024)
