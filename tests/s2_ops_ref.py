"""TEST INFRASTRUCTURE: float64 restatements of the System-2 token kernels (internnav_amd/csrc/rope.hip) and of the norm family
(internnav_amd/csrc/norm.hip), written from the contract comments of include/internnav_amd.h and the docstrings of `internnav_amd.ops`,
not from the kernels. The conventions are those of tests/train_ops_ref.py: every function takes the arguments of the ops wrapper of the same
name, upcasts the (already bf16- / fp32-rounded) inputs to float64 and returns `(ref, scale)` (tuples of them for ops with two results), `scale`
being the float64 sum of the |terms| that enter each element. In-place ops (rope) and ops that keep part of `out` read the buffers they are
given, so call the reference BEFORE the kernel.

  rope         ((x_ref, x_scale), (kv_ref, kv_scale) | None): the FULL buffers x and kv_out as they must look afterwards. scale is
               |lo*cos| + |hi*sin| on rotated elements and 0 on every element that is copied or must stay as it is - those compare exactly.
  mrope_table  ((cos, 1), (sin, 1)) of shape [n, D]. The angle is the fp32 product fp32(pos) * inv_freq, ROUNDED to fp32: that is the contract
               (and what the HF module computes); cos / sin of that fp32 number are then taken in float64. Keeping the angle in float64 instead
               moves the result by 1e-3 at position 40000 (tests/test_s2_ops_ref_cpu.py shows it).
  gather_rows  (expected `out` buffer in its own dtype, None): a bit copy, compared with torch.equal.
  argmax_rows  (torch.argmax(x, 1), None): first maximum.
  norm         ((t, scale), (t2, scale2) | None) over the LOGICAL rows [rows, C]; `map_rows` gives their physical rows.
               LayerNorm's d = x - mean carries an absolute error ~ 2^-24 * |x|max, i.e. 2^-24 * cond in xhat with cond = |x|max * rstd
               (train_ops_ref explains and measures this for norm_bwd): xhat enters with |xhat| * (1 + cond) + cond, cond = 0 for RMS.
               1 + mod_scale enters with 1 + |mod_scale| (the fp32 sum is rounded relative to that), tanh(g) with |tanh g| * (1 + |g|).
               The chained second norm is computed from the fp32-ROUNDED first result t. The kernel's own t differs from that by e <= bound(scale),
               which moves xhat2 by at most p + max_row(p) * (1 + |xhat2|), p = scale * rstd2 (the element itself, the row mean, and rstd2
               through the variance): that term is part of scale2, so the same constant k bounds both results.
"""
from __future__ import annotations

import torch

from tests.train_ops_ref import BF, TINY, U, F64, _d, f32, fp32_bound, out_bound  # noqa: F401  (re-exported for the tests)


def map_rows(rows, m, device="cpu"):
    """physical row of logical rows 0..rows-1 under a row map (seg_len, seg_stride, off); None = identity."""
    r = torch.arange(rows, device=device)
    if m is None or int(m[0]) <= 0:
        return r
    seg_len, seg_stride, off = (int(v) for v in m)
    return (r // seg_len) * seg_stride + off + r % seg_len


# ---------------------------------------------------------------------------------------------------------------- rope.hip
def rope(x, cos, sin, heads, D, col0=0, rows=None, row_map=None, tab=None, kv_out=None, kv_dst=None, kv_head0=0, v_heads=0):
    """lo' = lo * cos[:half] - hi * sin[:half], hi' = hi * cos[half:] + lo * sin[half:] per head (x * cos + rotate_half(x) * sin), table row
    tab[r] or r, physical row row_map(r). With kv_out the heads [kv_head0, heads) are key heads: rotated into kv_out[kv_dst[r]], followed there
    by the v_heads value heads of the row, unrotated; the k and v columns of x stay as they are."""
    X = _d(x)
    rows = X.shape[0] if rows is None else rows
    half = D // 2
    dev = X.device
    r = torch.arange(rows, device=dev)
    pr = map_rows(rows, row_map, dev)
    tr = tab[:rows].long() if tab is not None else r
    c, s = _d(cos).reshape(-1, D)[tr][:, None, :], _d(sin).reshape(-1, D)[tr][:, None, :]
    blk = X[pr, col0: col0 + heads * D].reshape(rows, heads, D)
    lo, hi = blk[..., :half], blk[..., half:]
    rot = torch.cat([lo * c[..., :half] - hi * s[..., :half], hi * c[..., half:] + lo * s[..., half:]], -1)
    mag = torch.cat([(lo * c[..., :half]).abs() + (hi * s[..., :half]).abs(), (hi * c[..., half:]).abs() + (lo * s[..., half:]).abs()], -1)
    ref, scale = X.clone(), torch.zeros_like(X)
    nq = heads if kv_out is None else kv_head0
    ref[pr, col0: col0 + nq * D] = rot[:, :nq].reshape(rows, nq * D)
    scale[pr, col0: col0 + nq * D] = mag[:, :nq].reshape(rows, nq * D)
    if kv_out is None:
        return (ref, scale), None
    KV = _d(kv_out)
    kref, kscale = KV.clone(), torch.zeros_like(KV)
    nk = heads - kv_head0
    d = kv_dst[:rows].long()
    kref[d, : nk * D] = rot[:, kv_head0:].reshape(rows, nk * D)
    kscale[d, : nk * D] = mag[:, kv_head0:].reshape(rows, nk * D)
    kref[d, nk * D: (nk + v_heads) * D] = X[pr, col0 + heads * D: col0 + (heads + v_heads) * D]
    return (ref, scale), (kref, kscale)


def rope_bound(ref, scale):
    """4 roundings of the fp32 expression (two products, one sum, the table read is exact) + round-to-nearest to bf16."""
    return 4.0 * U * scale + BF * ref.abs()


def mrope_angle(pos, inv_freq, axis_of):
    """fp32 [n, D/2]: fp32(pos[axis_of[f], t]) * inv_freq[f], one fp32 rounding (positions below 2^24 convert exactly)."""
    p = pos[axis_of.long()].t().to(torch.float32)                      # [n, D/2]
    return p * inv_freq.to(torch.float32)[None, :]


def mrope_table(pos, inv_freq, axis_of, cos=None, sin=None):
    a = mrope_angle(pos, inv_freq, axis_of).to(F64)
    c, s = torch.cos(a), torch.sin(a)
    c, s = torch.cat([c, c], 1), torch.cat([s, s], 1)
    one = torch.ones_like(c)
    return (c, one), (s, one)


def gather_rows(x, out, src=None, dst=None, rows=None):
    """out[dst[r] or r] = x[src[r] or r] for r < rows; every other row of out keeps its content."""
    if rows is None:
        rows = src.numel() if src is not None else (dst.numel() if dst is not None else x.shape[0])
    r = torch.arange(rows, device=x.device)
    sr = src[:rows].long() if src is not None else r
    dr = dst[:rows].long() if dst is not None else r
    ref = out.clone()
    ref[dr] = x[sr]
    return ref, None


def argmax_rows(x, out=None):
    return torch.argmax(x, dim=1), None


# ---------------------------------------------------------------------------------------------------------------- norm.hip
def _stats(x, rms, eps):
    """xhat, its scale, rstd of float64 rows."""
    mean = torch.zeros_like(x[:, :1]) if rms else x.mean(1, keepdim=True)
    d = x - mean
    rstd = torch.rsqrt((d * d).mean(1, keepdim=True) + eps)
    xh = d * rstd
    cond = torch.zeros_like(mean) if rms else x.abs().amax(1, keepdim=True) * rstd
    return xh, xh.abs() * (1.0 + cond) + cond, rstd


def norm(x, gamma=None, beta=None, eps=1e-5, rms=False, mod_scale=None, gate=None, base=None, mod_div=1, pos=None, out=None, out32=None,
         rows=None, in_map=None, out_map=None, out2=None, gamma2=None, mod_scale2=None):
    """t = norm(x[in_map(r)]) * gamma + beta; t *= 1 + mod_scale[r // mod_div]; t *= tanh(gate[r // mod_div]); t += base[r];
    t += pos[r % len(pos)]; out2 = norm(fp32(t)) * gamma2 * (1 + mod_scale2[r // mod_div]). Modulation, base and pos follow the logical row."""
    X = _d(x).reshape(-1, x.shape[-1])
    C = X.shape[1]
    rows = X.shape[0] if rows is None else rows
    dev = X.device
    r = torch.arange(rows, device=dev)
    e = f32(eps)
    t, m, _ = _stats(X[map_rows(rows, in_map, dev)], rms, e)
    if gamma is not None:
        t, m = t * _d(gamma), m * _d(gamma).abs()
    if beta is not None:
        t, m = t + _d(beta), m + _d(beta).abs()
    mr = r // mod_div
    if mod_scale is not None:
        s = _d(mod_scale)[mr]
        t, m = t * (1.0 + s), m * (1.0 + s.abs())
    if gate is not None:
        g = _d(gate)[mr]
        t, m = t * torch.tanh(g), m * torch.tanh(g).abs() * (1.0 + g.abs())
    if base is not None:
        b = _d(base).reshape(-1, C)[r]
        t, m = t + b, m + b.abs()
    if pos is not None:
        p = _d(pos).reshape(-1, C)[r % (pos.numel() // C)]
        t, m = t + p, m + p.abs()
    if out2 is None:
        return (t, m), None
    t32 = t.to(torch.float32).to(F64)
    t2, m2, rstd2 = _stats(t32, rms, e)
    p = m * rstd2
    m2 = m2 + p + p.amax(1, keepdim=True) * (1.0 + t2.abs())
    if gamma2 is not None:
        t2, m2 = t2 * _d(gamma2), m2 * _d(gamma2).abs()
    if mod_scale2 is not None:
        s = _d(mod_scale2)[mr]
        t2, m2 = t2 * (1.0 + s), m2 * (1.0 + s.abs())
    return (t, m), (t2, m2)
