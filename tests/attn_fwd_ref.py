"""TEST INFRASTRUCTURE: float64 restatement of the attention forward (ina_attention_bf16: internnav_amd/csrc/attention.hip and attention_wide.hip),
its error-bound model, a float32 / bf16 emulation of the kernels' rounding points, and the case table shared by tests/test_attn_fwd_ref_cpu.py and
tests/test_attention_fwd_fp64_gpu.py. Plain torch on the CPU; nothing of internnav_amd is imported.

The function restated is  o = f(q, k, v; scale, causal, kv_start, k_len | cu_q / cu_k, kv_bdiv, head_gate, accumulate base, dropout)  as the
kernels define it:
  * len_k = min(k_len[b // kv_bdiv], Lk), or the cu_k span of the sequence; len_q = Lq, or the cu_q span;
  * key j is allowed for query i iff kv_start <= j < len_k, and under `causal` also j <= i + (len_k - len_q);
  * P = softmax over the allowed keys; a row with no allowed key is exactly 0 - with `accumulate` it is the base, unchanged;
  * dropout: m = keep / (1 - p) from the host replica of ina_hash at the index ((b*H + h)*Lq + q)*Lk + k with the FULL Lk; it multiplies P AFTER
    the row sum (the normaliser stays un-dropped);
  * o = (P m) v, multiplied by tanh(gate[h]) (fp32 in the kernel), the base added, ONE rounding to bf16.
The rope + append launch (d = 128 decode kernel) first rotates q and k_new with rope.hip's fp32 formula (one bf16 rounding), writes
rotate(k_new) | v_new into cache rows len_k - Lq .. len_k - 1 and then is the function above (`rope_rotate`, `rope_apply`).

Bound (per element, all-or-nothing, limit 1.0; derived from the number formats and the kernels' rounding points, nothing in it comes from a
kernel's output). The kernels compute the logits with fp32 accumulation, e_j = exp2(s_j c - m) in fp32 for a row offset m (the running maximum;
in attention_wide.hip a deferred one, at most 2^6 below it, so e_j <= 2^6), round e_j m_j to bf16 just before the P V MFMA, keep the row sum of
the UN-rounded e_j, every rescale, the split partials and their merge in fp32, and round the stored value once. With u8 = 2^-8, u24 = 2^-24,
t = |tanh(gate)| (1 without a gate), A = sum_j |P_j m_j| |v_jd| in float64 and o = sum_j P_j m_j v_jd:
    bound = u8 * (t A + |ref|) * (1 + 2^-6)  +  t * (fK * (A + |o|) + E_S)            and bound = 0 where A = 0
  * u8 t A: the bf16 rounding of P (relative 2^-8 per key whatever the row offset, bf16 has fp32's exponent range); u8 |ref|: the rounding of
    the stored value; 2^-6 of head-room for their product;
  * fK = 16 u24 (sqrt(Lk) + 4), the project's fp32 model (test_s1_head_ops_gpu.py) over the key axis: the fp32 accumulation of the numerator
    (against A) and of the row sum (relative, so against |o|), the rescales, the merge of partials, 1 / l, tanhf and the base add;
  * E_S: the fp32 error of the exponent. The logit s_j carries f T_j, f = 16 u24 (sqrt(D) + 4), T_j = scale sum_d |q_d| |k_jd|; the argument
    s_j c - m is rounded at magnitude <= |s_j| + |M| (M the row maximum) and exp2 itself is good to a few ulp: eps_j = f T_j + 4 u24 (|M| + 8)
    (the 8: the deferred offset of up to 6 and exp2's own error). It enters through the numerator and through the normaliser:
    E_S = sum_j P_j m_j eps_j |v_jd| + |o| sum_j P_j eps_j.
Where A = 0 - a row without an allowed key (masked rows, k_len 0, len_k below kv_start, causal rows of Lq > len_k), or all of whose keys are
dropped - every product the kernel adds is 0: the result is exactly 0, or exactly the base, the bound is 0 and the check is `==`.
"""
from __future__ import annotations

import math
import zlib

import torch

from tests.attn_bwd_ref import U8, U24, _softmax, drop_keep, f32, ratio  # noqa: F401  (ratio is re-exported to the two test modules)

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16
DEFER_THR = 6.0      # attention_wide.hip: a row keeps its running maximum until it grows by more than 2^6
MUTATIONS = ("klen_plus", "klen_minus", "diag_plus", "diag_minus", "shift_Lk", "kvstart_plus", "kvstart_minus", "kv_head_mod", "no_bdiv",
             "gate_no_tanh", "drop_idx_lenk", "drop_before_sum", "cu_k_neighbour")
SALT = 12345         # the device word of the salted dropout runs


# ------------------------------------------------------------------------------------------------------------ rope (rope.hip's arithmetic)
def rope_rotate(x, cos, sin):
    """x bf16 [..., 128], cos / sin f32 broadcastable to it: lo' = fma(lo, c[d], -(hi * s[d])), hi' = fma(hi, c[d + 64], lo * s[d + 64]) in fp32, one
    bf16 rounding. The bf16 x fp32 products are exact in float64, so the inner product is rounded to fp32 exactly as the kernel does and the
    fused multiply-add is the float64 sum rounded to fp32 (the two roundings differ from the fused one only for a sum within 2^-29 ulp of an fp32 tie:
    none among the seeded cases, whose appended cache rows the GPU test finds bit-equal)."""
    h = x.shape[-1] // 2
    lo, hi = x[..., :h].to(F64), x[..., h:].to(F64)
    c, s = cos.to(F64).expand(x.shape), sin.to(F64).expand(x.shape)
    olo = (lo * c[..., :h] - (hi * s[..., :h]).to(F32).to(F64)).to(F32)
    ohi = (hi * c[..., h:] + (lo * s[..., h:]).to(F32).to(F64)).to(F32)
    return torch.cat([olo, ohi], -1).to(BF16)


def rope_apply(c, inp):
    """(q rotated, k cache, v cache) after the launch's rope + append: rotate(k_new) | v_new in rows len_k - Lq .. len_k - 1 of every sequence."""
    B, Lq, Lk, H, Hkv, D = c["dims"]
    cos, sin = inp["cos"].view(B, Lq, 1, D), inp["sin"].view(B, Lq, 1, D)
    q = rope_rotate(inp["q"], cos, sin)
    k, v = inp["k"].clone(), inp["v"].clone()
    kn = rope_rotate(inp["k_new"], cos, sin)
    for b in range(B):
        lk = min(int(inp["k_len"][b]), Lk) if inp["k_len"] is not None else Lk
        assert lk >= Lq, "rope + append: every k_len >= Lq (the launch writes cache rows len_k - Lq ..)"
        k[b, lk - Lq:lk], v[b, lk - Lq:lk] = kn[b], inp["v_new"][b]
    return q, k, v


# ------------------------------------------------------------------------------------------------------------ the restatement
def dense_inputs(c, inp, mut=None):
    """(q [B, Lq, H, D], k, v [Bk, Lk, Hkv, D], len_q [B], len_k [Bk]) - packed (varlen) inputs are unpacked into zero-padded dense ones."""
    B, Lq, Lk, H, Hkv, D = c["dims"]
    if c["lens_q"] is None:
        Bk = B // c["kv_bdiv"]
        len_k = torch.full((Bk,), Lk, dtype=torch.int64) if inp["k_len"] is None else inp["k_len"].to(torch.int64).clamp(max=Lk)
        if c["rope"]:
            q, k, v = rope_apply(c, inp)
            return q, k, v, torch.full((B,), Lq, dtype=torch.int64), len_k
        return inp["q"], inp["k"], inp["v"], torch.full((B,), Lq, dtype=torch.int64), len_k
    cu_q, cu_k = inp["cu_q"].to(torch.int64), inp["cu_k"].to(torch.int64)
    len_q, len_k = cu_q[1:] - cu_q[:-1], cu_k[1:] - cu_k[:-1]
    q = torch.zeros(B, Lq, H, D, dtype=BF16)
    k, v = torch.zeros(B, Lk, Hkv, D, dtype=BF16), torch.zeros(B, Lk, Hkv, D, dtype=BF16)
    Tk = inp["k"].shape[0]
    for b in range(B):
        q[b, :int(len_q[b])] = inp["q"][int(cu_q[b]):int(cu_q[b + 1])]
        k0 = int(cu_k[b + 1] if mut == "cu_k_neighbour" else cu_k[b])
        idx = (k0 + torch.arange(int(len_k[b]))).clamp(max=Tk - 1)
        k[b, :int(len_k[b])], v[b, :int(len_k[b])] = inp["k"][idx], inp["v"][idx]
    return q, k, v, len_q, len_k


def pack(c, inp, t):
    """dense [B, Lq, ...] -> the packed rows [T, ...] of a varlen case (identity for dense cases)."""
    if c["lens_q"] is None:
        return t
    cu_q = inp["cu_q"].to(torch.int64)
    return torch.cat([t[b, :int(cu_q[b + 1] - cu_q[b])] for b in range(c["dims"][0])], 0)


def _setup(c, len_q, len_k, mut):
    B, Lq, Lk, H, Hkv, D = c["dims"]
    Bk, G = len_k.numel(), H // Hkv
    bi = torch.arange(B) % Bk if mut == "no_bdiv" else torch.arange(B) // c["kv_bdiv"]
    hi = torch.arange(H) % Hkv if mut == "kv_head_mod" else torch.arange(H) // G
    lk = len_k[bi]
    ak, aq = torch.arange(Lk).view(1, 1, Lk), torch.arange(Lq).view(1, Lq, 1)
    lim = lk + (1 if mut == "klen_plus" else -1 if mut == "klen_minus" else 0)
    start = c["kv_start"] + (1 if mut == "kvstart_plus" else -1 if mut == "kvstart_minus" else 0)
    allowed = (ak < lim.view(B, 1, 1)) & (ak >= start) & (aq < len_q.view(B, 1, 1))
    if c["causal"]:
        shift = (torch.full_like(lk, Lk) if mut == "shift_Lk" else lk) - len_q
        shift = shift + (1 if mut == "diag_plus" else -1 if mut == "diag_minus" else 0)
        allowed = allowed & (ak <= aq + shift.view(B, 1, 1))
    return bi, hi, lk, allowed[:, None]                 # allowed: bool [B, 1, Lq, Lk]


def _drop(c, lk, mut, dtype, salt=0):
    if c["drop"] is None:
        return None
    B, Lq, Lk, H, Hkv, D = c["dims"]
    p, seed = c["drop"]
    keep = drop_keep(B, H, Lq, Lk, p, seed + salt, lk if mut == "drop_idx_lenk" else None)
    return keep.to(dtype) * f32(1.0 / (1.0 - p))


def _gate(c, inp, mut, dtype):
    if inp.get("gate") is None:
        return None
    g = inp["gate"].to(dtype)
    return (g if mut == "gate_no_tanh" else torch.tanh(g)).view(1, 1, -1, 1)


# ---- the bound's arithmetic (module docstring), shared with tests/attn_decode_ref.py
def fp32_factor(n):
    """16 u24 (sqrt(n) + 4): the project's model of an fp32 accumulation over n terms; n a number or a tensor."""
    return 16.0 * U24 * ((torch.sqrt(n) if torch.is_tensor(n) else math.sqrt(n)) + 4.0)


def exponent_eps(T, M, D):
    """eps_j = f T_j + 4 u24 (|M| + 8): T the float64 sum_d |q_d| |k_jd| scale per key, M the row maximum of the allowed logits with a trailing
    key axis of 1 (-inf for a row without a key: taken as 0), D the head dim."""
    M = torch.where(torch.isinf(M), torch.zeros_like(M), M).abs()
    return fp32_factor(D) * T + 4.0 * U24 * (M + 8.0)


def bound_of(A, o, ref, ES, fK, ta=1.0):
    """u8 (t A + |ref|)(1 + 2^-6) + t (fK (A + |o|) + E_S), and 0 where A = 0."""
    bound = U8 * (ta * A + ref.abs()) * (1.0 + 2.0 ** -6) + ta * (fK * (A + o.abs()) + ES)
    return torch.where(A > 0, bound, torch.zeros_like(bound))


def reference(c, inp, mut=None, bounds=True, salt=0):
    """(ref, bound): float64 [B, Lq, H, D] (dense; `pack` gives the varlen rows); bound None with bounds=False."""
    B, Lq, Lk, H, Hkv, D = c["dims"]
    sc = f32(c["scale"])
    q, k, v, len_q, len_k = dense_inputs(c, inp, mut)
    bi, hi, lk, allowed = _setup(c, len_q, len_k, mut)
    q64, kk, vv = q.to(F64), k.to(F64)[bi][:, :, hi], v.to(F64)[bi][:, :, hi]
    S = torch.einsum("bqhd,bkhd->bhqk", q64, kk) * sc
    P = _softmax(S, allowed)
    m = _drop(c, lk, mut, F64, salt)
    Pm = P if m is None else P * m
    if mut == "drop_before_sum" and m is not None:
        den = Pm.sum(-1, keepdim=True)
        Pm = Pm / torch.where(den > 0, den, torch.ones_like(den))
    o = torch.einsum("bhqk,bkhd->bqhd", Pm, vv)
    t = _gate(c, inp, mut, F64)
    ref = o if t is None else o * t
    if inp.get("base") is not None:
        ref = ref + inp["base"].to(F64)
    if not bounds:
        return ref, None
    ta = 1.0 if t is None else t.abs()
    A = torch.einsum("bhqk,bkhd->bqhd", Pm.abs(), vv.abs())
    T = torch.einsum("bqhd,bkhd->bhqk", q64.abs(), kk.abs()) * sc
    M = S.masked_fill(~allowed, float("-inf")).amax(-1, keepdim=True)
    eps = exponent_eps(T, M, D)
    ES = torch.einsum("bhqk,bkhd->bqhd", Pm.abs() * eps, vv.abs()) + o.abs() * (P * eps).sum(-1).permute(0, 2, 1)[..., None]
    return ref, bound_of(A, o, ref, ES, fp32_factor(Lk), ta)


def emulate(c, inp, block=64, defer=None, salt=0, trace=None):
    """the kernels' arithmetic on the CPU: fp32 everywhere, 64-key blocks from (kv_start / 64) * 64 with a running maximum (defer = DEFER_THR: the
    deferred one of attention_wide.hip), P rounded to bf16 before the second product, un-rounded row sum, one bf16 result. `trace` (a list)
    receives per block (block maximum, running maximum before the block) in the exp2 domain, each [B, H, Lq]."""
    B, Lq, Lk, H, Hkv, D = c["dims"]
    q, k, v, len_q, len_k = dense_inputs(c, inp)
    bi, hi, lk, allowed = _setup(c, len_q, len_k, None)
    qf, kk, vv = q.to(F32), k.to(F32)[bi][:, :, hi], v.to(F32)[bi][:, :, hi]
    sc2 = torch.tensor(f32(c["scale"]), dtype=F32) * torch.tensor(1.4426950408889634, dtype=F32)
    S = (torch.einsum("bqhd,bkhd->bhqk", qf, kk) * sc2).masked_fill(~allowed.expand(B, H, Lq, Lk), float("-inf"))
    m = _drop(c, lk, None, F32, salt)
    m_run = torch.full((B, H, Lq), float("-inf"), dtype=F32)
    l_run = torch.zeros(B, H, Lq, dtype=F32)
    acc = torch.zeros(B, H, Lq, D, dtype=F32)
    for k0 in range((c["kv_start"] // block) * block, Lk, block):
        s = S[..., k0:k0 + block]
        mx = s.amax(-1)
        if trace is not None:
            trace.append((mx.clone(), m_run.clone()))
        m_new = torch.maximum(m_run, mx) if defer is None else torch.where(mx > m_run + defer, torch.maximum(m_run, mx), m_run)
        m_use = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        alpha = torch.exp2(m_run - m_use)
        e = torch.exp2(s - m_use[..., None])
        l_run = l_run * alpha + e.sum(-1)
        pb = (e if m is None else e * m[..., k0:k0 + block]).to(BF16).to(F32)
        acc = acc * alpha[..., None] + torch.einsum("bhqk,bkhd->bhqd", pb, vv[:, k0:k0 + block])
        m_run = m_new
    o = (acc * torch.where(l_run > 0, 1.0 / l_run, torch.zeros_like(l_run))[..., None]).permute(0, 2, 1, 3)
    t = _gate(c, inp, None, F32)
    if t is not None:
        o = o * t
    if inp.get("base") is not None:
        o = o + inp["base"].to(F32)
    return o.to(BF16)


# ------------------------------------------------------------------------------------------------------------ cases
def case(group, B, Lq, Lk, H, Hkv, D, causal=False, k_len=None, kv_start=0, kv_bdiv=1, kernels=(1,), drop=None, scale=None, gate=False, acc=False,
         lens_q=None, lens_k=None, layout="plain", rope=False, ramp=None, edges=()):
    """kernels: the ina_attn_args.kernel values the GPU suite runs the case with (each against float64 on its own). lens_q / lens_k: varlen (B, Lq, Lk
    are then their count and maxima). edges: "zero" - the case has real rows without an allowed key, or with every key dropped (bound 0)."""
    if lens_q is not None:
        lens_k = lens_q if lens_k is None else lens_k
        assert B == len(lens_q) == len(lens_k) and Lq == max(lens_q) and Lk == max(lens_k) and layout == "varlen"
    name = f"{group}-{B}x{Lq}x{Lk}x{H}x{Hkv}x{D}" + ("-causal" if causal else "") + (f"-klen{'_'.join(map(str, k_len))}" if k_len else "") \
        + (f"-start{kv_start}" if kv_start else "") + (f"-bdiv{kv_bdiv}" if kv_bdiv > 1 else "") + (f"-p{drop[0]}" if drop else "") \
        + (f"-scale{scale}" if scale else "") + ("-gate" if gate else "") + ("-acc" if acc else "") \
        + (f"-q{'_'.join(map(str, lens_q))}-k{'_'.join(map(str, lens_k))}" if lens_q else "") + (f"-{layout}" if layout not in ("plain", "varlen") else "") \
        + ("-rope" if rope else "") + (f"-ramp{'_'.join(map(str, ramp))}" if ramp else "")
    return dict(name=name, group=group, dims=(B, Lq, Lk, H, Hkv, D), causal=causal, k_len=k_len, kv_start=kv_start, kv_bdiv=kv_bdiv, kernels=tuple(kernels),
                drop=drop, scale=scale if scale else D ** -0.5, gate=gate, acc=acc, lens_q=lens_q, lens_k=lens_k, layout=layout, rope=rope, ramp=ramp,
                edges=tuple(edges))


Z = ("zero",)
# scale 0.3 goes to cases with D <= 64 only: the planted logit 3 |q|^2 scale stays below 70 there, so every probability that the float64 reference
# keeps stays a normal fp32 number (attn_bwd_ref.py; at D 128 it would be exp(-115))
# ---- row16: attn_fwd_kernel<DP, DV, NW, KVB>. Lq 16 | 17 and 32 | 33 switch the workgroup width (1 / 2 / 4 waves), Lk 48 | 49 the key block (32 / 64)
ROW16 = [
    case("row16", 2, 1, 1, 2, 2, 48), case("row16", 1, 16, 32, 2, 2, 64), case("row16", 1, 17, 33, 2, 1, 80), case("row16", 1, 32, 48, 2, 2, 128),
    case("row16", 1, 33, 49, 2, 2, 48), case("row16", 1, 65, 64, 2, 2, 64, scale=0.3), case("row16", 1, 16, 65, 4, 2, 80), case("row16", 1, 17, 129, 2, 2, 128),
    case("row16", 1, 33, 65, 2, 2, 64, True), case("row16", 1, 65, 65, 2, 1, 128, True), case("row16", 1, 65, 33, 2, 2, 48, True, scale=0.3, edges=Z),
    case("row16", 1, 32, 129, 2, 2, 80, True), case("row16", 1, 17, 1, 2, 2, 64, True, edges=Z),
    case("row16", 1, 17, 129, 2, 2, 64, kv_start=5), case("row16", 1, 33, 48, 2, 2, 64, kv_start=32), case("row16", 1, 17, 129, 2, 2, 64, kv_start=64, scale=0.3),
    case("row16", 1, 17, 129, 2, 2, 64, kv_start=70), case("row16", 1, 17, 129, 2, 2, 64, kv_start=128), case("row16", 1, 17, 129, 2, 2, 64, kv_start=129, edges=Z),
    case("row16", 1, 65, 129, 2, 2, 128, True, kv_start=70, edges=Z),
    case("row16", 3, 20, 65, 2, 2, 64, False, [65, 37, 0], edges=Z), case("row16", 3, 20, 65, 2, 2, 64, True, [65, 37, 0], edges=Z),
    case("row16", 3, 20, 65, 2, 2, 64, False, [65, 37, 0], kv_start=37, edges=Z),
    case("row16", 4, 17, 65, 4, 2, 64, False, [65, 37], kv_bdiv=2), case("row16", 2, 17, 33, 2, 1, 128, True, kv_bdiv=2),
    case("row16", 2, 33, 65, 2, 2, 48, gate=True, acc=True), case("row16", 1, 40, 33, 2, 2, 64, True, gate=True, acc=True, edges=Z),
    case("row16", 2, 20, 65, 2, 2, 128, False, [65, 0], gate=True, acc=True, edges=Z),
    case("row16", 5, 33, 65, 2, 2, 80, lens_q=[17, 0, 1, 33, 4], lens_k=[40, 7, 1, 65, 0], layout="varlen", edges=Z),
    case("row16", 4, 33, 40, 2, 1, 64, True, lens_q=[17, 1, 33, 0], lens_k=[40, 1, 20, 5], layout="varlen", edges=Z),
]
# ---- dropout: attn_fwd_kernel<.., DROP = true> (d 48 / 64), each case run unsalted and salted
DROPOUT = [
    case("dropout", 2, 33, 65, 2, 2, 48, True, drop=(0.1, 777), scale=0.3), case("dropout", 2, 17, 48, 2, 2, 64, False, [40, 23], drop=(0.25, 4242)),
    case("dropout", 1, 40, 40, 2, 1, 64, True, drop=(0.1, 99), edges=Z), case("dropout", 2, 17, 129, 2, 2, 48, False, [129, 50], drop=(0.25, 31337)),
]
# ---- decode: the split + combine pair (kernel 1), the 4-wave one-launch kernel (d 128: kernel 3, else kernel 0), the 8-wave one (d 128, kernel 0).
#      Contract: Lk >= 256, Lq <= 8, G * Lq <= 48, no gate / accumulate / kv_start / varlen. Lk 1024 | 1025: the automatic path leaves the one-launch
#      kernels (16 chunks) for the pair. G * Lq 16 | 17 | 48: one full row tile, one row more, three tiles.
K013, K01 = (0, 1, 3), (0, 1)
DECODE = [
    case("decode", 2, 1, 256, 4, 4, 128, kernels=K013), case("decode", 1, 2, 257, 8, 1, 128, True, kernels=K013),
    case("decode", 1, 1, 320, 17, 1, 128, True, kernels=K013), case("decode", 1, 8, 1024, 12, 2, 128, True, kernels=K013),
    case("decode", 1, 4, 1025, 7, 1, 128, True, kernels=K01), case("decode", 2, 1, 320, 28, 4, 128, kernels=K013),
    case("decode", 7, 2, 320, 4, 2, 128, True, [320, 300, 64, 9, 2, 1, 0], kernels=K013, edges=Z),
    case("decode", 7, 2, 320, 4, 2, 128, False, [320, 300, 64, 9, 2, 1, 0], kernels=K013, edges=Z),
    case("decode", 2, 2, 257, 4, 2, 48, True, kernels=K01), case("decode", 1, 8, 320, 12, 2, 64, kernels=K01),
    case("decode", 3, 1, 256, 4, 4, 80, False, [256, 64, 0], kernels=K01, edges=Z), case("decode", 1, 4, 1025, 7, 1, 80, True, kernels=K01),
    case("decode", 2, 4, 1024, 4, 1, 64, True, [1024, 3], kernels=K01, edges=Z), case("decode", 1, 1, 1024, 17, 1, 48, kernels=K01),
    # rope + append (8-wave kernel only): G * Lq 16 and 28, every k_len >= Lq
    case("decode", 3, 1, 320, 16, 1, 128, True, [320, 300, 1], kernels=(0,), rope=True),
    case("decode", 3, 4, 320, 14, 2, 128, True, [320, 131, 4], kernels=(0,), rope=True),
    case("decode", 1, 4, 256, 14, 2, 128, True, kernels=(0,), rope=True),
]
# ---- wide: attn_fwd_wide_kernel<D, 4> (32 rows per wave, 128-row tiles aligned to the END of the sequence: Lq 129 / 257 leave a first tile of one row)
K20 = (2, 0)
WIDE = [
    case("wide", 1, 128, 128, 2, 2, 64, kernels=K20), case("wide", 1, 129, 128, 2, 1, 80, kernels=K20), case("wide", 1, 160, 193, 2, 2, 128, kernels=K20),
    case("wide", 2, 257, 257, 2, 1, 64, kernels=K20, layout="strided", scale=0.3), case("wide", 1, 128, 321, 2, 2, 80, kernels=K20),
    case("wide", 1, 128, 321, 2, 1, 128, True, kernels=K20), case("wide", 1, 128, 128, 2, 2, 80, True, kernels=K20),
    case("wide", 1, 129, 128, 2, 2, 128, True, kernels=K20, edges=Z), case("wide", 1, 257, 257, 2, 2, 64, True, kernels=K20, layout="strided"),
    case("wide", 1, 193, 160, 2, 2, 64, True, kernels=K20, scale=0.3, edges=Z),
    case("wide", 1, 160, 193, 2, 2, 64, kv_start=5, kernels=K20), case("wide", 1, 160, 193, 2, 2, 80, kv_start=64, kernels=K20),
    case("wide", 1, 160, 193, 2, 2, 128, kv_start=70, kernels=K20), case("wide", 1, 160, 193, 2, 2, 64, True, kv_start=70, kernels=K20, edges=Z),
    case("wide", 4, 128, 193, 2, 2, 128, False, [193, 131, 40, 0], kernels=K20, edges=Z),
    case("wide", 4, 128, 193, 2, 1, 80, True, [193, 131, 40, 0], kernels=K20, edges=Z),
    case("wide", 4, 129, 128, 4, 2, 64, False, [128, 40], kv_bdiv=2, kernels=K20),
    case("wide", 5, 300, 300, 2, 2, 80, lens_q=[300, 128, 1, 0, 131], layout="varlen", kernels=K20),
    case("wide", 5, 300, 300, 2, 1, 128, True, lens_q=[300, 128, 1, 0, 131], layout="varlen", kernels=K20),
    # deferred running maximum: one row's block maxima grow by 4, 4 (skipped, then taken: 8 above the kept maximum) and 10 / by 5.5, 3 and 7 (exp2 domain)
    case("wide", 1, 128, 321, 2, 2, 64, kernels=K20, ramp=(4, 4, 10)), case("wide", 1, 257, 257, 2, 2, 128, True, kernels=K20, ramp=(5.5, 3, 7)),
]
# ---- window: the packed d-80 sequences of <= 64 tokens (attn_fwd_wide_kernel<80, 2, 1> for kernel 0 / 2, the 16-row kernel for kernel 1)
WINDOW = [case("window", 5, 64, 64, 2, 2, 80, lens_q=[64, 1, 33, 64, 16], layout="varlen", kernels=(0, 1, 2)),
          case("window", 4, 64, 64, 4, 4, 80, lens_q=[16, 64, 0, 17], layout="varlen", kernels=(0, 1, 2))]
GROUPS = {"row16": ROW16, "dropout": DROPOUT, "decode": DECODE, "wide": WIDE, "window": WINDOW}
ALL = [c for g in GROUPS.values() for c in g]
assert len({c["name"] for c in ALL}) == len(ALL)
RAMP_BASE = 16.0     # exp2-domain logit of the first ramp key: above what the random and the planted keys give the ramp query


def mid_query(Lq):
    """a query in the middle of a 16-row tile (row 7 of one) whose diagonal is planted in causal cases; None below 3 queries."""
    cands = [x for x in range(Lq - 2) if x % 16 == 7]
    return cands[len(cands) // 2] if cands else (Lq - 3 if Lq >= 3 else None)


def ramp_query(c):
    return c["dims"][1] - 20


def make_inputs(c):
    """seeded bf16 CPU tensors as the launcher receives them: q [B, Lq, H, D], k / v [B / kv_bdiv, Lk, Hkv, D] (varlen: packed [T, H, D] / [Tk, Hkv, D]
    with int32 cu_q / cu_k), k_len (int32 or None), gate (f32 [H] or None), base (bf16 like the output, or None), rope tables and new tokens.
    Planted edges, in the even kv heads of every sequence with at least one query: the last allowed key len_k - 1 and the first masked key len_k are 3 * q[last query] of
    the kv group's first head; so are the keys kv_start - 1 and kv_start; causal cases repeat it at the diagonal (key qm + len_k - len_q and the
    one after it) of the mid-tile query qm = mid_query(len_q). A mask that is off by one key moves the result by thousands of bounds.
    Rope cases plant in the rotated frame: k_new = 3 * q of the same token (the rotation is orthogonal), key len_k = 3 * rotate(q)[last].
    Ramp cases: for query ramp_query(c) of head 0, key 10 of each 64-key block is a multiple of q that puts its exp2-domain logit at
    RAMP_BASE + the running sum of c["ramp"]."""
    B, Lq, Lk, H, Hkv, D = c["dims"]
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()))
    Bk, G = B // c["kv_bdiv"], H // Hkv
    rnd = lambda *s: torch.randn(s, generator=g).to(BF16)                       # noqa: E731
    out = dict(k_len=None if c["k_len"] is None else torch.tensor(c["k_len"], dtype=torch.int32), gate=None, base=None, cu_q=None, cu_k=None)
    if c["gate"]:
        out["gate"] = torch.randn(H, generator=g)
    if c["lens_q"] is not None:
        lq, lk = torch.tensor(c["lens_q"]), torch.tensor(c["lens_k"])
        cu_q, cu_k = (torch.cat([torch.zeros(1, dtype=torch.int64), t.cumsum(0)]) for t in (lq, lk))
        q, k, v = rnd(int(cu_q[-1]), H, D), rnd(int(cu_k[-1]), Hkv, D), rnd(int(cu_k[-1]), Hkv, D)
        qrow = lambda b, i: q[int(cu_q[b]) + i]                                  # noqa: E731
        krow = lambda kb, j: k[int(cu_k[kb]) + j]                                # noqa: E731
        out.update(cu_q=cu_q.to(torch.int32), cu_k=cu_k.to(torch.int32))
        lens = [(int(lq[b]), int(lk[b]), int(lk[b])) for b in range(B)]          # (len_q, len_k, rows that exist)
    else:
        q, k, v = rnd(B, Lq, H, D), rnd(Bk, Lk, Hkv, D), rnd(Bk, Lk, Hkv, D)
        qrow = lambda b, i: q[b, i]                                              # noqa: E731
        krow = lambda kb, j: k[kb, j]                                            # noqa: E731
        lens = [(Lq, Lk if out["k_len"] is None else min(int(out["k_len"][kb]), Lk), Lk) for kb in range(Bk)]
    if c["acc"]:
        out["base"] = rnd(B, Lq, H, D)
    if c["rope"]:
        ang = torch.rand(B * Lq, D // 2, generator=g) * 6.28
        out["cos"], out["sin"] = torch.cat([ang.cos(), ang.cos()], 1).contiguous(), torch.cat([ang.sin(), ang.sin()], 1).contiguous()
        out["k_new"] = (3.0 * q[:, :, ::G].float()).to(BF16)
        out["v_new"] = rnd(B, Lq, Hkv, D)
        qrot = rope_rotate(q, out["cos"].view(B, Lq, 1, D), out["sin"].view(B, Lq, 1, D))
    plant = lambda b, i: (3.0 * qrow(b, i)[::G].float()).to(BF16)                # noqa: E731

    def kset(kb, j, val):               # the even kv heads only: the odd ones keep a spread softmax at every edge
        krow(kb, j)[0::2] = val[0::2]
    for kb, (n_q, n_k, rows) in enumerate(lens):
        b = kb * c["kv_bdiv"]
        if n_q == 0:
            continue
        if c["rope"]:
            if n_k < rows:
                kset(kb, n_k, (3.0 * qrot[b, -1, ::G].float()).to(BF16))
            continue
        qm = mid_query(n_q) if c["causal"] else None
        if qm is not None:
            for key in (qm + n_k - n_q, qm + n_k - n_q + 1):
                if 0 <= key < rows:
                    kset(kb, key, plant(b, qm))
        for key in (n_k - 1, n_k) + ((c["kv_start"] - 1, c["kv_start"]) if c["kv_start"] else ()):
            if 0 <= key < rows:
                kset(kb, key, plant(b, n_q - 1))
    if c["ramp"]:
        qr = q[0, ramp_query(c), 0].float()
        level, sc2 = RAMP_BASE, f32(c["scale"]) * 1.4426950408889634
        for blk, step in enumerate((0,) + tuple(c["ramp"])):
            level += step
            k[0, blk * 64 + 10, 0] = (qr * (level / (sc2 * float(qr @ qr)))).to(BF16)
    out.update(q=q, k=k, v=v)
    return out


_CACHE = {}


def case_reference(c, salt=0):
    """(inputs, ref, bound) of a case, computed once per process and never modified (dense [B, Lq, H, D]; `pack` for varlen rows)."""
    key = (c["name"], salt)
    if key not in _CACHE:
        inp = _CACHE[(c["name"], 0)][0] if (c["name"], 0) in _CACHE else make_inputs(c)
        _CACHE[key] = (inp,) + reference(c, inp, salt=salt)
    return _CACHE[key]
