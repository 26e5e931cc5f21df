"""TEST INFRASTRUCTURE: float64 restatement of the attention backward (internnav_amd/csrc/attention_bwd.hip), its error-bound model, a float32 /
bf16 emulation of the kernel's rounding points, and the case table shared by tests/test_attn_bwd_ref_cpu.py and
tests/test_attention_bwd_fp64_gpu.py. Plain torch on the CPU; nothing of internnav_amd is imported.

The function restated is  (dq, dk, dv) = f(q, k, v, o, do; scale, causal, k_len, kv_row0, kv_bdiv, dropout mask)  as the kernel defines it:
  * delta = rowsum(dO * O) of the GIVEN bf16 o (never recomputed);
  * len_k = min(k_len[b // kv_bdiv], Lk); causal: key k allowed for query q iff k <= q + (len_k - Lq);
  * P = softmax over the allowed keys, a row without an allowed key is all zero; dP = dO V^T;
  * dS = P * (dP * m - delta) * scale, dV uses P * m; m = keep / (1 - p) from the host replica of ina_hash at the index
    ((b*H + h)*Lq + q)*Lk + k with the FULL Lk;
  * dk / dv per QUERY head [B, rows, H, D], row r = key row0 + r, row0 = kv_row0 or max(0, len_k - Lq) for kv_row0 = -1 (rows = min(Lq, Lk));
    rows of keys at or past len_k are zero.

Bound (per element, all-or-nothing; derived from the number formats, nothing in it comes from a kernel's output). The kernel rounds P and dS to
bf16 once, just before the second MFMA, and the result to bf16; everything else is fp32. With u8 = 2^-8, u24 = 2^-24, f = 16 * u24 * (sqrt(D) + 4)
(the project's fp32 model, test_s1_head_ops_gpu.py) and A the float64 sum of |terms| of the output's own contraction
(dq: sum_k |dS| |K|, dk: sum_q |dS| |Q|, dv: sum_q |P m| |dO|):
    bound = u8 * (A + |ref|) * (1 + 2^-6)  +  f * C  +  E_S
  * first term: rounding of the MFMA operand + rounding of the stored result, 2^-6 of head-room for their product;
  * C: the same contraction with P * scale * (sum_d |dO||V| + sum_d |dO||O|) in place of |dS| - the un-cancelled magnitude of dP - delta, which
    cancels to exactly 0 in float64 on a row whose weight sits on one key (C = A for dv);
  * E_S: the fp32 error of the logits carried into P: the contraction's |terms|, each weighted f * scale * sum_d |q||k|.
Where ref == 0 and A == 0 (masked rows, padded rows) the bound is 0 and the check is `== 0`.
"""
from __future__ import annotations

import math
import zlib

import numpy as np
import torch

U8 = 2.0 ** -8
U24 = 2.0 ** -24
F64 = torch.float64
BF16 = torch.bfloat16
MUTATIONS = ("mask_long", "mask_short", "diag_plus", "diag_minus", "shift_Lk", "no_scale", "delta_f64", "dv_no_dropscale", "drop_idx_lenk",
             "kv_head_mod", "no_bdiv")


def f32(v: float) -> float:
    """a Python float as the kernel receives it (c_float argument)."""
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------------------ dropout mask
def _fmix32(h):
    M = 0xFFFFFFFF
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & M
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & M
    return h ^ (h >> 16)


def _keep_mask(seed, idx, p):
    """host replica of ina_hash (csrc/common.h) on int64 tensors: keep iff hash(seed, idx) >= p * 2^32."""
    M = 0xFFFFFFFF
    lo, hi = idx & M, idx >> 32
    h = _fmix32((_fmix32(torch.full_like(lo, seed)) + 0x9E3779B9 * lo) & M)
    h = _fmix32((h + 0x9E3779B9 * hi + 0x7F4A7C15) & M)
    return h >= max(1, int(p * 4294967296.0))


def drop_keep(B, H, Lq, Lk, p, seed, lk_index=None):
    """bool [B, H, Lq, Lk]: kept probabilities. lk_index (int64 [B]) replaces Lk in the index (a mutation)."""
    ar = lambda n, *shape: torch.arange(n, dtype=torch.int64).view(*shape)      # noqa: E731
    lk = torch.full((B,), Lk, dtype=torch.int64) if lk_index is None else lk_index.to(torch.int64)
    idx = ((ar(B, B, 1, 1, 1) * H + ar(H, 1, H, 1, 1)) * Lq + ar(Lq, 1, 1, Lq, 1)) * lk.view(B, 1, 1, 1) + ar(Lk, 1, 1, 1, Lk)
    return _keep_mask(seed & 0xFFFFFFFF, idx, p)


# ------------------------------------------------------------------------------------------------------------ the restatement
def _setup(q, k, k_len, kv_bdiv, causal, mut):
    B, Lq, H, D = q.shape
    Bk, Lk, Hkv, _ = k.shape
    G = H // Hkv
    bi = torch.arange(B) // kv_bdiv
    if mut == "no_bdiv":
        bi = torch.arange(B) % Bk
    hi = torch.arange(H) // G
    if mut == "kv_head_mod":
        hi = torch.arange(H) % Hkv
    len_k = torch.full((B,), Lk, dtype=torch.int64) if k_len is None else k_len.to(torch.int64)[bi].clamp(max=Lk)
    ak, aq = torch.arange(Lk).view(1, 1, Lk), torch.arange(Lq).view(1, Lq, 1)
    lim = len_k + (1 if mut == "mask_long" else -1 if mut == "mask_short" else 0)
    allowed = (ak < lim.view(B, 1, 1)).expand(B, Lq, Lk)
    if causal:
        shift = (torch.full_like(len_k, Lk) if mut == "shift_Lk" else len_k) - Lq
        shift = shift + (1 if mut == "diag_plus" else -1 if mut == "diag_minus" else 0)
        allowed = allowed & (ak <= aq + shift.view(B, 1, 1))
    return bi, hi, len_k, allowed[:, None]        # allowed: bool [B, 1, Lq, Lk]


def _softmax(s, allowed):
    """softmax over the allowed keys; all zero where there is none."""
    s = s.masked_fill(~allowed, float("-inf"))
    mx = s.amax(-1, keepdim=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = torch.exp(s - mx)
    den = e.sum(-1, keepdim=True)
    return e / torch.where(den > 0, den, torch.ones_like(den))


def _m(B, H, Lq, Lk, drop, len_k, mut, dtype):
    """(m for dS, m for dV) or (None, None)"""
    if drop is None:
        return None, None
    p, seed = drop
    keep = drop_keep(B, H, Lq, Lk, p, seed, len_k if mut == "drop_idx_lenk" else None).to(dtype)
    m = keep * f32(1.0 / (1.0 - p))
    return m, (keep if mut == "dv_no_dropscale" else m)


def forward_o64(q, k, v, *, scale, causal=False, k_len=None, kv_bdiv=1, drop=None):
    """o = (softmax * m) v in float64, unrounded: [B, Lq, H, D]."""
    B, Lq, H, D = q.shape
    Lk = k.shape[1]
    bi, hi, len_k, allowed = _setup(q, k, k_len, kv_bdiv, causal, None)
    q, kk, vv = q.to(F64), k.to(F64)[bi][:, :, hi], v.to(F64)[bi][:, :, hi]
    P = _softmax(torch.einsum("bqhd,bkhd->bhqk", q, kk) * f32(scale), allowed)
    m, _ = _m(B, H, Lq, Lk, drop, len_k, None, F64)
    return torch.einsum("bhqk,bkhd->bqhd", P if m is None else P * m, vv)


def forward_o(q, k, v, **kw):
    """the o handed to the backward when it is not to come from the forward kernel: float64, rounded once to bf16."""
    return forward_o64(q, k, v, **kw).to(BF16).contiguous()


def select_rows(full, len_k, kv_row0, Lq):
    """[B, Lk, H, D] per key -> the op's [B, rows, H, D]; rows of keys at or past len_k are zero."""
    B, Lk = full.shape[:2]
    if kv_row0 >= 0:
        out = full[:, kv_row0:].clone()
        row0 = torch.full((B,), kv_row0, dtype=torch.int64)
    else:
        rows = min(Lq, Lk)
        row0 = (len_k - Lq).clamp(min=0)
        out = torch.stack([full[b, int(row0[b]):int(row0[b]) + rows] for b in range(B)])
    key = row0.view(B, 1) + torch.arange(out.shape[1]).view(1, -1)
    out[key >= len_k.view(B, 1)] = 0
    return out


def reference(q, k, v, o, do, *, scale, causal=False, k_len=None, kv_row0=0, kv_bdiv=1, drop=None, mut=None, bounds=True):
    """{"dq": (ref, bound), "dk": ..., "dv": ...} in float64 (bound None with bounds=False). drop = (p, seed + salt)."""
    B, Lq, H, D = q.shape
    Lk = k.shape[1]
    sc = f32(scale)
    bi, hi, len_k, allowed = _setup(q, k, k_len, kv_bdiv, causal, mut)
    q64, do64 = q.to(F64), do.to(F64)
    kk, vv = k.to(F64)[bi][:, :, hi], v.to(F64)[bi][:, :, hi]
    o64 = forward_o64(q, k, v, scale=scale, causal=causal, k_len=k_len, kv_bdiv=kv_bdiv, drop=drop) if mut == "delta_f64" else o.to(F64)
    P = _softmax(torch.einsum("bqhd,bkhd->bhqk", q64, kk) * sc, allowed)
    m, mv = _m(B, H, Lq, Lk, drop, len_k, mut, F64)
    Pv = P if mv is None else P * mv
    dP = torch.einsum("bqhd,bkhd->bhqk", do64, vv)
    delta = (do64 * o64).sum(-1).permute(0, 2, 1)[..., None]                 # [B, H, Lq, 1]
    dS = P * ((dP if m is None else dP * m) - delta) * (1.0 if mut == "no_scale" else sc)
    to_q, to_k = "bhqk,bkhd->bqhd", "bhqk,bqhd->bkhd"
    sel = lambda t: select_rows(t, len_k, kv_row0, Lq)                        # noqa: E731
    ref = {"dq": torch.einsum(to_q, dS, kk), "dk": sel(torch.einsum(to_k, dS, q64)), "dv": sel(torch.einsum(to_k, Pv, do64))}
    if not bounds:
        return {n: (r, None) for n, r in ref.items()}
    f = 16.0 * U24 * (math.sqrt(D) + 4.0)
    aq, ak, ado = q64.abs(), kk.abs(), do64.abs()
    W = P * sc * (torch.einsum("bqhd,bkhd->bhqk", ado, vv.abs()) + (ado * o64.abs()).sum(-1).permute(0, 2, 1)[..., None])
    T = torch.einsum("bqhd,bkhd->bhqk", aq, ak) * sc
    adS, aPv = dS.abs(), Pv.abs()
    A = {"dq": torch.einsum(to_q, adS, ak), "dk": sel(torch.einsum(to_k, adS, aq)), "dv": sel(torch.einsum(to_k, aPv, ado))}
    Cc = {"dq": torch.einsum(to_q, W, ak), "dk": sel(torch.einsum(to_k, W, aq)), "dv": A["dv"]}
    ES = {"dq": f * torch.einsum(to_q, adS * T, ak), "dk": f * sel(torch.einsum(to_k, adS * T, aq)), "dv": f * sel(torch.einsum(to_k, aPv * T, ado))}
    return {n: (ref[n], U8 * (A[n] + ref[n].abs()) * (1.0 + 2.0 ** -6) + f * Cc[n] + ES[n]) for n in ref}


def emulate(q, k, v, o, do, *, scale, causal=False, k_len=None, kv_row0=0, kv_bdiv=1, drop=None):
    """the kernel's arithmetic on the CPU: fp32 everywhere, P and dS rounded to bf16 before the second product, bf16 results."""
    F32 = torch.float32
    B, Lq, H, D = q.shape
    Lk = k.shape[1]
    sc = f32(scale)
    bi, hi, len_k, allowed = _setup(q, k, k_len, kv_bdiv, causal, None)
    qf, dof, of = q.to(F32), do.to(F32), o.to(F32)
    kk, vv = k.to(F32)[bi][:, :, hi], v.to(F32)[bi][:, :, hi]
    P = _softmax(torch.einsum("bqhd,bkhd->bhqk", qf, kk) * sc, allowed)
    m, _ = _m(B, H, Lq, Lk, drop, len_k, None, F32)
    dP = torch.einsum("bqhd,bkhd->bhqk", dof, vv)
    delta = (dof * of).sum(-1).permute(0, 2, 1)[..., None]
    dS = (P * ((dP if m is None else dP * m) - delta) * sc).to(BF16).to(F32)
    Pv = (P if m is None else P * m).to(BF16).to(F32)
    sel = lambda t: select_rows(t, len_k, kv_row0, Lq)                        # noqa: E731
    return {"dq": torch.einsum("bhqk,bkhd->bqhd", dS, kk).to(BF16), "dk": sel(torch.einsum("bhqk,bqhd->bkhd", dS, qf)).to(BF16),
            "dv": sel(torch.einsum("bhqk,bqhd->bkhd", Pv, dof)).to(BF16)}


def ratio(out, ref, bound):
    """(worst |err| / bound over the elements with bound > 0, every element inside its bound - `== 0` where the bound is 0, NaN never)."""
    err = (out.to(F64) - ref).abs()
    ok = bool((err <= bound).all())               # NaN compares false
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    return (worst if worst == worst else float("inf")), ok


# ------------------------------------------------------------------------------------------------------------ cases
def case(group, B, Lq, Lk, H, Hkv, D, causal=False, k_len=None, kv_row0=0, kv_bdiv=1, nsplit=1, drop=None, scale=None, layout="plain"):
    name = f"{group}-{B}x{Lq}x{Lk}x{H}x{Hkv}x{D}" + ("-causal" if causal else "") + (f"-klen{'_'.join(map(str, k_len))}" if k_len else "") \
        + (f"-row{kv_row0}" if kv_row0 else "") + (f"-bdiv{kv_bdiv}" if kv_bdiv > 1 else "") + (f"-nsplit{nsplit}" if nsplit != 1 else "") \
        + (f"-p{drop[0]}" if drop else "") + (f"-scale{scale}" if scale else "") + (f"-{layout}" if layout != "plain" else "")
    return dict(name=name, group=group, dims=(B, Lq, Lk, H, Hkv, D), causal=causal, k_len=k_len, kv_row0=kv_row0, kv_bdiv=kv_bdiv, nsplit=nsplit,
                drop=drop, scale=scale if scale else D ** -0.5, layout=layout)


# scale 0.3 goes to one case per group with D <= 72: the planted logit 3 |q|^2 scale stays below 70, so every probability that a float64
# reference keeps stays a normal fp32 number (at D 128 it would be exp(-115))
DENSE = [case("dense", 2, 33, 65, 2, 2, 64), case("dense", 1, 65, 64, 2, 2, 40, scale=0.3), case("dense", 2, 1, 1, 2, 2, 8),
         case("dense", 1, 32, 129, 3, 3, 72), case("dense", 1, 17, 63, 2, 1, 120), case("dense", 1, 16, 32, 2, 2, 128)]
CAUSAL = [case("causal", 1, 65, 65, 2, 2, 64, True), case("causal", 1, 200, 200, 2, 2, 64, True), case("causal", 2, 4, 130, 4, 2, 128, True),
          case("causal", 1, 70, 40, 2, 2, 48, True, scale=0.3), case("causal", 1, 33, 97, 2, 1, 128, True)]
RAGGED_LAST = [case("ragged_last", 3, 4, 200, 4, 2, 128, True, [200, 131, 64], -1, layout="llm"),
               case("ragged_last", 2, 33, 130, 2, 1, 64, True, [130, 33], -1, layout="llm", scale=0.3),
               case("ragged_last", 2, 8, 40, 2, 2, 64, True, [40, 5], -1, layout="llm")]
RAGGED_ROW0 = [case("ragged_row0", 3, 20, 70, 2, 2, 64, True, [70, 37, 0]), case("ragged_row0", 3, 20, 70, 2, 2, 64, False, [70, 37, 0], scale=0.3),
               case("ragged_row0", 3, 20, 70, 2, 2, 64, True, [70, 37, 0], 40), case("ragged_row0", 3, 20, 70, 2, 2, 64, False, [70, 37, 0], 40)]
SPLITS = [case("splits", 2, 4, 200, 4, 2, 128, True, nsplit=3), case("splits", 2, 4, 200, 4, 2, 128, True, nsplit=4),
          case("splits", 2, 4, 200, 4, 2, 128, True, [200, 70], nsplit=2), case("splits", 1, 32, 130, 2, 2, 64, False, nsplit=2, scale=0.3),
          case("splits", 1, 70, 200, 2, 1, 64, True, nsplit=2), case("splits", 1, 4, 520, 2, 1, 128, True, nsplit=None)]
DROPOUT = [case("dropout", 2, 33, 65, 2, 2, 48, True, drop=(0.1, 777), scale=0.3), case("dropout", 1, 4, 70, 4, 2, 128, False, [50], drop=(0.25, 4242))]
LAYOUT = [case("layout", 2, 65, 65, 2, 2, 40, layout="packed3"), case("layout", 4, 8, 40, 2, 2, 64, kv_bdiv=2, scale=0.3),
          case("layout", 4, 8, 40, 2, 2, 64, True, [40, 23], kv_bdiv=2)]
# o from the forward kernel: one more case per group (never k_len 0 or a fully masked query row: those belong to the forward kernel's own suite)
FWD_O = [case("dense", 2, 33, 65, 4, 2, 64), case("causal", 2, 65, 65, 2, 2, 64, True), case("ragged_last", 2, 4, 200, 4, 2, 128, True, [200, 131], -1, layout="llm"),
         case("ragged_row0", 3, 20, 70, 2, 2, 64, False, [70, 37, 9]), case("splits", 1, 4, 200, 4, 2, 128, True, nsplit=2),
         case("dropout", 2, 33, 65, 2, 2, 48, True, drop=(0.1, 99)), case("layout", 4, 8, 40, 2, 2, 64, kv_bdiv=2)]
for _c in FWD_O:
    _c["name"] += "-fwd_o"
GROUPS = {"dense": DENSE, "causal": CAUSAL, "ragged_last": RAGGED_LAST, "ragged_row0": RAGGED_ROW0, "splits": SPLITS, "dropout": DROPOUT,
          "layout": LAYOUT}
ALL = [c for g in GROUPS.values() for c in g]
# the long-prefix shape of the automatic split (emulation only: 2100 keys)
LONG = case("long", 2, 4, 2100, 4, 2, 128, True, [2100, 1999])
SALT = 12345         # the device word of the salted dropout runs


def mid_query(Lq):
    """a query in the middle of a 16-row tile (row 7 of one) whose diagonal is planted in causal cases; None below 3 queries."""
    cands = [x for x in range(Lq - 2) if x % 16 == 7]
    return cands[len(cands) // 2] if cands else (Lq - 3 if Lq >= 3 else None)


def make_inputs(c):
    """seeded bf16 CPU tensors q [B,Lq,H,D], k / v [B / kv_bdiv, Lk, Hkv, D], do, k_len (int32 or None), with the planted edges: in every sequence
    the last allowed key len_k - 1 and the first masked key len_k (where they exist) are 3 * q[b, -1] of the kv group's first head; causal
    cases repeat that at the diagonal (key qm + len_k - Lq and the one after it) of the query qm = mid_query(Lq)."""
    B, Lq, Lk, H, Hkv, D = c["dims"]
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()))
    Bk, G = B // c["kv_bdiv"], H // Hkv
    q, k, v, do = (torch.randn(s, generator=g).to(BF16) for s in ((B, Lq, H, D), (Bk, Lk, Hkv, D), (Bk, Lk, Hkv, D), (B, Lq, H, D)))
    k_len = None if c["k_len"] is None else torch.tensor(c["k_len"], dtype=torch.int32)
    for kb in range(Bk):
        b = kb * c["kv_bdiv"]
        len_k = Lk if k_len is None else min(int(k_len[kb]), Lk)
        qm = mid_query(Lq) if c["causal"] else None
        if qm is not None:
            for key in (qm + len_k - Lq, qm + len_k - Lq + 1):
                if 0 <= key < Lk:
                    k[kb, key] = (3.0 * q[b, qm, ::G].float()).to(BF16)
        for key in (len_k - 1, len_k):
            if 0 <= key < Lk:
                k[kb, key] = (3.0 * q[b, -1, ::G].float()).to(BF16)
    return dict(q=q, k=k, v=v, do=do, k_len=k_len)


def ref_kwargs(c, salt=0):
    d = None if c["drop"] is None else (c["drop"][0], c["drop"][1] + salt)
    return dict(scale=c["scale"], causal=c["causal"], k_len=None, kv_row0=c["kv_row0"], kv_bdiv=c["kv_bdiv"], drop=d)


def case_reference(c, inp=None, o=None, salt=0, **kw):
    """(inputs, o, reference dict) of a case; o defaults to forward_o of the inputs."""
    inp = make_inputs(c) if inp is None else inp
    a = ref_kwargs(c, salt)
    a["k_len"] = inp["k_len"]
    if o is None:
        o = forward_o(inp["q"], inp["k"], inp["v"], **{n: a[n] for n in ("scale", "causal", "k_len", "kv_bdiv", "drop")})
    a.update(kw)
    return inp, o, reference(inp["q"], inp["k"], inp["v"], o, inp["do"], **a)
