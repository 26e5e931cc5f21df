"""TEST INFRASTRUCTURE: float64 restatement of the NextDiT block kernels (internnav_amd/csrc/dit_attention.hip: dit_attn_kernel<6>,
dit_attn_stats_kernel<6, KT>, dit_v2t_kernel; internnav_amd/csrc/dit_rowchain.hip: the four dit_rowchain_kernel instances), their error-bound
models, a float32 / bf16 emulation of the kernels' rounding points, and the case tables shared by tests/test_dit_block_ref_cpu.py and
tests/test_dit_block_fp64_gpu.py. Plain torch on the CPU; nothing of internnav_amd is imported.

Every bound is per element, all-or-nothing, limit 1.0, and derived from the number formats and the kernels' rounding points; nothing in it
comes from a kernel's output. u8 = 2^-8 (bf16 rounding), u24 = 2^-24, f(n) = 16 u24 (sqrt(n) + 4) the project's fp32 model of an n-term
accumulation (tests/attn_fwd_ref.py).

ATTENTION   out = SDPA(LN(q1), LN(k1), v1) + tanh(gate[h]) * SDPA(LN(q2), K2[env], V2[env]),  env = seq // S, LN across the 384-wide segment.
  * LayerNorm value y = (x - mean) rstd g + b, rounded to bf16 by the kernel:
        dy = u8 |y| + |c g| rho + dm rstd |g| + 4 u24 (|c g| + |b|),   c = (x - mean) rstd
    with the statistics term (rho relative on rstd, dm absolute on mean):
      - self-computed (dit_attn_kernel: fp32 sums of x and x^2 on the matrix cores, var = E[x^2] - mean^2): the cancellation makes the fp32 error
        of E[x^2] relative to var: rho = f(384) E[x^2] / (var + eps) + 4 u24 (rsqrtf), dm = f(384) E|x|;
      - handed over (dit_attn_stats_kernel): the reference normalises with the SAME (mean, rstd) pairs it is given, so rho = dm = 0; a caller that
        compares against the exact statistics instead passes how far its pairs are from them (`stat_err`, the hand-over test);
  * logits s_j = scale sum_d q_d k_jd with fp32 accumulation over 64: ds_j = scale sum_d (dq |k| + |q| dk + dq dk) + f(64) scale sum_d |q| |k|
    (dk = 0 for the condition keys, which are inputs); the exponent's argument is rounded at magnitude |s_j| + |M| and exp2 is good to a few ulp:
    eps_j = ds_j + 4 u24 (|s_j| + |M| + 8); e_j is then off by the factor expm1(eps_j) =: r_j at most, in the numerator and in the row sum:
        E_S = (sum_j P_j r_j |v_jd| + |o| sum_j P_j r_j) / (1 - sum_j P_j r_j)
  * P is rounded to bf16 before each P V MFMA (u8 A, A = sum_j P_j |v_jd|) while the row sum keeps the un-rounded e_j; accumulation, 1 / l, tanhf
    and the add in fp32: f(keys) (A + |o|);
  * the self branch is rounded to bf16 before the add (dit_attention.hip:221 and :446): u8 (|o1| + E1); the stored sum once more: u8 (|ref| + E).
  NOT in the model because the kernels do not have it: any rounding of V (inputs), of the condition K, of the gate (fp32 tanhf is in f).

V2T   exact image V2T[env][head][d][dit_vt_pos(key)] = V[env][key][head][d], zero in the slots of keys >= Lz: bit for bit, no bound.

ROW CHAIN   staged, so that no error is counted twice.
  stage X   X = x0 + tanh(gate[b]) gamma1 P / sqrt(mean(P^2) + eps), P = a_in W1^T, b = r // mod_div, against float64 from the inputs.
        dP = f(K1) sum|a||w| + u8 (|P| + f(K1) sum|a||w|)                (fp32 accumulation, then the bf16 rounding of P)
        d(mean P^2) = mean(2 |P| dP + dP^2) + f(384) mean(P^2),  rho1 = (1 - d / (mean P^2 + eps))^-1/2 - 1 + 4 u24   (rsqrtf)
        dX = |tanh(gate) gamma1| (dP r (1 + rho1) + |P| r rho1) + 8 u24 (|term| + |x0|)      (tanhf, the two products, the add)
    and 0 for a row whose a_in is all zero: every product is 0, X = x0 bit for bit.
  stage H / C2 / seg_stats   against float64 computed from the X THE KERNEL WROTE (fp32, an exact input once stage X has passed):
        H = X r2 gamma2 (1 + mod_scale2[b]),  r2 = 1 / sqrt(mean(X^2) + eps),  rho2 = f(384) + 8 u24   (sum of squares: no cancellation)
        H stored (no W2): u8 |H| (1 + rho2) + rho2 |H|
        C2 = H W2^T: the GEMM-2 operand is rounded to bf16 once - bf16(U), U = X gamma2 (1 + mod_scale2), with r2 applied to the fp32
        accumulators, or bf16(r2 U): the same relative step either way - dC = (u8 + f(384) + rho2) sum_k |H_k| |W_k| (1 + 2^-6), stored: + u8 (|C| + dC)
        GLU: out = silu(G) U with G / U the [gate16 | up16] interleaved rows of w2: d = 1.1 dG (|U| + dU) + |silu(G)| dU + 16 u24 |out|
        (|silu'| <= 1.1; the fp32 silu), stored: + u8 (|out| + d)
        seg_stats = (mean, rsqrt(var + seg_eps)) of the UN-rounded float64 C2 row segments; the kernel takes them from its fp32 accumulators.
        A worst-case sum over the operand rounding (every H_k off by u8 in the direction that hurts) is a change of scale of the whole row by
        1 + u8, i.e. u8 on rstd: three times the 1 / 766 by which a biased and an unbiased variance differ. The operand VALUES are known,
        so here their rounding is not bounded but evaluated: C' = bf16(operand) W2^T in float64 for both places of the 1 / rms, and around each
            dmean = mean(d) + f(384) mean|C'|;  dvar = 2 sigma rms(d) + rms(d)^2 + 3 f(384) E[C'^2]   (E[x^2] - mean^2 in fp32)
            drstd = rsqrt(max(var - dvar, 0) + seg_eps) - rstd + 4 u24 rstd                          (`stats_bound`)
        with d = (f(384) + rho2) sum_k |H_k| |W_k| the fp32 part alone; bound = max over the two places of |stats(C') - stats(C)| + (dmean, drstd).
"""
from __future__ import annotations

import math
import zlib

import torch

from tests.attn_bwd_ref import U8, U24, f32, ratio  # noqa: F401  (ratio is re-exported to the two test modules)

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16
HEADS, HD, D = 6, 64, 384
LOG2E = 1.4426950408889634
ATTN_MUTATIONS = ("T_long", "T_short", "Lz_long", "Lz_short", "env_mod", "gate_no_tanh", "gate_self", "ln_per_head", "no_beta", "no_eps",
                  "q2_slot2", "no_scale", "vt_swap")
RC_MUTATIONS = ("mod_row0", "no_tanh", "no_gamma2", "ms2_no_one", "rstd2_old_x", "glu_swap", "glu_no_interleave", "var_unbiased", "seg_shift")
MUTATIONS = ATTN_MUTATIONS + RC_MUTATIONS


def fK(n):
    return 16.0 * U24 * (math.sqrt(n) + 4.0)


# ------------------------------------------------------------------------------------------------------------ V2T
def dit_vt_pos(key):
    """slot of a key inside its 32-key sub-block: MFMA k index g*8 + j <-> key (j < 4 ? g*4 + j : 16 + g*4 + (j - 4))."""
    sub, w = key >> 5, key & 31
    t, x = w >> 4, w & 15
    return (sub << 5) + ((x >> 2) << 3) + (x & 3) + (t << 2)


def v2t_ref(kv2, mut=None):
    """kv2 bf16 [envs, Lz, 2, heads, 64] -> bf16 [envs, heads, 64, 64]."""
    envs, Lz, _, H, hd = kv2.shape
    out = torch.zeros(envs, H, hd, 64, dtype=kv2.dtype)
    keys = list(range(Lz))
    if mut == "vt_swap" and Lz >= 2:
        keys[0], keys[1] = 1, 0
    out[:, :, :, [dit_vt_pos(k) for k in range(Lz)]] = kv2[:, keys, 1].permute(0, 2, 3, 1)
    return out


# ------------------------------------------------------------------------------------------------------------ attention
def stats_ref(x, eps):
    """f32 [rows, 4, 2]: float64 (mean, rstd) of the four segments of every row, rounded to fp32; the v1 pair is NaN (it must never be read)."""
    seg = x.to(F64).view(x.shape[0], 4, D)
    mean = seg.mean(-1)
    var = ((seg - mean[..., None]) ** 2).mean(-1)
    st = torch.stack([mean, (var + f32(eps)).rsqrt()], -1).to(F32)
    st[:, 2] = float("nan")
    return st.contiguous()


def _branch(q, dq, k, dk, v, sc, nkeys):
    """one SDPA in float64 with its error terms. q [n, Tq, H, 64], k / v [n, L, H, 64]; dq / dk the bounds on the operands (dk None: exact)."""
    if k.shape[1] == 0:                           # no key at all (only a mutant gets here): 0 / 0
        nan = torch.full_like(q, float("nan"))
        return nan, nan
    s = torch.einsum("nqhd,nkhd->nhqk", q, k) * sc
    ds = torch.einsum("nqhd,nkhd->nhqk", dq, k.abs())
    if dk is not None:
        ds = ds + torch.einsum("nqhd,nkhd->nhqk", q.abs() + dq, dk)
    ds = sc * ds + fK(HD) * sc * torch.einsum("nqhd,nkhd->nhqk", q.abs(), k.abs())
    M = s.amax(-1, keepdim=True)
    r = torch.expm1(ds + 4.0 * U24 * (s.abs() + M.abs() + 8.0))
    P = torch.softmax(s, -1)
    o = torch.einsum("nhqk,nkhd->nqhd", P, v)
    A = torch.einsum("nhqk,nkhd->nqhd", P, v.abs())
    EN = torch.einsum("nhqk,nkhd->nqhd", P * r, v.abs())
    EL = (P * r).sum(-1).permute(0, 2, 1)[..., None]
    E = U8 * A + fK(nkeys) * (A + o.abs()) + (EN + o.abs() * EL) / (1.0 - EL.clamp(max=0.5))
    return o, E


def attention_ref(x, norms, kv2, gate, T, S, eps, scale, stats=None, mut=None, bounds=True, stat_err=None):
    """(ref, bound) float64 [rows, 384]. x bf16 [nseq * T, 4 * 384]; norms ((g, b) of q1, k1, q2) f32; kv2 bf16 [envs, Lz, 2, 6, 64]; gate f32 [6] or
    None; stats f32 [rows, 4, 2] or None. stat_err (dm, rho) [rows, 4]: how far the statistics the KERNEL uses are from the ones the reference uses.
    The `_long` mutations add what the kernels' clamped loads would bring in: key T = a copy of key T - 1, condition key Lz = K[Lz - 1] with the
    zero V of its empty V2T slot."""
    rows = x.shape[0]
    nseq, (envs, Lz) = rows // T, kv2.shape[:2]
    eps, sc = f32(eps), (1.0 if mut == "no_scale" else f32(scale))
    xs = x.to(F64).view(nseq, T, 4, D)

    def ln(slot, ni):
        seg, (g, b) = xs[:, :, slot], (t.to(F64) for t in norms[ni])
        if mut == "no_beta":
            b = torch.zeros_like(b)
        if mut == "ln_per_head":
            s4 = seg.reshape(nseq, T, HEADS, HD)
            mean = s4.mean(-1, keepdim=True)
            var = ((s4 - mean) ** 2).mean(-1, keepdim=True)
            return ((s4 - mean) * (var + eps).rsqrt()).reshape(nseq, T, D) * g + b, torch.zeros_like(seg)
        src = 2 if (mut == "q2_slot2" and slot == 3) else slot
        if stats is not None:
            st = stats.to(F64).view(nseq, T, 4, 2)
            mean, rstd = st[:, :, src, 0], st[:, :, src, 1]
            dm, rho = torch.zeros_like(mean), torch.zeros_like(mean)
        else:
            sseg = xs[:, :, src]
            mean = sseg.mean(-1)
            var = ((sseg - mean[..., None]) ** 2).mean(-1)
            rstd = (var + (0.0 if mut == "no_eps" else eps)).rsqrt()
            dm, rho = fK(D) * sseg.abs().mean(-1), fK(D) * (sseg ** 2).mean(-1) / (var + eps) + 4.0 * U24
        if stat_err is not None:
            dm, rho = stat_err[0].to(F64).view(nseq, T, 4)[:, :, slot], stat_err[1].to(F64).view(nseq, T, 4)[:, :, slot]
        cg = (seg - mean[..., None]) * rstd[..., None] * g
        y = cg + b
        dy = U8 * y.abs() + cg.abs() * rho[..., None] + (dm * rstd)[..., None] * g.abs() + 4.0 * U24 * (cg.abs() + b.abs())
        return y, dy * (1.0 + U8)

    hv = lambda t: t.reshape(nseq, -1, HEADS, HD)                                  # noqa: E731
    (q1, dq1), (k1, dk1), (q2, dq2) = ln(0, 0), ln(1, 1), ln(3, 2)
    q1, dq1, k1, dk1, q2, dq2, v1 = (hv(t) for t in (q1, dq1, k1, dk1, q2, dq2, xs[:, :, 2]))
    if mut == "T_short":
        k1, dk1, v1 = k1[:, :T - 1], dk1[:, :T - 1], v1[:, :T - 1]
    elif mut == "T_long" and T < 32:
        k1, dk1, v1 = (torch.cat([t, t[:, -1:]], 1) for t in (k1, dk1, v1))
    o1, E1 = _branch(q1, dq1, k1, dk1, v1, sc, 32)
    env = torch.arange(nseq) % envs if mut == "env_mod" else torch.arange(nseq) // S
    k2, v2 = kv2[:, :, 0].to(F64), kv2[:, :, 1].to(F64)
    if mut == "vt_swap" and Lz >= 2:
        v2 = v2[:, [1, 0] + list(range(2, Lz))]
    if mut == "Lz_short":
        k2, v2 = k2[:, :Lz - 1], v2[:, :Lz - 1]
    elif mut == "Lz_long" and Lz < 64:
        k2, v2 = torch.cat([k2, k2[:, -1:]], 1), torch.cat([v2, torch.zeros_like(v2[:, -1:])], 1)
    o2, E2 = _branch(q2, dq2, k2[env], None, v2[env], sc, 64)
    if gate is None:
        t = torch.ones(1, 1, HEADS, 1, dtype=F64)
    else:
        t = (gate.to(F64) if mut == "gate_no_tanh" else torch.tanh(gate.to(F64))).view(1, 1, HEADS, 1)
    ref = (o1 * t if mut == "gate_self" else o1) + t * o2
    if not bounds:
        return ref.reshape(rows, D), None
    err = E1 + U8 * (o1.abs() + E1) + t.abs() * E2
    bound = err * (1.0 + U8) + (U8 + 4.0 * U24) * ref.abs()
    return ref.reshape(rows, D), bound.reshape(rows, D)


def attention_emulate(x, norms, kv2, gate, T, S, eps, scale, stats=None):
    """the kernels' arithmetic on the CPU: fp32 statistics as E[x^2] - mean^2 (or the pairs handed over), bf16 LN(q) / LN(k), fp32 logits in the
    exp2 domain, bf16 P against the un-rounded row sum, the self branch rounded to bf16 before the add, one bf16 result."""
    rows = x.shape[0]
    nseq, (envs, Lz) = rows // T, kv2.shape[:2]
    xs = x.to(F32).view(nseq, T, 4, D)
    eps32 = torch.tensor(eps, dtype=F32)

    def ln(slot, ni):
        seg, (g, b) = xs[:, :, slot], (t.to(F32) for t in norms[ni])
        if stats is not None:
            st = stats.view(nseq, T, 4, 2)
            mean, rstd = st[:, :, slot, 0], st[:, :, slot, 1]
        else:
            mean = seg.sum(-1) * f32(1.0 / D)
            var = ((seg * seg).sum(-1) * f32(1.0 / D) - mean * mean).clamp(min=0.0)
            rstd = torch.rsqrt(var + eps32)
        return ((seg - mean[..., None]) * rstd[..., None] * g + b).to(BF16).to(F32).view(nseq, T, HEADS, HD)

    sc2 = torch.tensor(f32(scale), dtype=F32) * torch.tensor(LOG2E, dtype=F32)

    def sdpa(q, k, v):
        s = torch.einsum("nqhd,nkhd->nhqk", q, k) * sc2
        e = torch.exp2(s - s.amax(-1, keepdim=True))
        return torch.einsum("nhqk,nkhd->nqhd", e.to(BF16).to(F32), v), e.sum(-1).permute(0, 2, 1)[..., None]

    n1, l1 = sdpa(ln(0, 0), ln(1, 1), xs[:, :, 2].view(nseq, T, HEADS, HD))
    o1 = (n1 * (1.0 / l1)).to(BF16).to(F32)
    env = torch.arange(nseq) // S
    n2, l2 = sdpa(ln(3, 2), kv2[:, :, 0].to(F32)[env], kv2[:, :, 1].to(F32)[env])
    w = (torch.tanh(gate.to(F32)).view(1, 1, HEADS, 1) if gate is not None else torch.ones(1, 1, HEADS, 1)) / l2
    return (o1 + n2 * w).to(BF16).reshape(rows, D)


# ------------------------------------------------------------------------------------------------------------ row chain
def stats_bound(seg, dseg, eps):
    """(mean, rstd, dmean, drstd) float64 of the last axis of `seg`, for statistics that fp32 code takes as E[x^2] - mean^2 from values within
    `dseg` of `seg`."""
    n = seg.shape[-1]
    mean = seg.mean(-1)
    var = ((seg - mean[..., None]) ** 2).mean(-1)
    msq = (seg ** 2).mean(-1)
    rms_d = (dseg ** 2).mean(-1).sqrt()
    dmean = dseg.mean(-1) + fK(n) * seg.abs().mean(-1)
    dvar = 2.0 * var.sqrt() * rms_d + rms_d ** 2 + 3.0 * fK(n) * msq
    rstd = (var + eps).rsqrt()
    drstd = ((var - dvar).clamp(min=0.0) + eps).rsqrt() - rstd + 4.0 * U24 * rstd
    return mean, rstd, dmean, drstd


def _mod_rows(c, t, M, mut):
    """per-row modulation [M, 384] (float64) of a [nb, 384] table, or None."""
    if t is None:
        return None
    b = torch.zeros(M, dtype=torch.int64) if mut == "mod_row0" else torch.arange(M) // c["mod_div"]
    return t.to(F64)[b]


def _split_glu(w2, mut):
    N2 = w2.shape[0]
    if mut == "glu_no_interleave":
        return w2[:N2 // 2], w2[N2 // 2:]
    w4 = w2.view(N2 // 32, 2, 16, D)
    wg, wu = w4[:, 0].reshape(N2 // 2, D), w4[:, 1].reshape(N2 // 2, D)
    return (wu, wg) if mut == "glu_swap" else (wg, wu)


def rowchain_ref(c, inp, x_dev=None, mut=None):
    """staged reference: {"X": (ref, bound)} from the inputs, and "H" (no W2) or "C2" (+ "seg" [M, nseg, 2]) from x_dev, the fp32 X the kernel wrote
    (None: the float64 X rounded to fp32)."""
    M, K1 = c["M"], c["K1"]
    eps, seg_eps = f32(c["eps"]), f32(c["seg_eps"])
    a, w1, x0 = inp["a_in"].to(F64), inp["w1"].to(F64), inp["x0"].to(F64)
    g1 = inp["gamma1"].to(F64)
    gate = _mod_rows(c, inp["gate"], M, mut)
    tg = torch.ones(M, D, dtype=F64) if gate is None else (gate if mut == "no_tanh" else torch.tanh(gate))
    P, AP = a @ w1.t(), a.abs() @ w1.abs().t()
    dP = fK(K1) * AP + U8 * (P.abs() + fK(K1) * AP)
    msq = (P ** 2).mean(-1, keepdim=True)
    dmsq = (2.0 * P.abs() * dP + dP ** 2).mean(-1, keepdim=True) + fK(D) * msq
    rho1 = (1.0 - (dmsq / (msq + eps)).clamp(max=0.5)) ** -0.5 - 1.0 + 4.0 * U24
    r1 = (msq + eps).rsqrt()
    term = tg * g1 * P * r1
    X = x0 + term
    dX = (tg * g1).abs() * (dP * r1 * (1.0 + rho1) + P.abs() * r1 * rho1) + 8.0 * U24 * (term.abs() + x0.abs())
    dX = torch.where(AP.sum(-1, keepdim=True) > 0, dX, torch.zeros_like(dX))
    out = {"X": (X, dX)}
    if inp["w2"] is None and not c["h"]:
        return out
    Xk = (X.to(F32) if x_dev is None else x_dev).to(F64)
    r2 = (((x0 if mut == "rstd2_old_x" else Xk) ** 2).mean(-1, keepdim=True) + eps).rsqrt()
    tab2 = torch.ones(M, D, dtype=F64) if (inp["gamma2"] is None or mut == "no_gamma2") else inp["gamma2"].to(F64).expand(M, D)
    ms = _mod_rows(c, inp["ms2"], M, mut)
    if ms is not None:
        tab2 = tab2 * (ms if mut == "ms2_no_one" else 1.0 + ms)
    H = Xk * r2 * tab2
    rho2 = fK(D) + 8.0 * U24
    bf = lambda t: t.to(F32).to(BF16).to(F64)                                      # noqa: E731
    if inp["w2"] is None:
        out["H"] = (H, U8 * H.abs() * (1.0 + rho2) + rho2 * H.abs())
        return out
    rel = (U8 + fK(D) + rho2) * (1.0 + 2.0 ** -6)
    if c["glu"]:
        wg, wu = (t.to(F64) for t in _split_glu(inp["w2"], mut))
        G, U = H @ wg.t(), H @ wu.t()
        dG, dU = rel * (H.abs() @ wg.abs().t()), rel * (H.abs() @ wu.abs().t())
        sG = G * torch.sigmoid(G)
        C = sG * U
        dC = 1.1 * dG * (U.abs() + dU) + sG.abs() * dU + 16.0 * U24 * C.abs()
    else:
        w2 = inp["w2"].to(F64)
        C = H @ w2.t()
        dC = rel * (H.abs() @ w2.abs().t())
    out["C2"] = (C, dC + U8 * (C.abs() + dC))
    if c["seg"]:
        nseg = C.shape[1] // D
        mean, rstd, _, _ = stats_bound(C.view(M, nseg, D), dC.view(M, nseg, D), seg_eps)
        dacc = ((fK(D) + rho2) * (1.0 + 2.0 ** -6) * (H.abs() @ w2.abs().t())).view(M, nseg, D)
        dmean, drstd = torch.zeros_like(mean), torch.zeros_like(rstd)
        for op in (bf(Xk * tab2) * r2, bf(H)):                       # the operand as either place of the 1 / rms rounds it
            m_o, r_o, dm_o, dr_o = stats_bound((op @ w2.t()).view(M, nseg, D), dacc, seg_eps)
            dmean, drstd = torch.maximum(dmean, (m_o - mean).abs() + dm_o), torch.maximum(drstd, (r_o - rstd).abs() + dr_o)
        if mut == "var_unbiased":
            var = ((C.view(M, nseg, D) - mean[..., None]) ** 2).sum(-1) / (D - 1)
            rstd = (var + seg_eps).rsqrt()
        ref = torch.stack([mean, rstd], -1)
        if mut == "seg_shift":                  # every pair one slot further; slot 0 keeps its NaN pre-fill
            ref = torch.cat([torch.full_like(ref[:, :1], float("nan")), ref[:, :-1]], 1)
        out["seg"] = (ref, torch.stack([dmean, drstd], -1))
    return out


def rowchain_emulate(c, inp, order="after"):
    """the kernel's arithmetic on the CPU in fp32 with its bf16 rounding points. order: where the row's 1 / rms meets GEMM 2 - "after": on the fp32
    accumulators of bf16(U) (the kernels with a second GEMM), "before": inside the operand, bf16(r2 U) (the H the no-W2 kernels store, and the
    unfused chain). Returns {"X", "H", "C2", "seg"} as the kernel would store them."""
    M = c["M"]
    eps = torch.tensor(c["eps"], dtype=F32)
    rowb = torch.arange(M) // c["mod_div"]
    bf = lambda t: t.to(BF16).to(F32)                                              # noqa: E731
    P = bf(inp["a_in"].to(F32) @ inp["w1"].to(F32).t())
    r1 = torch.rsqrt((P * P).sum(-1, keepdim=True) * f32(1.0 / D) + eps)
    tab1 = inp["gamma1"].to(F32).expand(M, D) if inp["gate"] is None else inp["gamma1"].to(F32) * torch.tanh(inp["gate"].to(F32)[rowb])
    X = P * r1 * tab1 + inp["x0"]
    out = {"X": X}
    r2 = torch.rsqrt((X * X).sum(-1, keepdim=True) * f32(1.0 / D) + eps)
    tab2 = torch.ones(M, D) if inp["gamma2"] is None else inp["gamma2"].to(F32).expand(M, D)
    if inp["ms2"] is not None:
        tab2 = tab2 * (1.0 + inp["ms2"].to(F32)[rowb])
    out["H"] = (X * r2 * tab2).to(BF16)
    if inp["w2"] is None:
        return out
    mm = (lambda w: (bf(X * tab2) @ w.to(F32).t()) * r2) if order == "after" else (lambda w: out["H"].to(F32) @ w.to(F32).t())
    if c["glu"]:
        wg, wu = _split_glu(inp["w2"], None)
        acc = torch.nn.functional.silu(mm(wg)) * mm(wu)
    else:
        acc = mm(inp["w2"])
    out["C2"] = acc.to(BF16)
    if c["seg"]:
        seg = acc.view(M, -1, D)
        mean = seg.sum(-1) * f32(1.0 / D)
        var = ((seg * seg).sum(-1) * f32(1.0 / D) - mean * mean).clamp(min=0.0)
        out["seg"] = torch.stack([mean, torch.rsqrt(var + torch.tensor(c["seg_eps"], dtype=F32))], -1)
    return out


# ------------------------------------------------------------------------------------------------------------ attention cases
def acase(T, Lz, envs=2, S=3, gate="rand"):
    """gate: "rand" | "none" | "zero" (the cross branch contributes exactly 0) | "sat" (+-20: tanh saturated)."""
    kt = (Lz + 15) // 16
    return dict(name=f"attn-T{T}-Lz{Lz}-e{envs}xS{S}-{gate}", T=T, Lz=Lz, envs=envs, S=S, gate=gate, KT=kt, eps=1e-5, scale=HD ** -0.5)


# T in {1, 2, 15, 16, 17, 31, 32} (both 16-token tiles at both ends) crossed sparsely with Lz in {1, 15, 16, 17, 32, 33, 48, 49, 63, 64}: every
# dit_attn_stats_kernel<6, KT> at its first and last Lz; every case also runs dit_attn_kernel<6>
ATTN = [
    acase(1, 1, 1, 1), acase(1, 17, 3, 1, "none"), acase(1, 64), acase(2, 15), acase(2, 33, 2, 32), acase(2, 64, 3, 1, "zero"),
    acase(15, 16), acase(15, 33, 1, 1, "sat"), acase(15, 49, 3, 1), acase(16, 17), acase(16, 32, 1, 1, "none"), acase(16, 63), acase(16, 64, 3, 1),
    acase(17, 1, 3, 1), acase(17, 15, 2, 3, "sat"), acase(17, 32), acase(17, 48, 2, 3, "zero"), acase(31, 16, 1, 1), acase(31, 33),
    acase(31, 49, 2, 3, "none"), acase(31, 63, 3, 1), acase(32, 1, 2, 3, "zero"), acase(32, 15), acase(32, 48), acase(32, 49, 1, 1),
    acase(32, 64, 2, 32), acase(32, 36, 3, 1, "sat"),
]
assert len({c["name"] for c in ATTN}) == len(ATTN)
V2T_LZ = (1, 5, 32, 33, 64)
V2T_ENVS = 44           # 44 * 6 * 4096 elements > 4096 blocks * 256 threads: the grid-stride loop takes a second trip


def plant_cols(T):
    """columns per head that the planted self key shares with its query: a logit near ln(T) + 1, i.e. a moderate weight."""
    return min(HD, 8 + int(round(8.0 * math.log(max(T, 1)))))


def make_attn_inputs(c):
    """seeded CPU tensors: x bf16 [nseq * T, 1536], norms, kv2 bf16 [envs, Lz, 2, 6, 64], gate. Planted rows:
      * the q2 segment of (sequence 0, token 0) is the constant 1.5: variance 0, its LayerNorm is beta and eps decides rstd;
      * the k1 segment of (0, token 0) and the q1 segment of (0, token T - 1) have mean 8 and unit spread (E[x^2] / var = 65);
      * in every sequence the last self key T - 1 shares plant_cols(T) columns per head with the raw q1 of query T // 2, and v1[T - 1] is offset by
        +4; in every env the last condition key Lz - 1 is a multiple of LN(q2) of the env's first sequence at query T // 2 that puts its logit at
        ln(Lz) + 1, and V2[Lz - 1] is offset by -4: a mask that is off by one key in either direction moves the result by many bounds."""
    T, Lz, envs, S = c["T"], c["Lz"], c["envs"], c["S"]
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()))
    nseq = envs * S
    x = torch.randn(nseq, T, 4, D, generator=g)
    kv2 = torch.randn(envs, Lz, 2, HEADS, HD, generator=g)
    norms = [((1.0 + 0.2 * torch.randn(D, generator=g)), 0.2 * torch.randn(D, generator=g)) for _ in range(3)]
    gate = {"rand": torch.randn(HEADS, generator=g), "none": None, "zero": torch.zeros(HEADS),
            "sat": torch.tensor([20.0, -20.0, 20.0, -20.0, 0.5, -0.5])}[c["gate"]]
    x[0, 0, 3] = 1.5
    x[0, 0, 1] += 8.0
    x[0, T - 1, 0] += 8.0
    nc = plant_cols(T)
    xh = x.view(nseq, T, 4, HEADS, HD)
    xh[:, T - 1, 1, :, :nc] = xh[:, T // 2, 0, :, :nc]
    xh[:, T - 1, 2] += 4.0
    x = x.to(BF16)
    # condition key Lz - 1 from the float64 LN(q2) of the rounded inputs
    seg = x.view(nseq, T, 4, D)[::S, T // 2, 3].to(F64)
    mean = seg.mean(-1, keepdim=True)
    y = ((seg - mean) * (((seg - mean) ** 2).mean(-1, keepdim=True) + 1e-5).rsqrt() * norms[2][0].to(F64) + norms[2][1].to(F64)).view(envs, HEADS, HD)
    alpha = (math.log(Lz) + 1.0) / (c["scale"] * (y ** 2).sum(-1, keepdim=True))
    kv2[:, Lz - 1, 0] = (alpha * y).to(F32)
    kv2[:, Lz - 1, 1] -= 4.0
    return dict(x=x.view(nseq * T, 4 * D), norms=norms, kv2=kv2.to(BF16), gate=gate)


_CACHE = {}


def attn_reference(c, with_stats):
    """(inputs, stats or None, ref, bound), computed once per process and never modified."""
    key = (c["name"], with_stats)
    if key not in _CACHE:
        inp = _CACHE[(c["name"], not with_stats)][0] if (c["name"], not with_stats) in _CACHE else make_attn_inputs(c)
        st = stats_ref(inp["x"], c["eps"]) if with_stats else None
        _CACHE[key] = (inp, st) + attention_ref(inp["x"], inp["norms"], inp["kv2"], inp["gate"], c["T"], c["S"], c["eps"], c["scale"], stats=st)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------ row-chain cases
def rcase(K1, M, mod_div, N2=0, glu=False, seg=False, gate=True, gamma2=True, ms2=True, h=False):
    assert (N2 == 0 and not glu and not seg) or (N2 % 128 == 0 and glu == (K1 == 384)) and (not seg or N2 % D == 0) and not (h and N2)
    inst = f"K{K1}-" + ("glu" if glu else "plain" if N2 else "noW2")
    name = f"rc-{inst}-M{M}-div{mod_div}" + (f"-N{N2}" if N2 else "") + ("-seg" if seg else "") + ("-h" if h else "") \
        + ("" if gate else "-nogate") + ("" if gamma2 else "-nog2") + ("" if ms2 else "-noms2")
    return dict(name=name, inst=inst, K1=K1, M=M, mod_div=mod_div, N2=N2, glu=glu, seg=seg, gate=gate, gamma2=gamma2, ms2=ms2, h=h, eps=1e-5, seg_eps=1e-5)


# the four built instances; mod_div 128: every workgroup has its own modulation row, 384: three workgroups share one
ROWCHAIN = [
    rcase(384, 128, 128, h=True), rcase(384, 384, 384), rcase(384, 256, 128, h=True, gate=False, gamma2=False), rcase(384, 384, 128, h=True, ms2=False),
    rcase(384, 128, 128, 128, True), rcase(384, 256, 128, 256, True, gate=False), rcase(384, 384, 384, 3072, True), rcase(384, 256, 384, 128, True, gamma2=False, ms2=False),
    rcase(384, 384, 128, 256, True, ms2=False),
    rcase(1024, 128, 128, h=True), rcase(1024, 384, 384, h=True, gate=False, ms2=False), rcase(1024, 256, 128, gamma2=False),
    rcase(1024, 128, 128, 128), rcase(1024, 256, 128, 384, seg=True), rcase(1024, 384, 384, 640), rcase(1024, 384, 128, 768, seg=True, gate=False),
    rcase(1024, 256, 384, 1536, seg=True, gamma2=False), rcase(1024, 128, 128, 1536, seg=True, ms2=False), rcase(1024, 384, 128, 384),
]
assert len({c["name"] for c in ROWCHAIN}) == len(ROWCHAIN)
ZERO_A, ZERO_AX, BIG_A, SMALL_A, BIG_X, SMALL_X = 3, 37, 70, 101, 12, 45      # planted rows (each in another wave of the first workgroup)
LOCAL_ROWS = (66, 5)          # row-locality launch: a_in row 66 and x0 row 5 are NaN
HANDOVER = rcase(1024, 128, 128, 1536, seg=True)
HANDOVER_T, HANDOVER_S = 32, 2                                                # 4 sequences of 32 tokens, 2 envs


def make_rowchain_inputs(c):
    """seeded CPU tensors: a_in bf16 [M, K1], w1 bf16 [384, K1], gamma1 / gamma2 f32 [384], x0 f32 [M, 384], gate / ms2 f32 [M / mod_div, 384] (or None),
    w2 bf16 [N2, 384] or None. Planted rows: a_in row ZERO_A all zero (P = 0: X unchanged); row ZERO_AX with a_in and x0 zero (X = 0: H, C2 exactly
    0); a_in rows of magnitude 1e4 / 1e-4 (P^2 far above / below eps); x0 rows of magnitude 1e4 / 1e-4."""
    M, K1, N2 = c["M"], c["K1"], c["N2"]
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()))
    nb = (M + c["mod_div"] - 1) // c["mod_div"]
    a = torch.randn(M, K1, generator=g)
    x0 = torch.randn(M, D, generator=g)
    a[ZERO_A], a[ZERO_AX], x0[ZERO_AX] = 0.0, 0.0, 0.0
    a[BIG_A] *= 1e4
    a[SMALL_A] *= 1e-4
    x0[BIG_X] *= 1e4
    x0[SMALL_X] *= 1e-4
    out = dict(a_in=a.to(BF16), x0=x0, w1=(torch.randn(D, K1, generator=g) * K1 ** -0.5).to(BF16),
               gamma1=1.0 + 0.1 * torch.randn(D, generator=g), gamma2=(1.0 + 0.1 * torch.randn(D, generator=g)) if c["gamma2"] else None,
               gate=0.5 * torch.randn(nb, D, generator=g) if c["gate"] else None, ms2=0.5 * torch.randn(nb, D, generator=g) if c["ms2"] else None,
               w2=(torch.randn(N2, D, generator=g) * D ** -0.5).to(BF16) if N2 else None)
    return out


def rowchain_inputs(c):
    if c["name"] not in _CACHE:
        _CACHE[c["name"]] = make_rowchain_inputs(c)
    return _CACHE[c["name"]]
