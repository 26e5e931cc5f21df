"""TEST INFRASTRUCTURE: float64 restatement of `ops.linear` (ina_gemm_bf16: csrc/gemm.hip, gemm_glds.hip, gemm_w4.hip, gemm_rowpanel.hip,
gemm_skinny.hip and the two epilogues of gemm_epilogue.h), its bound model, and the case tables shared by tests/test_gemm_fp64_gpu.py (the
kernels) and tests/test_gemm_ref_cpu.py (fp32 torch and the stand-in of tests/_cpu_kernels.py), written from the contract in
include/internnav_amd.h and independent of tests/_cpu_kernels.py.

`linear_ref` returns `(ref, scale)`: `ref` is the exact result for the (already bf16- / fp32-rounded) inputs in the kernels' order
    A.W^T -> +bias[n] -> act -> *colscale[n] -> *rowscale[m // div] -> +R            (GLU: act(gate + b_g) * (up + b_u) * rowscale)
and `scale` the float64 sum of the |terms| that enter each element, carried through the epilogue (an activation of slope <= LIP multiplies it
by LIP), so that a correct kernel obeys
    fp32 results: |err| <= k * 2^-24 * (sqrt(K) + 4) * scale  (+ the evaluation error of the activation, `act_err`)
    bf16 results: + 2^-8 * |ref|.
`act_err` follows tests/test_train_kernels_fp64_gpu.py: 4 x the worst |err| / (2^-24 * act scale) measured for the same `ina_act` on an MI355X
(train_ops_cases.ACT_WORST; mish: MISH_WORST below, measured by test_gemm_fp64_gpu.py::test_mish_error_table with the same grid), never looser
than 2e-6 of max|act|, and carried through the factors that follow the activation.

Exact cases: A, W, bias, R hold integers in [-4, 4], colscale / rowscale come from {0.5, 1, 2}, act is none or relu and 16 * K < 2^24, so every
partial sum of every summation order is an integer below 2^24 and the epilogue yields multiples of 1/4 below 2^19: exactly representable in
fp32. Any correct kernel - whatever its tile, split or ring depth - must then equal the reference bit for bit (fp32), or its single rounding
to bf16 (ties such as 257 included)."""
from __future__ import annotations

import math

import torch

from tests import train_ops_ref as R
from tests.train_ops_cases import ACT_WORST

U, BF, TINY = R.U, R.BF, R.TINY
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
SENT = -2.0 ** 100            # exact in bf16 and fp32, never a result
LIP = 1.13                    # largest slope of the activations below (gelu: 1.129, silu: 1.100, mish: 1.089, tanh / relu: 1)
MISH_WORST = 2.733            # worst |err| / (2^-24 * scale) of ina_act(mish), fp32 in / out, measured on an MI355X (see the GPU file's docstring)
ACT_CODE = {None: 0, "none": 0, "gelu": 1, "gelu_erf": 1, "gelu_tanh": 2, "relu": 3, "silu": 4, "mish": 5, "tanh": 6}
ACT_CAP = 2e-6                # of max|act(x)|: the whole-tensor tolerance the activation bound is never looser than

# tile geometry of the forced configs: cfg -> (BM, BN)
REG_TILES = {1: (128, 128), 2: (64, 128), 3: (64, 128), 4: (64, 64), 5: (128, 64)}
DMA_TILES = {11: (128, 128), 14: (256, 128), 22: (128, 128), 26: (128, 256), 27: (256, 128), 33: (256, 256), 18: (256, 256), 21: (192, 256)}
FAMILY = {**{c: "register-staged" for c in REG_TILES}, **{c: "LDS-DMA" for c in DMA_TILES}, 39: "four-wave", 40: "four-wave",
          34: "row-panel", 35: "row-panel", 32: "weight-streaming", 30: "weight-streaming"}


def act_worst(act):
    if act in (None, "none"):
        return 0.0
    if act == "mish":
        return MISH_WORST
    return ACT_WORST[("gelu_erf" if act == "gelu" else act, "fwd")]


def act_value(x, act):
    """(act(x), scale of its evaluation) in float64; the forms of train_ops_ref.act_value plus none and mish = x * tanh(log1p(exp(x)))."""
    x = x.to(F64)
    if act in (None, "none"):
        return x, torch.zeros_like(x)
    if act == "mish":
        sp = x.clamp_min(0.0) + torch.log1p(torch.exp(-x.abs()))
        y = x * torch.tanh(sp)
        # exp(x) is an intermediate here (silu divides by 1 + exp(-x) instead): below the smallest normal it may be flushed, an absolute
        # error of 2^-126 that x multiplies (x = -88: the whole result, 5e-37)
        return y, y.abs() * (1.0 + x.abs()) + x.abs() * (TINY / U)
    return R.act_value(x, "gelu_erf" if act == "gelu" else act)


def prenorm_operand(x, gamma, eps):
    """bf16(x * rsqrt(mean(x^2) + eps) * gamma), the operand of the fused input RMSNorm, from float64 statistics."""
    xd = x.to(F64)
    y = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + R.f32(eps)) * gamma.to(F64)
    return y.to(F32).to(BF16)


def linear_full(x, w, bias=None, act=None, colscale=None, residual=None, glu=False, rowscale=None, rowscale_div=1, batched=False,
                prenorm=None, acc=None):
    """(ref, scale, act_err) in float64. x [M, K] (batched: [Bt, M, K]), w [N, K]; residual [.., M, N_out] or, batched, an [M, N_out] table
    broadcast over the batch. acc: (A.W^T, |A|.|W|^T) computed earlier for the same operands (the case tables slice one product)."""
    if acc is None:
        a = (prenorm_operand(x, *prenorm) if prenorm is not None else x).to(F64)
        wd = w.to(F64)
        acc = (a @ wd.t(), a.abs() @ wd.abs().t())
    y, s = acc
    M = y.shape[-2]
    if bias is not None:
        y, s = y + bias.to(F64), s + bias.to(F64).abs()
    cap = None
    if glu:
        N = y.shape[-1]
        y4, s4 = y.reshape(*y.shape[:-1], N // 32, 2, 16), s.reshape(*s.shape[:-1], N // 32, 2, 16)
        g, u, sg, su = y4[..., 0, :], y4[..., 1, :], s4[..., 0, :], s4[..., 1, :]
        a, sa = act_value(g, act)
        lip = 1.0 if act in (None, "none", "relu") else LIP
        y = (a * u).reshape(*y.shape[:-1], N // 2)
        s = ((lip * sg + a.abs()) * su).reshape(y.shape)           # |d(a u)| <= |da| |u| + |a| |du|, |u| <= su
        aerr = (4.0 * act_worst(act) * U * sa * u.abs()).reshape(y.shape)
        cap = ACT_CAP * float(a.abs().max()) * u.abs().reshape(y.shape)
    else:
        y, sa = act_value(y, act)
        s = s * (1.0 if act in (None, "none", "relu") else LIP)
        aerr = 4.0 * act_worst(act) * U * sa
        cap = torch.full_like(y, ACT_CAP * float(y.abs().max())) if act not in (None, "none") else None
        if colscale is not None:
            c = colscale.to(F64)
            y, s, aerr = y * c, s * c.abs(), aerr * c.abs()
            cap = None if cap is None else cap * c.abs()
    if cap is not None:
        aerr = torch.minimum(aerr, cap)
    if rowscale is not None:
        r = rowscale.to(F64)[torch.arange(M, device=y.device) // rowscale_div][:, None]
        y, s, aerr = y * r, s * r.abs(), aerr * r.abs()
    if residual is not None:
        y, s = y + residual.to(F64), s + residual.to(F64).abs()
    return y, s, aerr


def linear_ref(*args, **kw):
    """(ref, scale) of ops.linear(*args, **kw) in float64 (see the module docstring)."""
    return linear_full(*args, **kw)[:2]


def ratio(out, ref, scale, aerr, K):
    """worst |err| / (2^-24 (sqrt(K) + 4) scale) of a result, the quantity k multiplies (the activation's own allowance taken off first)."""
    err = ((out.to(F64) - ref).abs() - aerr).clamp_min(0.0)
    return float((err / (U * (math.sqrt(K) + 4.0) * scale + TINY)).max())


def check(out, ref, scale, aerr, K, k, what):
    """every element within k * 2^-24 (sqrt(K) + 4) scale + act_err (+ 2^-8 |ref| for bf16); returns `ratio` of the result."""
    assert out.shape == ref.shape and bool(torch.isfinite(ref).all()), what
    err = (out.to(F64) - ref).abs()
    bound = R.out_bound(ref, R.fp32_bound(scale, K, k) + aerr, out.dtype)
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int((err / bound).nan_to_num(nan=float("inf")).reshape(-1).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())}/{err.numel()} elements out of bound; worst at flat index {i}: out "
                             f"{out.reshape(-1)[i].item():.9g} ref {ref.reshape(-1)[i].item():.9g} bound {bound.reshape(-1)[i].item():.3g}")
    return ratio(out, ref, scale, aerr, K)


def preshuffle_index(N, K, dev="cpu"):
    """flat position of element (n, k) in the fragment-ordered copy (ina_gemm_preshuffle): fragment (n / 16, k / 32) is one contiguous KiB, lane
    (k % 32) / 8 * 16 + n % 16 of it holds 8 consecutive k."""
    n = torch.arange(N, device=dev)[:, None]
    k = torch.arange(K, device=dev)[None, :]
    return ((n // 16) * (K // 32) + k // 32) * 512 + ((k % 32) // 8 * 16 + n % 16) * 8 + k % 8


# ---------------------------------------------------------------------------------------------------------------- layouts
class Buf:
    """a sentinel-filled buffer of (batch x) rows + 3 rows and at least 8 columns more than the [rows, n] result view `v` inside it.
    aligned: 16-byte rows on a 16-byte base (the LDS-transposed epilogue runs where a kernel has it); unaligned: bf16 rows of ld % 8 == 4
    elements, fp32 rows (ld % 4 == 0 is the contract) on a base 8 bytes past a 16-byte boundary - the direct epilogue."""

    def __init__(self, rows, n, dtype, layout, dev, batch=None):
        ld = (n + 8 + 7) // 8 * 8 + (4 if layout == "unaligned" and dtype == BF16 else 0)
        off = 2 if layout == "unaligned" and dtype == F32 else 0
        nb = batch or 1
        self.flat = torch.full((nb * (rows + 3) * ld + 8,), SENT, dtype=dtype, device=dev)
        body = self.flat[off: off + nb * (rows + 3) * ld].view(nb, rows + 3, ld)
        self.v = body[:, :rows, :n] if batch else body[0, :rows, :n]
        es = self.flat.element_size()
        al = self.v.data_ptr() % 16 == 0 and (ld * es) % 16 == 0
        assert al == (layout == "aligned") and ld - n >= 8

    def fill(self, t):
        self.v.copy_(t)
        return self.v

    def outside_untouched(self):
        keep = self.v.clone()
        self.v.fill_(SENT)
        ok = bool((self.flat == SENT).all())
        self.v.copy_(keep)
        return ok


def strided_rows(t, extra=8):
    """the same [rows, C] values as a row-strided view of a wider buffer."""
    buf = torch.zeros(t.shape[0], t.shape[1] + extra, dtype=t.dtype, device=t.device)
    v = buf[:, :t.shape[1]]
    v.copy_(t)
    return v


def run_case(linear, c, layout, dev):
    """one launch of case `c` in `layout` through `linear` (ops.linear or a stand-in with its signature) into sentinel-filled buffers.
    Returns (out view, residual handed over); asserts that nothing outside [M, N_out] was written."""
    x, w = c["x"], c["w"]
    n_out = w.shape[0] // 2 if c.get("glu") else w.shape[0]
    M = x.shape[-2]
    bt = x.shape[0] if c.get("batched") else None
    out = Buf(M, n_out, c["out_dtype"], layout, dev, batch=bt)
    res = c.get("residual")
    if c.get("alias"):                                   # x = x + f(x): the residual stream is the output buffer
        res = out.fill(res)
    elif res is not None:
        rb = Buf(M, n_out, res.dtype, layout, dev, batch=bt if res.dim() == 3 else None)
        res = rb.fill(res)
    if c.get("strided"):
        x, w = strided_rows(x), strided_rows(w, 16)
    kw = {k: c[k] for k in ("bias", "act", "colscale", "rowscale", "rowscale_div", "glu", "batched", "prenorm", "group_m", "w_frag") if c.get(k) is not None}
    linear(x, w, residual=res, out=out.v, force_cfg=c.get("cfg", 0), **kw)
    if dev != "cpu":
        torch.cuda.synchronize()
    assert out.outside_untouched(), f"{c['id']} [{layout}]: written outside the [{M}, {n_out}] result"
    return out.v


# ---------------------------------------------------------------------------------------------------------------- exact cases
VARIANTS = ("plain", "bias", "relu", "colscale", "rowscale", "res_bf16", "res_f32", "full_bf16", "full_f32", "glu")


class Pool:
    """integer operands of one (M, N, K) maximum; cases are slices of it, their references slices of ONE float64 product."""

    def __init__(self, M, N, K, seed, dev, batch=None):
        assert 16 * K < 2 ** 24, "every partial sum must stay an exact fp32 integer"
        g = torch.Generator(device=dev).manual_seed(seed)
        lead = (batch,) if batch else ()

        def ints(*shape):
            return torch.randint(-4, 5, shape, generator=g, device=dev).to(F32)

        def pow2(n):
            return torch.tensor([0.5, 1.0, 2.0], device=dev)[torch.randint(0, 3, (n,), generator=g, device=dev)]

        self.M, self.N, self.K, self.dev = M, N, K, dev
        self.x, self.w = ints(*lead, M, K).to(BF16), ints(N, K).to(BF16)
        self.bias, self.res = ints(N), ints(*lead, M, N)
        self.colscale, self.rowscale = pow2(N), pow2(M)
        a, wd = self.x.to(F64), self.w.to(F64)
        self.acc = (a @ wd.t(), a.abs() @ wd.abs().t())
        assert bool((self.acc[0] != 0).any(-1).all()), "a reference row is all zero"

    def case(self, id, M, N, variant="plain", out_dtype=BF16, cfg=0, **extra):
        assert M <= self.M and N <= self.N and variant in VARIANTS
        glu = variant == "glu"
        n_out = N // 2 if glu else N
        c = dict(id=f"{id}-{M}x{N}x{self.K}-{variant}-{'bf16' if out_dtype == BF16 else 'f32'}", cfg=cfg, K=self.K, out_dtype=out_dtype,
                 x=self.x[..., :M, :], w=self.w[:N], acc=(self.acc[0][..., :M, :N], self.acc[1][..., :M, :N]), **extra)
        full = variant.startswith("full")
        if variant == "bias" or full or glu:
            c["bias"] = self.bias[:N]
        if variant == "relu" or full or glu:
            c["act"] = "relu"
        if variant == "colscale" or full:
            c["colscale"] = self.colscale[:N]
        if variant == "rowscale":
            c["rowscale"] = self.rowscale[:M]
        if full or glu:
            c.update(rowscale=self.rowscale[:(M + 2) // 3], rowscale_div=3)
        if variant in ("res_bf16", "full_bf16"):
            c["residual"] = self.res[..., :M, :n_out].to(BF16)
        if variant in ("res_f32", "full_f32"):
            c["residual"] = self.res[..., :M, :n_out].contiguous()
        if glu:
            c["glu"] = True
        return c


def case_ref(c):
    """(ref, scale, act_err) of a case dict."""
    kw = {k: c.get(k) for k in ("bias", "act", "colscale", "residual", "rowscale", "prenorm")}
    return linear_full(c["x"], c["w"], glu=bool(c.get("glu")), rowscale_div=c.get("rowscale_div", 1), acc=c.get("acc"), **kw)


def expected_exact(c):
    """the exact result in the case's output dtype: the float64 reference is an fp32 number, bf16 is its single rounding."""
    ref = case_ref(c)[0]
    # multiples of 1/4 below 2^19 (GLU: the gate x up product of two such integers, asserted to stay below 2^22): exact in fp32 at every step
    assert float(ref.abs().max()) < (2.0 ** 22 if c.get("glu") else 2.0 ** 19) and bool((ref * 4 == (ref * 4).round()).all())
    return ref.to(F32).to(c["out_dtype"])


def edge_sizes(B):
    return (1, B - 1, B, B + 1, 2 * B + 3)


def n_sizes(BN):
    return (4, 12, BN - 4, BN, BN + 4, BN + 12)


def _grid(pool, id, cfg, Ms, Ns, variants=(("plain", BF16), ("full_bf16", BF16), ("full_f32", F32)), **extra):
    return [pool.case(id, M, N, v, dt, cfg=cfg, **extra) for M in Ms for N in Ns for v, dt in variants]


def reg_cases(cfg, K, dev):
    """register-staged tiles (gemm.hip, BK = 64, K % 8 == 0): both sides of BM / BN, and of the ragged N % 8 == 4 chunk of the staged bf16 store."""
    BM, BN = REG_TILES[cfg]
    Ms, Ns = edge_sizes(BM), n_sizes(BN)
    return _grid(Pool(max(Ms), max(Ns), K, 1000 + cfg * 10 + K, dev), f"cfg{cfg}", cfg, Ms, Ns)


def dma_cases(cfg, K, dev):
    """LDS-DMA tiles (gemm_glds.hip, K % 64 == 0): fewer K steps than ring stages, as many, one more."""
    BM, BN = DMA_TILES[cfg]
    Ms = edge_sizes(BM) + ((193, 385) if cfg == 21 else ())
    Ns = n_sizes(BN)
    return _grid(Pool(max(Ms), max(Ns), K, 2000 + cfg * 10 + K, dev), f"cfg{cfg}", cfg, Ms, Ns)


def group_m_cases(cfg, dev):
    """tile orders of the LDS-DMA kernels on a 3 x 3 (or larger) tile grid."""
    BM, BN = DMA_TILES.get(cfg, (256, 256))
    M, N = 2 * BM + 3, 2 * BN + 12
    pool = Pool(M, N, 128, 2500 + cfg, dev)
    return [pool.case(f"cfg{cfg}-gm{gm}", M, N, v, dt, cfg=cfg, group_m=gm) for gm in (1, 3, 8) for v, dt in (("plain", BF16), ("full_f32", F32))]


W4_M = (1, 255, 256, 257, 515)
W4_N = (4, 12, 252, 256, 260, 268)        # cfg 39: any N % 4 == 0 (aligned rows are the layout's business)
W4P_N = (16, 240, 256, 272)               # cfg 40: N % 16 == 0


def w4_cases(cfg, K, dev):
    Ns = W4_N if cfg == 39 else W4P_N
    return _grid(Pool(max(W4_M), max(Ns), K, 3000 + K, dev), f"cfg{cfg}", cfg, W4_M, Ns)


RP_M, RP_N = (32, 224, 256, 288, 544), (128, 384, 640)


def rowpanel_cases(cfg, dev, Ns=RP_N, variants=(("plain", BF16), ("bias_relu", BF16))):
    pool = Pool(max(RP_M), max(Ns), 384, 3400 + cfg, dev)
    out = []
    for M in RP_M:
        for N in Ns:
            for v, dt in variants:
                c = pool.case(f"cfg{cfg}", M, N, "bias" if v == "bias_relu" else v, dt, cfg=cfg)
                if v == "bias_relu":
                    c.update(act="relu", id=c["id"].replace("-bias-", "-bias_relu-"))
                out.append(c)
    return out


SK_M = (1, 15, 16, 17, 32, 33, 48, 49, 64)


def skinny_cases(K, dev):
    """weight-streaming kernel (cfg 32): K = 128 .. 1024 at N = 260 reach the four group widths of sk_group_waves (1, 2, 4, 8 K steps of 128),
    K = 8 / 136 / 1032 the K tails; M crosses every MF (16-row fragments); GLU (NT16 = 2) on interleaved rows."""
    pool = Pool(64, 288, K, 3200 + K, dev)
    out = _grid(pool, "cfg32", 32, SK_M, (4, 20, 260))
    out += [pool.case("cfg32", M, N, "glu", dt, cfg=32) for M in (1, 17, 64) for N in (32, 288) for dt in (BF16, F32)]
    return out


def skinny_wide_cases(dev):
    """the `tiles` thresholds of sk_group_waves (1024 / 2048 / 4096 column tiles) at M = 1, K = 1024: 4, 2, 1 waves per group."""
    pool = Pool(1, 65536, 1024, 3300, dev)
    return [pool.case("cfg32-wide", 1, N, v, dt, cfg=32) for N in (16384, 32768, 65536) for v, dt in (("plain", BF16), ("full_f32", F32))]


def prenorm_cases(K, dev):
    """fused input RMSNorm (kernel 30): every row holds one power-of-two magnitude with random signs, gamma integers in [-4, 4]: x * rstd is
    within 1e-6 of +-1 for eps in {0, 1e-6} (magnitudes >= 1), so the bf16 operand is exactly sign * gamma[k] and the GEMM is exact."""
    g = torch.Generator(device=dev).manual_seed(3600 + K)
    Mx, Nx = 16, 288
    sign = torch.randint(0, 2, (Mx, K), generator=g, device=dev).to(F32) * 2 - 1
    mag = 2.0 ** torch.randint(0, 7, (Mx, 1), generator=g, device=dev).to(F32)
    gamma = torch.randint(-4, 5, (K,), generator=g, device=dev).to(F32)
    pool = Pool(Mx, Nx, K, 3700 + K, dev)
    a, wd = (sign * gamma).to(F64), pool.w.to(F64)
    acc = (a @ wd.t(), a.abs() @ wd.abs().t())
    assert bool((acc[0] != 0).any(-1).all())
    out = []
    i = 0
    for xdt in (F32, BF16):
        for M in (1, 7, 16):
            for N, variant in ((256, "plain"), (272, "full_f32"), (256, "glu"), (288, "glu")):
                eps = (0.0, 1e-6)[i % 2]
                i += 1
                c = pool.case(f"prenorm-{'f32' if xdt == F32 else 'bf16'}-eps{eps:g}", M, N, variant, F32 if variant == "full_f32" else BF16)
                x = (sign * mag)[:M].to(xdt).contiguous()
                assert torch.equal(prenorm_operand(x, gamma, eps).to(F64), a[:M]), "the normalised operand is not sign * gamma"
                c.update(x=x, prenorm=(gamma, eps), acc=(acc[0][:M, :N], acc[1][:M, :N]))
                out.append(c)
    return out


# representative tile of every family for the epilogue features: (cfg, M, N, K); M is no multiple of 3, N % 8 == 4 where the kernel admits it
FEATURE_SHAPES = {1: (131, 140, 136), 2: (67, 140, 72), 4: (67, 76, 136), 22: (131, 140, 192), 14: (259, 140, 256), 18: (259, 268, 128),
                  21: (193, 268, 192), 33: (259, 268, 192), 39: (259, 268, 128), 32: (17, 260, 264)}


def feature_cases(cfg, dev):
    """every optional operand alone, all together (rowscale_div = 3), both output and residual dtypes, GLU with bias + relu, the residual
    aliasing the output (x = x + f(x) of the ViT blocks), row-strided A and W."""
    M, N, K = FEATURE_SHAPES[cfg]
    pool = Pool(M, N + 20, K, 4000 + cfg, dev)
    out = [pool.case(f"cfg{cfg}", M, N, v, dt, cfg=cfg) for v in VARIANTS[:-1] for dt in (BF16, F32)]
    Ng = (N + 20) // 32 * 32
    out += [pool.case(f"cfg{cfg}", M, Ng, "glu", dt, cfg=cfg) for dt in (BF16, F32)]
    for dt in (BF16, F32):
        c = pool.case(f"cfg{cfg}-alias", M, N, "full_bf16" if dt == BF16 else "full_f32", dt, cfg=cfg, alias=True)
        out.append(c)
        out.append(pool.case(f"cfg{cfg}-strided", M, N, "full_bf16", dt, cfg=cfg, strided=True))
    return out


def batched_cases(cfg, dev):
    """a batch of 3 with unequal batch strides of A, C and R (A rows of K + 8, C / R rows and batches of the sentinel buffers) and a residual
    table broadcast over the batch (strideR = 0)."""
    M, N, K = FEATURE_SHAPES[cfg]
    pool = Pool(M, N, K, 4500 + cfg, dev, batch=3)
    out = []
    for dt in (BF16, F32):
        c = pool.case(f"cfg{cfg}-batch3", M, N, "full_bf16" if dt == BF16 else "full_f32", dt, cfg=cfg, batched=True)
        wide = torch.zeros(3, M + 1, K + 8, dtype=BF16, device=dev)
        wide[:, :M, :K] = c["x"]
        c["x"] = wide[:, :M, :K]
        out.append(c)
        b = dict(c, id=c["id"] + "-bcastR", residual=c["residual"][0].contiguous())
        out.append(b)
    return out


# ---------------------------------------------------------------------------------------------------------------- random-value cases
ACTS = ("gelu", "gelu_tanh", "silu", "mish", "tanh", "relu")
# cfg -> (M, N, K): the smallest shape with more than one K step, ragged in M and N where the kernel admits it
RANDOM_SHAPES = {1: (131, 140, 136), 4: (67, 76, 136), 22: (131, 140, 128), 18: (259, 268, 128), 39: (259, 268, 128), 34: (288, 256, 384),
                 35: (160, 256, 384), 32: (17, 260, 264)}


def random_case(cfg, act, out_dtype, dev, glu=False):
    M, N, K = RANDOM_SHAPES[cfg]
    if glu:
        N = (N + 31) // 32 * 32
    g = torch.Generator(device=dev).manual_seed(5000 + cfg * 16 + ACTS.index(act) + (8 if glu else 0))
    x = torch.randn(M, K, generator=g, device=dev).to(BF16)
    w = (torch.randn(N, K, generator=g, device=dev) * K ** -0.5).to(BF16)
    c = dict(id=f"cfg{cfg}-{act}{'-glu' if glu else ''}-{'bf16' if out_dtype == BF16 else 'f32'}", cfg=cfg, K=K, x=x, w=w, act=act, out_dtype=out_dtype)
    if glu:
        c["glu"] = True
    if not (glu and cfg in (34, 35)):             # the row-panel GLU takes no bias
        c["bias"] = torch.randn(N, generator=g, device=dev)
    return c
