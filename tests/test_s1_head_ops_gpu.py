"""Op-level GPU tests of the small kernels that finish the System-1 policies (NavDP, NextDiT heads): head3, embed3, seqpool_head,
select_traj, pool_act and goal_slots, each against a plain float64 restatement of the same operation on the same (bf16 / fp32) inputs.

Tolerance model (as in test_ops_gpu.py, made explicit per element):
  fp32 outputs: |err| <= k * 2^-24 * sqrt(reduction length) * scale, where scale is the float64 sum of |terms| of the element
                (every fp32 rounding is relative to a partial sum no larger than that);
  bf16 outputs: 2^-8 * |ref| (one rounding to 8 mantissa bits) plus the fp32 term above.
Where a kernel's comments promise identical arithmetic (launch paths, load paths, embed3 vs goal_slots) the test asserts torch.equal.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24          # fp32 unit roundoff
BF = 2.0 ** -8          # bf16 relative spacing
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def ops(built_lib):
    from internnav_amd import ops

    return ops


def _randn(shape, g, scale=1.0, dtype=F32):
    return (torch.randn(shape, generator=g, dtype=torch.float32) * scale).to(dtype).to(DEV)


def _check(out, ref, bound, what):
    """every element within its bound (a NaN in out counts as a failure)."""
    err = (out.double() - ref).abs()
    ok = err <= bound
    n_bad = int((~ok).sum())
    if n_bad:
        ratio = (err / bound).nan_to_num(nan=float("inf"))
        i = int(ratio.reshape(-1).argmax())
        raise AssertionError(f"{what}: {n_bad}/{err.numel()} elements out of bound; worst at flat index {i}: out "
                             f"{out.reshape(-1)[i].item():.9g} ref {ref.reshape(-1)[i].item():.9g} bound {bound.reshape(-1)[i].item():.3g}")


def _out_bound(ref, fp32_bound, dtype):
    return fp32_bound + (BF * ref.abs() if dtype == BF16 else 0.0)


def _misaligned(t):
    """a copy of t whose storage starts 4 bytes past a 16-byte boundary (forces the kernels' scalar-load path)."""
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    out = flat[1: 1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


def _colview(rows, C, dtype, extra, fill=0.0, off=0):
    """a [rows, C] column view of a [rows, C + extra] buffer (row stride > C), starting at column off."""
    buf = torch.full((rows, C + extra), fill, dtype=dtype, device=DEV)
    return buf, buf[:, off: off + C]


# ------------------------------------------------------------------------------------------------ head3
def _ln64(x, gamma, beta, eps, ms=None, mod_div=1):
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    t = (xd - mean) / torch.sqrt(((xd - mean) ** 2).mean(1, keepdim=True) + eps)
    if gamma is not None:
        t = t * gamma.double()
    if beta is not None:
        t = t + beta.double()
    if ms is not None:
        idx = torch.arange(x.shape[0], device=DEV) // mod_div
        t = t * (1.0 + ms.double()[idx])
    return t


def _head3_ref(x, w, b, gamma, beta, eps, ms=None, mod_div=1):
    """eps prediction e [rows, 3] in float64 and the fp32 error bound of the kernel's e."""
    t = _ln64(x, gamma, beta, eps, ms, mod_div)
    wd, bd = w.double(), b.double()
    e = t @ wd.t() + bd
    scale = t.abs() @ wd.abs().t() + bd.abs()
    return e, 16 * U * (math.sqrt(x.shape[1]) + 4) * scale


def _ddpm_ref(s0, e, e_bound, coef, clip, noise):
    c0, c1, c2, c3, c4 = coef
    s, x0p = s0.double(), (s0.double() - c1 * e) * c0
    x0 = x0p.clamp(-clip, clip)
    n = c2 * x0 + c3 * s
    mag = abs(c2) * abs(c0) * (s.abs() + abs(c1) * e.abs()) + abs(c3) * s.abs()
    if noise is not None:
        n = n + c4 * noise.double()
        mag = mag + abs(c4) * noise.double().abs()
    return n, abs(c0 * c1 * c2) * e_bound + 8 * U * mag


H3_CASES = [(C, rows, dt) for C in (8, 384, 520, 1024) for rows in (1, 200, 32768 + 5) for dt in (F32, BF16)]


@pytest.mark.parametrize("C,rows,xdt", H3_CASES, ids=[f"C{c}-r{r}-{str(d)[6:]}" for c, r, d in H3_CASES])
def test_head3_modes(ops, C, rows, xdt):
    """modes 0 / 1 (with and without noise, eps_out alongside) / 2, gamma / beta on and off, mod_scale with mod_div = 6."""
    g = torch.Generator().manual_seed(C * 31 + rows)
    view = ((C // 8) + rows) % 2 == 1                      # ldx > C (a column view) for about half the cases, both dtypes
    if view:
        _, x = _colview(rows, C, xdt, 24, off=8)
        x.copy_(_randn((rows, C), g, dtype=xdt) + 0.25)
        assert x.stride(0) == C + 24
    else:
        x = _randn((rows, C), g, dtype=xdt) + 0.25
    gamma, beta = _randn(C, g, 0.5) + 1.0, _randn(C, g, 0.3)
    w, b = _randn((3, C), g, C ** -0.5), _randn(3, g)
    s0, noise = _randn((rows, 3), g), _randn((rows, 3), g)
    coef, clip = (1.3, 0.7, 0.4, 0.55, 0.2), 1.0

    # mode 0: gamma + beta -> eps_out
    e_out = torch.full((rows, 3), float("nan"), device=DEV)
    ops.head3(x, w, b, gamma, beta, mode=0, eps_out=e_out)
    e, eb = _head3_ref(x, w, b, gamma, beta, 1e-5)
    _check(e_out, e, eb, "mode 0 eps_out")

    # mode 1 with noise, eps_out alongside, gamma only
    s, e_out = s0.clone(), torch.full((rows, 3), float("nan"), device=DEV)
    ops.head3(x, w, b, gamma, None, mode=1, sample=s, noise=noise, eps_out=e_out, coef=coef, clip=clip)
    e, eb = _head3_ref(x, w, b, gamma, None, 1e-5)
    _check(e_out, e, eb, "mode 1 eps_out")
    _check(s, *_ddpm_ref(s0, e, eb, coef, clip, noise), "mode 1 sample (noise)")

    # mode 1 without noise (the last DDPM step), beta only, eps 1e-6
    s = s0.clone()
    ops.head3(x, w, b, None, beta, eps=1e-6, mode=1, sample=s, coef=coef, clip=clip)
    e, eb = _head3_ref(x, w, b, None, beta, 1e-6)
    _check(s, *_ddpm_ref(s0, e, eb, coef, clip, None), "mode 1 sample (no noise)")

    # mode 2 (Euler step) with a per-env modulation changing every 6 rows: mid-wave reloads in the 4-row path
    nmod = (rows + 5) // 6
    ms = _randn((nmod, C), g, 0.5)
    s = s0.clone()
    ops.head3(x, w, b, None, None, eps=1e-6, mode=2, sample=s, coef=(-0.1, 0, 0, 0, 0), mod_scale=ms, mod_div=6)
    e, eb = _head3_ref(x, w, b, None, None, 1e-6, ms, 6)
    _check(s, s0.double() - 0.1 * e, 0.1 * eb + 4 * U * (s0.double().abs() + 0.1 * e.abs()), "mode 2 sample (mod_scale)")


@pytest.mark.parametrize("C,xdt", [(384, F32), (520, BF16), (1024, F32)])
def test_head3_four_row_waves_bit_equal_single_row_waves(ops, C, xdt):
    """rows of a >= 32768-row call (4 rows per wave, short final wave) equal the same rows computed by < 32768-row calls."""
    g = torch.Generator().manual_seed(C)
    rows = 32768 + 5
    x = _randn((rows, C), g, dtype=xdt)
    gamma, beta = _randn(C, g, 0.5) + 1.0, _randn(C, g, 0.3)
    w, b = _randn((3, C), g, C ** -0.5), _randn(3, g)
    s0, noise = _randn((rows, 3), g), _randn((rows, 3), g)
    ms = _randn(((rows + 5) // 6, C), g, 0.5)
    coef = (1.3, 0.7, 0.4, 0.55, 0.2)
    s, e_out = s0.clone(), torch.empty(rows, 3, device=DEV)
    ops.head3(x, w, b, gamma, beta, mode=1, sample=s, noise=noise, eps_out=e_out, coef=coef, mod_scale=ms, mod_div=6)
    for r0, n in ((0, 1), (6000, 1203), (32766, 7)):        # r0 a multiple of mod_div: the slice sees the same modulation rows
        ss, es = s0[r0: r0 + n].clone(), torch.empty(n, 3, device=DEV)
        ops.head3(x[r0: r0 + n], w, b, gamma, beta, mode=1, sample=ss, noise=noise[r0: r0 + n].contiguous(), eps_out=es, coef=coef,
                  mod_scale=ms[r0 // 6:], mod_div=6)
        assert torch.equal(es, e_out[r0: r0 + n]), f"eps rows {r0}..{r0 + n}"
        assert torch.equal(ss, s[r0: r0 + n]), f"sample rows {r0}..{r0 + n}"


@pytest.mark.parametrize("rows", [997, 32768 + 5])
@pytest.mark.parametrize("C,xdt", [(384, BF16), (520, F32)])
def test_head3_scalar_load_path_bit_equal(ops, rows, C, xdt):
    """4-byte-offset W / gamma / beta / mod_scale, or a mod_scale row stride that is not a multiple of 4, select the scalar-load path;
    it computes the same bits as the 16-byte path."""
    g = torch.Generator().manual_seed(rows + C)
    x = _randn((rows, C), g, dtype=xdt)
    gamma, beta = _randn(C, g, 0.5) + 1.0, _randn(C, g, 0.3)
    w, b = _randn((3, C), g, C ** -0.5), _randn(3, g)
    ms = _randn(((rows + 5) // 6, C), g, 0.5)
    ms_odd = torch.empty(ms.shape[0], C + 1, device=DEV)[:, :C]           # mod_ld = C + 1
    ms_odd.copy_(ms)
    s0 = _randn((rows, 3), g)

    def run(w_, ga_, be_, ms_):
        s, e = s0.clone(), torch.empty(rows, 3, device=DEV)
        ops.head3(x, w_, b, ga_, be_, mode=2, sample=s, eps_out=e, coef=(-0.1, 0, 0, 0, 0), mod_scale=ms_, mod_div=6)
        return s, e

    s_ref, e_ref = run(w, gamma, beta, ms)
    for name, args in (("W", (_misaligned(w), gamma, beta, ms)), ("gamma", (w, _misaligned(gamma), beta, ms)),
                       ("beta", (w, gamma, _misaligned(beta), ms)), ("mod_scale", (w, gamma, beta, _misaligned(ms))),
                       ("mod_ld", (w, gamma, beta, ms_odd))):
        s, e = run(*args)
        assert torch.equal(e, e_ref) and torch.equal(s, s_ref), f"scalar path via misaligned {name} differs from the vector path"


# ------------------------------------------------------------------------------------------------ embed3
def _embed3_ref(x, w, b, pos, rows, x_div):
    r = torch.arange(rows, device=DEV)
    ref = torch.zeros(rows, w.shape[0] if w is not None else pos.shape[1], dtype=torch.float64, device=DEV)
    mag = torch.zeros_like(ref)
    if x is not None:
        xr = x.double()[r // x_div]
        ref += xr @ w.double().t()
        mag += xr.abs() @ w.double().abs().t()
    if b is not None:
        ref += b.double()
        mag += b.double().abs()
    if pos is not None:
        p = pos.double()[r % pos.shape[0]]
        ref += p
        mag += p.abs()
    return ref, 8 * U * mag


EMB_CASES = [(100, 384, 1, 7), (37, 12, 2, 5), (24579, 384, 3, 24), (9000, 1024, 1, 7)]    # the last two: > 8192 blocks of 256 groups


@pytest.mark.parametrize("odt", [F32, BF16])
@pytest.mark.parametrize("rows,C,x_div,pmod", EMB_CASES)
def test_embed3_paths(ops, odt, rows, C, x_div, pmod):
    """fp32 / bf16 out with ldy > C, a pos period that does not divide rows, x_div; scalar-load path bit-equal to the vector path."""
    g = torch.Generator().manual_seed(rows + C)
    x = _randn(((rows + x_div - 1) // x_div, 3), g)
    w, b, pos = _randn((C, 3), g), _randn(C, g), _randn((pmod, C), g)
    sentinel = -3.25
    buf, out = _colview(rows, C, odt, 8, fill=sentinel)
    ops.embed3(x, w, b, out=out, pos=pos, rows=rows, x_div=x_div)
    ref, fb = _embed3_ref(x, w, b, pos, rows, x_div)
    _check(out, ref, _out_bound(ref, fb, odt), f"embed3 {str(odt)}")
    assert bool((buf[:, C:] == sentinel).all()), "columns past C were written"
    for name, args in (("W", (_misaligned(w), b, pos)), ("b", (w, _misaligned(b), pos)), ("pos", (w, b, _misaligned(pos)))):
        buf2, out2 = _colview(rows, C, odt, 8, fill=sentinel)
        ops.embed3(x, args[0], args[1], out=out2, pos=args[2], rows=rows, x_div=x_div)
        assert torch.equal(buf2, buf), f"scalar path via misaligned {name} differs from the vector path"
    # table fill (no x) through the scalar path too
    buf3, out3 = _colview(rows, C, odt, 8, fill=sentinel)
    ops.embed3(None, None, None, out=out3, pos=_misaligned(pos), rows=rows)
    ref3, fb3 = _embed3_ref(None, None, None, pos, rows, 1)
    _check(out3, ref3, _out_bound(ref3, fb3, odt), "embed3 table fill")


@pytest.mark.parametrize("odt", [F32, BF16])
def test_embed3_out_map_scatter(ops, odt):
    """out_map scatters rows into a [env, L] slot layout; every row outside the map keeps its bits."""
    g = torch.Generator().manual_seed(5)
    B, L, C = 13, 7, 384
    x, w, b, pos = _randn((B, 3), g), _randn((C, 3), g), _randn(C, g), _randn((5, C), g)
    sentinel = 7.5
    out = torch.full((B * L, C), sentinel, dtype=odt, device=DEV)
    ops.embed3(x, w, b, out=out, pos=pos[2:3], rows=B, out_map=(1, L, 2))                 # slot 2 of every env
    ops.embed3(x, w, b, out=out, pos=pos, rows=3 * B, x_div=3, out_map=(3, L, 4))          # slots 4..6, pos rows 0, 1, 2, 3, 4, 0, ...
    ops.embed3(None, None, None, out=out, pos=pos[4:5], rows=B, out_map=(1, L, 0))        # table fill of slot 0
    o = out.view(B, L, C)
    r1, b1 = _embed3_ref(x, w, b, pos[2:3], B, 1)
    _check(o[:, 2], r1, _out_bound(r1, b1, odt), "slot 2")
    r2, b2 = _embed3_ref(x, w, b, pos, 3 * B, 3)
    _check(o[:, 4:7].reshape(3 * B, C), r2, _out_bound(r2, b2, odt), "slots 4..6")
    r3, b3 = _embed3_ref(None, None, None, pos[4:5], B, 1)
    _check(o[:, 0], r3, _out_bound(r3, b3, odt), "slot 0")
    assert bool((o[:, [1, 3]] == sentinel).all()), "rows outside the map were written"


# ------------------------------------------------------------------------------------------------ seqpool_head
SP_CASES = [(C, T, dt) for C in (64, 384, 512) for T in (1, 3, 5, 24) for dt in (F32, BF16)]


@pytest.mark.parametrize("C,T,xdt", SP_CASES, ids=[f"C{c}-T{t}-{str(d)[6:]}" for c, t, d in SP_CASES])
def test_seqpool_head(ops, C, T, xdt):
    g = torch.Generator().manual_seed(C + T)
    nseq = 7
    rows = nseq * T
    if (C // 64 + T) % 2:
        _, x = _colview(rows, C, xdt, 16, off=8)
        x.copy_(_randn((rows, C), g, dtype=xdt) + 0.5)
    else:
        x = _randn((rows, C), g, dtype=xdt) + 0.5
    gamma = None if T == 3 else _randn(C, g, 0.5) + 1.0
    beta = None if T == 5 else _randn(C, g, 0.3)
    w, b = _randn((1, C), g, C ** -0.5), _randn(1, g)
    out = torch.full((nseq,), float("nan"), device=DEV)
    ops.seqpool_head(x, T, gamma, beta, w, b, out)
    t = _ln64(x, gamma, beta, 1e-5).view(nseq, T, C)
    ref = (t.mean(1) @ w.double().t())[:, 0] + b.double()
    scale = (t.abs().mean(1) @ w.double().abs().t())[:, 0] + b.double().abs()
    _check(out, ref, 16 * U * (math.sqrt(C) + T + 4) * scale, "seqpool_head")


# ------------------------------------------------------------------------------------------------ select_traj
SEL_CASES = [(S, k) for S in (8, 17, 32, 64) for k in sorted({1, 8, S}) if k <= S]


@pytest.mark.parametrize("S,k", SEL_CASES)
def test_select_traj_stable_order_with_ties(ops, S, k):
    """k lowest critic values ascending / k highest descending, ties in index order (torch.sort stable), cumsum of sample * scale."""
    g = torch.Generator().manual_seed(S * 100 + k)
    B, scale = 5, 0.3
    for T in (1, 24, 32):
        critic = (torch.randint(-2, 3, (B, S), generator=g).float() * 0.5).to(DEV)        # 5 distinct values: many exact ties
        critic[0] = 1.0                                                                     # one env where every value ties
        sample = _randn((B, S, T, 3), g)
        neg = torch.full((B, k, T, 3), float("nan"), device=DEV)
        pos = torch.full((B, k, T, 3), float("nan"), device=DEV)
        ops.select_traj(critic, sample, neg, pos, k=k, scale=scale)
        traj = torch.cumsum(sample.double() * scale, dim=2)
        mag = torch.cumsum(sample.double().abs() * scale, dim=2)
        lo = torch.sort(critic, dim=1, stable=True).indices[:, :k]
        hi = torch.sort(-critic, dim=1, stable=True).indices[:, :k]
        ar = torch.arange(B, device=DEV)[:, None]
        _check(neg, traj[ar, lo], 4 * U * (T + 1) * mag[ar, lo], f"neg T={T}")
        _check(pos, traj[ar, hi], 4 * U * (T + 1) * mag[ar, hi], f"pos T={T}")


# ------------------------------------------------------------------------------------------------ pool_act
ACTS = {None: lambda v: v, "gelu": torch.nn.functional.gelu, "gelu_tanh": lambda v: torch.nn.functional.gelu(v, approximate="tanh"),
        "relu": torch.relu, "silu": torch.nn.functional.silu, "mish": torch.nn.functional.mish}


def _pool_act_check(ops, x, out, T, pos, act, what):
    nseq, C = out.shape
    ops.pool_act(x, out, T=T, pos=pos, act=act)
    xd = x.double().view(nseq, T, C)
    a, mag = xd.mean(1), xd.abs().mean(1)
    if pos is not None:
        p = pos.double()[torch.arange(nseq, device=DEV) % pos.shape[0]]
        a, mag = a + p, mag + p.abs()
    ref = ACTS[act](a)
    # mean: T + 2 roundings of partial sums <= mag, times the activation's slope (<= 1.2); the activation's own fp32 evaluation
    # (exp / tanh / erf, argument roundings that grow with |a|) adds a few ulp of |ref| + |a|
    fb = 1.2 * 2 * U * (T + 2) * mag + 16 * U * (ref.abs() + a.abs()) * (1.0 + a.abs())
    _check(out, ref, _out_bound(ref, fb, out.dtype), f"{what} act={act}")


PA_CASES = [(i, o, T) for i in (F32, BF16) for o in (F32, BF16) for T in (1, 7, 256)]


@pytest.mark.parametrize("idt,odt,T", PA_CASES, ids=[f"{str(i)[6:]}-{str(o)[6:]}-T{t}" for i, o, t in PA_CASES])
def test_pool_act_every_activation(ops, idt, odt, T):
    g = torch.Generator().manual_seed(T)
    nseq, C = 6, 392
    x = _randn((nseq * T, C), g, 8.0 if T == 1 else 3.0, dtype=idt)          # T = 1: inputs past Mish's softplus threshold (|x| > 20)
    pos = _randn((4, C), g)
    for act in ACTS:
        _pool_act_check(ops, x, torch.empty(nseq, C, dtype=odt, device=DEV), T, pos if act else None, act, "pool_act")


@pytest.mark.parametrize("idt,odt", [(F32, BF16), (BF16, F32)])
def test_pool_act_grid_stride_and_strides(ops, idt, odt):
    """nseq * C above 2048 blocks x 256 threads, strided ldx / ldy, a positional period of 5; columns outside the view untouched."""
    g = torch.Generator().manual_seed(17)
    nseq, T, C = 1400, 7, 384
    _, x = _colview(nseq * T, C, idt, 5)
    x.copy_(_randn((nseq * T, C), g, 2.0, dtype=idt))
    sentinel = 1.5
    buf, out = _colview(nseq, C, odt, 3, fill=sentinel, off=2)
    assert x.stride(0) == C + 5 and out.stride(0) == C + 3
    _pool_act_check(ops, x, out, T, _randn((5, C), g), "mish", "pool_act grid")
    assert bool((buf[:, :2] == sentinel).all()) and bool((buf[:, 2 + C:] == sentinel).all())


# ------------------------------------------------------------------------------------------------ goal_slots
def _goal_inputs(g, D, E, ntok, counts):
    """point / image / pixel inputs with one spare row each (the plan's rows are a permuted subset)."""
    n_pt, n_img, n_pix = (c + 1 for c in counts)
    point = (_randn((n_pt, 3), g), _randn((D, 3), g), _randn(D, g))
    image = (_randn((n_img * ntok, E), g) + 0.5, _randn((D, E), g, E ** -0.5), _randn(D, g), ntok)
    pixel = (_randn((n_pix * ntok, E), g) - 0.5, _randn((D, E), g, E ** -0.5), _randn(D, g), ntok)
    return point, image, pixel


def _goal_ref(kind, row, point, image, pixel, D):
    """float64 goal embedding e [B, D] and the fp32 bound of the kernel's e (NaN rows stay for bad entries)."""
    B = kind.numel()
    e = torch.zeros(B, D, dtype=torch.float64, device=DEV)
    eb = torch.zeros_like(e)
    for b in range(B):
        k, r = int(kind[b]), int(row[b])
        if k == 1:
            x, w, bias = point
            xd = x.double()[r]
            e[b] = w.double() @ xd + bias.double()
            eb[b] = 8 * U * (w.double().abs() @ xd.abs() + bias.double().abs())
        elif k in (2, 3):
            tok, w, bias, ntok = image if k == 2 else pixel
            seg = tok.double()[r * ntok: (r + 1) * ntok]
            E = seg.shape[1]
            e[b] = w.double() @ seg.mean(0) + bias.double()
            scale = w.double().abs() @ seg.abs().mean(0) + bias.double().abs()
            eb[b] = 8 * U * (math.sqrt(ntok) + math.sqrt(E) + 8) * scale
    return e, eb


def _goal_plan(g, counts, B):
    kinds = torch.tensor([0] * (B - sum(counts)) + [1] * counts[0] + [2] * counts[1] + [3] * counts[2], dtype=torch.int32)
    kinds = kinds[torch.randperm(B, generator=g)]
    rows = torch.zeros(B, dtype=torch.int32)
    for k, c in zip((1, 2, 3), counts):
        rows[kinds == k] = torch.randperm(c + 1, generator=g)[:c].int()
    return kinds.to(DEV), rows.to(DEV)


def _goal_check(out, buf, embed, kind, row, e, eb, pos, L, slot0, nslots, D, sentinel):
    B = kind.numel()
    o = out.view(B, L, D) if out.is_contiguous() else out.reshape(B, L, D)
    for j in range(nslots):
        ref = e + (pos.double()[slot0 + j] if pos is not None else 0.0)
        fb = eb + 4 * U * (ref.abs() + (pos.double()[slot0 + j].abs() if pos is not None else 0.0))
        _check(o[:, slot0 + j], ref, _out_bound(ref, fb, out.dtype), f"slot {slot0 + j}")
    if embed is not None:
        _check(embed, e, eb, "embed")
    keep = torch.ones(B, L, buf.shape[1], dtype=torch.bool, device=DEV)
    keep[:, slot0: slot0 + nslots, :D] = False
    assert bool((buf.view(B, L, -1)[keep] == sentinel).all()), "a row or column outside the goal slots was written"


TAIL_CASES = [(nt, E) for nt in (1, 7, 37, 256) for E in (4, 100, 384, 1024)]


@pytest.mark.parametrize("ntok,E", TAIL_CASES)
def test_goal_slots_mixed_kinds_token_tails(ops, ntok, E):
    """one batch of all four kinds with permuted rows; token means over ntok tokens with 256 / (E / 4) phases (1 .. 256)."""
    i = TAIL_CASES.index((ntok, E))
    g = torch.Generator().manual_seed(100 + i)
    D = (384, 96, 1024, 384)[i % 4]
    odt = (F32, BF16)[i % 2]
    L, slot0, nslots = ((6, 2, 3), (4, 0, 1), (8, 3, 5), (5, 1, 3))[i % 4]
    use_pos = i % 3 != 2
    counts, B = (3, 2, 3), 11
    point, image, pixel = _goal_inputs(g, D, E, ntok, counts)
    kind, row = _goal_plan(g, counts, B)
    pos = _randn((L, D), g) if use_pos else None
    sentinel = -9.0
    buf, out = _colview(B * L, D, odt, 8, fill=sentinel)
    embed = torch.full((B, D), float("nan"), device=DEV)
    ops.goal_slots(out, L, kind, row, pos=pos, slot0=slot0, nslots=nslots, embed=embed, point=point, image=image, pixel=pixel)
    e, eb = _goal_ref(kind, row, point, image, pixel, D)
    _goal_check(out, buf, embed, kind, row, e, eb, pos, L, slot0, nslots, D, sentinel)


@pytest.mark.parametrize("odt", [F32, BF16])
def test_goal_slots_point_bit_equal_embed3(ops, odt):
    """a point env's slots carry the bits embed3 writes for the same point and pos row."""
    g = torch.Generator().manual_seed(21)
    D, E, ntok, L, slot0, nslots = 384, 384, 16, 6, 1, 3
    counts, B = (5, 2, 2), 12
    point, image, pixel = _goal_inputs(g, D, E, ntok, counts)
    kind, row = _goal_plan(g, counts, B)
    pos = _randn((L, D), g)
    out = torch.zeros(B * L, D, dtype=odt, device=DEV)
    ops.goal_slots(out, L, kind, row, pos=pos, slot0=slot0, nslots=nslots, point=point, image=image, pixel=pixel)
    pts = (kind == 1).nonzero()[:, 0]
    for j in range(nslots):
        e3 = torch.empty(point[0].shape[0], D, dtype=odt, device=DEV)
        ops.embed3(point[0], point[1], point[2], out=e3, pos=pos[slot0 + j: slot0 + j + 1].contiguous())
        assert torch.equal(out.view(B, L, D)[pts, slot0 + j], e3[row[pts].long()]), f"slot {slot0 + j}"


def test_goal_slots_bad_entries_poison_only_their_env(ops):
    """a bad kind or an out-of-range row gives NaN in exactly that env's slots and embed row; every other env is exact."""
    g = torch.Generator().manual_seed(33)
    D, E, ntok, L, slot0, nslots = 384, 384, 7, 5, 1, 3
    counts = (2, 2, 2)
    point, image, pixel = _goal_inputs(g, D, E, ntok, counts)                 # 3 rows of each kind
    kind = torch.tensor([1, 4, 2, 3, 0, -1, 2, 1, 3, 1, 2], dtype=torch.int32, device=DEV)
    row = torch.tensor([2, 0, 1, 0, 0, 0, 3, -1, 2, 0, 1 << 20], dtype=torch.int32, device=DEV)
    bad = torch.tensor([0, 1, 0, 0, 0, 1, 1, 1, 0, 0, 1], dtype=torch.bool, device=DEV)
    B = kind.numel()
    pos = _randn((L, D), g)
    sentinel = 2.0
    for odt in (F32, BF16):
        buf, out = _colview(B * L, D, odt, 8, fill=sentinel)
        embed = torch.zeros(B, D, device=DEV)
        ops.goal_slots(out, L, kind, row, pos=pos, slot0=slot0, nslots=nslots, embed=embed, point=point, image=image, pixel=pixel)
        o = out.reshape(B, L, D)
        assert bool(o[bad][:, slot0: slot0 + nslots].isnan().all()) and bool(embed[bad].isnan().all())
        ok_kind = torch.where(bad, torch.zeros_like(kind), kind)
        ok_row = torch.where(bad, torch.zeros_like(row), row)
        e, eb = _goal_ref(ok_kind, ok_row, point, image, pixel, D)
        good = ~bad
        for j in range(nslots):
            ref = e[good] + pos.double()[slot0 + j]
            fb = eb[good] + 4 * U * (ref.abs() + pos.double()[slot0 + j].abs())
            _check(o[good][:, slot0 + j], ref, _out_bound(ref, fb, odt), f"good envs, slot {slot0 + j}")
        _check(embed[good], e[good], eb[good], "good envs, embed")
        keep = torch.ones(B, L, D + 8, dtype=torch.bool, device=DEV)
        keep[:, slot0: slot0 + nslots, :D] = False
        assert bool((buf.view(B, L, -1)[keep] == sentinel).all())
