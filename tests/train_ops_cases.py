"""TEST INFRASTRUCTURE: the argument sets of the SFT-step kernel tests, shared by the GPU test (kernels against tests/train_ops_ref.py) and the
CPU test (tests/_cpu_kernels.py stand-ins against the same reference with the same arguments), so that "stand-in == kernel" is checked from
both sides. A case is a dict: op (name in train_ops), args, kw, n (reduction length of the bound), id, and optionally k (bound constant)."""
from __future__ import annotations

import torch

from tests import train_ops_ref as R

F32, BF16 = torch.float32, torch.bfloat16
DTN = {F32: "f32", BF16: "bf16"}

# Worst |err| / (2^-24 * scale) of the activation values / slopes as the kernels evaluate them (__expf, erff, tanhf), measured on an MI355X against
# train_ops_ref.act_value / act_slope over x in [-12, 12] (step 2^-10) plus +-{20, 50, 88, 100} - the table in the docstring of
# tests/test_train_kernels_fp64_gpu.py, printed again by its test_activation_error_table. The bound of the evaluation is 4 x that; the fp32
# operations around it (times dy, accumulate, the GLU product) keep the model's k = 16. fp32_bound multiplies k by (sqrt(1) + 4) = 5.
ACT_WORST = {("gelu_erf", "fwd"): 2.000, ("gelu_erf", "bwd"): 1.898, ("gelu_tanh", "fwd"): 1.889, ("gelu_tanh", "bwd"): 1.898,
             ("relu", "fwd"): 0.0, ("relu", "bwd"): 0.0, ("silu", "fwd"): 2.020, ("silu", "bwd"): 2.605, ("tanh", "fwd"): 1.273, ("tanh", "bwd"): 1.227}


def act_k(act, which):
    return 16.0 + 4.0 * ACT_WORST[(act, which)] / 5.0


def randn(shape, g, scale=1.0, dtype=F32, dev="cpu", shift=0.0):
    return (torch.randn(shape, generator=g, dtype=torch.float32) * scale + shift).to(dtype).to(dev)


def misaligned(t):
    """a copy of t whose storage starts 4 bytes (fp32) / 2 bytes (bf16) past a 16-byte boundary: forces the scalar kernels."""
    flat = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    out = flat[1: 1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == t.element_size()
    return out


def layout(t, how):
    """t [rows, C] re-stored as: dense | strided (row stride C + 8, aligned) | oddcol (a view starting at column 1, row stride C + 3) | mis."""
    if how == "dense":
        return t.contiguous()
    if how == "mis":
        return misaligned(t.contiguous())
    rows, C = t.shape
    extra, off = (8, 0) if how == "strided" else (3, 1)
    buf = torch.zeros(rows, C + extra, dtype=t.dtype, device=t.device)
    v = buf[:, off: off + C]
    v.copy_(t)
    return v


def case(op, id, n, *args, k=16.0, **kw):
    # cap: the fp32 part of an activation bound is never looser than the whole-tensor tolerance of test_train_ops_gpu.py (of max|ref|)
    cap = {"act_fwd": 2e-6, "glu_fwd": 2e-6, "act_bwd": 2e-5, "glu_bwd": 2e-5}.get(op)
    return dict(op=op, id=f"{op}-{id}", n=n, args=args, kw=kw, k=k, cap=cap)


# ---------------------------------------------------------------------------------------------------------------- element-wise
def ew_cases(dev):
    g = torch.Generator().manual_seed(100)
    out = []
    rows, C = 75, 384
    sfs = ("id", "one_plus", "tanh")
    i = 0
    for adt in (F32, BF16):
        for sdt in (F32, BF16):
            for bdt in (F32, BF16):
                for ydt in (F32, BF16):
                    s_div = (1, 32, 7)[i % 3]
                    x = randn((rows, C), g, dtype=adt, dev=dev)
                    s = randn(((rows + s_div - 1) // s_div, C), g, dtype=sdt, dev=dev)
                    b = randn((rows, C), g, dtype=bdt, dev=dev)
                    tab = randn((32, C), g, dev=dev) if i % 2 else None
                    out.append(case("affine", f"{DTN[adt]}-{DTN[sdt]}-{DTN[bdt]}-{DTN[ydt]}-div{s_div}", 1, x, scale=s, s_div=s_div, s_f=sfs[i % 3],
                                    base=b, tab=tab, out_dtype=ydt))
                    i += 1
    for how, Cc in (("dense", 384), ("strided", 384), ("oddcol", 384), ("mis", 384), ("dense", 390), ("strided", 6)):
        for s_div in (1, 32, 7):
            x = layout(randn((rows, Cc), g, dev=dev), how)
            s = layout(randn(((rows + s_div - 1) // s_div, Cc), g, dtype=BF16, dev=dev), how)
            b = layout(randn((rows, Cc), g, dev=dev), how)
            y = layout(torch.full((rows, Cc), float("nan"), device=dev), how)
            out.append(case("affine", f"{how}-C{Cc}-div{s_div}", 1, x, scale=s, s_div=s_div, s_f="tanh", base=b, tab=randn((32, Cc), g, dev=dev), out=y))
    for ydt in (F32, BF16):
        for how in ("dense", "oddcol"):
            x = layout(randn((rows, C), g, dev=dev), how)
            y = layout(randn((rows, C), g, dtype=ydt, dev=dev), how)
            out.append(case("affine", f"acc-{DTN[ydt]}-{how}", 1, x, scale=randn((rows, C), g, dev=dev), s_f="one_plus", out=y, accumulate=True))
    for act in R.ACTS:
        for xdt in (F32, BF16):
            for ydt in (F32, BF16):
                for how, Cc in (("dense", 384), ("dense", 390), ("strided", 384), ("mis", 384)):
                    x = layout(randn((rows, Cc), g, 3.0, dtype=xdt, dev=dev), how)
                    dy = layout(randn((rows, Cc), g, dtype=ydt, dev=dev), how)
                    tag = f"{act}-{DTN[xdt]}-{DTN[ydt]}-{how}-C{Cc}"
                    out.append(case("act_fwd", tag, 1, x, act, out_dtype=ydt, k=act_k(act, "fwd")))
                    out.append(case("act_bwd", tag, 1, x, dy, act, out_dtype=ydt, k=act_k(act, "bwd")))
        y = randn((rows, C), g, dtype=BF16, dev=dev)
        out.append(case("act_bwd", f"{act}-acc-bf16", 1, randn((rows, C), g, 3.0, dev=dev), randn((rows, C), g, dev=dev), act, out=y, accumulate=True,
                        k=act_k(act, "bwd")))
    kf, kb = act_k("silu", "fwd"), act_k("silu", "bwd")
    for dts in ((F32,) * 5, (BF16,) * 5, (BF16, F32, BF16, F32, BF16), (F32, BF16, F32, BF16, F32)):
        for how, Cc in (("dense", 384), ("strided", 384), ("oddcol", 384), ("mis", 384), ("dense", 390)):
            a, b, dy = (layout(randn((rows, Cc), g, 2.0, dtype=dt, dev=dev), how) for dt in dts[:3])
            da, db = (layout(torch.full((rows, Cc), float("nan"), dtype=dt, device=dev), how) for dt in dts[3:])
            tag = "-".join(DTN[d] for d in dts) + f"-{how}-C{Cc}"
            out.append(case("glu_fwd", tag, 1, a, b, out=layout(torch.full((rows, Cc), float("nan"), dtype=dts[3], device=dev), how), k=kf))
            out.append(case("glu_bwd", tag, 1, a, b, dy, da=da, db=db, k=max(kf, kb)))
    return out


def ew_big_cases(dev):
    """more elements than one trip of the grid-stride loops covers: 8192 blocks x 256 threads (x 4 columns in the vector kernel)."""
    g = torch.Generator().manual_seed(101)
    out = []
    for rows, C, tag in ((8200, 1028, "vec"), (2100, 1001, "scalar")):
        assert rows * C > 8192 * 256 * (4 if tag == "vec" else 1)
        x = randn((rows, C), g, dtype=BF16, dev=dev)
        s = randn(((rows + 6) // 7, C), g, dev=dev)
        out.append(case("affine", f"big-{tag}", 1, x, scale=s, s_div=7, s_f="one_plus", base=randn((rows, C), g, dev=dev), tab=randn((32, C), g, dev=dev),
                        out_dtype=BF16))
        out.append(case("act_bwd", f"big-{tag}", 1, randn((rows, C), g, 3.0, dev=dev), x, "gelu_tanh", out_dtype=F32, k=act_k("gelu_tanh", "bwd")))
    return out


# ---------------------------------------------------------------------------------------------------------------- column sums
VEC6 = [(F32, None), (BF16, None), (F32, BF16), (F32, F32), (BF16, BF16), (BF16, F32)]


def colsum_cases(dev):
    g = torch.Generator().manual_seed(200)
    out = []
    # chunk switch points, and chunk counts with nchunk % 8 in {0, 1, 7}: 224 -> 7, 256 -> 8, 288 -> 9, 768 -> 24, 2048 -> 64, 2049 / 4097 / 8193 -> 33
    for i, gr in enumerate((1, 31, 32, 33, 96, 224, 256, 288, 768, 2048, 2049, 4097, 8193)):
        groups = 3 if gr < 4000 else 2
        xdt, x2dt = VEC6[i % 6]
        x = randn((groups * gr, 200), g, dtype=xdt, dev=dev, shift=0.1)
        x2 = None if x2dt is None else randn((groups * gr, 200), g, dtype=x2dt, dev=dev)
        out.append(case("colsum", f"g{gr}-{DTN[xdt]}-{DTN.get(x2dt)}", gr, x, x2, group_rows=gr))
    for xdt, x2dt in VEC6:                                       # every vector instance on 3 chunks + 520 columns (3 column blocks, the last short)
        x = layout(randn((192, 520), g, dtype=xdt, dev=dev), "strided")
        x2 = None if x2dt is None else layout(randn((192, 520), g, dtype=x2dt, dev=dev), "strided")
        out.append(case("colsum", f"vec-{DTN[xdt]}-{DTN.get(x2dt)}", 96, x, x2, group_rows=96))
    # the scalar kernel by each trigger
    x, x2 = randn((192, 203), g, dev=dev), randn((192, 203), g, dtype=BF16, dev=dev)
    out.append(case("colsum", "scalar-C203", 96, x, x2, group_rows=96))
    x, x2 = randn((130, 200), g, dtype=BF16, dev=dev), randn((130, 200), g, dev=dev)
    out.append(case("colsum", "scalar-mis-x", 130, misaligned(x), x2))
    out.append(case("colsum", "scalar-mis-x2", 130, x, misaligned(x2)))
    out.append(case("colsum", "scalar-oddcol", 130, layout(x, "oddcol"), layout(x2, "oddcol")))
    col = randn((130, 3), g, dev=dev)
    W = randn((200, 3), g, dev=dev)
    out.append(case("colsum", "x2_bcast-out_cs3", 130, x, col[:, 1], out=W[:, 1], x2_bcast=True, out_cs=3))
    out.append(case("colsum", "x2_bcast-out_cs3-acc", 130, x, col[:, 2], out=W[:, 2], x2_bcast=True, out_cs=3, accumulate=True, scale=0.25))
    out.append(case("colsum", "x_bcast", 130, col[:, 0], x2, x_bcast=True))
    out.append(case("colsum", "x_bcast-groups", 26, col[:, 0:1], x, x_bcast=True, group_rows=26))
    # accumulate + scale, scale = 0 (meaning 1), single- and two-stage
    for gr in (24, 96):
        x = randn((gr * 2, 200), g, dev=dev)
        out.append(case("colsum", f"acc-scale-g{gr}", gr, x, None, out=randn((2, 200), g, dev=dev), group_rows=gr, accumulate=True, scale=0.5))
        out.append(case("colsum", f"scale0-g{gr}", gr, x, None, group_rows=gr, scale=0.0))
    return out


def colsum_big_case(dev):
    """the row count of the squared-gradient-norm reduction (256-row chunks: 372 of them)."""
    g = torch.Generator().manual_seed(201)
    x = randn((95232, 256), g, dev=dev)
    return case("colsum", "95232-sumsq", 95232, x, x)


# ---------------------------------------------------------------------------------------------------------------- norm backward
def _norm_case(g, dev, tag, rows, C, rms, gamma, xdt, dydt, dxdt, acc, how_x="dense", how_dx="dense", shift=0.6, spread=2.0, const_row=False):
    x = randn((rows, C), g, spread, dev=dev, shift=shift)
    if const_row:
        x[rows // 2] = 0.3
    x = layout(x.to(xdt), how_x)
    dy = randn((rows, C), g, dtype=dydt, dev=dev)
    ga = randn(C, g, 0.2, dev=dev, shift=1.0) if gamma else None
    kw = dict(eps=1e-5 if C != 4096 else 1e-6, rms=rms, want_xhat=True)
    if acc or how_dx != "dense":
        dx = randn((rows, C), g, dtype=dxdt, dev=dev) if acc else torch.full((rows, C), float("nan"), dtype=dxdt, device=dev)
        if how_dx == "odd":
            buf = torch.zeros(rows, C + 1, dtype=dxdt, device=dev)
            buf[:, :C] = dx
            dx = buf[:, :C]
        kw.update(dx=dx, accumulate=acc)
    else:
        kw.update(dx_dtype=dxdt)
    name = f"{tag}-r{rows}-C{C}-{'rms' if rms else 'ln'}-{'g' if gamma else 'nog'}-{DTN[xdt]}-{DTN[dydt]}-{DTN[dxdt]}{'-acc' if acc else ''}"
    return case("norm_bwd", name, C, x, dy, ga, **kw)


def norm_bwd_cases(dev):
    g = torch.Generator().manual_seed(300)
    out = []
    combos = [(F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16)]
    i = 0
    for C in (4, 64, 384, 4096, 5120, 770):
        for rms in (False, True):
            for gamma in (False, True):
                xdt, dydt = combos[i % 4]
                out.append(_norm_case(g, dev, "grid", (1, 3, 70)[i % 3], C, rms, gamma, xdt, dydt, (F32, BF16)[(i // 2) % 2], acc=i % 5 == 0))
                i += 1
    for xdt, dydt in combos:                       # all four vector instances, with the sft_llm form (bf16 x, f32 dy, accumulate into f32 dx)
        for rms in (False, True):
            out.append(_norm_case(g, dev, "inst", 70, 384, rms, True, xdt, dydt, F32, acc=True))
            out.append(_norm_case(g, dev, "inst", 3, 4096, rms, False, xdt, dydt, BF16, acc=True))
    for rms in (False, True):                      # the scalar kernel by pointer / stride
        out.append(_norm_case(g, dev, "mis-x", 70, 384, rms, True, F32, F32, F32, acc=False, how_x="mis"))
        out.append(_norm_case(g, dev, "mis-x", 3, 384, rms, True, BF16, BF16, BF16, acc=False, how_x="mis"))
        out.append(_norm_case(g, dev, "odd-lddx", 70, 384, rms, False, F32, BF16, F32, acc=True, how_dx="odd"))
        out.append(_norm_case(g, dev, "odd-lddx", 3, 64, rms, True, BF16, F32, BF16, acc=False, how_dx="odd"))
    for C in (8, 384, 770):                        # LayerNorm far from the origin: mean = 64 x spread
        out.append(_norm_case(g, dev, "offset", 70, C, False, True, F32, F32, F32, acc=False, shift=64.0, spread=1.0))
        out.append(_norm_case(g, dev, "offset", 70, C, True, True, F32, F32, F32, acc=False, shift=64.0, spread=1.0))
    for C in (384, 770):                           # one constant row: variance 0, rstd = eps^-1/2
        for rms in (False, True):
            out.append(_norm_case(g, dev, "const-row", 3, C, rms, True, F32, F32, F32, acc=False, const_row=True))
    return out


# ---------------------------------------------------------------------------------------------------------------- the small ones
def transpose_cases(dev):
    g = torch.Generator().manual_seed(400)
    out = []
    for rows, cols in ((1, 1), (63, 65), (64, 64), (257, 130), (128, 200)):
        for pad in (1, 8, 64):
            for dt in (F32, BF16):
                x = randn((rows, cols), g, dtype=dt, dev=dev)
                ldy = (rows + pad - 1) // pad * pad
                out.append(case("transpose", f"{rows}x{cols}-pad{pad}-{DTN[dt]}", 1, x, pad=pad, out=torch.full((cols, ldy), float("nan"), dtype=BF16, device=dev)))
    x = randn((257, 140), g, dtype=BF16, dev=dev)
    out.append(case("transpose", "view", 1, x[:, 3:133], pad=8, out=torch.full((130, 264), float("nan"), dtype=BF16, device=dev)))
    out.append(case("transpose", "rowslice", 1, randn((300, 70), g, dev=dev)[41:], pad=64))
    return out


def sparse_rows_cases(dev):
    g = torch.Generator().manual_seed(500)
    out = []
    for C in (3, 96, 384, 1000):
        for taps in (1, 16):
            n_in, n_out = 50, 20
            inp = randn((n_in, C), g, dev=dev)
            idx = torch.randint(-1, n_in, (n_out, taps), generator=g).int()
            idx[0] = -1                                    # a row without any tap
            idx[1] = 7                                     # the same source row in every tap
            idx, coef = idx.to(dev), randn((n_out, taps), g, dev=dev)
            out.append(case("sparse_rows", f"C{C}-taps{taps}", taps, inp, idx, coef, out=torch.full((n_out, C), float("nan"), device=dev)))
            out.append(case("sparse_rows", f"C{C}-taps{taps}-acc", taps, inp, idx, coef, out=randn((n_out, C), g, dev=dev), accumulate=True))
    return out


def small_linear_cases(dev):
    g = torch.Generator().manual_seed(600)
    out = []
    for rows, K, N in ((64, 3, 384), (64, 384, 3), (128, 384, 1), (5, 1, 8), (4200, 3, 384)):
        for xdt in (F32, BF16):
            for ydt in (F32, BF16):
                x = randn((rows, K), g, dtype=xdt, dev=dev)
                w, b = randn((N, K), g, K ** -0.5, dev=dev), randn(N, g, dev=dev)
                tab = randn((32, N), g, dev=dev) if ydt == F32 else None          # 32 does not divide 5, 4200
                out.append(case("small_linear", f"{rows}x{K}x{N}-{DTN[xdt]}-{DTN[ydt]}", K, x, w, b, tab, out_dtype=ydt))
    assert 4200 * 384 > 4096 * 256
    rows, K, N = 80, 3, 384
    wide = randn((rows + 16, K + 5), g, dtype=BF16, dev=dev)
    w, b, tab = randn((N, K), g, dev=dev), randn(N, g, dev=dev), randn((32, N), g, dev=dev)
    out.append(case("small_linear", "x-colview-tab32-rows80", K, wide[:rows, :K], w, b, tab))
    out.append(case("small_linear", "x-rowslice-tab32-rows80", K, wide[16:, 2: 2 + K], w, None, tab, out_dtype=BF16))
    big = torch.full((rows, N), 1000.0, device=dev)                                    # a table that is the head of a longer buffer: rows past it are not the table
    big[:32] = tab
    out.append(case("small_linear", "tab-head-of-80-rows", K, randn((rows, K), g, dev=dev), w, b, big[:32]))
    wt = randn((N, K), g, dev=dev).t()                                               # [K, N] view with strides (1, K): dX = dy @ W of nn.Linear(N, K)
    assert not wt.is_contiguous()
    out.append(case("small_linear", "w_transposed-noncontig", K, randn((rows, K), g, dev=dev), wt, w_transposed=True))
    w2 = randn((3, 384), g, dev=dev)
    out.append(case("small_linear", "w_transposed", 3, randn((rows, 3), g, dev=dev), w2, w_transposed=True))
    outv = torch.zeros(rows, N + 8, device=dev)[:, 4: 4 + N]
    out.append(case("small_linear", "out-view", K, randn((rows, K), g, dev=dev), w, b, out=outv))
    return out


def mse_cases(dev):
    g = torch.Generator().manual_seed(700)
    out = []
    for nseq, T, D in ((6, 32, 3), (300, 1, 1), (1, 1, 1), (64, 24, 3)):
        masks = {"ones": torch.ones(nseq), "mixed": (torch.rand(nseq, generator=g) < 0.6).float(), "zero": torch.zeros(nseq),
                 "frac": torch.rand(nseq, generator=g) * 1.5}
        if nseq > 1:
            masks["mixed"][0], masks["mixed"][-1] = 1.0, 0.0
        for i, (mname, mask) in enumerate(masks.items()):
            for ls in (1.0, 0.4 / 3):
                pdt = (F32, BF16)[i % 2] if ls == 1.0 else (BF16, F32)[i % 2]
                rows = nseq * T
                how = ("dense", "wide", "tail")[(i + (ls != 1.0)) % 3]
                p = randn((rows, D), g, dtype=pdt, dev=dev)
                if how == "wide":
                    buf = randn((rows, D + 5), g, dtype=pdt, dev=dev)
                    buf[:, :D] = p
                    p = buf[:, :D + 2]                     # pred may be wider than D: the kernel reads the first D columns of a free row stride
                elif how == "tail":
                    buf = randn((rows + 7, D), g, dtype=pdt, dev=dev)
                    buf[7:] = p
                    p = buf[7:]
                tgt = randn((rows, D), g, dev=dev)
                n = rows * D + nseq
                out.append(case("mse_masked", f"{nseq}x{T}x{D}-{mname}-ls{ls:.3f}-{DTN[pdt]}-{how}", n, p, tgt, mask.to(dev), T, loss_scale=ls))
        out.append(case("mse_masked", f"{nseq}x{T}x{D}-nograd", nseq * T * D + nseq, randn((nseq * T, D), g, dev=dev), randn((nseq * T, D), g, dev=dev),
                        torch.ones(nseq).to(dev), T, want_grad=False))
    return out


ALL = dict(ew=ew_cases, ew_big=ew_big_cases, colsum=colsum_cases, norm_bwd=norm_bwd_cases, transpose=transpose_cases, sparse_rows=sparse_rows_cases,
           small_linear=small_linear_cases, mse=mse_cases)


# ---------------------------------------------------------------------------------------------------------------- running a case
def check(out, ref, bound, what):
    """every element within its bound (a NaN in out counts as a failure); returns the worst |err| / bound."""
    err = (out.double() - ref).abs()
    ok = err <= bound
    n_bad = int((~ok).sum())
    ratio = (err / bound).nan_to_num(nan=float("inf"))
    if n_bad:
        i = int(ratio.reshape(-1).argmax())
        raise AssertionError(f"{what}: {n_bad}/{err.numel()} elements out of bound; worst at flat index {i}: out "
                             f"{out.reshape(-1)[i].item():.9g} ref {ref.reshape(-1)[i].item():.9g} bound {bound.reshape(-1)[i].item():.3g}")
    return float(ratio.max()) if ratio.numel() else 0.0


def _pairs(res):
    return [res] if isinstance(res[0], torch.Tensor) else list(res)


def run_case(impl, c):
    """call the reference, then impl[op] with the case's arguments; every result element within the case's bound. impl: name -> callable."""
    op, args, kw = c["op"], c["args"], c["kw"]
    if op == "transpose":
        y = impl[op](*args, **kw)
        ref = R.transpose(*args, **kw)
        assert y.dtype == BF16 and y.shape == ref.shape and torch.equal(y, ref), f"{c['id']}: transpose is exact (zero tail included)"
        return 0.0
    refs = _pairs(getattr(R, op)(*args, **kw))
    res = impl[op](*args, **kw)
    outs = list(res) if isinstance(res, (tuple, list)) else [res]
    worst = 0.0
    for j, ((ref, scale), o) in enumerate(zip(refs, outs)):
        if o is None:
            assert op in ("norm_bwd", "mse_masked") and j == 1
            continue
        assert torch.isfinite(ref).all()
        fb = R.fp32_bound(scale, c["n"], c["k"])
        if c.get("cap"):
            fb = torch.minimum(fb, torch.full_like(fb, c["cap"] * float(ref.abs().max())))
        bound = R.out_bound(ref, fb, o.dtype)
        if op == "norm_bwd" and j == 1:                                  # xhat is stored in bf16
            assert o.dtype == BF16
        worst = max(worst, check(o.reshape(ref.shape), ref, bound, f"{c['id']} result {j}"))
    if op == "mse_masked" and not c["kw"].get("want_grad", True):
        assert outs[1] is None
    return worst


# ---------------------------------------------------------------------------------------------------------------- AdamW
ADAMW_VARIANTS = [dict(id="clip-scale1", grad_scale=1.0, max_norm=1.0, p_bf16=True, norm_out=True, zero_grad=True, step0=1),
                  dict(id="clip-scale.125", grad_scale=0.125, max_norm=1.0, p_bf16=True, norm_out=True, zero_grad=False, step0=1),
                  dict(id="noclip-scale.125", grad_scale=0.125, max_norm=0.0, p_bf16=False, norm_out=False, zero_grad=True, step0=1),
                  dict(id="nonorm", grad_scale=1.0, max_norm=0.0, p_bf16=False, norm_out=False, zero_grad=False, step0=1, no_parts=True),
                  dict(id="step10000", grad_scale=1.0, max_norm=1.0, p_bf16=True, norm_out=True, zero_grad=True, step0=10000),
                  dict(id="slice", grad_scale=1.0, max_norm=1.0, p_bf16=True, norm_out=True, zero_grad=True, step0=1, slice=True)]
ADAMW_N = 4096 * 256 + 777            # a second trip of the grid-stride loop (grid capped at 4096 blocks) and a ragged last block
HP = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)


def adamw_run(adamw, sumsq_parts, dev, var, n=ADAMW_N, steps=4):
    """4 steps of the fused AdamW; every step is checked against the float64 restatement applied to the state that step received (p, m, v as
    given), per element. Gradient scales alternate so that the norm is far above (odd steps) and far below (even steps) max_norm."""
    g = torch.Generator().manual_seed(800)
    npad = (n + 1023) // 1024 * 1024
    p = randn(n, g, dev=dev)
    m, v = randn(n, g, 0.01, dev=dev), (randn(n, g, 0.01, dev=dev) ** 2)
    if var["step0"] == 1:
        m.zero_(), v.zero_()
    lo, hi = (1235, n - 77) if var.get("slice") else (0, n)          # the slice form: p32[lo:hi] with the norm of the whole buffer
    pb = torch.zeros(n, dtype=BF16, device=dev) if var["p_bf16"] else None
    norm = torch.full((1,), float("nan"), device=dev) if var["norm_out"] else None
    worst = 0.0
    for s in range(steps):
        step = var["step0"] + s
        gpad = torch.zeros(npad, device=dev)
        gpad[:n] = randn(n, g, (3.0 if s % 2 == 0 else 1e-5) / var["grad_scale"], dev=dev)
        grad = gpad[:n].clone()
        parts = None if var.get("no_parts") else sumsq_parts(gpad)
        ref = R.adamw(p[lo:hi], grad[lo:hi], m[lo:hi], v[lo:hi], step=step, sumsq=None if parts is None else gpad.double().pow(2).sum().item(),
                      max_norm=var["max_norm"], grad_scale=var["grad_scale"], **HP)
        if var["max_norm"] > 0:
            assert (ref["clip"] < 0.5) == (s % 2 == 0), "the cases are meant to clip on steps 0, 2 and not on 1, 3"
        g_before, p_before = grad.clone(), p.clone()
        adamw(p[lo:hi], grad[lo:hi], m[lo:hi], v[lo:hi], step=step, p_bf16=None if pb is None else pb[lo:hi], sumsq_parts=parts,
              max_norm=var["max_norm"], grad_scale=var["grad_scale"], norm_out=norm, zero_grad=var["zero_grad"], **HP)
        rel = R.norm_rel_bound(npad)
        for key in ("p", "m", "v"):
            o = dict(p=p, m=m, v=v)[key][lo:hi]
            bound = R.fp32_bound(ref["s" + key], 1) + 2.0 * rel * ref["c" + key]
            worst = max(worst, check(o, ref[key], bound, f"adamw {var['id']} step {step} {key}"))
        if norm is not None:
            assert abs(norm.item() - ref["norm"]) <= rel * ref["norm"], f"norm_out {norm.item()} vs {ref['norm']}"
        if pb is not None:
            assert torch.equal(pb[lo:hi], p[lo:hi].to(BF16)), "the bf16 working copy is the rounded fp32 weight"
        if var["zero_grad"]:
            assert bool((grad[lo:hi] == 0).all()), "zero_grad"
        else:
            assert torch.equal(grad, g_before), "the gradient is read-only without zero_grad"
        assert torch.equal(grad[:lo], g_before[:lo]) and torch.equal(grad[hi:], g_before[hi:]), "elements outside the slice were written"
        assert torch.equal(p[:lo], p_before[:lo]) and torch.equal(p[hi:], p_before[hi:]), "weights outside the slice were written"
    return worst
