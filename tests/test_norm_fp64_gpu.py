"""Op-level GPU tests of the norm family (internnav_amd/csrc/norm.hip, 14 instances: 8-element chunks per lane NCH 1 / 2 / 4 / 8 / 16, rows per
wave RPW 4 / 2 / 1, bf16 / f32 input) against the float64 restatement of tests/s2_ops_ref.py on the same inputs: both sides of every dispatch
edge (C = 128|136, 256|264, 512|520, 1024|1032, 2048|2056, 4096|4104, 8192|8200 refused), row counts that leave partial row groups, rows with
a mean far from zero, every optional operand in one launch with the logical / physical row distinction that in_map / out_map create, and the
chained second norm.

Tolerance model (that of test_train_kernels_fp64_gpu.py), per element, every element checked:
  fp32 results: |err| <= k * 2^-24 * (sqrt(C) + 4) * scale, scale the float64 sum of |terms| (s2_ops_ref.norm: LayerNorm carries
                |x|max * rstd, tanh(g) carries 1 + |g|, the chained norm carries the error bound of its input);
  bf16 results: + 2^-8 * |ref|;
  rows and columns of the output buffers that no logical row maps to: unchanged (sentinel).
k is measured, per statistic type: every check records the worst |err| / (2^-24 * (sqrt(C) + 4) * scale) of the fp32 results and the last test
of the file prints it; k = 4 x the value measured on an MI355X (ROCm 7) over all launches of this file, far under the cap of 16:
    LayerNorm  worst 0.162 (C = 8, fp32 rows with mean 64 x spread; width edges alone: 0.119 at C = 8, 0.010 at C = 8192)  -> k = 0.648
    RMSNorm    worst 0.396 (C = 8, the same rows;                    width edges alone: 0.258 at C = 8, 0.050 at C = 8192)  -> k = 1.584
(fp32 torch on the CPU against the same reference: 0.24 / 0.29, tests/test_s2_ops_ref_cpu.py.)
"""
import pytest
import torch

from tests import s2_ops_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U = S.U
WIDTHS = (8, 128, 136, 256, 264, 512, 520, 1024, 1032, 2048, 2056, 4096, 4104, 8192)
LN_WORST, RMS_WORST = 0.162, 0.396      # measured, see above
K = {False: min(16.0, 4.0 * LN_WORST), True: min(16.0, 4.0 * RMS_WORST)}          # keyed by `rms`
SENT = -7.0
WORST = {False: 0.0, True: 0.0}         # worst fp32 ratio seen by _check so far, per statistic type (printed by the last test of the file)


@pytest.fixture(scope="module")
def ops(built_lib):
    from internnav_amd import ops

    return ops


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, g, dtype=F32, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=g, device=DEV, dtype=F32) * scale + shift).to(dtype)


def _check(out, ref, scale, C, rms, what):
    """every element of one result within its bound; returns the worst |err| / (2^-24 * (sqrt(C) + 4) * scale), the quantity k multiplies."""
    assert out.shape == ref.shape and torch.isfinite(ref).all()
    err = (out.to(F64) - ref).abs()
    bound = S.out_bound(ref, S.fp32_bound(scale, C, K[rms]), out.dtype)
    bad = ~(err <= bound)
    if bad.any():
        i = int((err / bound).nan_to_num(nan=float("inf")).reshape(-1).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())}/{err.numel()} elements out of bound; worst at flat index {i}: out "
                             f"{out.reshape(-1)[i].item():.9g} ref {ref.reshape(-1)[i].item():.9g} bound {bound.reshape(-1)[i].item():.3g}")
    ratio = (err / S.fp32_bound(scale, C, 1.0)).max().item()
    if out.dtype == F32:
        WORST[rms] = max(WORST[rms], ratio)
    return ratio


def _launch(ops, x, rows, C, rms, what, out_map=None, phys_out=None, chained=False, **kw):
    """reference, then one launch writing out (bf16), out32 (f32) (and out2) into sentinel-filled buffers 8 columns wider than C; checks all
    results and the sentinel. Returns (worst fp32 ratio, out32 rows, out2 rows)."""
    phys_out = phys_out or rows
    out = torch.full((phys_out, C + 8), SENT, dtype=BF16, device=DEV)
    out32 = torch.full((phys_out, C + 8), SENT, dtype=F32, device=DEV)
    out2 = torch.full((phys_out, C + 8), SENT, dtype=BF16, device=DEV) if chained else None
    kw = dict(kw, rms=rms, rows=rows, out_map=out_map, out=out[:, :C], out32=out32[:, :C], out2=out2[:, :C] if chained else None)
    (ref, scale), second = S.norm(x, **kw)
    ops.norm(x, **kw)
    torch.cuda.synchronize()
    pr = S.map_rows(rows, out_map, DEV)
    worst = _check(out32[pr, :C], ref, scale, C, rms, what + " out32")
    _check(out[pr, :C], ref, scale, C, rms, what + " out")
    bufs = [out, out32]
    if chained:
        _check(out2[pr, :C], *second, C, rms, what + " out2")
        bufs.append(out2)
    untouched = torch.ones(phys_out, dtype=torch.bool, device=DEV)
    untouched[pr] = False
    for b in bufs:
        assert (b[untouched] == SENT).all() and (b[:, C:] == SENT).all(), f"{what}: written outside the mapped rows / the C columns"
    return worst, out32[pr, :C], (out2[pr, :C] if chained else None)


# ------------------------------------------------------------------------------------------------------------------------ dispatch edges
@pytest.mark.parametrize("rms", [False, True], ids=["layernorm", "rms"])
def test_norm_width_edges(ops, rms):
    """both sides of every launch_norm edge x bf16 / f32 input x rows in (1, 37, 50): 37 leaves a partial rows-per-wave group for RPW 4 and 2
    (C <= 256), 50 is no multiple of 4 * RPW for any RPW; out and out32 in the same launch, gamma and beta present. Prints the measurement k is
    derived from."""
    g = _gen(1 + int(rms))
    worst = {}
    for C in WIDTHS:
        gamma, beta = _randn((C,), g, shift=1.0), _randn((C,), g)
        for xdt in (BF16, F32):
            for rows in (1, 37, 50):
                x = _randn((rows, C), g, xdt, scale=1.5, shift=0.25)
                w, _, _ = _launch(ops, x, rows, C, rms, f"C={C} {xdt} rows={rows}", gamma=gamma, beta=beta, eps=1e-6)
                worst[C] = max(worst.get(C, 0.0), w)
    print(f"NORM_K rms={rms}: worst |err| / (2^-24 (sqrt(C) + 4) scale) per C: " + ", ".join(f"{c}: {v:.3f}" for c, v in worst.items()))
    print(f"NORM_K rms={rms}: overall worst {max(worst.values()):.3f} (bound constant in use: {K[rms]})")


def test_norm_refuses_8200(ops):
    x = torch.zeros(3, 8200, dtype=BF16, device=DEV)
    with pytest.raises(Exception, match="too wide"):
        ops.norm(x)
    torch.cuda.synchronize()


@pytest.mark.parametrize("C", [8, 384, 8192])
def test_norm_mean_offset(ops, C):
    """LayerNorm rows whose mean is 64 x their spread (and an RMS launch of the same rows): a one-pass E[x^2] - mean^2 variance loses 12 bits
    here, the two-pass form the kernel uses does not."""
    g = _gen(10 + C)
    gamma, beta = _randn((C,), g, shift=1.0), _randn((C,), g)
    for xdt in (F32, BF16):
        for rows in (5, 37):
            x = _randn((rows, C), g, xdt, scale=1.0, shift=64.0)
            x[1] = -x[1]
            for rms in (False, True):
                w, _, _ = _launch(ops, x, rows, C, rms, f"offset C={C} {xdt} rows={rows} rms={rms}", gamma=gamma, beta=beta, eps=1e-5)
                print(f"norm mean offset C={C} {xdt} rows={rows} rms={rms}: worst ratio {w:.3f}")


# ------------------------------------------------------------------------------------------------------------------------ every operand
@pytest.mark.parametrize("rms", [False, True], ids=["layernorm", "rms"])
@pytest.mark.parametrize("C", [128, 136, 384, 1032])
def test_norm_every_operand_in_one_launch(ops, C, rms):
    """gamma, beta, mod_scale, gate, base (bf16 and f32), pos, in_map, out_map in one launch of 50 logical rows:
    mod_div = 8 (7 modulation rows, the last one used by 2 rows), pos of 12 rows (50 % 12 != 0), mod_scale / gate column slices of one
    [*, 3 C] tensor, in_map = segments of 5 rows every 8 from row 3, out_map = segments of 10 every 13 from row 2 into a wider, longer
    sentinel-filled buffer. Modulation, base and pos follow the logical row. (The modulation tensor and the bf16 base are allocated taller than
    what a correct kernel reads, so that a wrongly indexed or wrongly typed read returns wrong values instead of leaving the allocation.)"""
    g = _gen(100 + C + int(rms))
    rows, mod_div, in_map, out_map = 50, 8, (5, 8, 3), (10, 13, 2)
    x_rows = int(S.map_rows(rows, in_map)[-1]) + 3
    phys_out = int(S.map_rows(rows, out_map)[-1]) + 4
    gamma, beta = _randn((C,), g, shift=1.0), _randn((C,), g)
    mod = _randn((64, 3 * C), g, scale=0.7)          # rows 0..6 are the ones in use
    pos = _randn((12, C), g)
    for xdt in (BF16, F32):
        xb = _randn((x_rows, C + 8), g, xdt, scale=2.0, shift=0.5)
        for bdt in (BF16, F32):
            base = _randn((2 * rows, C + 8), g, bdt)[:rows, :C]
            w, _, _ = _launch(ops, xb[:, :C], rows, C, rms, f"all operands C={C} x {xdt} base {bdt}", out_map=out_map, phys_out=phys_out,
                              gamma=gamma, beta=beta, eps=1e-5, mod_scale=mod[:, C:2 * C], gate=mod[:, 2 * C:], base=base, mod_div=mod_div,
                              pos=pos, in_map=in_map)
            print(f"norm all operands C={C} rms={rms} x {xdt} base {bdt}: worst ratio {w:.3f}")


# ------------------------------------------------------------------------------------------------------------------------ chained second norm
@pytest.mark.parametrize("rms", [False, True], ids=["layernorm", "rms"])
@pytest.mark.parametrize("C", [128, 384, 3584])
def test_norm_chained_out2(ops, C, rms):
    """out2 = norm(t) * gamma2 * (1 + mod_scale2) of the row just produced, against the reference (from the fp32-rounded t), with every first-stage
    operand present and a residual whose mean is 64 x its spread; out32 is bit-equal to the launch without out2."""
    g = _gen(200 + C + int(rms))
    rows, mod_div = 37, 5
    gamma, gamma2 = _randn((C,), g, shift=1.0), _randn((C,), g, shift=1.0)
    mod = _randn((40, 3 * C), g, scale=0.7)          # rows 0..7 are the ones in use (allocated taller, see above)
    x = _randn((rows, C), g, BF16, scale=2.0)
    base = _randn((rows, C), g, F32, shift=64.0)
    base[3] = -base[3]
    kw = dict(gamma=gamma, eps=1e-6, mod_scale=mod[:, :C], gate=mod[:, C:2 * C], base=base, mod_div=mod_div)
    w, y32, _ = _launch(ops, x, rows, C, rms, f"chained C={C}", chained=True, gamma2=gamma2, mod_scale2=mod[:, 2 * C:], **kw)
    _, y32_plain, _ = _launch(ops, x, rows, C, rms, f"unchained C={C}", **kw)
    assert torch.equal(y32.view(torch.int32), y32_plain.view(torch.int32)), "out32 of the chained launch differs from the unchained one"
    print(f"norm chained C={C} rms={rms}: worst first-stage ratio {w:.3f}")


@pytest.mark.parametrize("rms", [False, True], ids=["layernorm", "rms"])
def test_norm_chained_in_place_on_base(ops, rms):
    """the residual update as the engine issues it: out32 IS base (each element is read and written by the same lane), out2 the next pre-norm."""
    g = _gen(300 + int(rms))
    rows, C = 50, 384
    gamma, gamma2 = _randn((C,), g, shift=1.0), _randn((C,), g, shift=1.0)
    x = _randn((rows, C), g, BF16, scale=2.0)
    resid = _randn((rows, C), g, F32, shift=8.0)
    out2 = torch.full((rows, C), SENT, dtype=BF16, device=DEV)
    kw = dict(gamma=gamma, eps=1e-6, rms=rms, base=resid, out32=resid, out2=out2, gamma2=gamma2)
    (ref, scale), (ref2, scale2) = S.norm(x, **kw)
    ops.norm(x, **kw)
    torch.cuda.synchronize()
    _check(resid, ref, scale, C, rms, "in place out32")
    _check(out2, ref2, scale2, C, rms, "in place out2")


def test_norm_worst_ratio_report(ops):
    """runs last: the worst fp32 ratio over every launch of this file, the figure LN_WORST / RMS_WORST record."""
    print(f"NORM_K_ALL LayerNorm {WORST[False]:.3f} (K {K[False]:.3f}), RMSNorm {WORST[True]:.3f} (K {K[True]:.3f})")
    assert WORST[False] <= K[False] and WORST[True] <= K[True]
