"""ops.linear_w8 (ina_gemm_w8, csrc/gemm_skinny_w8.hip) on the GPU.

Two assertions per case, on every element:
  * the fp8 kernel's result has the BITS of the bf16 weight-streaming kernels (ina_gemm_bf16 kernel 32, with prenorm= kernel 30) run on the
    dequantised weights w_deq = q * 2^e - the contract of the entry: same K decomposition and summation order, exact conversions, exact scale;
  * it obeys the float64 reference of tests/gemm_ref.py on w_deq with the bound tests/test_gemm_fp64_gpu.py applies to the weight-streaming
    family (k = 4 x its measured worst ratio). The reference is never the code under test.
Shapes are the smallest that reach every branch: every MF (M = 1 .. 64), a ragged last column tile, GLU, one K step (the group clamps to one
wave), 3 steps (2 waves), 8 and 9 steps (uneven slices of 8 waves), the three `tiles` thresholds of the group width, the 4-wave and 8-wave
forms of the fused input RMSNorm. Weight rows carry magnitudes over 2^-6 .. 2^4, one zero row and one outlier element, so the exponents differ
along N and inside a GLU pair. Every launch writes into sentinel-filled buffers whose outside is checked.

Size of the outlier: 8 x the row's largest |w| (the row's exponent rises by 3, its other weights drop three binades inside e4m3). The bound
model of gemm_ref is statistical - k * (sqrt(K) + 4) units of 2^-24 * scale with k = 0.116, i.e. 1.77 units at K = 128 - and presumes that no
single term carries the sum: the final rounding alone costs |ref| / scale units and each of the K / 32 chained MFMA accumulations up to as much
again, so an element whose sum IS one term (|ref| ~ scale) can exceed 1.77 units in any correct fp32-accumulating kernel. With 8 x the outlier's
term stays below a quarter of scale at K = 128 (8 * 3 sigma against 128 * 0.8 sigma of the other terms). A first version of this file used
40 x: one element of 2560 (M = 64, N = 40, K = 128, out 525.122437, ref 525.122353) sat at 1.02 x the bound - in the fp8 AND in the bf16 kernel,
whose results were bit-equal."""
import pytest
import torch

from tests import gemm_ref as G
from tests.test_gemm_fp64_gpu import KFAM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
KWS = KFAM["weight-streaming"]
_POOLS = {}


@pytest.fixture(scope="module")
def ops(built_lib):
    from internnav_amd import ops

    return ops


def _pool(ops, N, K):
    """(w8, wexp, w_deq, x f32 [64, K], bias, colscale, rowscale, residual f32 [64, N]) of one (N, K): built once, shared, never written"""
    if (N, K) not in _POOLS:
        g = torch.Generator(device=DEV).manual_seed(8000 + N * 7 + K)
        w = torch.randn(N, K, generator=g, device=DEV) * K ** -0.5 * torch.exp2(torch.randint(-6, 5, (N, 1), generator=g, device=DEV).float())
        w[1] = 0.0
        w[N // 2 + 3, K // 3] = 8.0 * float(w[N // 2 + 3].abs().max())              # (the factor: module docstring)
        w8, wexp, wd = ops.w8_quantize(w.to(BF16))
        assert int(wexp.max()) > int(wexp.min()) and int(wexp[1]) == 0
        x = torch.randn(64, K, generator=g, device=DEV) * torch.exp2(torch.randint(-2, 3, (64, 1), generator=g, device=DEV).float())
        _POOLS[(N, K)] = dict(w8=w8, wexp=wexp, wd=wd, x=x, bias=torch.randn(N, generator=g, device=DEV),
                              colscale=torch.rand(N, generator=g, device=DEV) + 0.5, rowscale=torch.rand(64, generator=g, device=DEV) + 0.5,
                              res=torch.randn(64, N, generator=g, device=DEV))
    return _POOLS[(N, K)]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _pair(ops, P, M, N, what, out_dtype=BF16, glu=False, prenorm=None, x_dtype=BF16, residual=None, alias=False, strided=False,
          layout="aligned", use=(), x=None, fp64=True):
    """one case through both kernels into sentinel buffers: bit equality, then (fp64=True) the fp64 bound. residual: None | dtype; use: the
    epilogue operands; x: the activations instead of the pool's"""
    K = P["w8"].shape[1]
    n_out = N // 2 if glu else N
    w8, wexp, wd = P["w8"][:N], P["wexp"][:N].contiguous(), P["wd"][:N]
    x = (P["x"] if x is None else x)[:M].to(x_dtype).contiguous()
    ep = {}
    if "bias" in use:
        ep["bias"] = P["bias"][:N].contiguous()
    if "colscale" in use:
        ep["colscale"] = P["colscale"][:N].contiguous()
    if "rowscale" in use:
        ep.update(rowscale=P["rowscale"][:(M + 2) // 3].contiguous(), rowscale_div=3)
    if "silu" in use:
        ep["act"] = "silu"
    res_val = None if residual is None else P["res"][:M, :n_out].to(residual).contiguous()
    xx, w8x, wdx = (G.strided_rows(x), G.strided_rows(w8, 16), G.strided_rows(wd, 16)) if strided else (x, w8, wd)
    outs = []
    for fp8 in (True, False):
        buf = G.Buf(M, n_out, out_dtype, layout, DEV)
        res = None
        if res_val is not None:
            res = buf.fill(res_val) if alias else G.Buf(M, n_out, res_val.dtype, layout, DEV).fill(res_val)
        if fp8:
            ops.linear_w8(xx, w8x, wexp, residual=res, out=buf.v, glu=glu, prenorm=prenorm, **ep)
        else:
            ops.linear(xx, wdx, residual=res, out=buf.v, glu=glu, prenorm=prenorm, force_cfg=0 if prenorm is not None else 32, **ep)
        torch.cuda.synchronize()
        assert buf.outside_untouched(), f"{what}: written outside the [{M}, {n_out}] result ({'fp8' if fp8 else 'bf16'} kernel)"
        outs.append(buf.v)
    a, b = outs
    if not torch.equal(_bits(a), _bits(b)):
        bad = _bits(a) != _bits(b)
        i = int(bad.reshape(-1).float().argmax())
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements differ from the bf16 kernel on w_deq; first at flat index {i}: "
                             f"fp8 {a.reshape(-1)[i].item():.9g} bf16 {b.reshape(-1)[i].item():.9g}")
    if not fp64:
        return
    ref, scale, aerr = G.linear_full(x, wd, residual=res_val, glu=glu, prenorm=prenorm, **ep)
    r = G.check(a, ref, scale, aerr, K, KWS, what)
    if a.dtype == F32:                                   # (the ratio leaves the 2^-8 |ref| allowance of a bf16 result out: fp32 results only)
        print(f"W8_RATIO {what:44s} {r:.3f}")


@pytest.mark.parametrize("K", [128, 384, 1024, 1152])
def test_every_row_fragment_and_k_split(ops, K):
    P, Pg = _pool(ops, 40, K), _pool(ops, 96, K)
    for M in (1, 7, 16, 17, 33, 64):
        for N in (16, 40):
            _pair(ops, P, M, N, f"plain {M}x{N}x{K}", out_dtype=BF16 if M % 2 else F32)
        for N in (64, 96):
            _pair(ops, Pg, M, N, f"glu {M}x{N}x{K}", glu=True, use=("silu",), out_dtype=F32 if M % 2 else BF16)


@pytest.mark.parametrize("N,K,waves", [(65536, 256, 1), (32768, 256, 2), (16384, 512, 4)])
def test_group_width_thresholds(ops, N, K, waves):
    P = _pool(ops, N, K)
    _pair(ops, P, 7, N, f"{waves}-wave groups 7x{N}x{K}", use=("bias",))
    _pair(ops, P, 33, N, f"{waves}-wave groups 33x{N}x{K}", out_dtype=F32)


@pytest.mark.parametrize("layout", ["aligned", "unaligned"])
def test_epilogues(ops, layout):
    K = 384
    P, Pg = _pool(ops, 40, K), _pool(ops, 96, K)
    for dt in (BF16, F32):
        n = "bf16" if dt == BF16 else "f32"
        _pair(ops, P, 17, 40, f"bias -> {n}", out_dtype=dt, use=("bias",), layout=layout)
        _pair(ops, Pg, 17, 96, f"silu-glu + bias + rowscale -> {n}", out_dtype=dt, glu=True, use=("bias", "silu", "rowscale"), layout=layout)
        _pair(ops, P, 17, 40, f"colscale + rowscale -> {n}", out_dtype=dt, use=("colscale", "rowscale"), layout=layout)
        _pair(ops, P, 17, 40, f"silu + bias + colscale -> {n}", out_dtype=dt, use=("bias", "silu", "colscale"), layout=layout)
        for rdt in (BF16, F32):
            _pair(ops, P, 17, 40, f"residual {rdt} -> {n}", out_dtype=dt, residual=rdt, use=("bias",), layout=layout)
        _pair(ops, P, 17, 40, f"residual in place -> {n}", out_dtype=dt, residual=dt, alias=True, layout=layout)
        _pair(ops, P, 33, 40, f"row-strided A, W8 -> {n}", out_dtype=dt, strided=True, use=("bias", "colscale", "rowscale"), residual=F32, layout=layout)


@pytest.mark.parametrize("K,N,waves", [(512, 256, 4), (3584, 256, 8), (3584, 16384, 4)])
def test_fused_input_rmsnorm(ops, K, N, waves):
    """Bit equality on random rows (the normalisation itself is exercised: per-row magnitudes, random gamma). The fp64 bound needs an operand
    the reference can state exactly - bf16(x * rstd * gamma) of random values sits within an fp32 rounding of a bf16 tie for a few of the
    M * K elements, where the fp32 kernels and the fp64 reference legitimately round to different bf16 neighbours (2^-9 of one term, far
    above the GEMM's bound). So that check runs on gemm_ref.prenorm_cases' construction: rows of one power-of-two magnitude with random signs and
    integer gamma in [-4, 4], for which x * rstd is within 1e-6 of +-1 and the operand is exactly sign * gamma."""
    P = _pool(ops, N, K)
    g = torch.Generator(device=DEV).manual_seed(K + N)
    gamma = torch.randn(K, generator=g, device=DEV) * 0.25 + 1.0
    sign = torch.randint(0, 2, (16, K), generator=g, device=DEV).to(F32) * 2 - 1
    xs = sign * 2.0 ** torch.randint(0, 7, (16, 1), generator=g, device=DEV).to(F32)
    gi = torch.randint(-4, 5, (K,), generator=g, device=DEV).to(F32)
    i = 0
    for xdt in (F32, BF16):
        for M in (1, 7, 16):
            eps = (1e-6, 1e-5)[i % 2]
            i += 1
            n = f"{'f32' if xdt == F32 else 'bf16'} x {M}x{N}x{K} ({waves} waves)"
            _pair(ops, P, M, N, f"prenorm random {n}", x_dtype=xdt, prenorm=(gamma, eps), use=("bias",), fp64=False)
            eps0 = (0.0, 1e-6)[i % 2]
            assert torch.equal(G.prenorm_operand(xs[:M].to(xdt), gi, eps0).float(), (sign * gi)[:M]), "the normalised operand is not sign * gamma"
            _pair(ops, P, M, N, f"prenorm {n}", x_dtype=xdt, prenorm=(gi, eps0), use=("bias",), x=xs)
            if N == 256:
                _pair(ops, P, M, N, f"prenorm glu random {n}", x_dtype=xdt, prenorm=(gamma, eps), glu=True, use=("silu",), fp64=False)
                _pair(ops, P, M, N, f"prenorm glu {n}", x_dtype=xdt, prenorm=(gi, eps0), glu=True, use=("silu",), x=xs)
            if M == 7:
                _pair(ops, P, M, N, f"prenorm residual random {n}", x_dtype=xdt, prenorm=(gamma, eps), out_dtype=F32, residual=F32, alias=True, fp64=False)
                _pair(ops, P, M, N, f"prenorm residual {n}", x_dtype=xdt, prenorm=(gi, eps0), out_dtype=F32, residual=F32, alias=True, x=xs)


def test_refused_on_the_device_too(ops):
    """what the entry refuses raises, it is never computed another way"""
    P = _pool(ops, 40, 384)
    x = torch.zeros(65, 384, dtype=BF16, device=DEV)
    with pytest.raises(Exception, match="M <= 64"):
        ops.linear_w8(x, P["w8"], P["wexp"])
    with pytest.raises(Exception, match="M <= 16"):
        ops.linear_w8(x[:17].float(), P["w8"], P["wexp"], prenorm=(torch.ones(384, device=DEV), 1e-6))
