"""ops.linear_mx4 (ina_gemm_mx4, csrc/gemm_skinny_mx4.hip) on the GPU; tests/test_w8_gemm_gpu.py case for case.

Two assertions per case, on every element:
  * the MXFP4 kernel's result has the BITS of the bf16 weight-streaming kernels (ina_gemm_bf16 kernel 32, with prenorm= kernel 30) run on
    the dequantised weights w_deq = q * 2^e - the contract of the entry: same K decomposition and summation order, an exact conversion with
    the block scale inside it;
  * it obeys the float64 reference of tests/gemm_ref.py on w_deq with the bound tests/test_gemm_fp64_gpu.py applies to the weight-streaming
    family (k = 4 x its measured worst ratio). The reference is never the code under test.
Shapes are the smallest that reach every branch: every MF (M = 1 .. 64), a ragged last column tile, GLU, one K step (the group clamps to one
wave), 3 steps (2 waves), 8 and 9 steps (uneven slices of 8 waves), the three `tiles` thresholds of the group width, the 4-wave and 8-wave
forms of the fused input RMSNorm. Weight rows carry magnitudes over 2^-6 .. 2^4, one zero row and one outlier element, so the block scales
differ along N, along K and inside a GLU pair. Row 2 holds e2m1 grid values * 2^64 and row 5 grid values * 2^-64: every block of them sits
at a clamp end of the scale (e8m0 bytes 191 and 63), the edges of the scale operand of the conversion, and both are still exact. Every
launch writes into sentinel-filled buffers whose outside is checked.

Size of the outlier: 8 x the row's largest |w|, as in the fp8 test, whose docstring has the reasoning (the fp64 bound is statistical and
presumes that no single term carries the sum; at 40 x one element of 2560 sat at 1.02 x the bound in the bf16 kernel too). The two clamp-end
rows are whole rows of one magnitude for the same reason: all K terms of their sums are comparable."""
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
    """(w4, wscale, w_deq, x f32 [64, K], bias, colscale, rowscale, residual f32 [64, N]) of one (N, K): built once, shared, never written"""
    if (N, K) not in _POOLS:
        g = torch.Generator(device=DEV).manual_seed(4000 + N * 7 + K)
        w = torch.randn(N, K, generator=g, device=DEV) * K ** -0.5 * torch.exp2(torch.randint(-6, 5, (N, 1), generator=g, device=DEV).float())
        w[1] = 0.0
        w[N // 2 + 3, K // 3] = 8.0 * float(w[N // 2 + 3].abs().max())              # (the factor: module docstring)
        grid = torch.tensor([0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], device=DEV)
        for row, e in ((2, 64), (5, -64)):                                            # (module docstring: the clamp ends of the block scale)
            v = grid[torch.randint(0, 7, (K,), generator=g, device=DEV)] * (torch.randint(0, 2, (K,), generator=g, device=DEV).float() * 2 - 1)
            v[::32] = 4.0
            w[row] = torch.ldexp(v, torch.tensor(e, device=DEV))
        w4, wscale, wd = ops.mx4_quantize(w.to(BF16))
        assert bool((wscale[2] == 191).all()) and bool((wscale[5] == 63).all()) and bool((wscale[1] == 127).all())
        assert torch.equal(wd[2].float(), w[2]) and torch.equal(wd[5].float(), w[5]) and int(wscale[8:].max()) > int(wscale[8:].min())
        x = torch.randn(64, K, generator=g, device=DEV) * torch.exp2(torch.randint(-2, 3, (64, 1), generator=g, device=DEV).float())
        _POOLS[(N, K)] = dict(w4=w4, wscale=wscale, wd=wd, x=x, bias=torch.randn(N, generator=g, device=DEV),
                              colscale=torch.rand(N, generator=g, device=DEV) + 0.5, rowscale=torch.rand(64, generator=g, device=DEV) + 0.5,
                              res=torch.randn(64, N, generator=g, device=DEV))
    return _POOLS[(N, K)]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _pair(ops, P, M, N, what, out_dtype=BF16, glu=False, prenorm=None, x_dtype=BF16, residual=None, alias=False, strided=False,
          layout="aligned", use=(), x=None, fp64=True):
    """one case through both kernels into sentinel buffers: bit equality, then (fp64=True) the fp64 bound. residual: None | dtype; use: the
    epilogue operands; x: the activations instead of the pool's"""
    K = P["wd"].shape[1]
    n_out = N // 2 if glu else N
    w4, wscale, wd = P["w4"][:N], P["wscale"][:N].contiguous(), P["wd"][:N]
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
    xx, w4x, wdx = (G.strided_rows(x), G.strided_rows(w4, 16), G.strided_rows(wd, 16)) if strided else (x, w4, wd)
    outs = []
    for mx4 in (True, False):
        buf = G.Buf(M, n_out, out_dtype, layout, DEV)
        res = None
        if res_val is not None:
            res = buf.fill(res_val) if alias else G.Buf(M, n_out, res_val.dtype, layout, DEV).fill(res_val)
        if mx4:
            ops.linear_mx4(xx, w4x, wscale, residual=res, out=buf.v, glu=glu, prenorm=prenorm, **ep)
        else:
            ops.linear(xx, wdx, residual=res, out=buf.v, glu=glu, prenorm=prenorm, force_cfg=0 if prenorm is not None else 32, **ep)
        torch.cuda.synchronize()
        assert buf.outside_untouched(), f"{what}: written outside the [{M}, {n_out}] result ({'mx4' if mx4 else 'bf16'} kernel)"
        outs.append(buf.v)
    a, b = outs
    if not torch.equal(_bits(a), _bits(b)):
        bad = _bits(a) != _bits(b)
        i = int(bad.reshape(-1).float().argmax())
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements differ from the bf16 kernel on w_deq; first at flat index {i}: "
                             f"mx4 {a.reshape(-1)[i].item():.9g} bf16 {b.reshape(-1)[i].item():.9g}")
    if not fp64:
        return
    ref, scale, aerr = G.linear_full(x, wd, residual=res_val, glu=glu, prenorm=prenorm, **ep)
    r = G.check(a, ref, scale, aerr, K, KWS, what)
    if a.dtype == F32:                                   # (the ratio leaves the 2^-8 |ref| allowance of a bf16 result out: fp32 results only)
        print(f"MX4_RATIO {what:44s} {r:.3f}")


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
        _pair(ops, P, 33, 40, f"row-strided A, W4 -> {n}", out_dtype=dt, strided=True, use=("bias", "colscale", "rowscale"), residual=F32, layout=layout)


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
        ops.linear_mx4(x, P["w4"], P["wscale"])
    with pytest.raises(Exception, match="M <= 16"):
        ops.linear_mx4(x[:17].float(), P["w4"], P["wscale"], prenorm=(torch.ones(384, device=DEV), 1e-6))
