"""FP8 weights of the weight-streaming GEMMs without a GPU: the quantiser (ops.w8_quantize), the packed row layout (ops.w8_pack / w8_unpack),
the C-ABI entry's presence and everything ina_gemm_w8 refuses - its validation is host arithmetic that runs before any HIP call."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops(built_lib):
    from internnav_amd import ops

    return ops


def _matrix(seed, N=48, K=256):
    """rows of magnitudes 2^-6 .. 2^4, an outlier element, a zero row, a row that needs e > 0 and a row with amax exactly 448 * 2^-3"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-6, 5, (N, 1), generator=g).float())
    w[3] = 0.0
    w[5, 7] = 3000.0
    w[9] *= 1.0e4
    w[11] = w[11].clamp(-56.0, 56.0)
    w[11, 0] = 56.0
    return w.to(BF16)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_quantiser_properties(ops, seed):
    w = _matrix(seed)
    w8, wexp, w_deq = ops.w8_quantize(w)
    assert w8.dtype == torch.uint8 and w8.shape == w.shape and wexp.dtype == torch.int8 and wexp.shape == (w.shape[0],) and w_deq.dtype == BF16
    e = wexp.to(torch.int32)
    q = ops.w8_unpack(w8).view(torch.float8_e4m3fn).double()
    assert bool(torch.isfinite(q).all()) and float(q.abs().max()) <= 448.0
    # w_deq is q * 2^e without any rounding: exact in bf16
    assert torch.equal(w_deq.double(), torch.ldexp(q, e[:, None].double()))
    # the exponent is the smallest that fits the row's amax (0 for the zero row)
    amax = w.double().abs().amax(1)
    fits = amax <= 448.0 * torch.exp2(e.double())
    tighter = amax <= 448.0 * torch.exp2(e.double() - 1)
    assert bool(fits.all()) and int(wexp[3]) == 0 and bool((~tighter | (amax == 0)).all())
    assert int(wexp[9]) > 0 and int(wexp[11]) == -3 and int(e.min()) >= -64 and int(e.max()) <= 64
    # q is the round-to-nearest-even e4m3 value of w / 2^e: never further than half an e4m3 step (2^-4 relative, 2^-10 absolute below 2^-6)
    x = torch.ldexp(w.double(), -e[:, None].double())
    assert bool(((q - x).abs() <= torch.maximum(x.abs() * 2.0 ** -4, torch.tensor(2.0 ** -10, dtype=torch.float64))).all())
    # idempotent on its own output
    w8b, _, w_deq2 = ops.w8_quantize(w_deq)
    assert torch.equal(w_deq2, w_deq)
    err = (w_deq.double() - w.double()).abs().mean() / w.double().abs().mean()
    print(f"W8_QUANT seed {seed}: mean |w_deq - w| / mean |w| = {float(err):.4f}")


def test_pack_layout(ops):
    N, K = 3, 384
    idx = torch.arange(K, dtype=torch.int32)
    x = (idx[None] + 7 * torch.arange(N, dtype=torch.int32)[:, None]).remainder(251).to(torch.uint8)
    p = ops.w8_pack(x)
    assert p.shape == x.shape and p.is_contiguous()
    assert torch.equal(ops.w8_unpack(p), x)
    for k in range(K):
        step, s, g, j = k // 128, (k % 128) // 32, (k % 32) // 8, k % 8
        assert torch.equal(p[:, step * 128 + g * 32 + s * 8 + j], x[:, k]), k
    with pytest.raises(AssertionError):
        ops.w8_pack(torch.zeros(4, 192, dtype=torch.uint8))


def test_entry_is_declared_and_bound(ops):
    from internnav_amd import _lib

    header = (ROOT / "include" / "internnav_amd.h").read_text()
    assert re.search(r"int ina_gemm_w8\(const ina_gemm_args\* args, const void\* W8, const int8_t\* wexp, void\* stream\);", header)
    assert "ina_gemm_w8" in _lib.SYMBOLS
    h = _lib.lib()
    assert h.ina_gemm_w8 is not None
    assert h.ina_abi_version() == 8 == _lib.ABI_VERSION
    assert re.search(r"#define INA_ABI_VERSION 8\b", header)


def _args(_lib, **kw):
    a = _lib.GemmArgs()
    a.A = a.C = 0x1000
    a.M, a.N, a.K = 7, 512, 256
    a.lda = a.ldw = 256
    a.ldc = a.ldr = 512
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,needle", [
    (dict(M=65), "M <= 64"),
    (dict(K=192, lda=192, ldw=192), "K % 128"),
    (dict(batch=2), "batch"),
    (dict(seg_stats=0x4000), "seg_stats"),
    (dict(Wp=0x4000), "Wp"),
    (dict(norm_gamma=0x4000, M=17), "M <= 16"),
    (dict(glu=1, R=0x2000), "residual"),
    (dict(glu=1, colscale=0x2000), "colscale"),
    (dict(glu=1, N=48, ldc=24), "N % 32"),
    (dict(act=7), "activation"),
    (dict(force_cfg=32), "force_cfg"),
    (dict(M=0), "empty"),
])
def test_refusals_need_no_gpu(ops, kw, needle):
    from internnav_amd import _lib

    h = _lib.lib()
    rc = h.ina_gemm_w8(C.byref(_args(_lib, **kw)), 0x8000, 0x9000, None)
    msg = h.ina_last_error().decode()
    assert rc != 0 and msg.startswith("gemm_w8") and needle in msg, (rc, msg)


def test_null_weight_pointers_are_refused(ops):
    from internnav_amd import _lib

    h = _lib.lib()
    assert h.ina_gemm_w8(C.byref(_args(_lib)), None, 0x9000, None) != 0 and "null" in h.ina_last_error().decode()
    assert h.ina_gemm_w8(C.byref(_args(_lib)), 0x8000, None, None) != 0 and "null" in h.ina_last_error().decode()
