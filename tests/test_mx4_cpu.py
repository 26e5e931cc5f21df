"""MXFP4 weights of the weight-streaming GEMMs without a GPU: the quantiser (ops.mx4_quantize), the packed row layout (ops.mx4_pack /
mx4_unpack), the C-ABI entry's presence and everything ina_gemm_mx4 refuses - its validation is host arithmetic that runs before any HIP
call."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
BF16 = torch.bfloat16
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


@pytest.fixture(scope="module")
def ops(built_lib):
    from internnav_amd import ops

    return ops


def _matrix(seed, N=48, K=256):
    """rows of magnitudes 2^-6 .. 2^4 with: a zero row (3), a zero block inside a non-zero row (5, block 2), an outlier element (7), a block
    whose amax is exactly 6 * 2^-3 (11, block 0), a block with amax 7 * 2^-3 in (6, 8) * 2^e (13, block 1), a block below the exponent
    clamp whose largest elements survive as 0.5 * 2^-64 (15, block 0) and one that rounds to zero entirely (15, block 1)"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-6, 5, (N, 1), generator=g).float())
    w[3] = 0.0
    w[5, 64:96] = 0.0
    w[7, 100] = 3000.0
    w[11, :32] = w[11, :32].clamp(-0.75, 0.75)
    w[11, 4] = 0.75
    w[13, 32:64] = w[13, 32:64].clamp(-0.5, 0.5)
    w[13, 40] = -0.875
    w[15, :32] = torch.randn(32, generator=g).clamp(-1, 1) * 2.0 ** -66
    w[15, 9] = 2.0 ** -65
    w[15, 32:64] = torch.randn(32, generator=g).clamp(-1, 1) * 2.0 ** -70
    return w.to(BF16)


def _decode(ops, w4, wscale):
    """(q float64 [N, K] signed e2m1 values, e float64 [N, K / 32]) from the stored bytes"""
    code = ops.mx4_unpack(w4).long()
    q = E2M1[code & 7] * (1.0 - 2.0 * ((code >> 3) & 1).double())
    return q, wscale.double() - 127.0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_quantiser_properties(ops, seed):
    w = _matrix(seed)
    N, K = w.shape
    w4, wscale, w_deq = ops.mx4_quantize(w)
    assert w4.dtype == torch.uint8 and w4.shape == (N, K // 2) and wscale.dtype == torch.uint8 and wscale.shape == (N, K // 32)
    assert w_deq.dtype == BF16 and w_deq.shape == w.shape
    q, e = _decode(ops, w4, wscale)
    assert int(wscale.max()) < 0xFF and float(e.min()) >= -64 and float(e.max()) <= 64
    # w_deq is q * 2^e without any rounding: exact in bf16
    deq = (q.reshape(N, K // 32, 32) * torch.exp2(e)[..., None]).reshape(N, K)
    assert torch.equal(w_deq.double(), deq)
    # the block rule: e = floor(log2(amax)) - 2 (amax / 2^e in [4, 8)), 0 for a block that stores only zeros, clamped to [-64, 64]
    wb = w.double().reshape(N, K // 32, 32)
    amax = wb.abs().amax(2)
    allzero = (q.reshape(N, K // 32, 32) == 0).all(2)
    top = amax / torch.exp2(e)
    free = ~allzero & (e > -64) & (e < 64)
    assert bool(((top >= 4) & (top < 8))[free].all()) and bool((e[allzero] == 0).all())
    assert bool(allzero[3].all()) and bool(allzero[5, 2]) and not bool(allzero[5, 1]) and bool((amax[allzero] < 0.25 * 2.0 ** -64).all())
    assert float(e[11, 0]) == -3 and float(top[11, 0]) == 6.0 and float(q[11, 4]) == 6.0
    assert float(e[13, 1]) == -3 and float(top[13, 1]) == 7.0 and float(q[13, 40]) == -6.0          # saturates
    assert float(e[15, 0]) == -64 and float(q[15, 9]) == 0.5 and bool(allzero[15, 1]) and float(e[15, 1]) == 0
    assert float(e[7, 3]) == 9 and float(q[7, 100]) == 6.0                                          # 3000 = 5.86 * 2^9
    # the element rule: q is the nearest grid value of w / 2^e (never further than half the local step), saturated at 6
    x = wb / torch.exp2(e)[..., None]
    qb = q.reshape(N, K // 32, 32)
    step = torch.where(x.abs() < 2, 0.5, torch.where(x.abs() < 4, 1.0, 2.0))
    ok = ((qb - x).abs() <= step / 2) | ((x.abs() > 6) & (qb == 6 * x.sign()))
    assert bool(ok[~allzero].all()) and bool((x.abs()[allzero] <= 0.25).all())
    assert bool((qb.sign() * x.sign() >= 0).all())
    # idempotent on its own output: the same three tensors
    w4b, wscale_b, w_deq2 = ops.mx4_quantize(w_deq)
    assert torch.equal(w4b, w4) and torch.equal(wscale_b, wscale) and torch.equal(w_deq2, w_deq)
    plain = torch.ones(N, dtype=torch.bool)
    plain[[3, 7, 15]] = False
    err = ((w_deq.double() - w.double())[plain] ** 2).mean().sqrt() / (w.double()[plain] ** 2).mean().sqrt()
    print(f"MX4_QUANT seed {seed}: rms(w_deq - w) / rms(w) = {float(err):.4f}; saturated {float((x.abs() > 6).double().mean()):.4f}")


def test_ties_go_to_the_even_code_and_large_values_saturate(ops):
    """one block per probe value, with a 4.0 beside it so that e = 0 and the probe is rounded on the unit grid"""
    ties = {0.25: 0.0, 0.75: 1.0, 1.25: 1.0, 1.75: 2.0, 2.5: 2.0, 3.5: 4.0, 5.0: 4.0}
    sat = [6.5, 7.0, 7.5, 7.96875]
    probes = list(ties) + [-v for v in ties] + sat + [-v for v in sat]
    w = torch.zeros(len(probes), 128)
    w[:, 0] = 4.0
    w[:, 1] = torch.tensor(probes)
    w4, wscale, w_deq = ops.mx4_quantize(w.to(BF16))
    assert torch.equal(w.to(BF16).float(), w) and bool((wscale[:, 0] == 127).all()) and bool((wscale[:, 1:] == 127).all())
    got = w_deq[:, 1].double().tolist()
    want = list(ties.values()) + [-v for v in ties.values()] + [6.0] * len(sat) + [-6.0] * len(sat)
    assert got == want, list(zip(probes, got, want))
    code = ops.mx4_unpack(w4)[:, 1].tolist()
    assert code[:7] == [0, 2, 2, 4, 4, 6, 6] and code[7:14] == [8, 10, 10, 12, 12, 14, 14] and code[14:18] == [7] * 4 and code[18:] == [15] * 4


def test_pack_layout(ops):
    N, K = 3, 384
    idx = torch.arange(K, dtype=torch.int32)
    x = (idx[None] * 5 + 7 * torch.arange(N, dtype=torch.int32)[:, None]).remainder(16).to(torch.uint8)
    p = ops.mx4_pack(x)
    assert p.shape == (N, K // 2) and p.dtype == torch.uint8 and p.is_contiguous()
    assert torch.equal(ops.mx4_unpack(p), x)
    for k in range(K):
        step, s, g, j = k // 128, (k % 128) // 32, (k % 32) // 8, k % 8
        byte = p[:, step * 64 + (g * 4 + s) * 4 + j // 2]
        assert torch.equal((byte >> (4 * (j % 2))) & 15, x[:, k]), k
    # a few named elements: k = 0 -> byte 0 low nibble; k = 1 -> byte 0 high; k = 8 (g = 1) -> byte 16; k = 32 (s = 1) -> byte 4;
    # k = 127 (s = 3, g = 3, j = 7) -> byte 63 high nibble; k = 128 -> byte 64; as dwords: nibble j of dword g * 4 + s
    for k, byte, hi in ((0, 0, 0), (1, 0, 1), (8, 16, 0), (32, 4, 0), (47, 23, 1), (127, 63, 1), (128, 64, 0), (300, 128 + 22, 0)):
        assert int((p[1, byte] >> (4 * hi)) & 15) == int(x[1, k]), (k, byte, hi)
    dw = p.view(torch.int32)
    assert int((dw[2, 1 * 16 + 2 * 4 + 3] >> (4 * 5)) & 15) == int(x[2, 128 + 3 * 32 + 2 * 8 + 5])
    with pytest.raises(AssertionError):
        ops.mx4_pack(torch.zeros(4, 192, dtype=torch.uint8))
    with pytest.raises(AssertionError):
        ops.mx4_unpack(torch.zeros(4, 96, dtype=torch.uint8))


def test_entry_is_declared_and_bound(ops):
    from internnav_amd import _lib

    header = (ROOT / "include" / "internnav_amd.h").read_text()
    assert re.search(r"int ina_gemm_mx4\(const ina_gemm_args\* args, const void\* W4, const void\* wscale, void\* stream\);", header)
    assert "ina_gemm_mx4" in _lib.SYMBOLS
    h = _lib.lib()
    assert h.ina_gemm_mx4 is not None
    assert h.ina_abi_version() == 8 == _lib.ABI_VERSION
    assert re.search(r"#define INA_ABI_VERSION 8\b", header)


def _args(_lib, **kw):
    a = _lib.GemmArgs()
    a.A = a.C = 0x1000
    a.M, a.N, a.K = 7, 512, 256
    a.lda = 256
    a.ldw = 128
    a.ldc = a.ldr = 512
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,needle", [
    (dict(M=65), "M <= 64"),
    (dict(K=192, lda=192, ldw=96), "K % 128"),
    (dict(ldw=64), "pitch"),
    (dict(ldw=136), "pitch"),
    (dict(batch=2), "batch"),
    (dict(seg_stats=0x4000), "seg_stats"),
    (dict(Wp=0x4000), "Wp"),
    (dict(norm_gamma=0x4000, M=17), "M <= 16"),
    (dict(norm_gamma=0x4000, K=4224, lda=4224, ldw=2112), "K <= 4096"),
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
    rc = h.ina_gemm_mx4(C.byref(_args(_lib, **kw)), 0x8000, 0x9000, None)
    msg = h.ina_last_error().decode()
    assert rc != 0 and msg.startswith("gemm_mx4") and needle in msg, (rc, msg)


def test_null_and_misaligned_pointers_are_refused(ops):
    from internnav_amd import _lib

    h = _lib.lib()
    assert h.ina_gemm_mx4(C.byref(_args(_lib)), None, 0x9000, None) != 0 and "null" in h.ina_last_error().decode()
    assert h.ina_gemm_mx4(C.byref(_args(_lib)), 0x8000, None, None) != 0 and "null" in h.ina_last_error().decode()
    assert h.ina_gemm_mx4(None, 0x8000, 0x9000, None) != 0 and "null" in h.ina_last_error().decode()
    assert h.ina_gemm_mx4(C.byref(_args(_lib)), 0x8008, 0x9000, None) != 0 and "16-byte" in h.ina_last_error().decode()
    assert h.ina_gemm_mx4(C.byref(_args(_lib)), 0x8000, 0x9002, None) != 0 and "4-byte" in h.ina_last_error().decode()
