"""Anchors of tests/s2_ops_ref.py (no GPU): the float64 restatements the System-2 token-kernel and norm tests compare against are themselves
compared with the installed transformers implementation of Qwen2.5-VL's rotary embedding, with torch.nn.functional.layer_norm, and with fp32
restatements of the same formulas - the latter back the bounds the GPU tests use (a sound fp32 evaluation fits them with room to spare).
"""
import math

import pytest
import torch

from tests import s2_ops_ref as S

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U, BF = S.U, S.BF
NORM_WIDTHS = (8, 128, 136, 256, 264, 512, 520, 1024, 1032, 2048, 2056, 4096, 4104, 8192)


def _hf():
    return pytest.importorskip("transformers.models.qwen2_5_vl.modeling_qwen2_5_vl")


def _tables(rows, D, g, duplicated):
    """cos / sin f32 [rows, D]: independent random halves (a table no model produces, but the one that tells the halves apart) or unit
    (cos a, sin a) with the halves repeated, as every real table is."""
    if not duplicated:
        return torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    a = torch.rand(rows, D // 2, generator=g, dtype=F64) * 2 * math.pi
    return torch.cat([a.cos(), a.cos()], 1).float(), torch.cat([a.sin(), a.sin()], 1).float()


@pytest.mark.parametrize("duplicated", [False, True])
def test_rope_reference_equals_transformers(duplicated):
    hf = _hf()
    g = torch.Generator().manual_seed(1)
    rows, heads, D = 19, 5, 128
    x = torch.randn(rows, heads * D, generator=g).to(BF16)
    cos, sin = _tables(rows, D, g, duplicated)
    (ref, scale), _ = S.rope(x, cos, sin, heads, D)
    q = x.to(F64).view(1, rows, heads, D).transpose(1, 2)                                  # [batch, heads, seq, D]
    c3, s3 = cos.to(F64).expand(3, 1, rows, D), sin.to(F64).expand(3, 1, rows, D)          # equal axes: the section interleave is the identity
    qe, ke = hf.apply_multimodal_rotary_pos_emb(q, q.clone(), c3, s3, [16, 24, 24])
    assert qe.dtype == F64 and torch.equal(qe, ke)
    assert (qe.transpose(1, 2).reshape(rows, heads * D) - ref).abs().max().item() <= 1e-14 * scale.max().item()
    # the vision form converts to fp32 inside: agreement to fp32 rounding of the two products and the sum
    qv, _ = hf.apply_rotary_pos_emb_vision(x.to(F64).view(rows, heads, D), x.to(F64).view(rows, heads, D), cos.to(F64), sin.to(F64))
    err = (qv.to(F64).reshape(rows, heads * D) - ref).abs()
    assert (err <= 4.0 * U * scale).all(), (err / (U * scale)).max().item()


def test_rope_reference_tab_rowmap_and_kv_append():
    """the index plumbing of the reference, against a loop written out row by row."""
    g = torch.Generator().manual_seed(2)
    rows, heads, kv0, vh, D, col0 = 6, 3, 2, 1, 16, 8
    ld = col0 + (heads + vh) * D + 8
    x = torch.randn(4 * 5, ld, generator=g).to(BF16)
    cos, sin = _tables(4, D, g, False)
    tab = torch.tensor([3, 0, 0, 2, 1, 3], dtype=torch.int32)
    row_map = (3, 5, 2)
    kv = torch.full((9, (heads - kv0 + vh) * D + 8), 7.0, dtype=BF16)
    dst = torch.tensor([8, 1, 4, 0, 6, 2], dtype=torch.int32)
    (ref, _), (kref, _) = S.rope(x, cos, sin, heads, D, col0=col0, rows=rows, row_map=row_map, tab=tab, kv_out=kv, kv_dst=dst, kv_head0=kv0, v_heads=vh)
    want, kwant = x.to(F64).clone(), kv.to(F64).clone()
    h = D // 2
    for r in range(rows):
        pr = (r // 3) * 5 + 2 + r % 3
        c, s = cos[tab[r]].to(F64), sin[tab[r]].to(F64)
        for k in range(heads + vh):
            v = x[pr, col0 + k * D: col0 + (k + 1) * D].to(F64)
            if k < heads:
                v = torch.cat([v[:h] * c[:h] - v[h:] * s[:h], v[h:] * c[h:] + v[:h] * s[h:]])
            if k < kv0:
                want[pr, col0 + k * D: col0 + (k + 1) * D] = v
            else:
                kwant[dst[r], (k - kv0) * D: (k - kv0 + 1) * D] = v
    assert torch.equal(ref, want) and torch.equal(kref, kwant)
    assert torch.equal(kref[:, -8:], kv.to(F64)[:, -8:]) and torch.equal(kref[[3, 5, 7]], kv.to(F64)[[3, 5, 7]])


def test_rope_fp32_restatement_fits_the_bound():
    """fp32 evaluation in the order x * cos + (+-partner * sin) with one fused multiply-add, stored round-to-nearest as bf16: inside
    4 * 2^-24 * (|lo c| + |hi s|) + 2^-8 * |ref| (worst ratio printed); a truncating bf16 store is outside it."""
    g = torch.Generator().manual_seed(3)
    rows, heads, D = 512, 4, 128
    x = torch.randn(rows, heads * D, generator=g).to(BF16)
    cos, sin = _tables(rows, D, g, False)
    (ref, scale), _ = S.rope(x, cos, sin, heads, D)
    bound = S.rope_bound(ref, scale)
    xf = x.float().view(rows, heads, D)
    lo, hi, h = xf[..., :D // 2], xf[..., D // 2:], D // 2
    c, s = cos[:, None, :], sin[:, None, :]
    # fma(lo, c, -(hi * s)): the product hi * s is rounded to fp32, the rest is exact until the final rounding
    olo = (lo.double() * c[..., :h].double() - (hi * s[..., :h]).double()).float()
    ohi = (hi.double() * c[..., h:].double() + (lo * s[..., h:]).double()).float()
    y32 = torch.cat([olo, ohi], -1).reshape(rows, heads * D)
    ratio = ((y32.to(BF16).double() - ref).abs() / bound).max().item()
    print(f"fp32 rope restatement: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    trunc = (y32.view(torch.int32) & -65536).view(F32)
    assert ((trunc.double() - ref).abs() > bound).any(), "a truncating store must not fit the bound"


def test_rotation_inverse():
    """rope(rope(x, cos, sin), cos, -sin) == x for unit (cos, sin) with repeated halves - the transpose the rope backward of the SFT step relies
    on - within the bf16 rounding of the intermediate."""
    g = torch.Generator().manual_seed(4)
    rows, heads, D = 33, 7, 128
    x = torch.randn(rows, heads * D, generator=g).to(BF16)
    cos, sin = _tables(rows, D, g, True)
    (y, _), _ = S.rope(x, cos, sin, heads, D)
    (z, _), _ = S.rope(y, cos, -sin, heads, D)
    assert (z - x.double()).abs().max().item() <= 1e-6                    # fp32 tables: cos^2 + sin^2 = 1 to 2^-24
    yb = y.to(BF16)
    (zb, sb), _ = S.rope(yb, cos, -sin, heads, D)
    # each rounded intermediate is off by <= 2^-8 |y|; the inverse rotation mixes a lo / hi pair with weights |cos|, |sin|
    assert ((zb - x.double()).abs() <= BF * sb + 1e-6).all()


def test_mrope_reference_equals_transformers():
    hf = _hf()
    from transformers.models.qwen2_5_vl.configuration_qwen2_5_vl import Qwen2_5_VLTextConfig

    rot = hf.Qwen2_5_VLRotaryEmbedding(Qwen2_5_VLTextConfig())
    D = 128
    assert rot.inv_freq.numel() == D // 2 and rot.attention_scaling == 1.0
    g = torch.Generator().manual_seed(5)
    n = 300
    pos = torch.stack([torch.randint(0, 40001, (n,), generator=g) for _ in range(3)]).to(torch.int32)
    pos[:, 0] = torch.tensor([40000, 39999, 17])
    assert not torch.equal(pos[0], pos[1]) and not torch.equal(pos[1], pos[2])
    axis_of = torch.tensor([0] * 16 + [1] * 24 + [2] * 24, dtype=torch.int32)
    (cref, _), (sref, _) = S.mrope_table(pos, rot.inv_freq, axis_of)
    cos3, sin3 = rot(torch.zeros(1, dtype=F32), pos.long()[:, None, :])                     # [3, 1, n, D] fp32
    # the section interleave as transformers does it: q = 1, "sin" = 0 returns the interleaved first argument
    one, zero = torch.ones(1, 1, n, D, dtype=F64), torch.zeros(3, 1, n, D, dtype=F64)
    c_hf, _ = hf.apply_multimodal_rotary_pos_emb(one, one, cos3.to(F64), zero, [16, 24, 24])
    s_hf, _ = hf.apply_multimodal_rotary_pos_emb(one, one, sin3.to(F64), zero, [16, 24, 24])
    ec, es = (c_hf[0, 0] - cref).abs().max().item() / U, (s_hf[0, 0] - sref).abs().max().item() / U
    print(f"fp32 libm cos / sin of the fp32 angle against the reference: {ec:.2f} / {es:.2f} x 2^-24")
    assert ec <= 2.0 and es <= 2.0
    # the rounding of the angle is part of the contract: a float64 angle is somewhere else entirely at these positions
    a64 = pos[axis_of.long()].t().to(F64) * rot.inv_freq.to(F64)[None, :]
    assert (torch.cos(a64) - cref[:, :D // 2]).abs().max().item() > 1e-4
    # an ignored axis_of is visible with distinct rows
    (c0, _), _ = S.mrope_table(pos, rot.inv_freq, torch.zeros_like(axis_of))
    assert (c0 - cref).abs().max().item() > 0.1


def test_gather_and_argmax_reference():
    x = torch.arange(40, dtype=F32).view(10, 4)
    out = torch.full((12, 4), -1.0)
    src = torch.tensor([9, 9, 0, 3], dtype=torch.int32)
    dst = torch.tensor([11, 2, 5, 0], dtype=torch.int32)
    ref, _ = S.gather_rows(x, out, src, dst, rows=3)
    assert torch.equal(ref[11], x[9]) and torch.equal(ref[2], x[9]) and torch.equal(ref[5], x[0]) and (ref[[0, 1, 3, 4, 6, 7, 8, 9, 10]] == -1).all()
    a, _ = S.argmax_rows(torch.tensor([[1.0, 3.0, 3.0], [-math.inf] * 3]))
    assert a.tolist() == [1, 0]


@pytest.mark.parametrize("C", [8, 384, 8192])
def test_norm_reference_equals_torch(C):
    g = torch.Generator().manual_seed(6)
    x = torch.randn(5, C, generator=g) * 2 + 3
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    eps = 1e-6
    e = float(torch.tensor(eps, dtype=F32))
    (t, _), _ = S.norm(x, w, b, eps=eps)
    assert (t - torch.nn.functional.layer_norm(x.double(), (C,), w.double(), b.double(), e)).abs().max().item() < 1e-12
    (t, _), _ = S.norm(x, w, eps=eps, rms=True)
    xd = x.double()
    assert (t - xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + e) * w.double()).abs().max().item() < 1e-12


def test_norm_reference_full_chain():
    """every operand at once against the docstring written out row by row, logical-row indexing of modulation, base and pos included."""
    g = torch.Generator().manual_seed(7)
    rows, C, mod_div = 7, 16, 3
    x = torch.randn(40, C, generator=g)
    w, b, w2 = (torch.randn(C, generator=g) for _ in range(3))
    mod = torch.randn(3, 3 * C, generator=g)
    ms, gt, ms2 = mod[:, :C], mod[:, C:2 * C], mod[:, 2 * C:]
    base = torch.randn(rows, C, generator=g).to(BF16)
    pos = torch.randn(4, C, generator=g)
    in_map = (2, 9, 5)
    (t, _), (t2, _) = S.norm(x, w, b, eps=1e-5, mod_scale=ms, gate=gt, base=base, mod_div=mod_div, pos=pos, rows=rows, in_map=in_map,
                             out2=torch.empty(rows, C, dtype=BF16), gamma2=w2, mod_scale2=ms2)
    e = float(torch.tensor(1e-5, dtype=F32))
    for r in range(rows):
        xr = x[(r // 2) * 9 + 5 + r % 2].double()
        v = torch.nn.functional.layer_norm(xr, (C,), w.double(), b.double(), e)
        v = v * (1 + ms[r // mod_div].double()) * torch.tanh(gt[r // mod_div].double()) + base[r].double() + pos[r % 4].double()
        assert (t[r] - v).abs().max().item() < 1e-12
        v2 = torch.nn.functional.layer_norm(v.float().double(), (C,), w2.double(), None, e) * (1 + ms2[r // mod_div].double())
        assert (t2[r] - v2).abs().max().item() < 1e-12


@pytest.mark.parametrize("rms", [False, True])
def test_norm_fp32_restatement_against_the_model(rms):
    """fp32 torch against the float64 reference at every width edge, with and without a mean offset of 64 x the spread: the worst
    |err| / (2^-24 * (sqrt(C) + 4) * scale) is printed and stays below 1 - the error model the GPU test scales by its measured k."""
    g = torch.Generator().manual_seed(8)
    worst = 0.0
    for C in NORM_WIDTHS:
        for shift in (0.0, 64.0):
            x = torch.randn(9, C, generator=g) + shift
            w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
            (ref, scale), _ = S.norm(x, w, b, eps=1e-6, rms=rms)
            if rms:
                y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * w + b
            else:
                y = torch.nn.functional.layer_norm(x, (C,), w, b, 1e-6)
            worst = max(worst, ((y.double() - ref).abs() / S.fp32_bound(scale, C, 1.0)).max().item())
    print(f"fp32 torch norm (rms={rms}): worst |err| / (2^-24 (sqrt(C) + 4) scale) = {worst:.3f}")
    assert worst < 1.0
