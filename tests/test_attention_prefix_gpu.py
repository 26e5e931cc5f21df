"""GPU: ops.attention_prefix (csrc/attention_prefix.hip) against the float64 restatement of tests/attn_prefix_ref.py on its poisoned cases:
every cache row at or behind pfx_len, every row of an unnamed slot and every fused q|k|v row at or behind suf_len is NaN, and the reference is
finite on them (tests/test_attn_prefix_ref_cpu.py) - a NaN or an out-of-tolerance value in a live output row is a mask or bound error."""
import functools

import numpy as np
import pytest
import torch

import attn_prefix_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _case(i):
    c = R.make_case(R.CASES[i])
    return c, R.reference_of(c)


def _run(c, slot=None, out=None):
    from internnav_amd import ops

    fused, cache = c["fused"].to(DEV), c["cache"].to(DEV)
    q, k, v, kc, vc = R.views(fused, cache, c["H"], c["Hkv"], c["m"])
    if out is None:
        out = torch.full((c["P"], c["m"], c["H"], R.D), 7.0, dtype=torch.bfloat16, device=DEV)     # a row the launch skips keeps the 7
    ops.attention_prefix(q, k, v, kc, vc, (c["slot"] if slot is None else slot).to(DEV), c["pfx_len"].to(DEV), c["suf_len"].to(DEV), out=out)
    torch.cuda.synchronize()
    return out


def _yardstick(c):
    """ops.attention on a materialised [prefix | suffix] copy of every pair (the poison replaced by zeros: only rows the mask hides)"""
    from internnav_amd import ops

    q, k, v, kc, vc = R.views(c["fused"], c["cache"], c["H"], c["Hkv"], c["m"])
    P, m, pfx = c["P"], c["m"], c["pfx_len"].tolist()
    Lk = max(pfx) + m
    K, V = (torch.zeros(P, Lk, c["Hkv"], R.D, dtype=torch.bfloat16) for _ in range(2))
    for p in range(P):
        s = int(c["slot"][p])
        for dst, cch, suf in ((K, kc, k), (V, vc, v)):
            dst[p, : pfx[p]] = cch[s, : pfx[p]]
            dst[p, pfx[p]: pfx[p] + m] = torch.nan_to_num(suf[p].float(), nan=0.0).to(torch.bfloat16)
    qd = torch.nan_to_num(q.float(), nan=0.0).to(torch.bfloat16).to(DEV)
    k_len = torch.tensor([n + m for n in pfx], dtype=torch.int32, device=DEV)
    return ops.attention(qd, K.to(DEV), V.to(DEV), causal=True, k_len=k_len)


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.CASE_IDS)
def test_attention_prefix_against_fp64_on_poisoned_inputs(built_lib, i):
    c, ref = _case(i)
    suf = c["suf_len"].tolist()
    out = _run(c)
    got = out.float().cpu().numpy()
    ratio = yard = 0.0
    y = _yardstick(c).float().cpu().numpy()
    for p in range(c["P"]):
        n = suf[p]
        assert not got[p, n:].any(), f"pair {p}: rows behind suf_len={n} are not exactly zero"
        live, want = got[p, :n], ref[p, :n]
        assert np.isfinite(live).all(), f"pair {p}: NaN / inf in a live row (a poisoned row was read)"
        if n:
            ratio = max(ratio, float((np.abs(live - want) / R.tolerance(want)).max()))
            yard = max(yard, float((np.abs(y[p, :n] - want) / R.tolerance(want)).max()))
    print(f"{R.CASE_IDS[i]}: worst |err| / tolerance {ratio:.3f} (ops.attention on the materialised copy: {yard:.3f})")
    assert ratio <= 1.0, f"worst |err| / (1.5e-2 + |ref| / 128) = {ratio:.3f}"
    # two launches: the same bits (fixed combine order, no atomics)
    assert torch.equal(_run(c).view(torch.int16), out.view(torch.int16))
    # a slot outside the cache: NaN in that pair's live rows, zeros behind them, the neighbours unchanged bit for bit
    for bad_p, bad in ((0, R.N_SLOTS), (c["P"] - 1, -1)):
        slot = c["slot"].clone()
        slot[bad_p] = bad
        o2 = _run(c, slot=slot)
        assert bool(torch.isnan(o2[bad_p, : suf[bad_p]]).all()) and not bool(o2[bad_p, suf[bad_p]:].float().abs().sum())
        keep = [p for p in range(c["P"]) if p != bad_p]
        assert torch.equal(o2[keep].view(torch.int16), out[keep].view(torch.int16))


def test_python_binding_checks_its_arguments(built_lib):
    from internnav_amd import ops

    c, _ = _case(0)
    fused, cache = c["fused"].to(DEV), c["cache"].to(DEV)
    q, k, v, kc, vc = R.views(fused, cache, c["H"], c["Hkv"], c["m"])
    t = [c[n].to(DEV) for n in ("slot", "pfx_len", "suf_len")]
    with pytest.raises(AssertionError):
        ops.attention_prefix(q, k, v, kc, vc, t[0].long(), t[1], t[2])
    with pytest.raises(AssertionError):
        ops.attention_prefix(q, k, v, kc, vc, *t, max_pfx=R.S_CACHE + 1)
    with pytest.raises(AssertionError):
        ops.attention_prefix(q[..., :64], k[..., :64], v[..., :64], kc[..., :64], vc[..., :64], *t)
    # max_pfx clips pfx_len: the result of the clipped table
    a = ops.attention_prefix(q, k, v, kc, vc, *t, max_pfx=40)
    b = ops.attention_prefix(q, k, v, kc, vc, t[0], torch.clamp(t[1], max=40), t[2])
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
