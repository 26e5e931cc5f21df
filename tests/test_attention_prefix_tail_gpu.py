"""GPU: ops.attention_prefix_tail (csrc/attention_prefix.hip) against the float64 restatement of tests/attn_prefix_tail_ref.py on its poisoned
cases: every cache row at or behind pfx_len, every tail row at or behind tail_len, every row of an unnamed slot or tail and every fused q|k|v row
at or behind suf_len is NaN, and the reference is finite on them (tests/test_attn_prefix_tail_ref_cpu.py) - a NaN or an out-of-tolerance value in
a live output row is a mask or bound error. And the two bit equalities with ops.attention_prefix: without a tail on that kernel's own cases, and
behind a prefix of whole chunks on a slot that holds [prefix | tail]."""
import functools

import numpy as np
import pytest
import torch

import attn_prefix_ref as R0
import attn_prefix_tail_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TABLES = ("slot", "pfx_len", "suf_len", "tail_row", "tail_len")


@functools.lru_cache(maxsize=None)
def _case(i):
    c = R.make_case(R.CASES[i])
    return c, R.reference_of(c)


def _bits(t):
    return t.view(torch.int16)


def _run(c, bufs=None, **tables):
    """one launch on device copies of the case's buffers (or on `bufs`, kept by the caller) -> out; a row the launch skips keeps the 7"""
    from internnav_amd import ops

    fused, cache, tails = bufs if bufs is not None else (c[n].to(DEV) for n in ("fused", "cache", "tails"))
    q, k, v, kc, vc, kt, vt = R.views(fused, cache, tails, c["H"], c["Hkv"], c["m"])
    t = {n: tables.get(n, c[n]).to(DEV) for n in TABLES}
    out = torch.full((c["P"], c["m"], c["H"], R.D), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.attention_prefix_tail(q, k, v, kc, vc, t["slot"], t["pfx_len"], t["suf_len"], kt, vt, t["tail_row"], t["tail_len"], out=out)
    torch.cuda.synchronize()
    return out


def _on_materialised(c):
    """ops.attention_prefix on P slots that hold [prefix | tail] of every pair (tests/attn_prefix_tail_ref.materialised)"""
    from internnav_amd import ops

    mat, slot, plen = R.materialised(c)
    fused = c["fused"].to(DEV)
    H, Hkv, m, P = c["H"], c["Hkv"], c["m"], c["P"]
    q = fused[:, : H * R.D].view(P, m, H, R.D)
    k = fused[:, H * R.D:(H + Hkv) * R.D].view(P, m, Hkv, R.D)
    v = fused[:, (H + Hkv) * R.D:].view(P, m, Hkv, R.D)
    m5 = mat.to(DEV).view(P, R.S_CACHE, 2, Hkv, R.D)
    out = ops.attention_prefix(q, k, v, m5[:, :, 0], m5[:, :, 1], slot.to(DEV), plen.to(DEV), c["suf_len"].to(DEV))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.CASE_IDS)
def test_attention_prefix_tail_against_fp64_on_poisoned_inputs(built_lib, i):
    c, ref = _case(i)
    suf, pfx, tlen = (c[n].tolist() for n in ("suf_len", "pfx_len", "tail_len"))
    bufs = tuple(c[n].to(DEV) for n in ("fused", "cache", "tails"))
    before = [b.clone() for b in bufs]
    out = _run(c, bufs)
    got = out.float().cpu().numpy()
    mat = _on_materialised(c)
    y = mat.float().cpu().numpy()
    ratio = yard = 0.0
    for p in range(c["P"]):
        n = suf[p]
        assert not got[p, n:].any(), f"pair {p}: rows behind suf_len={n} are not exactly zero"
        live, want = got[p, :n], ref[p, :n]
        assert np.isfinite(live).all(), f"pair {p}: NaN / inf in a live row (a poisoned row was read)"
        if n:
            ratio = max(ratio, float((np.abs(live - want) / R.tolerance(want)).max()))
            yard = max(yard, float((np.abs(y[p, :n] - want) / R.tolerance(want)).max()))
    print(f"{R.CASE_IDS[i]}: worst |err| / tolerance {ratio:.3f} (ops.attention_prefix on the materialised [prefix | tail] slots: {yard:.3f})")
    assert ratio <= 1.0, f"worst |err| / (1.5e-2 + |ref| / 128) = {ratio:.3f}"
    # a prefix of whole chunks: the chunks and their owners are those of attention_prefix on [prefix | tail] - the same bits
    whole = [p for p in range(c["P"]) if pfx[p] % 64 == 0]
    assert whole or i == 1
    for p in whole:
        assert torch.equal(_bits(out[p]), _bits(mat[p])), f"pair {p} (pfx_len {pfx[p]}, tail_len {tlen[p]}) differs from attention_prefix on [prefix | tail]"
    # two launches: the same bits (fixed combine order, no atomics); nothing was written to the cache, the tails or the projection buffer
    assert torch.equal(_bits(_run(c, bufs)), _bits(out))
    for name, b, b0 in zip(("fused", "cache", "tails"), bufs, before):
        assert torch.equal(_bits(b), _bits(b0)), f"the launch wrote the {name} buffer"
    # a slot outside the cache, a tail outside the buffer under a positive tail_len: NaN in that pair's live rows, zeros behind them, the
    # neighbours unchanged bit for bit
    with_tail = [p for p in range(c["P"]) if tlen[p] > 0 and suf[p] > 0]
    for name, bad_p, bad in (("slot", 0, R.N_SLOTS), ("slot", c["P"] - 1, -1), ("tail_row", with_tail[0], R.N_TAILS), ("tail_row", with_tail[-1], -1)):
        t = c[name].clone()
        t[bad_p] = bad
        o2 = _run(c, bufs, **{name: t})
        assert bool(torch.isnan(o2[bad_p, : suf[bad_p]]).all()) and not bool(o2[bad_p, suf[bad_p]:].float().abs().sum()), (name, bad_p, bad)
        keep = [p for p in range(c["P"]) if p != bad_p]
        assert torch.equal(_bits(o2[keep]), _bits(out[keep])), (name, bad_p, bad)
    # tail_len 0 does not look at tail_row
    t = c["tail_row"].clone()
    t[torch.tensor([p for p in range(c["P"]) if tlen[p] == 0], dtype=torch.long)] = 1 << 30
    assert torch.equal(_bits(_run(c, bufs, tail_row=t)), _bits(out))


@pytest.mark.parametrize("i", range(len(R0.CASES)), ids=R0.CASE_IDS)
def test_without_a_tail_the_bits_are_attention_prefix_s(built_lib, i):
    from internnav_amd import ops

    c = R0.make_case(R0.CASES[i])
    fused, cache = c["fused"].to(DEV), c["cache"].to(DEV)
    q, k, v, kc, vc = R0.views(fused, cache, c["H"], c["Hkv"], c["m"])
    slot, pfx, suf = (c[n].to(DEV) for n in ("slot", "pfx_len", "suf_len"))
    want = ops.attention_prefix(q, k, v, kc, vc, slot, pfx, suf)
    none = ops.attention_prefix_tail(q, k, v, kc, vc, slot, pfx, suf)
    # a tail buffer of NaN that no pair may read: every tail_len is 0, the rows named are anything
    tails = torch.full((3 * 8, 2 * c["Hkv"] * R0.D), float("nan"), dtype=torch.bfloat16, device=DEV).view(3, 8, 2, c["Hkv"], R0.D)
    trow = torch.tensor([(-1, 0, 2, 7)[p % 4] for p in range(c["P"])], dtype=torch.int32, device=DEV)
    zero = ops.attention_prefix_tail(q, k, v, kc, vc, slot, pfx, suf, tails[:, :, 0], tails[:, :, 1], trow, torch.zeros_like(trow))
    torch.cuda.synchronize()
    assert torch.equal(_bits(none), _bits(want)), "null tail arguments: not the bits of ops.attention_prefix"
    assert torch.equal(_bits(zero), _bits(want)), "tail_len = 0 everywhere: not the bits of ops.attention_prefix"


def test_python_binding_checks_its_arguments(built_lib):
    from internnav_amd import ops

    c, _ = _case(0)
    fused, cache, tails = (c[n].to(DEV) for n in ("fused", "cache", "tails"))
    q, k, v, kc, vc, kt, vt = R.views(fused, cache, tails, c["H"], c["Hkv"], c["m"])
    t = {n: c[n].to(DEV) for n in TABLES}
    head = (q, k, v, kc, vc, t["slot"], t["pfx_len"], t["suf_len"])
    with pytest.raises(AssertionError):
        ops.attention_prefix_tail(*head, kt, vt, t["tail_row"])                                   # three of the four tail arguments
    with pytest.raises(AssertionError):
        ops.attention_prefix_tail(*head, kt, vt, t["tail_row"].long(), t["tail_len"])
    with pytest.raises(AssertionError):
        ops.attention_prefix_tail(*head, kt, vt, t["tail_row"], t["tail_len"], max_tail=R.T_TAIL + 1)
    with pytest.raises(AssertionError):
        ops.attention_prefix_tail(*head, kt[:, :, :2], vt[:, :, :2], t["tail_row"], t["tail_len"])   # another KV head count
    # max_tail clips tail_len: the result of the clipped table
    a = ops.attention_prefix_tail(*head, kt, vt, t["tail_row"], t["tail_len"], max_tail=40)
    b = ops.attention_prefix_tail(*head, kt, vt, t["tail_row"], torch.clamp(t["tail_len"], max=40))
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b))
