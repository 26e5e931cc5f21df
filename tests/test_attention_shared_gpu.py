"""GPU: ops.attention_shared (csrc/attention_shared.hip) against the float64 restatement of tests/attn_shared_ref.py on its poisoned cases: every
cache row at or behind pfx_len, every unnamed slot, every tail row at or behind tail_len and the whole tail of a row no tile names is NaN, and the
reference is finite on them (tests/test_attn_shared_ref_cpu.py) - a NaN or an out-of-tolerance value in a live output row is a mask or bound error.
Then the properties the decode path builds on: the same bits on two launches, the bits of a row computed alone in its tile, NaN rows for a slot
outside the cache, zero rows without a tail, a cache that is never written."""
import functools

import numpy as np
import pytest
import torch

import attn_shared_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TABLES = ("tile_rows", "tile_slot", "tile_pfx", "tail_len")


@functools.lru_cache(maxsize=None)
def _case(i):
    c = R.make_case(R.CASES[i])
    return c, R.reference_of(c)


def _run(c, bufs=None, **tables):
    from internnav_amd import ops

    fused, tail, cache = bufs if bufs is not None else (c["fused"].to(DEV), c["tail"].to(DEV), c["cache"].to(DEV))
    q, kt, vt, kc, vc = R.views(fused, tail, cache, c["H"], c["Hkv"])
    out = torch.full((c["R"] + 1, c["H"], R.D), R.FILL, dtype=torch.bfloat16, device=DEV)          # a row the launch skips keeps the 7
    ops.attention_shared(q, kt, vt, kc, vc, *[(tables[n] if n in tables else c[n]).to(DEV) for n in TABLES], out=out)
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.CASE_IDS)
def test_attention_shared_against_fp64_on_poisoned_inputs(built_lib, i):
    c, ref = _case(i)
    n = c["R"]
    bufs = (c["fused"].to(DEV), c["tail"].to(DEV), c["cache"].to(DEV))
    cache_before = bufs[2].clone()
    out = _run(c, bufs)
    got = out.float().cpu().numpy()
    assert (got[n] == R.FILL).all(), "the row no tile names was written"
    assert np.isfinite(got[:n]).all(), "NaN / inf in a live row (a poisoned row was read)"
    ratio = float((np.abs(got[:n] - ref[:n]) / R.tolerance(ref[:n])).max())
    print(f"{R.CASE_IDS[i]}: {n} rows in {c['tile_rows'].shape[0]} tiles of {c['tile_rows'].shape[1]}, worst |err| / tolerance {ratio:.3f}")
    assert ratio <= 1.0, f"worst |err| / (1.5e-2 + |ref| / 128) = {ratio:.3f}"
    # two launches: the same bits (fixed chunk owners, fixed combine order, no atomics)
    assert torch.equal(_bits(_run(c, bufs)), _bits(out))
    # every row alone in its tile (a table that holds only that row): the bits it has when packed with its neighbours, nothing else written
    cpt = c["tile_rows"].shape[1]
    for t in range(c["tile_rows"].shape[0]):
        for r in (int(x) for x in c["tile_rows"][t] if x >= 0):
            alone = torch.full((1, cpt), -1, dtype=torch.int32)
            alone[0, 0] = r
            o1 = _run(c, bufs, tile_rows=alone, tile_slot=c["tile_slot"][t:t + 1], tile_pfx=c["tile_pfx"][t:t + 1])
            assert torch.equal(_bits(o1[r]), _bits(out[r])), f"row {r}: its bits depend on the rows that share its tile"
            rest = [x for x in range(n + 1) if x != r]
            assert bool((o1[rest].float() == R.FILL).all()), f"a launch of row {r} alone wrote another row"
    # ... nor on the neighbours' tail lengths: a row without a tail is a zero row, every other row keeps its bits
    for z in (0, n - 1):
        tl = c["tail_len"].clone()
        tl[z] = 0
        o2 = _run(c, bufs, tail_len=tl)
        keep = [x for x in range(n + 1) if x != z]
        assert not bool(o2[z].float().abs().sum()) and torch.equal(_bits(o2[keep]), _bits(out[keep]))
    # a slot outside the cache: NaN in that tile's rows, the other tiles unchanged bit for bit
    for bad_t, bad in ((0, R.N_SLOTS), (c["tile_rows"].shape[0] - 1, -1)):
        slot = c["tile_slot"].clone()
        slot[bad_t] = bad
        o3 = _run(c, bufs, tile_slot=slot)
        rows = [int(x) for x in c["tile_rows"][bad_t] if x >= 0]
        assert bool(torch.isnan(o3[rows]).all())
        keep = [x for x in range(n + 1) if x not in rows]
        assert torch.equal(_bits(o3[keep]), _bits(out[keep]))
    # the cache is read only (bit-equal, its NaN poison included)
    assert torch.equal(_bits(bufs[2]), _bits(cache_before))


def test_python_binding_checks_its_arguments(built_lib):
    from internnav_amd import ops

    c, _ = _case(0)
    fused, tail, cache = c["fused"].to(DEV), c["tail"].to(DEV), c["cache"].to(DEV)
    q, kt, vt, kc, vc = R.views(fused, tail, cache, c["H"], c["Hkv"])
    t = [c[n].to(DEV) for n in TABLES]
    with pytest.raises(AssertionError):
        ops.attention_shared(q, kt, vt, kc, vc, t[0].long(), *t[1:])
    with pytest.raises(AssertionError):
        ops.attention_shared(q, kt, vt, kc, vc, t[0][:, :1].contiguous(), *t[1:])                  # a table of another tile width
    with pytest.raises(AssertionError):
        ops.attention_shared(q, kt, vt, kc, vc, *t, max_pfx=R.S_CACHE + 1)
    with pytest.raises(AssertionError):
        ops.attention_shared(q[..., :64], kt[..., :64], vt[..., :64], kc[..., :64], vc[..., :64], *t)
    # max_pfx clips tile_pfx: the result of the clipped table
    a = ops.attention_shared(q, kt, vt, kc, vc, *t, max_pfx=40)
    b = ops.attention_shared(q, kt, vt, kc, vc, t[0], t[1], torch.clamp(t[2], max=40), t[3])
    torch.cuda.synchronize()
    n = c["R"]
    assert torch.equal(_bits(a[:n]), _bits(b[:n]))
