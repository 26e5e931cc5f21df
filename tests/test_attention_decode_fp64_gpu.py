"""The three single-token attention entries built on csrc/attention_chunk.h - ops.attention_prefix, ops.attention_prefix_tail (attn_prefix_kernel /
attn_prefix_tail_kernel, csrc/attention_prefix.hip) and ops.attention_shared (attn_shared_kernel, csrc/attention_shared.hip) - against the float64
restatement of tests/attn_decode_ref.py, element by element, under the bound derived from the number formats (limit 1.0, never tuned). Reference,
bound, emulation and case tables live in tests/attn_decode_ref.py; tests/test_attn_decode_ref_cpu.py checks them without a GPU (agreement with
the three older references and with SDPA, the emulated chunk walk inside the bound, the fourteen mutations that must leave it).

One launch per case. Everything a launch must not read is NaN; the inputs carry planted edges, so a mask that is off by one key moves the result
by tens to thousands of bounds at any prefix length (769 and 832 keys included: 13 chunks, every wave in the prefetch steady state). The output
sits in a sentinel-filled buffer, 4 columns in (8-byte, not 16-byte aligned) under a row stride above H * D, with guard columns on both sides and
a guard row above and below every pair / the row block: everything outside the result, and the row no tile names, must keep the sentinel. Rows
that must be zero carry a zero bound (==); rows that must be NaN (a tail row outside the buffer under tail_len > 0) must be NaN.
The properties of the three older suites (same bits on two launches, a row alone in its tile, a bad slot gives NaN, the cache is never written)
are not repeated here, except that the shared ramp row is also computed alone in its tile and must keep its bits.

Measured worst |err| / bound per entry (MI355X, ROCm 7), next to the float32 / bf16 emulation of tests/test_attn_decode_ref_cpu.py on the same seed:
    prefix       ops.attention_prefix       (attn_prefix_kernel)        0.678   emulation 0.678   (9 cases; the clamps case, else <= 0.58)
    prefix_tail  ops.attention_prefix_tail  (attn_prefix_tail_kernel)   0.635   emulation 0.635   (8 cases)
    shared       ops.attention_shared       (attn_shared_kernel)        0.525   emulation 0.525   (8 cases; the ramp case)
(case by case the device and the emulation agree to the three digits printed: the two bf16 roundings dominate. Every case takes below 0.2 s.)
With these single edits of a scratch copy of the kernels (never committed), each run against this file and the three older suites
(test_attention_prefix_gpu.py, test_attention_prefix_tail_gpu.py, test_attention_shared_gpu.py), the failures are these and everything else passes:
    `kv < len` as `kv < len - 1` in the prefix kernels' mask lambda (it also drops the suffix's last key): all 9 + 8 prefix and prefix_tail cases
        here; the older suites caught it too (7 of 7 and 6 of 6 fp64 cases);
    the same for prefix chunks only (`kv < (c < nc ? len - 1 : len)`): the same 17 cases here, and again all 13 older fp64 cases;
    the prefetch guard `c + PFX_WAVES <= ns` as `<` (the suffix chunk is multiplied with the registers of the chunk before): 16 of the 17 cases
        here (prefix-m64 passes: with pfx_len 1 / 64 / 65 no pair of it has more than three chunks, so no wave owns a second one and nothing
        is ever prefetched); the older suites caught it too (6 of 7 and 6 of 6);
    the prefetch kept for a wave's first chunk only (`&& c < PFX_WAVES`: a wave's third chunk reuses the second's K / V): the seven cases here
        whose pairs give a wave three chunks (prefix-m3, -m16, -m17, -m64-H28, -ramp, prefix_tail-long, -ramp); test_attention_prefix_gpu.py
        passes entirely (no wave of it walks more than two chunks), test_attention_prefix_tail_gpu.py fails in 2 of 6 cases (pfx_len 300 with a
        130-key tail);
    `ac_scale_o` without effect (attention_chunk.h, in the builds of attention_prefix.hip and attention_shared.hip): 23 of 25 here (shared-H16
        and prefix-m64 pass: no row of them has two chunks in one wave); the older suites caught it in 5 of 7, 5 of 6 and 2 of 4 cases;
    `wl` forced to 1 in `ac_combine` (same two builds): all 25 here; the older suites caught it in every fp64 case (7, 6, 4);
    `a.scale` replaced by the default d^-0.5 in both files: the three -scale cases here and nothing else - the older suites pass entirely
        (none of them passes a scale).
Not measured: the shared kernel's own prefetch (`if (jn < cpt) fetch(jn, cn)`) was not edited.
"""
import pytest
import torch

from tests import attn_decode_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
GUARD = 4          # guard columns on each side of the result: the result starts 8 bytes into a 16-byte aligned row


@pytest.fixture(scope="module")
def ops(built_lib):
    from internnav_amd import ops

    return ops


def _bits(t):
    return t.view(torch.int16)


def _framed(blocks, rows, H):
    """a sentinel buffer [blocks, rows + 2, H * D + 2 * GUARD] and its [blocks, rows, H, D] result view (a guard row above and below every block)"""
    W = H * R.D + 2 * GUARD
    buf = torch.full((blocks, rows + 2, W), R.SENTINEL, dtype=BF16, device=DEV)
    out = buf.as_strided((blocks, rows, H, R.D), ((rows + 2) * W, W, R.D, 1), W + GUARD)
    assert out.data_ptr() % 16 == 8 and out.stride(1) > H * R.D
    frame = torch.ones_like(buf, dtype=torch.bool)
    frame[:, 1:-1, GUARD:GUARD + H * R.D] = False
    return buf, out, frame


def _launch_pairs(ops, c, inp):
    fused, cache = inp["fused"].to(DEV), inp["cache"].to(DEV)
    tails = None if inp["tails"] is None else inp["tails"].to(DEV)
    q, k, v, kc, vc, kt, vt = R.pair_views(c, fused, cache, tails)
    buf, out, frame = _framed(inp["P"], c["m"], c["H"])
    t = {n: inp[n].to(DEV) for n in ("slot", "pfx_len", "suf_len", "tail_row", "tail_len")}
    if c["entry"] == "prefix":
        ops.attention_prefix(q, k, v, kc, vc, t["slot"], t["pfx_len"], t["suf_len"], out=out, scale=c["scale"], max_pfx=c["max_pfx"])
    else:
        ops.attention_prefix_tail(q, k, v, kc, vc, t["slot"], t["pfx_len"], t["suf_len"], kt, vt, t["tail_row"], t["tail_len"], out=out, scale=c["scale"],
                                  max_pfx=c["max_pfx"], max_tail=c["max_tail"])
    torch.cuda.synchronize()
    return buf, out, frame


def _launch_shared(ops, c, inp, **tables):
    fused, tail, cache = inp["fused"].to(DEV), inp["tail"].to(DEV), inp["cache"].to(DEV)
    q, kt, vt, kc, vc = R.shared_views(c, fused, tail, cache)
    buf, out, frame = _framed(1, inp["R"] + 1, c["H"])
    t = [tables.get(n, inp[n]).to(DEV) for n in ("tile_rows", "tile_slot", "tile_pfx", "tail_len")]
    ops.attention_shared(q, kt, vt, kc, vc, *t, out=out[0], scale=c["scale"], max_pfx=c["max_pfx"])
    torch.cuda.synchronize()
    return buf, out[0], frame


def _judge(c, out, buf, frame, ref, bound, nan, written):
    assert bool((buf[frame] == R.SENTINEL).all()), f"{c['name']}: the launch wrote outside its result"
    got = out.cpu()
    skipped = ~written.view(written.shape + (1,) * (got.dim() - written.dim())).expand(got.shape)
    assert bool((got[skipped] == R.SENTINEL).all()), f"{c['name']}: a row no table names was written"
    w, ok = R.check(got, ref, bound, nan, written)
    print(f"{c['name']}: worst |err| / bound {w:.3f}" + (f", {int(nan.sum())} NaN rows as promised" if bool(nan.any()) else ""))
    assert ok, f"{c['name']}: worst |err| / bound {w:.3f} (limit 1.0; == where the bound is 0, NaN where the contract says NaN)"


@pytest.mark.parametrize("c", R.PREFIX, ids=lambda c: c["name"])
def test_attention_prefix_against_fp64(ops, c):
    inp, ref, bound, nan, written = R.case_reference(c)
    buf, out, frame = _launch_pairs(ops, c, inp)
    _judge(c, out, buf, frame, ref, bound, nan, written)


@pytest.mark.parametrize("c", R.PREFIX_TAIL, ids=lambda c: c["name"])
def test_attention_prefix_tail_against_fp64(ops, c):
    inp, ref, bound, nan, written = R.case_reference(c)
    buf, out, frame = _launch_pairs(ops, c, inp)
    _judge(c, out, buf, frame, ref, bound, nan, written)


@pytest.mark.parametrize("c", R.SHARED, ids=lambda c: c["name"])
def test_attention_shared_against_fp64(ops, c):
    inp, ref, bound, nan, written = R.case_reference(c)
    buf, out, frame = _launch_shared(ops, c, inp)
    _judge(c, out, buf, frame, ref, bound, nan, written)
    if c["ramp"]:
        # the ramp row alone in its tile: the bits it has among rows whose tails are longer than its own, and nothing else written
        r = c["ramp"][0]
        tile = next(t for t in range(inp["tile_rows"].shape[0]) if r in inp["tile_rows"][t].tolist())
        assert any(int(inp["tail_len"][x]) > int(inp["tail_len"][r]) for x in inp["tile_rows"][tile].tolist() if x >= 0)
        alone = torch.full((1, inp["tile_rows"].shape[1]), -1, dtype=torch.int32)
        alone[0, 0] = r
        buf1, out1, frame1 = _launch_shared(ops, c, inp, tile_rows=alone, tile_slot=inp["tile_slot"][tile:tile + 1], tile_pfx=inp["tile_pfx"][tile:tile + 1])
        assert torch.equal(_bits(out1[r]), _bits(out[r])), "the ramp row's bits depend on the rows that share its tile"
        rest = [x for x in range(inp["R"] + 1) if x != r]
        assert bool((out1[rest] == R.SENTINEL).all()) and bool((buf1[frame1] == R.SENTINEL).all())
