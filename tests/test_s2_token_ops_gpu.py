"""Op-level GPU tests of the System-2 token kernels (internnav_amd/csrc/rope.hip: gather_kernel, rope_kernel<1>, rope_kernel<4>,
mrope_table_kernel, argmax_kernel), each against the float64 restatement of tests/s2_ops_ref.py on the same inputs, at the shapes where the
launchers switch kernels, cut a head chunk short or take a second trip through a grid-stride loop.

rope: tables with independent random halves (a sign flip, a table value read from the wrong half or a head chunk that is cut at the wrong count
are all visible), x buffers wider than the rotated columns, all-or-nothing per element:
    |out - ref| <= 4 * 2^-24 * (|lo*cos| + |hi*sin|) + 2^-8 * |ref|      rotated elements (round-to-nearest to bf16; a truncating store fails)
    out == ref                                                           everything that is copied or must stay as it is
Which of the two kernels runs is decided by ina_launch_rope: rope_kernel<4> iff rows * (heads + v_heads) * D / 16 >= 2^19; every case states
which one it expects and asserts the rule.

mrope_table: |cos - ref|, |sin - ref| <= K_MROPE * 2^-24 against cos / sin (float64) of the fp32 angle. Measured on an MI355X (ROCm 7):
worst |err| / 2^-24 = 1.138 (cos, n = 5000; sin 1.097) over n in {1, 257, 5000}, positions up to 40000; K_MROPE = 4 x that = 4.552, under the
cap of 8 (fp32 CPU libm: 0.60).

gather_rows: torch.equal with the expected buffer, sentinel rows and padding columns included.

argmax_rows: torch.argmax (first maximum) for every tie placement the kernel's reduction tree has; a row without any entry above -inf returns 0
and a row of NaNs an index in [0, n). Before the clamp in argmax_kernel a 16-byte-aligned row of -inf or NaN returned 0x7fffffff when
n % 4 == 0 - the next gather_rows launch would have used it as an embedding row - and the first element of the scalar tail (1020 for n = 1023,
152064 for n = 152065) when n % 4 != 0.
"""
import math

import pytest
import torch

from tests import s2_ops_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32, BF16, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32
U = S.U
MROPE_WORST = 1.138        # measured, see above
K_MROPE = min(8.0, 4.0 * MROPE_WORST)


@pytest.fixture(scope="module")
def ops(built_lib):
    from internnav_amd import ops

    return ops


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, g, dtype=F32, scale=1.0):
    return (torch.randn(shape, generator=g, device=DEV, dtype=F32) * scale).to(dtype)


def _perm(n, g):
    return torch.randperm(n, generator=g, device=DEV)


# ------------------------------------------------------------------------------------------------------------------------ rope
def _check_rope(out, ref, scale, what):
    """exact where scale == 0, the rope bound elsewhere; returns the worst |err| / bound over the rotated elements."""
    o = out.to(F64)
    keep = scale == 0
    n_keep = int((o[keep] != ref[keep]).sum())
    assert n_keep == 0, f"{what}: {n_keep} elements outside the rotated columns / rows changed"
    err, bound = (o - ref).abs()[~keep], S.rope_bound(ref, scale)[~keep]
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())}/{err.numel()} rotated elements out of bound, worst |err| / bound {(err / bound).max().item():.3f}"
    return (err / bound).max().item() if err.numel() else 0.0


def _rope_case(ops, what, chunked, rows, heads, D, g, col0=0, extra=8, tab_rows=None, row_map=None, kv_head0=None, v_heads=0, dup=False):
    """build the buffers of one rope launch, run reference then kernel, check x (and the cache). chunked: rope_kernel<4> expected."""
    hv = heads + (v_heads if kv_head0 is not None else 0)
    assert ((rows * hv * (D // 16)) >= (1 << 19)) == chunked, f"{what}: expected rope_kernel<{4 if chunked else 1}>"
    phys = int(S.map_rows(rows, row_map)[-1]) + 1 + (3 if row_map else 0)
    ld = col0 + hv * D + extra
    x = _randn((phys, ld), g, BF16)
    n_tab = max(tab_rows or 0, rows)          # never fewer table rows than rows: a kernel that ignores tab reads wrong values, not foreign memory
    if dup:
        a = torch.rand(n_tab, D // 2, generator=g, device=DEV, dtype=F64) * 2 * math.pi
        cos, sin = torch.cat([a.cos(), a.cos()], 1).float(), torch.cat([a.sin(), a.sin()], 1).float()
    else:
        cos, sin = _randn((n_tab, D), g), _randn((n_tab, D), g)
    kw = dict(col0=col0, rows=rows, row_map=row_map)
    if tab_rows:
        tab = torch.randint(0, tab_rows, (rows,), generator=g, device=DEV).to(I32)           # a table smaller than the rows: repeats
        tab[: min(rows, tab_rows)] = _perm(tab_rows, g)[: min(rows, tab_rows)].to(I32)       # ... on top of a permutation
        kw["tab"] = tab
    kv = None
    if kv_head0 is not None:
        nk = heads - kv_head0
        kv = torch.full((rows + 5, (nk + v_heads) * D + 16), -7.0, dtype=BF16, device=DEV)   # wider and longer than what is written
        kw.update(kv_out=kv, kv_dst=_perm(rows + 5, g)[:rows].to(I32), kv_head0=kv_head0, v_heads=v_heads)
    x0 = x.clone()
    (ref, scale), kvr = S.rope(x, cos, sin, heads, D, **kw)
    ops.rope(x, cos, sin, heads, D, **kw)
    torch.cuda.synchronize()
    worst = _check_rope(x, ref, scale, what + " x")
    if kv is not None:
        a = col0 + kv_head0 * D
        assert torch.equal(x.view(torch.int16)[:, a:], x0.view(torch.int16)[:, a:]), f"{what}: the k / v columns of x must stay bit-unchanged"
        worst = max(worst, _check_rope(kv, *kvr, what + " cache"))
        written = torch.zeros(kv.shape[0], dtype=torch.bool, device=DEV)
        written[kw["kv_dst"].long()] = True
        assert (kv[~written] == -7.0).all() and (kv[:, (heads - kv_head0 + v_heads) * D:] == -7.0).all(), f"{what}: cache sentinel overwritten"
    print(f"rope {what}: rope_kernel<{4 if chunked else 1}>, worst |err| / bound {worst:.3f}")
    return worst


def test_rope_decoder_shape_both_kernels(ops):
    """28 q + 4 k heads of 128 in place (and from column 128 of a wider row): 37 rows -> rope_kernel<1>, 2100 rows -> rope_kernel<4>."""
    g = _gen(1)
    _rope_case(ops, "decoder 37 rows", False, 37, 32, 128, g)
    _rope_case(ops, "decoder 2100 rows", True, 2100, 32, 128, g)
    _rope_case(ops, "decoder 37 rows col0=128", False, 37, 32, 128, g, col0=128)
    _rope_case(ops, "decoder 2100 rows col0=8", True, 2100, 32, 128, g, col0=8)
    _rope_case(ops, "decoder 2100 rows, unit tables with repeated halves", True, 2100, 32, 128, g, dup=True)


def test_rope_fused_kv_append_both_kernels(ops):
    """q | k | v rows of the decoder (28 + 4 + 4 heads): q rotated in place, k rotated into the cache row, v copied; 37 rows -> <1>, 1900 rows
    -> <4> (hv = 36). The cache is wider and longer than what is written and keeps its sentinel; x's k / v columns keep their bits."""
    g = _gen(2)
    _rope_case(ops, "fused 37 rows", False, 37, 32, 128, g, kv_head0=28, v_heads=4)
    _rope_case(ops, "fused 1900 rows", True, 1900, 32, 128, g, kv_head0=28, v_heads=4)
    _rope_case(ops, "fused 1900 rows col0=16 tab", True, 1900, 32, 128, g, col0=16, kv_head0=28, v_heads=4, tab_rows=700)


def test_rope_ragged_head_chunks(ops):
    """heads = 7, kv_head0 = 5, v_heads = 2: hv = 9 -> chunks {0..3}, {4..7}, {8}: the second straddles kv_head0 and the key / value boundary,
    the last holds one value head. Both kernels."""
    g = _gen(3)
    _rope_case(ops, "ragged 7300 rows", True, 7300, 7, 128, g, kv_head0=5, v_heads=2)
    _rope_case(ops, "ragged 41 rows", False, 41, 7, 128, g, kv_head0=5, v_heads=2)
    _rope_case(ops, "ragged in place 9400 rows", True, 9400, 7, 128, g)                    # chunks {0..3}, {4..6}
    _rope_case(ops, "ragged keys only 9400 rows", True, 9400, 7, 128, g, kv_head0=3, v_heads=0)


def test_rope_vision_shape_and_d16(ops):
    """32 heads of 80 (five 8-wide groups per half-pair) at 3300 rows -> <4>; D = 16 (one group) with both kernels."""
    g = _gen(4)
    _rope_case(ops, "vision 3300 rows", True, 3300, 32, 80, g)
    _rope_case(ops, "vision 29 rows", False, 29, 32, 80, g)
    _rope_case(ops, "D=16 37 rows", False, 37, 3, 16, g)
    _rope_case(ops, "D=16 66000 rows", True, 66000, 8, 16, g)
    _rope_case(ops, "D=16 fused 75000 rows", True, 75000, 6, 16, g, kv_head0=4, v_heads=1)


def test_rope_tab_and_row_map(ops):
    """tab (a permutation plus repeats into a smaller table) and row_map (segments of 7 rows every 9, from row 2), alone and together."""
    g = _gen(5)
    for rows, heads, chunked in ((61, 6, False), (2100, 32, True)):
        _rope_case(ops, f"tab {rows} rows", chunked, rows, heads, 128, g, tab_rows=max(16, rows // 3))
        _rope_case(ops, f"row_map {rows} rows", chunked, rows, heads, 128, g, row_map=(7, 9, 2))
        _rope_case(ops, f"tab + row_map {rows} rows", chunked, rows, heads, 128, g, tab_rows=max(16, rows // 3), row_map=(7, 9, 2))
    _rope_case(ops, "tab + row_map + fused 1900 rows", True, 1900, 32, 128, g, tab_rows=500, row_map=(7, 9, 2), kv_head0=28, v_heads=4, col0=8)


def test_rope_second_grid_stride_trip(ops):
    """rope_kernel<4> with more threads than the 8192 x 256 grid: 262400 rows x 1 chunk x 8 groups = 2099200 threads (x is 135 MB)."""
    rows, heads, D = 262400, 2, 128
    assert rows * ((heads + 3) // 4) * (D // 16) > 8192 * 256
    _rope_case(ops, "grid-stride", True, rows, heads, D, _gen(6), extra=8, tab_rows=1000)


# ------------------------------------------------------------------------------------------------------------------------ mrope_table
def _mrope_inputs(n, g):
    inv_freq = (1.0 / (1000000.0 ** (torch.arange(0, 128, 2, dtype=F32) / 128))).to(DEV)
    axis_of = torch.tensor([0] * 16 + [1] * 24 + [2] * 24, dtype=I32, device=DEV)
    pos = torch.randint(0, 40001, (3, n), generator=g, device=DEV).to(I32)
    pos[:, 0] = torch.tensor([40000, 39999, 123], dtype=I32, device=DEV)
    return pos, inv_freq, axis_of


@pytest.mark.parametrize("n", [1, 257, 5000])
def test_mrope_table(ops, n):
    """distinct t / h / w rows reaching 40000; halves bit-equal; nothing written behind n * D; |err| <= K_MROPE * 2^-24 (see the module docstring)."""
    D = 128
    pos, inv_freq, axis_of = _mrope_inputs(n, _gen(10 + n))
    assert n == 1 or not (torch.equal(pos[0], pos[1]) or torch.equal(pos[1], pos[2]) or torch.equal(pos[0], pos[2]))
    assert int(pos.max()) == 40000
    cos = torch.full((n + 1, D), 9.0, dtype=F32, device=DEV)             # one row more than is written
    sin = torch.full((n + 1, D), 9.0, dtype=F32, device=DEV)
    (cref, _), (sref, _) = S.mrope_table(pos, inv_freq, axis_of)
    ops.mrope_table(pos, inv_freq, axis_of, cos, sin)
    torch.cuda.synchronize()
    assert (cos[n:] == 9.0).all() and (sin[n:] == 9.0).all(), "written behind n * D"
    c, s = cos[:n], sin[:n]
    assert torch.equal(c[:, : D // 2].view(I32), c[:, D // 2:].view(I32)) and torch.equal(s[:, : D // 2].view(I32), s[:, D // 2:].view(I32))
    ec, es = (c.double() - cref).abs().max().item() / U, (s.double() - sref).abs().max().item() / U
    print(f"MROPE_TABLE n={n}: worst |cos err| / 2^-24 = {ec:.3f}, |sin err| / 2^-24 = {es:.3f} (bound constant in use: {K_MROPE})")
    assert ec <= K_MROPE and es <= K_MROPE


# ------------------------------------------------------------------------------------------------------------------------ gather_rows
def _fill(shape, dtype, g):
    if dtype == torch.uint8:
        return torch.randint(0, 255, shape, generator=g, device=DEV, dtype=torch.uint8)     # 255 is the sentinel
    return _randn(shape, g, dtype)


def _sentinel(dtype):
    return 255 if dtype == torch.uint8 else -7.0


def _gather_case(ops, what, dtype, C, g, n_src_rows, n_idx, rows=None, use_src=True, use_dst=True, pad_x=0, pad_out=0):
    """x [n_src_rows, C] and out [n_out, C], optionally as column slices of buffers pad_* wider; src with repeats, dst a partial permutation."""
    rows_eff = n_idx if rows is None else rows
    n_x = n_src_rows if use_src else n_idx
    xb = _fill((n_x, C + pad_x), dtype, g)
    x = xb[:, :C]
    n_out = n_idx + 7
    ob = torch.full((n_out, C + pad_out), _sentinel(dtype), dtype=dtype, device=DEV)
    out = ob[:, :C]
    src = torch.randint(0, n_src_rows, (n_idx,), generator=g, device=DEV).to(I32) if use_src else None
    if use_src and n_idx >= 4:
        src[3] = src[1]                                                                      # a repeat for certain
    dst = _perm(n_out, g)[:n_idx].to(I32) if use_dst else None
    ref, _ = S.gather_rows(x, out, src, dst, rows)
    ops.gather_rows(x, out, src, dst, rows)
    torch.cuda.synchronize()
    assert torch.equal(out, ref), f"{what}: {int((out != ref).any(1).sum())} rows differ"
    named = torch.zeros(n_out, dtype=torch.bool, device=DEV)
    named[(dst[:rows_eff].long() if use_dst else torch.arange(rows_eff, device=DEV))] = True
    assert (ob[~named] == _sentinel(dtype)).all(), f"{what}: a row not named in dst lost its sentinel"
    assert pad_out == 0 or (ob[:, C:] == _sentinel(dtype)).all(), f"{what}: padding columns of out overwritten"


@pytest.mark.parametrize("dtype", [BF16, F32, torch.uint8], ids=["bf16", "f32", "u8"])
def test_gather_rows_index_forms_and_layouts(ops, dtype):
    """src only, dst only, both; rows of 16 and of 2352 bytes (the pixel rows); row-strided x / out; rows smaller than the index vectors."""
    es = torch.empty(0, dtype=dtype).element_size()
    g = _gen(20 + es)
    for nbytes in (16, 2352):
        C, pad = nbytes // es, 16 // es
        for use_src, use_dst in ((True, False), (False, True), (True, True)):
            what = f"{dtype} {nbytes} B src={use_src} dst={use_dst}"
            _gather_case(ops, what, dtype, C, g, 50, 37, use_src=use_src, use_dst=use_dst)
            _gather_case(ops, what + " strided", dtype, C, g, 50, 37, use_src=use_src, use_dst=use_dst, pad_x=pad, pad_out=2 * pad)
            _gather_case(ops, what + " rows < len(index)", dtype, C, g, 50, 37, rows=33, use_src=use_src, use_dst=use_dst, pad_out=pad)
    _gather_case(ops, f"{dtype} one row", dtype, 16 // es, g, 5, 1)


def test_gather_rows_past_the_grid_cap(ops):
    """5000 rows of 3584 bf16 (a prefill's embedding lookup): 2.24 M 16-byte vectors > 8192 x 256 threads, the grid-stride loop takes a second trip."""
    assert 5000 * 3584 * 2 // 16 > 8192 * 256
    _gather_case(ops, "prefill embed", BF16, 3584, _gen(29), 6000, 5000)
    _gather_case(ops, "prefill embed strided, src only", BF16, 3584, _gen(30), 6000, 5000, use_dst=False, pad_x=8, pad_out=8)


# ------------------------------------------------------------------------------------------------------------------------ argmax_rows
def _rows_view(vals, aligned):
    """vals [R, n] f32 -> a view with the same values whose rows all start on (aligned) / 4 bytes past (not aligned) a 16-byte boundary."""
    R, n = vals.shape
    ld = (n + 3) // 4 * 4 + 4
    buf = torch.zeros(R, ld, dtype=F32, device=DEV)
    v = buf[:, :n] if aligned else buf[:, 1: n + 1]
    v.copy_(vals)
    assert all(((v.data_ptr() + r * ld * 4) % 16 == 0) == aligned for r in (0, R - 1))
    return v


def _argmax(ops, v):
    out = torch.full((v.shape[0],), -5, dtype=I32, device=DEV)
    ops.argmax_rows(v, out)
    return out.tolist()


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
def test_argmax_rows_tie_placements(ops, aligned):
    """two equal maxima, the first must win. Aligned rows: thread t of 1024 reads the 16-byte vectors t, t + 1024, ... (elements 4t..4t+3,
    4t + 4096.., ...) and the elements behind the last whole vector one by one; unaligned rows are read one by one (element j by thread j % 1024).
    The pairs put the first maximum in the HIGHER thread / lane / wave wherever that is possible, so a reduction that prefers the lower one fails."""
    n = 152065
    pairs = [
        (21, 21 + 4096 * 3),          # one thread's own stream (aligned: vector stream of thread 5; unaligned: thread 21, j and j + 1024 * 12)
        (40, 4108),                   # aligned: threads 10 and 3 (second trip) of wave 0; unaligned: threads 40 and 12
        (280, 4104),                  # aligned: thread 70 (wave 1) and thread 2 (wave 0); unaligned: threads 280 (wave 4) and 8 (wave 0)
        (2, 152064),                  # aligned: vector part and scalar tail of thread 0; unaligned: thread 2 and thread 512
        (512, 152064),                # aligned: thread 128 (wave 2) vector part, thread 0 tail; unaligned: both thread 512
        (5, 5 + 2048),                # unaligned: one thread's scalar stream
        (152063, 152064),             # the last whole vector and the tail
    ]
    g = _gen(40)
    vals = _randn((len(pairs), n), g)
    for r, (a, b) in enumerate(pairs):
        vals[r, a] = vals[r, b] = 50.0
    got = _argmax(ops, _rows_view(vals, aligned))
    assert got == [a for a, _ in pairs] == vals.argmax(1).tolist(), got


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 1024, 12288, 12400, 12547, 16384, 16389, 28675, 152064, 152065])
def test_argmax_rows_sizes_and_edges(ops, n, aligned):
    """random rows, rows holding -inf entries, the maximum at either end; then the rows without a maximum: all -inf -> 0 (torch.argmax),
    all NaN -> some index in [0, n); NaN entries next to finite ones are never chosen."""
    g = _gen(50 + n)
    vals = _randn((8, n), g)
    vals[1, torch.rand(n, generator=g, device=DEV) < 0.5] = -math.inf
    vals[2, : n - 1] = -math.inf                                   # only the last entry is finite
    vals[3, 0] = 40.0
    vals[4, n - 1] = 40.0
    vals[5] = vals[5].abs().neg() - 1e30                           # every entry rounds to -1e30: an all-equal finite row, first index
    vals[6, 1:] = -math.inf                                        # only the first entry is finite
    vals[7] = -3.0e38
    got = _argmax(ops, _rows_view(vals, aligned))
    assert got == S.argmax_rows(vals)[0].tolist(), (n, got)
    edge = torch.full((3, n), -math.inf, device=DEV)
    edge[1] = math.nan
    edge[2] = math.nan
    edge[2, n // 2] = -math.inf
    got = _argmax(ops, _rows_view(edge, aligned))
    assert got[0] == 0, f"all -inf must give 0 as torch.argmax does, got {got[0]}"
    assert 0 <= got[1] < n and 0 <= got[2] < n, f"rows of NaN must give an index in [0, {n}), got {got[1:]}"
    if n >= 4:
        mixed = _randn((2, n), g)
        mixed[0, ::2] = math.nan
        mixed[1, 1::3] = math.nan
        mixed[1, 0] = math.nan
        got = _argmax(ops, _rows_view(mixed, aligned))
        assert got == mixed.nan_to_num(nan=-math.inf).argmax(1).tolist(), "a NaN entry was chosen over a finite one"
