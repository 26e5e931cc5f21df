"""The NextDiT block kernels (ops.dit_attention / ops.dit_v2t: dit_attn_kernel<6>, dit_attn_stats_kernel<6, 1..4>, dit_v2t_kernel of
internnav_amd/csrc/dit_attention.hip; ops.dit_rowchain: the four dit_rowchain_kernel instances of internnav_amd/csrc/dit_rowchain.hip) against the
float64 restatement of tests/dit_block_ref.py at their tile and mask edges. The reference, the per-element bounds (derived from the number formats,
limit 1.0) and the case tables live in tests/dit_block_ref.py; tests/test_dit_block_ref_cpu.py checks them without a GPU (independent float64
restatements, an emulation of the kernels' rounding points, the 22 mutations that must leave the bound).

One launch per case and kernel, every element against its bound (`==` where the bound is 0, NaN never passes). Inputs are views into NaN-filled
buffers (x a column slice between NaN guard rows, kv2 the [:, :Lz] slice of a 64-row condition buffer whose other rows are NaN: the clamped loads
must never bring one in); outputs are pre-filled with NaN inside sentinel buffers whose guard rows and columns must stay untouched; the v1 pair of
handed-over statistics is NaN.

Measured worst |err| / bound (MI355X, ROCm 7):
    dit_attn_kernel<6>            own statistics, 27 cases                                   0.200
    dit_attn_stats_kernel<6,1>    Lz 1, 15, 16 (statistics handed over)                      0.212
    dit_attn_stats_kernel<6,2>    Lz 17, 32                                                  0.093
    dit_attn_stats_kernel<6,3>    Lz 33, 36, 48                                              0.120
    dit_attn_stats_kernel<6,4>    Lz 49, 63, 64                                              0.113
    dit_v2t                       Lz 1, 5, 32, 33, 64 at 44 envs: bit-equal, 0 mismatches
    row chain (K1 384, no W2)     X 0.901   H 0.990
    row chain (K1 384, SwiGLU)    X 0.891   C2 0.138
    row chain (K1 1024, no W2)    X 0.839   H 0.990
    row chain (K1 1024, plain)    X 0.913   C2 0.279   seg_stats 0.598
    hand-over (K1 1024, N2 1536)  device statistics vs the float64 ones of the stored rows 0.230; attention with the device's pairs 0.139,
                                  against the exact statistics with the measured distance as the statistics term 0.137
(the float32 / bf16 emulation of tests/test_dit_block_ref_cpu.py gives the same figures: attention 0.200 / 0.212, X 0.913, H 0.990, C2 0.292,
seg_stats 0.598. The attention bound is a worst-case sum over the 64 bf16 roundings of a logit, hence the distance; X and H are one bf16
rounding of a value, which reaches its half ulp.)
With these single edits of a scratch copy of the kernels (never committed; arithmetic or a mask only) the suite fails as follows, and passes in
every other case:
    `kv < T` as `kv <= T`, dit_attn_kernel        the 18 own-statistics cases with 2 <= T <= 31 fail (the clamped loads add a copy of key T - 1; at
                                                  T = 1 the copy has the same V and nothing moves, at T = 32 there is no slot 32);
    the same in dit_attn_stats_kernel             the same 18 cases with handed-over statistics fail, no own-statistics case;
    `(t*16 + r) < lim` as `<=`, dit_attn_kernel   the 21 own-statistics cases with Lz < 64 and a gate other than 0 fail (key Lz = K[Lz - 1] with the zero V
                                                  of its empty V2T slot);
    the same in dit_attn_stats_kernel             16 handed-over cases fail: as above without Lz = 16, 32, 48, whose extra key lies in a tile that the
                                                  KT instance does not compute;
    `p.eps` dropped from the statistics           all 27 own-statistics cases fail (the constant segment: NaN), no handed-over one;
    bf16 rounding of `o1` removed (either kernel) NOT seen, all 98 pass: the model has that rounding as u8 |o1|, and a kernel without it is inside;
    `seq / p.seq_per_env` as `seq % ...` (clamped to the last env, so that the address stays valid), dit_attn_kernel: the 19 own-statistics
                                                  cases with more than one env or S > 1 and a gate other than 0 fail;
    the same in dit_attn_stats_kernel             the same 19 handed-over cases and the hand-over test fail;
    `tanhf(gt[i])` as `gt[i]`, row-chain table    the 15 row-chain cases with a gate and the hand-over test fail at stage X;
    `mb` fixed to 0                               the 8 cases with mod_div 128 and M > 128 fail at stage X, none with one modulation row;
    `rstd2` from `s1`, no-W2 form                 the 5 no-W2 cases that store H fail at stage H; with a second GEMM: its 12 cases and the hand-over at C2;
    segment pair written at `(nt/3 + 1)`          the 4 seg_stats cases, their row-locality case and the hand-over fail (slot 0 keeps its NaN, the last
                                                  pair lands in the next row or in the guard row below: the address stays inside the buffer);
    `seg_q` variance without `- mean * mean`      the 4 seg_stats cases and the hand-over test fail, C2 and everything else pass.
"""
import ctypes as C

import pytest
import torch

from tests import dit_block_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
F32 = torch.float32
NAN = float("nan")
SENTINEL = -7.0
WORST = {}


@pytest.fixture(scope="module")
def ops(built_lib):
    from internnav_amd import ops

    yield ops
    for k in sorted(WORST):
        print(f"worst |err|/bound  {k:<44s} {WORST[k]:.3f}")


def _note(group, w):
    WORST[group] = max(WORST.get(group, 0.0), w)


def _check(name, group, out, ref, bound):
    w, ok = R.ratio(out.cpu(), ref, bound)
    print(f"{name} [{group}]: worst |err|/bound {w:.3f}")
    _note(group, w)
    assert ok, f"{name} [{group}]: outside the bound (or not exact where the bound is 0, or NaN): {w:.3f}"


def _framed(rows, cols, dtype, pad_cols, fill=SENTINEL):
    """(buffer, view): a [rows, cols] view with one guard row above and below and pad_cols guard columns on each side."""
    buf = torch.full((rows + 2, cols + 2 * pad_cols), fill, dtype=dtype, device=DEV)
    return buf, buf[1:-1, pad_cols:pad_cols + cols]


def _guard_ok(buf, rows, cols, pad_cols, what):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[1:-1, pad_cols:pad_cols + cols] = False
    assert bool((buf[mask] == SENTINEL).all()), f"{what}: wrote outside the output view"


# ------------------------------------------------------------------------------------------------------------ attention
def _attn_device(inp, Lz):
    """x inside a NaN frame, kv2 as the [:, :Lz] slice of a 64-row condition buffer with NaN rows beyond, norms, gate."""
    x_cpu, kv_cpu = inp["x"], inp["kv2"]
    xbuf, x = _framed(x_cpu.shape[0], 4 * R.D, BF16, 8, fill=NAN)
    x.copy_(x_cpu)
    cond = torch.full((kv_cpu.shape[0], 64, 2, R.HEADS, R.HD), NAN, dtype=BF16, device=DEV)
    cond[:, :Lz] = kv_cpu.to(DEV)
    norms = [(g.to(DEV), b.to(DEV)) for g, b in inp["norms"]]
    gate = None if inp["gate"] is None else inp["gate"].to(DEV)
    return xbuf, x, cond, cond[:, :Lz], norms, gate


def _v2t(ops, kv2):
    v2t = torch.full((kv2.shape[0], R.HEADS, 64, 64), NAN, dtype=BF16, device=DEV)
    ops.dit_v2t(kv2, R.HEADS, v2t)
    return v2t


def _attn_launch(ops, c, x, kv2, v2t, norms, gate, stats):
    rows = x.shape[0]
    obuf, out = _framed(rows, R.D, BF16, 8)
    out.fill_(NAN)
    res = ops.dit_attention(x, out, norms, kv2, v2t, gate, T=c["T"], seq_per_env=c["S"], heads=R.HEADS, eps=c["eps"], scale=c["scale"], stats=stats)
    torch.cuda.synchronize()
    assert res is out
    _guard_ok(obuf, rows, R.D, 8, c["name"])
    return out


@pytest.mark.parametrize("with_stats", [False, True], ids=["own_stats", "stats_given"])
@pytest.mark.parametrize("c", R.ATTN, ids=lambda c: c["name"])
def test_attention(ops, c, with_stats):
    """dit_attn_kernel<6> (own statistics) and dit_attn_stats_kernel<6, KT> (float64 statistics rounded to fp32 handed over, the v1 pair NaN): T at
    both ends of both 16-token tiles, Lz at both ends of every KT instance, envs / S maps, gate given / None / exactly 0 / saturated."""
    inp, st, ref, bound = R.attn_reference(c, with_stats)
    xbuf, x, cond, kv2, norms, gate = _attn_device(inp, c["Lz"])
    x_before, cond_before = xbuf.clone(), cond.clone()
    v2t = _v2t(ops, kv2)
    assert torch.equal(v2t.cpu(), R.v2t_ref(inp["kv2"])), "V2T image"
    st_dev = None if st is None else st.to(DEV)
    out = _attn_launch(ops, c, x, kv2, v2t, norms, gate, st_dev)
    same = lambda a, b: torch.equal(a.view(torch.int16), b.view(torch.int16))          # noqa: E731  (bit pattern: NaN == NaN)
    assert same(xbuf, x_before) and same(cond, cond_before), "an input buffer was written"
    assert c["KT"] == (c["Lz"] + 15) // 16
    group = f"dit_attn_stats_kernel<6,{c['KT']}>" if with_stats else "dit_attn_kernel<6>"
    _check(c["name"], group, out, ref, bound)
    if c["gate"] == "zero":                      # the cross branch contributes exactly 0: the result does not depend on the condition at all
        kv_other = torch.randn(kv2.shape, generator=torch.Generator().manual_seed(1)).to(BF16).to(DEV)
        out2 = _attn_launch(ops, c, x, kv_other, _v2t(ops, kv_other), norms, gate, st_dev)
        assert torch.equal(out2, out), "gate 0: the cross branch leaked into the result"


@pytest.mark.parametrize("Lz", R.V2T_LZ)
def test_v2t(ops, Lz):
    """44 envs: more elements than the 4096-block grid covers in one trip. Every one of the 64 slots written (zero beyond Lz), bit for bit."""
    envs = R.V2T_ENVS
    assert envs * R.HEADS * 4096 > 4096 * 256
    kv_cpu = torch.randn(envs, Lz, 2, R.HEADS, R.HD, generator=torch.Generator().manual_seed(Lz)).to(BF16)
    cond = torch.full((envs, 64, 2, R.HEADS, R.HD), NAN, dtype=BF16, device=DEV)
    cond[:, :Lz] = kv_cpu.to(DEV)
    buf = torch.full((envs + 1, R.HEADS, 64, 64), NAN, dtype=BF16, device=DEV)
    buf[envs] = SENTINEL
    ops.dit_v2t(cond[:, :Lz], R.HEADS, buf[:envs])
    torch.cuda.synchronize()
    got = buf.cpu()
    assert not torch.isnan(got[:envs]).any(), "a slot was not written"
    assert torch.equal(got[:envs], R.v2t_ref(kv_cpu)), f"{(got[:envs] != R.v2t_ref(kv_cpu)).sum().item()} elements differ"
    assert bool((got[envs] == SENTINEL).all()), "wrote beyond the last env"
    _note("dit_v2t (bit-exact: mismatches)", 0.0)


# ------------------------------------------------------------------------------------------------------------ row chain
def _rc_launch(ops, c, inp, nan_rows=None):
    """one launch into framed buffers; returns the outputs and a closure that checks every guard."""
    M, K1, N2 = c["M"], c["K1"], c["N2"]
    abuf, a = _framed(M, K1, BF16, 8, fill=NAN)
    a.copy_(inp["a_in"])
    xbuf, x = _framed(M, R.D, F32, 4)
    x.copy_(inp["x0"])
    if nan_rows is not None:
        a[nan_rows[0]] = NAN
        x[nan_rows[1]] = NAN
    nb = (M + c["mod_div"] - 1) // c["mod_div"]
    mod = torch.full((nb, 2 * R.D + 16), NAN, dtype=F32, device=DEV)            # gate | mod_scale2 as row-strided views of one table
    gate = ms2 = None
    if inp["gate"] is not None:
        gate = mod[:, :R.D]
        gate.copy_(inp["gate"])
    if inp["ms2"] is not None:
        ms2 = mod[:, R.D:2 * R.D]
        ms2.copy_(inp["ms2"])
    dev = lambda t: None if t is None else t.to(DEV)                            # noqa: E731
    kw, frames, res = {}, [(xbuf, M, R.D, 4, "X")], {}
    if c["h"]:
        hbuf, h = _framed(M, R.D, BF16, 8)
        h.fill_(NAN)
        kw["h"], res["H"] = h, h
        frames.append((hbuf, M, R.D, 8, "H"))
    if N2:
        n_out = N2 // 2 if c["glu"] else N2
        cbuf, c2 = _framed(M, n_out, BF16, 8)
        c2.fill_(NAN)
        kw.update(w2=dev(inp["w2"]), c2=c2, glu2=c["glu"])
        res["C2"] = c2
        frames.append((cbuf, M, n_out, 8, "C2"))
    if c["seg"]:
        sbuf = torch.full((M + 2, N2 // R.D, 2), SENTINEL, dtype=F32, device=DEV)    # (contiguous by contract: guard rows only)
        sbuf[1:-1] = NAN
        kw.update(seg_stats=sbuf[1:-1], seg_eps=c["seg_eps"])
        res["seg"] = sbuf[1:-1]
    a_before = abuf.clone()
    ops.dit_rowchain(a, dev(inp["w1"]), dev(inp["gamma1"]), x, gate=gate, gamma2=dev(inp["gamma2"]), mod_scale2=ms2, mod_div=c["mod_div"], eps=c["eps"], **kw)
    torch.cuda.synchronize()
    res["X"] = x
    for buf, r, cc, pad, what in frames:
        _guard_ok(buf, r, cc, pad, f"{c['name']} {what}")
    if c["seg"]:
        assert bool((sbuf[0] == SENTINEL).all()) and bool((sbuf[-1] == SENTINEL).all()), f"{c['name']}: seg_stats guard rows written"
    assert torch.equal(abuf.view(torch.int16), a_before.view(torch.int16)), "a_in was written"
    return res


def _rc_check(c, inp, res):
    ref = R.rowchain_ref(c, inp, x_dev=res["X"].cpu())
    assert set(ref) == set(res)
    for stage in ("X", "H", "C2", "seg"):          # X first: the later stages take the X the kernel wrote as their exact input
        if stage in ref:
            _check(c["name"], f"rowchain {c['inst']} {stage}", res[stage], *ref[stage])
    x = res["X"].cpu()
    assert torch.equal(x[R.ZERO_A], inp["x0"][R.ZERO_A]), "all-zero a_in row: X must be unchanged"
    assert not x[R.ZERO_AX].any(), "all-zero a_in and x0 row: X must stay 0"
    for stage in ("H", "C2"):
        if stage in res:
            assert not res[stage][R.ZERO_AX].any(), f"all-zero X row: {stage} must be exactly 0"


@pytest.mark.parametrize("c", R.ROWCHAIN, ids=lambda c: c["name"])
def test_rowchain(ops, c):
    """the four built instances at M 128 / 256 / 384, mod_div 128 (a modulation row per workgroup) and 384 (shared), every N2 class, seg_stats,
    each optional input given and absent; staged: X against the inputs, H / C2 / seg_stats against float64 from the X the kernel wrote."""
    inp = R.rowchain_inputs(c)
    _rc_check(c, inp, _rc_launch(ops, c, inp))


LOCALITY = [c for c in R.ROWCHAIN if c["name"] in ("rc-K384-noW2-M256-div128-h-nogate-nog2", "rc-K384-glu-M256-div128-N256-nogate",
                                                   "rc-K1024-noW2-M128-div128-h", "rc-K1024-plain-M256-div128-N384-seg")]


@pytest.mark.parametrize("c", LOCALITY, ids=lambda c: c["name"])
def test_rowchain_is_local_to_a_row(ops, c):
    """a second launch with one a_in row and one x0 row set to NaN differs from the first in exactly those rows of X, H, C2 and seg_stats; every
    other row is bit-equal."""
    inp = R.rowchain_inputs(c)
    first, second = _rc_launch(ops, c, inp), _rc_launch(ops, c, inp, nan_rows=R.LOCAL_ROWS)
    keep = torch.ones(c["M"], dtype=torch.bool, device=DEV)
    keep[list(R.LOCAL_ROWS)] = False
    for stage, t in first.items():
        u = second[stage]
        assert not torch.isnan(t).any()
        assert torch.equal(t[keep], u[keep]), f"{stage}: {(t[keep] != u[keep]).any(-1).sum().item()} other rows changed"
        for r in R.LOCAL_ROWS:
            assert bool(torch.isnan(u[r]).any()), f"{stage}: row {r} did not see its NaN input"


def test_rowchain_hands_its_statistics_to_attention(ops):
    """K1 = 1024, N2 = 1536 with seg_stats: c2 and the (mean, rstd) pairs feed dit_attention(stats=). (a) the device pairs against the float64
    statistics of the STORED bf16 rows (they come from the fp32 accumulators: the rounding of the 384 stored values is the difference); (b) the
    attention against attention_ref normalising with the device's pairs; (c) against attention_ref with the exact statistics of the stored rows,
    whose statistics term is the measured distance of the device pairs from them."""
    c, T, S = R.HANDOVER, R.HANDOVER_T, R.HANDOVER_S
    inp = R.rowchain_inputs(c)
    res = _rc_launch(ops, c, inp)
    _rc_check(c, inp, res)
    c2, st = res["C2"], res["seg"]
    seg = c2.cpu().to(torch.float64).view(c["M"], 4, R.D)
    mean, rstd, dmean, drstd = R.stats_bound(seg, R.U8 * (1.0 + R.U8) * seg.abs(), R.f32(c["seg_eps"]))
    _check(c["name"], "hand-over: device statistics vs stored rows", st, torch.stack([mean, rstd], -1), torch.stack([dmean, drstd], -1))
    ca = R.acase(T, 36, c["M"] // (T * S), S)
    ai = R.make_attn_inputs(ca)
    kv_cpu = ai["kv2"]
    cond = torch.full((kv_cpu.shape[0], 64, 2, R.HEADS, R.HD), NAN, dtype=BF16, device=DEV)
    cond[:, :36] = kv_cpu.to(DEV)
    kv2 = cond[:, :36]
    norms = [(g.to(DEV), b.to(DEV)) for g, b in ai["norms"]]
    st4 = st.contiguous()
    out = _attn_launch(ops, ca, c2, kv2, _v2t(ops, kv2), norms, ai["gate"].to(DEV), st4)
    args = (c2.cpu(), ai["norms"], kv_cpu, ai["gate"], T, S, ca["eps"], ca["scale"])
    _check(c["name"], "hand-over: attention, device statistics", out, *R.attention_ref(*args, stats=st4.cpu()))
    err = ((st4.cpu()[..., 0].double() - mean).abs(), (st4.cpu()[..., 1].double() - rstd).abs() / rstd)
    _check(c["name"], "hand-over: attention, exact statistics", out, *R.attention_ref(*args, stat_err=err))


# ------------------------------------------------------------------------------------------------------------ refusals
def _attn_refusal_args(T, Lz, heads, rows):
    d = heads * 64
    x = torch.zeros(rows, 4 * d, dtype=BF16, device=DEV)
    out = torch.full((rows, d), NAN, dtype=BF16, device=DEV)
    kv2 = torch.zeros(1, 65, 2, heads, 64, dtype=BF16, device=DEV)[:, :Lz]
    norms = [(torch.ones(d, device=DEV), torch.zeros(d, device=DEV)) for _ in range(3)]
    v2t = torch.zeros(1, heads, 64, 64, dtype=BF16, device=DEV)
    return x, out, norms, kv2, v2t


@pytest.mark.parametrize("T,Lz,heads", [(33, 16, 6), (16, 0, 6), (16, 65, 6), (16, 16, 4), (16, 16, 8)], ids=["T33", "Lz0", "Lz65", "heads4", "heads8"])
@pytest.mark.parametrize("with_stats", [False, True], ids=["own_stats", "stats_given"])
def test_attention_refusals(ops, T, Lz, heads, with_stats):
    from internnav_amd import _lib

    x, out, norms, kv2, v2t = _attn_refusal_args(T, Lz, heads, T)
    stats = torch.zeros(T, 4, 2, device=DEV) if with_stats else None
    with pytest.raises(_lib.EngineError, match="dit_attention"):
        ops.dit_attention(x, out, norms, kv2, v2t, None, T=T, seq_per_env=1, heads=heads, stats=stats)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_attention_refuses_T0(ops):
    """T = 0 cannot be expressed through ops.dit_attention (rows = nseq * T): the launcher itself, with the arguments of a valid T = 16 call."""
    from internnav_amd import _lib

    x, out, norms, kv2, v2t = _attn_refusal_args(16, 16, 6, 16)
    a = _lib.DitAttnArgs()
    a.X, a.O, a.K2, a.V2T = x.data_ptr(), out.data_ptr(), kv2[:, :, 0].data_ptr(), v2t.data_ptr()
    (a.g_q1, a.b_q1), (a.g_k1, a.b_k1), (a.g_q2, a.b_q2) = [(g.data_ptr(), b.data_ptr()) for g, b in norms]
    a.k2_bs, a.k2_rs, a.nseq, a.T, a.heads, a.seq_per_env, a.Lz, a.ldx, a.ldo = kv2.stride(0), kv2.stride(1), 1, 0, 6, 1, 16, x.stride(0), out.stride(0)
    a.scale, a.eps = 0.125, 1e-5
    with pytest.raises(_lib.EngineError, match="dit_attention"):
        _lib.check(_lib.lib().ina_dit_attention(C.byref(a), torch.cuda.current_stream().cuda_stream), "dit_attention")
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


RC_REFUSALS = {
    "seg_stats_N640": (R.rcase(1024, 128, 128, 640), dict(seg=True)),
    "mod_div64": (R.rcase(1024, 128, 128, 128), dict(mod_div=64)),
    "K384_plain": (R.rcase(384, 128, 128, 128, True), dict(glu=False)),
    "K1024_glu": (R.rcase(1024, 128, 128, 128), dict(glu=True)),
}


@pytest.mark.parametrize("name", list(RC_REFUSALS))
def test_rowchain_refusals(ops, name):
    """refused before any launch (by the library's argument checks, seg_stats at N2 = 640 already by the wrapper's): X and C2 stay as they were."""
    from internnav_amd import _lib

    c, over = RC_REFUSALS[name]
    M, K1, N2 = c["M"], c["K1"], c["N2"]
    glu = over.get("glu", c["glu"])
    a, w1 = torch.zeros(M, K1, dtype=BF16, device=DEV), torch.zeros(R.D, K1, dtype=BF16, device=DEV)
    x = torch.full((M, R.D), 3.0, device=DEV)
    c2 = torch.full((M, N2 // 2 if glu else N2), NAN, dtype=BF16, device=DEV)
    kw = dict(w2=torch.zeros(N2, R.D, dtype=BF16, device=DEV), c2=c2, glu2=glu, mod_div=over.get("mod_div", c["mod_div"]))
    if over.get("seg"):
        kw["seg_stats"] = torch.full((M, max(N2 // R.D, 1), 2), NAN, device=DEV)
    with pytest.raises((_lib.EngineError, AssertionError)):
        ops.dit_rowchain(a, w1, torch.ones(R.D, device=DEV), x, **kw)
    torch.cuda.synchronize()
    assert bool((x == 3.0).all()) and torch.isnan(c2).all()
