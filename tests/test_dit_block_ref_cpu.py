"""CPU checks of tests/dit_block_ref.py (the float64 restatement of the NextDiT block kernels that tests/test_dit_block_fp64_gpu.py compares
dit_attention.hip and dit_rowchain.hip with): (a) attention_ref equals F.layer_norm + F.scaled_dot_product_attention in float64, rowchain_ref a
plain float64 composition of torch ops, v2t_ref an independently written inverse-permutation loop; (b) a float32 / bf16 emulation of the kernels'
rounding points stays inside the derived bounds on every case, with both places of the row chain's 1 / rms; (c) each deliberate mutation of the
restatement leaves the bound on the cases named for it, i.e. the GPU suite would notice a kernel that is wrong in that way.

Observed |mutant - ref| / bound on the named cases (the worst element; "nan": the mutant reads a NaN or has no key left, which never passes; the
attention figures are single digits because the attention bound is a worst-case sum over the 64 bf16 roundings of a logit, which the emulation
reaches to 0.20):
    T_long            attn-T15-Lz16 8.3, attn-T17-Lz32 (statistics handed over) 9.0, attn-T31-Lz33 8.3     (T = 32: no key slot 32 to add)
    T_short           attn-T16-Lz17 13.4, attn-T17-Lz32 (handed over) 14.0, attn-T32-Lz64 15.2, attn-T1-Lz1 nan
    Lz_long           attn-T16-Lz17 4.4, attn-T32-Lz48 (handed over) 3.9, attn-T2-Lz15 8.3, attn-T31-Lz63 (handed over) 5.2  (Lz = 64: no slot 64)
    Lz_short          attn-T2-Lz33 14.7, attn-T32-Lz49 (handed over) 11.4, attn-T16-Lz64 13.2, attn-T17-Lz1 nan
    env_mod           attn-T2-Lz33-e2xS32 12.8, attn-T16-Lz17-e2xS3 (handed over) 25.7                    (S = 1 or one env: the same map)
    gate_no_tanh      attn-T15-Lz33-sat 216, attn-T16-Lz17-rand (handed over) 7.4                         (gate None / 0: the same value)
    gate_self         attn-T31-Lz33-rand 20.5, attn-T2-Lz64-zero (handed over) 12.4
    ln_per_head       attn-T16-Lz63 7.1, attn-T2-Lz15 (handed over: the pairs are ignored) 4.7
    no_beta           attn-T17-Lz32 5.7, attn-T32-Lz15 (handed over) 7.0
    no_eps            attn-T15-Lz16 nan, attn-T32-Lz64 nan (the constant segment: 0 * inf); own statistics only, handed-over pairs carry their eps
    q2_slot2          attn-T16-Lz17 29.8 (own statistics of the v1 segment); handed over: nan on attn-T16-Lz17 and attn-T1-Lz64 (the v1 pair)
    no_scale          attn-T32-Lz48 56.0, attn-T1-Lz64 (handed over) 17.6
    vt_swap           attn-T31-Lz16 6.7, attn-T2-Lz15 (handed over) 4.8; v2t_ref itself: a bit difference at every Lz >= 2
    mod_row0          X of rc-K384-noW2-M384-div128-h-noms2 1.1e5, rc-K1024-plain-M256-div128-N384-seg 4.8e4 (the x0 rows of magnitude 1e-4 have tiny bounds)
    no_tanh           X of rc-K384-noW2-M128-div128-h 145, rc-K1024-plain-M128-div128-N128 124
    no_gamma2         H of rc-K384-noW2-M128-div128-h 91.6, C2 of rc-K1024-plain-M128-div128-N128 8.1
    ms2_no_one        H of rc-K1024-noW2-M128-div128-h 9.6e6, C2 of rc-K384-glu-M128-div128-N128 77.8
    rstd2_old_x       H of rc-K384-noW2-M128-div128-h 3.3e4, C2 of rc-K1024-plain-M384-div384-N640 8.0e3
    glu_swap          C2 of rc-K384-glu-M128-div128-N128 45.0, rc-K384-glu-M384-div384-N3072 74.4
    glu_no_interleave C2 of rc-K384-glu-M256-div128-N256-nogate 576, rc-K384-glu-M384-div384-N3072 1180
    var_unbiased      seg of rc-K1024-plain-M256-div128-N384-seg 2.4, rc-K1024-plain-M128-div128-N1536-seg-noms2 2.3 (rstd moves by 1 / 766 only:
                      this is why the seg_stats bound evaluates the operand rounding instead of bounding it, see dit_block_ref.py)
    seg_shift         seg of rc-K1024-plain-M384-div128-N768-seg-nogate: nan in slot 0 (its pre-fill)
Emulation worst |err| / bound: attention 0.200 (own statistics) / 0.212 (handed over); row chain X 0.913, H 0.990, C2 0.292, seg_stats 0.598 (X and H
are one bf16 rounding of a value: an element just above a power of two sits at the half-ulp 2^-8 that u8 is).
"""
import pytest
import torch

from tests import dit_block_ref as R

F64 = torch.float64
BY_NAME = {c["name"]: c for c in R.ATTN + R.ROWCHAIN}


def _attn_args(c, inp):
    return (inp["x"], inp["norms"], inp["kv2"], inp["gate"], c["T"], c["S"], c["eps"], c["scale"])


# ------------------------------------------------------------------------------------------------------------ (a) independent restatements
@pytest.mark.parametrize("c", R.ATTN, ids=lambda c: c["name"])
def test_attention_ref_equals_float64_layer_norm_and_sdpa(c):
    inp, _, ref, _ = R.attn_reference(c, False)
    T, S, nseq = c["T"], c["S"], c["envs"] * c["S"]
    fn = torch.nn.functional
    xs = inp["x"].to(F64).view(nseq, T, 4, R.D)
    ln = lambda slot, i: fn.layer_norm(xs[:, :, slot], (R.D,), inp["norms"][i][0].to(F64), inp["norms"][i][1].to(F64), R.f32(c["eps"]))   # noqa: E731
    hv = lambda t: t.reshape(nseq, -1, R.HEADS, R.HD).transpose(1, 2)                                                                   # noqa: E731
    o1 = fn.scaled_dot_product_attention(hv(ln(0, 0)), hv(ln(1, 1)), hv(xs[:, :, 2]), scale=R.f32(c["scale"]))
    kc = inp["kv2"][:, :, 0].to(F64).repeat_interleave(S, 0).transpose(1, 2)
    vc = inp["kv2"][:, :, 1].to(F64).repeat_interleave(S, 0).transpose(1, 2)
    o2 = fn.scaled_dot_product_attention(hv(ln(3, 2)), kc, vc, scale=R.f32(c["scale"]))
    if inp["gate"] is not None:
        o2 = o2 * torch.tanh(inp["gate"].to(F64)).view(1, R.HEADS, 1, 1)
    want = (o1 + o2).transpose(1, 2).reshape(nseq * T, R.D)
    assert (want - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    # the statistics the reference hands over are the float64 ones rounded to fp32: the same result to fp32 accuracy, the v1 pair NaN
    _, st, ref_s, _ = R.attn_reference(c, True)
    assert torch.isnan(st[:, 2]).all() and not torch.isnan(st[:, [0, 1, 3]]).any()
    assert (ref_s - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


@pytest.mark.parametrize("c", R.ROWCHAIN, ids=lambda c: c["name"])
def test_rowchain_ref_equals_plain_float64_composition(c):
    inp = R.rowchain_inputs(c)
    M, dv = c["M"], c["mod_div"]
    out = R.rowchain_ref(c, inp)
    rms = lambda t: t / (t.pow(2).mean(-1, keepdim=True) + R.f32(c["eps"])).sqrt()             # noqa: E731
    per_row = lambda t: torch.repeat_interleave(t.to(F64), dv, 0)[:M]                            # noqa: E731
    p = inp["a_in"].to(F64) @ inp["w1"].to(F64).t()
    x = rms(p) * inp["gamma1"].to(F64)
    if inp["gate"] is not None:
        x = x * torch.tanh(per_row(inp["gate"]))
    x = inp["x0"].to(F64) + x
    close = lambda a, b: (a - b).abs().max().item() <= 1e-12 * max(b.abs().max().item(), 1e-300)    # noqa: E731
    assert close(out["X"][0], x)
    assert torch.equal(out["X"][0][R.ZERO_A], inp["x0"][R.ZERO_A].to(F64)) and not out["X"][1][R.ZERO_A].any()
    if "H" not in out and "C2" not in out:
        return
    h = rms(x.to(torch.float32).to(F64))
    if inp["gamma2"] is not None:
        h = h * inp["gamma2"].to(F64)
    if inp["ms2"] is not None:
        h = h * (1.0 + per_row(inp["ms2"]))
    if "H" in out:
        assert close(out["H"][0], h) and not out["H"][0][R.ZERO_AX].any() and not out["H"][1][R.ZERO_AX].any()
        return
    y = h @ inp["w2"].to(F64).t()
    if c["glu"]:                                  # output column n = 16 q + i pairs W2 rows 32 q + i (gate) and 32 q + 16 + i (up)
        n = torch.arange(c["N2"] // 2)
        y = torch.nn.functional.silu(y[:, 32 * (n // 16) + n % 16]) * y[:, 32 * (n // 16) + 16 + n % 16]
    assert close(out["C2"][0], y) and not out["C2"][0][R.ZERO_AX].any() and not out["C2"][1][R.ZERO_AX].any()
    if c["seg"]:
        seg = y.view(M, -1, R.D)
        want = torch.stack([seg.mean(-1), (seg.var(-1, unbiased=False) + R.f32(c["seg_eps"])).rsqrt()], -1)
        assert (out["seg"][0] - want).abs().max().item() <= 1e-9 * want.abs().max().item()


@pytest.mark.parametrize("Lz", R.V2T_LZ)
def test_v2t_ref_equals_inverse_permutation_loop(Lz):
    """the kernel's direction: every slot looks up its key (slot -> key), written out as a loop; v2t_ref scatters key -> slot."""
    kv2 = torch.randn(3, Lz, 2, R.HEADS, R.HD, generator=torch.Generator().manual_seed(Lz)).to(torch.bfloat16)
    want = torch.zeros(3, R.HEADS, R.HD, 64, dtype=torch.bfloat16)
    seen = set()
    for slot in range(64):
        sub, w = slot // 32, slot % 32
        gg, j = w // 8, w % 8
        key = sub * 32 + (gg * 4 + j if j < 4 else 16 + gg * 4 + (j - 4))
        seen.add(key)
        if key < Lz:
            want[:, :, :, slot] = kv2[:, key, 1]
    assert seen == set(range(64))
    assert torch.equal(R.v2t_ref(kv2), want)
    if Lz >= 2:
        assert not torch.equal(R.v2t_ref(kv2, mut="vt_swap"), want)


# ------------------------------------------------------------------------------------------------------------ (b) emulation inside the bounds
def test_attention_emulation_stays_inside_the_bound():
    worst = {False: 0.0, True: 0.0}
    for c in R.ATTN:
        for with_stats in (False, True):
            inp, st, ref, bound = R.attn_reference(c, with_stats)
            assert not torch.isnan(ref).any() and bool((bound > 0).all()), c["name"]
            w, ok = R.ratio(R.attention_emulate(*_attn_args(c, inp), stats=st), ref, bound)
            assert ok, f"{c['name']} (stats handed over: {with_stats}): emulation at {w:.3f} x bound"
            worst[with_stats] = max(worst[with_stats], w)
    print(f"attention: emulation worst |err| / bound {worst[False]:.3f} (own statistics), {worst[True]:.3f} (handed over)")
    assert min(worst.values()) > 0.1, "the bound is far from what the rounding points produce"


def test_rowchain_emulation_stays_inside_the_bound_in_both_orders():
    worst = {}
    for c in R.ROWCHAIN + [R.HANDOVER]:
        inp = R.rowchain_inputs(c)
        for order in ("after", "before"):
            emu = R.rowchain_emulate(c, inp, order)
            ref = R.rowchain_ref(c, inp, x_dev=emu["X"])
            for stage, (r, b) in ref.items():
                assert not torch.isnan(r).any() and not torch.isnan(b).any(), (c["name"], stage)
                w, ok = R.ratio(emu[stage], r, b)
                assert ok, f"{c['name']} {stage} (1 / rms {order} the GEMM): emulation at {w:.3f} x bound"
                worst[stage] = max(worst.get(stage, 0.0), w)
    print("row chain: emulation worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert min(worst.values()) > 0.1, "a bound is far from what the rounding points produce"


def test_planted_rows_are_what_they_claim():
    for c in R.ATTN:
        inp = R.attn_reference(c, False)[0]
        seg = inp["x"].to(F64).view(-1, c["T"], 4, R.D)
        assert float(seg[0, 0, 3].var()) == 0.0
        k1 = seg[0, 0, 1]
        assert 30.0 < float((k1 ** 2).mean() / k1.var(unbiased=False)) < 130.0
        # the planted last keys carry a moderate weight for query T // 2: doubling them or dropping them both move the result
        T, S, Lz, nseq = c["T"], c["S"], c["Lz"], c["envs"] * c["S"]
        ln = lambda slot, i: torch.nn.functional.layer_norm(seg[:, :, slot], (R.D,), inp["norms"][i][0].to(F64), inp["norms"][i][1].to(F64),   # noqa: E731
                                                            1e-5).view(nseq, T, R.HEADS, R.HD)
        p1 = torch.softmax(torch.einsum("nqhd,nkhd->nhqk", ln(0, 0), ln(1, 1)) * c["scale"], -1)[:, :, T // 2, T - 1]
        k2 = inp["kv2"][:, :, 0].to(F64)[torch.arange(nseq) // S]
        p2 = torch.softmax(torch.einsum("nqhd,nkhd->nhqk", ln(3, 2), k2) * c["scale"], -1)[::S, :, T // 2, Lz - 1]
        assert T == 1 or bool(((p1 > 0.1) & (p1 < 0.9)).any()), (c["name"], p1)
        assert Lz == 1 or bool(((p2 > 0.3) & (p2 < 0.9)).all()), (c["name"], p2)


# ------------------------------------------------------------------------------------------------------------ (c) mutations
A = "attn-T{}-Lz{}-e{}xS{}-{}".format
ATTN_MUTANTS = {       # mutation -> [(case, statistics handed over)]
    "T_long": [(A(15, 16, 2, 3, "rand"), False), (A(17, 32, 2, 3, "rand"), True), (A(31, 33, 2, 3, "rand"), False)],
    "T_short": [(A(16, 17, 2, 3, "rand"), False), (A(17, 32, 2, 3, "rand"), True), (A(32, 64, 2, 32, "rand"), False), (A(1, 1, 1, 1, "rand"), True)],
    "Lz_long": [(A(16, 17, 2, 3, "rand"), False), (A(32, 48, 2, 3, "rand"), True), (A(2, 15, 2, 3, "rand"), False), (A(31, 63, 3, 1, "rand"), True)],
    "Lz_short": [(A(2, 33, 2, 32, "rand"), False), (A(32, 49, 1, 1, "rand"), True), (A(16, 64, 3, 1, "rand"), False), (A(17, 1, 3, 1, "rand"), True)],
    "env_mod": [(A(2, 33, 2, 32, "rand"), False), (A(16, 17, 2, 3, "rand"), True)],
    "gate_no_tanh": [(A(15, 33, 1, 1, "sat"), False), (A(16, 17, 2, 3, "rand"), True)],
    "gate_self": [(A(31, 33, 2, 3, "rand"), False), (A(2, 64, 3, 1, "zero"), True)],
    "ln_per_head": [(A(16, 63, 2, 3, "rand"), False), (A(2, 15, 2, 3, "rand"), True)],
    "no_beta": [(A(17, 32, 2, 3, "rand"), False), (A(32, 15, 2, 3, "rand"), True)],
    "no_eps": [(A(15, 16, 2, 3, "rand"), False), (A(32, 64, 2, 32, "rand"), False)],
    "q2_slot2": [(A(16, 17, 2, 3, "rand"), False), (A(16, 17, 2, 3, "rand"), True), (A(1, 64, 2, 3, "rand"), True)],
    "no_scale": [(A(32, 48, 2, 3, "rand"), False), (A(1, 64, 2, 3, "rand"), True)],
    "vt_swap": [(A(31, 16, 1, 1, "rand"), False), (A(2, 15, 2, 3, "rand"), True)],
}
RC_MUTANTS = {         # mutation -> [(case, stage)]
    "mod_row0": [("rc-K384-noW2-M384-div128-h-noms2", "X"), ("rc-K1024-plain-M256-div128-N384-seg", "X")],
    "no_tanh": [("rc-K384-noW2-M128-div128-h", "X"), ("rc-K1024-plain-M128-div128-N128", "X")],
    "no_gamma2": [("rc-K384-noW2-M128-div128-h", "H"), ("rc-K1024-plain-M128-div128-N128", "C2")],
    "ms2_no_one": [("rc-K1024-noW2-M128-div128-h", "H"), ("rc-K384-glu-M128-div128-N128", "C2")],
    "rstd2_old_x": [("rc-K384-noW2-M128-div128-h", "H"), ("rc-K1024-plain-M384-div384-N640", "C2")],
    "glu_swap": [("rc-K384-glu-M128-div128-N128", "C2"), ("rc-K384-glu-M384-div384-N3072", "C2")],
    "glu_no_interleave": [("rc-K384-glu-M256-div128-N256-nogate", "C2"), ("rc-K384-glu-M384-div384-N3072", "C2")],
    "var_unbiased": [("rc-K1024-plain-M256-div128-N384-seg", "seg"), ("rc-K1024-plain-M128-div128-N1536-seg-noms2", "seg")],
    "seg_shift": [("rc-K1024-plain-M384-div128-N768-seg-nogate", "seg")],
}


def test_every_mutation_is_listed():
    assert set(ATTN_MUTANTS) == set(R.ATTN_MUTATIONS) and set(RC_MUTANTS) == set(R.RC_MUTATIONS)
    assert set(R.MUTATIONS) == set(ATTN_MUTANTS) | set(RC_MUTANTS)


@pytest.mark.parametrize("mut", list(ATTN_MUTANTS))
def test_attention_mutation_leaves_the_bound(mut):
    for name, with_stats in ATTN_MUTANTS[mut]:
        c = BY_NAME[name]
        inp, st, ref, bound = R.attn_reference(c, with_stats)
        bad, _ = R.attention_ref(*_attn_args(c, inp), stats=st, mut=mut, bounds=False)
        w, ok = R.ratio(bad, ref, bound)
        print(f"{mut} on {name} (stats handed over: {with_stats}): |mutant - ref| / bound {w:.1f}")
        assert not ok and (w > 1.0 or bool(torch.isnan(bad).any())), (mut, name, w)


@pytest.mark.parametrize("mut", list(RC_MUTANTS))
def test_rowchain_mutation_leaves_the_bound(mut):
    for name, stage in RC_MUTANTS[mut]:
        c = BY_NAME[name]
        inp = R.rowchain_inputs(c)
        x = R.rowchain_emulate(c, inp)["X"]
        r, b = R.rowchain_ref(c, inp, x_dev=x)[stage]
        bad = R.rowchain_ref(c, inp, x_dev=x, mut=mut)[stage][0]
        w, ok = R.ratio(bad, r, b)
        print(f"{mut} on {name} {stage}: |mutant - ref| / bound {w:.1f}")
        assert not ok and (w > 1.0 or bool(torch.isnan(bad).any())), (mut, name, stage, w)
