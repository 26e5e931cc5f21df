"""CPU checks of tests/attn_decode_ref.py (the float64 restatement, bound and chunk-walk emulation that tests/test_attention_decode_fp64_gpu.py
holds ops.attention_prefix, ops.attention_prefix_tail and ops.attention_shared to): (a) the restatement agrees with the three older references on
their own cases and with float64 SDPA on the concatenated keys, (b) the reference is finite on every poisoned case, NaN only where the contract
says so, (c) the emulated chunk walk stays inside the bound on every case, (d) the bound is the stricter check on the older suites' cases,
(e) each single mutation of the restatement or of the emulation leaves the bound on the cases named for it, for two seeds, (f) the ramp cases
really make the maxima rise inside a wave and differ across the waves."""
import numpy as np
import pytest
import torch

import attn_prefix_ref as OP
import attn_prefix_tail_ref as OT
import attn_shared_ref as OS
from tests import attn_decode_ref as R

F64 = torch.float64
IDS = [c["name"] for c in R.ALL]


def _np(t):
    return t.double().numpy()


def _old(kind, i):
    """(problems, output shape, the older module's float64 reference, its tolerance) of case i of an older suite"""
    if kind == "prefix":
        c = OP.make_case(OP.CASES[i])
        v = OP.views(c["fused"], c["cache"], c["H"], c["Hkv"], c["m"])
        probs, nan = R.pair_problems(*v, c["slot"].tolist(), c["pfx_len"].tolist(), c["suf_len"].tolist())
        return probs, tuple(v[0].shape), OP.reference_of(c)
    if kind == "prefix_tail":
        c = OT.make_case(OT.CASES[i])
        v = OT.views(c["fused"], c["cache"], c["tails"], c["H"], c["Hkv"], c["m"])
        probs, nan = R.pair_problems(*v[:5], c["slot"].tolist(), c["pfx_len"].tolist(), c["suf_len"].tolist(), v[5], v[6], c["tail_row"].tolist(),
                                     c["tail_len"].tolist())
        return probs, tuple(v[0].shape), OT.reference_of(c)
    c = OS.make_case(OS.CASES[i])
    v = OS.views(c["fused"], c["tail"], c["cache"], c["H"], c["Hkv"])
    probs, nan, written = R.shared_problems(*v, c["tile_rows"].tolist(), c["tile_slot"].tolist(), c["tile_pfx"].tolist(), c["tail_len"].tolist())
    assert not bool(written[c["R"]]) and bool(written[:c["R"]].all())
    want = OS.reference_of(c)
    want[c["R"]] = 0.0                     # the older reference keeps its fill value in the row no tile names
    return probs, tuple(v[0].shape), want


OLD = [("prefix", i) for i in range(len(OP.CASES))] + [("prefix_tail", i) for i in range(len(OT.CASES))] + [("shared", i) for i in range(len(OS.CASES))]


@pytest.mark.parametrize("kind,i", OLD, ids=[f"{k}-{i}" for k, i in OLD])
def test_restatement_equals_the_older_references_and_the_bound_is_stricter(kind, i):
    probs, shape, want = _old(kind, i)
    ref, bound = R._scatter(probs, shape, lambda pr: R.attend(pr, R.D ** -0.5), F64)
    assert np.isfinite(want).all()
    assert float(np.abs(ref.numpy() - want).max()) <= 1e-12 * float(np.abs(want).max())
    live = bound.numpy() > 0
    rel = float((bound.numpy()[live] / OP.tolerance(want)[live]).max())
    print(f"{kind} case {i}: max(bound / (1.5e-2 + |ref| / 128)) = {rel:.3f}")
    assert rel < 1.0, "the derived bound is wider than the blanket tolerance somewhere"


def _sdpa(prob, scale):
    n = prob["Q"].shape[0]
    K, V = (torch.cat([s[j].to(F64) for s in prob["segs"]], 0) for j in (0, 1))
    mask = torch.cat([torch.ones(n, s[0].shape[0], dtype=torch.bool) if s[2] is None else s[2] for s in prob["segs"]], 1)
    return torch.nn.functional.scaled_dot_product_attention(prob["Q"].to(F64)[None], K[None], V[None], attn_mask=mask[None], scale=R.f32(scale))[0]


@pytest.mark.parametrize("c", R.ALL, ids=IDS)
def test_reference_is_finite_and_equals_float64_sdpa(c):
    inp, ref, bound, nan, written = R.case_reference(c)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()), "poison reached the reference"
    assert bool((bound >= 0).all()) and bool((bound > 0).any())
    probs, _, _, shape = R.problems(c, inp)
    o = R._scatter(probs, shape, lambda pr: (_sdpa(pr, c["scale"]), None), F64)[0]
    assert float((o - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    # rows that must be exactly zero carry a zero bound: rows behind suf_len, rows without a tail, pairs with nothing to score
    if c["entry"] == "shared":
        zero = [r for r in range(inp["R"]) if bool(written[r]) and int(inp["tail_len"][r]) <= 0]
        assert all(not bool(bound[r].any()) and not bool(ref[r].any()) for r in zero)
        assert not bool(written[inp["R"]]) and bool(written[:inp["R"]].all()), "exactly the rows of the prompts are named"
        assert bool((bound[[r for r in range(inp["R"]) if r not in zero]] > 0).all())
    else:
        for p, n in enumerate(inp["suf_eff"]):
            assert not bool(bound[p, n:].any()) and not bool(ref[p, n:].any())
            assert bool(nan[p, :n].all()) or bool((bound[p, :n] > 0).all())
    assert c["scale"] == R.D ** -0.5 or inp["planted_max"] < 110.0


# what the case tables promise, so that an edit of them cannot silently drop an edge
def test_case_tables_reach_their_edges():
    pfx = {R._clamp(c["pfx_of"][s], 1 << 30) for c in R.PREFIX for s, _, _, _ in c["pairs"]}
    assert {0, 1, 63, 64, 65, 256, 257, 769, 832} <= pfx
    assert {c["m"] for c in R.PREFIX} == {1, 3, 16, 17, 64} and {(c["H"], c["Hkv"]) for c in R.PREFIX} == {(28, 4), (4, 4), (16, 2)}
    assert all({0, 1, c["m"]} & {n for _, _, _, n in c["pairs"]} for c in R.PREFIX)
    combos = {(c["pfx_of"][s] % 64, max(tl, 0)) for c in R.PREFIX_TAIL[:2] for s, _, tl, _ in c["pairs"]}
    assert {(a, b) for a in (0, 1, 63) for b in (0, 1, 63, 64, 65, 130)} <= combos
    assert any(c["pfx_of"][s] == 769 and tl == 65 for c in R.PREFIX_TAIL for s, _, tl, _ in c["pairs"])
    assert any([tr for _, tr, tl, _ in c["pairs"] if tl > 0] != sorted(tr for _, tr, tl, _ in c["pairs"] if tl > 0) for c in R.PREFIX_TAIL)
    assert {(c["H"], c["Hkv"]) for c in R.SHARED} >= {(28, 4), (8, 2), (16, 1), (2, 2)}
    assert {p for c in R.SHARED for _, p, _ in c["prompts"]} >= {0, 1, 63, 64, 65, 769}
    assert {n for c in R.SHARED for _, _, tl in c["prompts"] for n in tl} >= {1, 2, 63, 64, 65, 128, 130, 200, -1}
    inp = R.case_reference(R.BY_NAME["shared-bad-places"])[0]
    assert {inp["R"] + 1, 1 << 20} <= set(inp["tile_rows"].flatten().tolist()) and -1 in inp["tile_rows"].flatten().tolist()
    for g in R.GROUPS.values():
        assert any(c["scale"] == R.ALT_SCALE for c in g) and any(c["ramp"] for c in g)


@pytest.mark.parametrize("entry", list(R.GROUPS))
def test_emulated_chunk_walk_stays_inside_the_bound(entry):
    worst = 0.0
    for c in R.GROUPS[entry]:
        for seed in (0, 1):
            inp, ref, bound, nan, written = R.case_reference(c, seed)
            keep = ~nan                                   # the emulation leaves zeros in NaN rows: they are compared on the device only
            w, ok = R.ratio(R.emulate(c, inp)[keep], ref[keep], bound[keep])
            assert ok and w < 1.0, f"{c['name']} (seed {seed}): emulation at {w:.3f} x bound"
            worst = max(worst, w)
    print(f"{entry}: emulation worst |err| / bound {worst:.3f}")
    assert worst > 0.1, "the bound is far from what the rounding points produce"


# mutation -> the cases named for it
MUTANTS = {
    "pfx_minus": ["prefix-m17", "prefix-m1", "prefix_tail-long", "shared-H2", "shared-H8"],      # pfx 769 (m17, long, H2) and pfx 1 (m1, H8)
    "pfx_plus": ["prefix-m3", "prefix_tail-m5", "shared-H28"],
    "tail_minus": ["prefix_tail-m5", "prefix_tail-long", "shared-H8", "shared-H16"],
    "tail_plus": ["prefix_tail-m17", "shared-H28"],
    "diag_minus": ["prefix-m16", "prefix-m64", "prefix_tail-m17"],
    "diag_plus": ["prefix-m16", "prefix-m64-H28", "prefix_tail-m64"],
    "chunk_skip": ["prefix-m17", "prefix-m3", "prefix_tail-long", "shared-H2"],
    "stale_prefetch": ["prefix-m3", "prefix-m16", "prefix_tail-long", "shared-H28"],
    "tail_of_neighbour": ["shared-H28", "shared-H8", "shared-H2"],
    "kv_head_mod": ["prefix-m3", "prefix-m16", "prefix_tail-m5", "shared-H28", "shared-H8"],
    "scale_ignored": ["prefix-scale", "prefix_tail-scale", "shared-scale"],
    "no_rescale": ["prefix-ramp", "prefix_tail-ramp", "shared-ramp"],
    "combine_unweighted": ["prefix-ramp", "prefix_tail-ramp", "shared-ramp"],
    "clamp_missing": ["prefix-clamps", "shared-clamps"],
}


def test_every_mutation_is_listed():
    assert set(MUTANTS) == set(R.MUTATIONS)
    assert all(name in R.BY_NAME for names in MUTANTS.values() for name in names)


@pytest.mark.parametrize("mut", list(MUTANTS))
def test_mutation_leaves_the_bound(mut):
    for name in MUTANTS[mut]:
        c = R.BY_NAME[name]
        for seed in (0, 1):
            inp, ref, bound, nan, written = R.case_reference(c, seed)
            bad = R.emulate(c, inp, mut=mut).to(F64) if mut in R.EMULATION_MUTATIONS else R.reference(c, inp, mut=mut, bounds=False)[0]
            keep = ~nan
            w, ok = R.ratio(bad[keep], ref[keep], bound[keep])
            what = f"{w:.1f}" if w == w and w != float("inf") else "NaN in a live row"
            print(f"{mut} on {name} (seed {seed}): |mutant - ref| / bound {what}" + ("" if w > 1.0 else " (differs where the bound is 0)"))
            assert not ok, (mut, name, seed, w)


@pytest.mark.parametrize("c", [c for c in R.ALL if c["ramp"]], ids=lambda c: c["name"])
def test_ramp_cases_carry_the_rescale_and_the_combine_weights(c):
    """the emulated chunk maxima of the ramp row: inside one wave they rise by >= 4 and then by >= 10, and the four waves' final maxima lie
    8 - 20 below the row's (so neither a missing rescale nor a missing combine weight can hide)."""
    inp = R.case_reference(c)[0]
    probs, _, _, _ = R.problems(c, inp)
    G = c["H"] // c["Hkv"]
    if c["entry"] == "shared":
        r, _ = c["ramp"]
        prob = next(p for p in probs if p["dst"][0][0] == (r, G))
        row = 0
    else:
        p_, i, _ = c["ramp"]
        prob = next(p for p in probs if p["dst"][0][0][0] == p_ and p["dst"][0][0][2] == G)
        row = i
    trace = []
    R.walk(prob, c["scale"], trace=trace)
    per_wave = [[float(mx[row]) for mx in seen] for seen in trace]
    print(f"{c['name']}: chunk maxima per wave (exp2 domain): " + " | ".join(" ".join(f"{x:.1f}" for x in w) for w in per_wave))
    steps = [[b - max(w[:j + 1]) for j, b in enumerate(w[1:])] for w in per_wave]
    assert any(any(3.5 <= s[j] <= 4.5 and s[j + 1] >= 9.5 for j in range(len(s) - 1)) for s in steps), steps
    finals = sorted(max(w) for w in per_wave)
    gaps = [finals[-1] - f for f in finals[:-1]]
    assert all(7.5 <= g <= 20.5 for g in gaps), finals
