"""CPU checks of tests/attn_fwd_ref.py (the float64 restatement of ina_attention_bf16 that tests/test_attention_fwd_fp64_gpu.py compares the six
forward kernels with): (a) without dropout it equals torch's scaled_dot_product_attention in float64 with the equivalent boolean mask, and
attn_bwd_ref.forward_o64 where both can express the case, (b) a float32 / bf16 emulation of the kernels' rounding points stays inside the derived
bound on every case, (c) each deliberate mutation of the restatement leaves the bound on the cases named for it, i.e. the GPU suite would notice
a kernel that is wrong in that way, (d) no case is vacuous: zero bounds where an edge promises them, and the ramp cases really make the deferred
running maximum skip one rescale and take another."""
import pytest
import torch

from tests import attn_bwd_ref as RB
from tests import attn_fwd_ref as R

F64 = torch.float64
IDS = [c["name"] for c in R.ALL]


def _defer(c):
    return R.DEFER_THR if c["group"] in ("wide", "window") else None


@pytest.mark.parametrize("c", R.ALL, ids=IDS)
def test_restatement_equals_float64_sdpa(c):
    """rows with at least one allowed key against SDPA (gate and base applied outside it); rows without one are exactly 0 / the base."""
    B, Lq, Lk, H, Hkv, D = c["dims"]
    inp, _, _ = R.case_reference(c)
    plain = dict(c, drop=None)
    ref, _ = R.reference(plain, inp, bounds=False)
    q, k, v, len_q, len_k = R.dense_inputs(c, inp)
    bi, hi, lk, allowed = R._setup(c, len_q, len_k, None)
    o = torch.nn.functional.scaled_dot_product_attention(q.to(F64).permute(0, 2, 1, 3), k.to(F64)[bi][:, :, hi].permute(0, 2, 1, 3),
                                                         v.to(F64)[bi][:, :, hi].permute(0, 2, 1, 3), attn_mask=allowed.expand(B, H, Lq, Lk),
                                                         scale=RB.f32(c["scale"])).permute(0, 2, 1, 3)
    if inp["gate"] is not None:
        o = o * torch.tanh(inp["gate"].to(F64)).view(1, 1, H, 1)
    base = torch.zeros_like(ref) if inp["base"] is None else inp["base"].to(F64)
    has_key = allowed.any(-1).permute(0, 2, 1)[..., None].expand(B, Lq, H, D)          # [B, Lq, 1 -> H, D]
    if bool(has_key.any()):
        assert (o + base - ref)[has_key].abs().max().item() <= 1e-12 * max(ref.abs().max().item(), 1e-300)
    else:
        assert c["kv_start"] >= Lk, "only kv_start = Lk leaves a case without a single key"
    assert torch.equal(ref[~has_key], base[~has_key])


@pytest.mark.parametrize("c", [c for c in R.ALL if c["lens_q"] is None and not c["kv_start"] and not c["gate"] and not c["acc"] and not c["rope"]],
                         ids=lambda c: c["name"])
def test_restatement_equals_backward_suites_forward(c):
    inp, ref, _ = R.case_reference(c)
    o = RB.forward_o64(inp["q"], inp["k"], inp["v"], scale=c["scale"], causal=c["causal"], k_len=inp["k_len"], kv_bdiv=c["kv_bdiv"], drop=c["drop"])
    assert (o - ref).abs().max().item() <= 1e-12 * max(ref.abs().max().item(), 1e-300)


@pytest.mark.parametrize("group", list(R.GROUPS))
def test_emulated_kernel_rounding_stays_inside_the_bound(group):
    worst = 0.0
    for c in R.GROUPS[group]:
        for salt in ((0, R.SALT) if c["drop"] else (0,)):
            inp, ref, bound = R.case_reference(c, salt)
            for defer in {None, _defer(c)}:          # the exact running maximum and, for the 32-row kernel's cases, the deferred one
                w, ok = R.ratio(R.emulate(c, inp, defer=defer, salt=salt), ref, bound)
                assert ok, f"{c['name']} (defer {defer}, salt {salt}): emulation at {w:.3f} x bound"
                worst = max(worst, w)
    print(f"{group}: emulation worst |err| / bound {worst:.3f}")
    assert worst > 0.1, "the bound is far from what the rounding points produce"


# mutation -> the cases named for it (one per kernel group that can express it)
MUTANTS = {
    "klen_plus": ["row16-3x20x65x2x2x64-klen65_37_0", "dropout-2x17x129x2x2x48-klen129_50-p0.25", "decode-7x2x320x4x2x128-klen320_300_64_9_2_1_0",
                  "wide-4x128x193x2x2x128-klen193_131_40_0"],
    "klen_minus": ["row16-1x33x49x2x2x48", "dropout-1x40x40x2x1x64-causal-p0.1", "decode-1x1x320x17x1x128-causal", "decode-1x4x1025x7x1x80-causal",
                   "wide-1x129x128x2x1x80", "window-5x64x64x2x2x80-q64_1_33_64_16-k64_1_33_64_16"],
    "diag_plus": ["row16-1x65x65x2x1x128-causal", "dropout-2x33x65x2x2x48-causal-p0.1-scale0.3", "decode-1x8x1024x12x2x128-causal",
                  "wide-1x129x128x2x2x128-causal", "wide-1x257x257x2x2x64-causal-strided"],
    "diag_minus": ["row16-1x65x33x2x2x48-causal-scale0.3", "dropout-2x33x65x2x2x48-causal-p0.1-scale0.3", "decode-1x2x257x8x1x128-causal",
                   "wide-1x128x321x2x1x128-causal"],
    "shift_Lk": ["row16-3x20x65x2x2x64-causal-klen65_37_0", "decode-7x2x320x4x2x128-causal-klen320_300_64_9_2_1_0",
                 "decode-3x4x320x14x2x128-causal-klen320_131_4-rope", "wide-4x128x193x2x1x80-causal-klen193_131_40_0"],
    "kvstart_plus": ["row16-1x17x129x2x2x64-start5", "row16-1x17x129x2x2x64-start64-scale0.3", "row16-1x17x129x2x2x64-start128",
                     "wide-1x160x193x2x2x80-start64", "wide-1x160x193x2x2x64-causal-start70"],
    "kvstart_minus": ["row16-1x17x129x2x2x64-start70", "row16-1x33x48x2x2x64-start32", "row16-1x17x129x2x2x64-start129", "wide-1x160x193x2x2x64-start5",
                      "wide-1x160x193x2x2x128-start70"],
    "kv_head_mod": ["row16-1x16x65x4x2x80", "decode-2x1x320x28x4x128", "decode-1x8x320x12x2x64", "wide-4x129x128x4x2x64-klen128_40-bdiv2"],
    "no_bdiv": ["row16-4x17x65x4x2x64-klen65_37-bdiv2", "wide-4x129x128x4x2x64-klen128_40-bdiv2"],
    "gate_no_tanh": ["row16-2x33x65x2x2x48-gate-acc", "row16-1x40x33x2x2x64-causal-gate-acc"],
    "drop_idx_lenk": ["dropout-2x17x48x2x2x64-klen40_23-p0.25", "dropout-2x17x129x2x2x48-klen129_50-p0.25"],
    "drop_before_sum": ["dropout-2x33x65x2x2x48-causal-p0.1-scale0.3", "dropout-1x40x40x2x1x64-causal-p0.1"],
    "cu_k_neighbour": ["row16-5x33x65x2x2x80-q17_0_1_33_4-k40_7_1_65_0", "wide-5x300x300x2x2x80-q300_128_1_0_131-k300_128_1_0_131",
                       "window-5x64x64x2x2x80-q64_1_33_64_16-k64_1_33_64_16"],
}


def test_every_mutation_is_listed():
    assert set(MUTANTS) == set(R.MUTATIONS)


@pytest.mark.parametrize("mut", list(MUTANTS))
def test_mutation_leaves_the_bound(mut):
    by_name = {c["name"]: c for c in R.ALL}
    for name in MUTANTS[mut]:
        c = by_name[name]
        inp, ref, bound = R.case_reference(c)
        bad, _ = R.reference(c, inp, mut=mut, bounds=False)
        w, ok = R.ratio(bad, ref, bound)
        print(f"{mut} on {name}: |mutant - ref| / bound {w:.1f}" + ("" if w > 1.0 else " (differs where the bound is 0)"))
        assert not ok, (mut, name, w)


@pytest.mark.parametrize("group", list(R.GROUPS))
def test_no_case_is_vacuous(group):
    for c in R.GROUPS[group]:
        inp, ref, bound = R.case_reference(c)
        assert bool((bound > 0).any()) or c["name"].endswith("-start129"), c["name"]            # kv_start = Lk: every row is empty, all bounds 0
        assert bool((bound == 0).any()) == ("zero" in c["edges"] or (c["lens_q"] is not None and min(c["lens_q"]) < c["dims"][1])), c["name"]
        assert not bool(torch.isnan(ref).any()) and not bool(torch.isnan(bound).any())
        if "zero" in c["edges"]:                 # real rows, not the padding of a packed case
            rows = torch.arange(c["dims"][1]).view(1, -1, 1, 1) < R.dense_inputs(c, inp)[3].view(-1, 1, 1, 1)
            assert bool(((bound == 0) & rows).any()), c["name"]
    assert any(bool((R.case_reference(c)[2] > 0).any()) for c in R.GROUPS[group])


@pytest.mark.parametrize("c", [c for c in R.ALL if c["ramp"]], ids=lambda c: c["name"])
def test_ramp_cases_skip_one_rescale_and_take_another(c):
    """on the emulated per-block maxima of the ramp query: a block whose maximum grows by less than 2^6 over the kept one (no rescale, P up to
    2^6), and blocks whose maximum grows by more (rescale)."""
    inp, _, _ = R.case_reference(c)
    trace = []
    R.emulate(c, inp, defer=R.DEFER_THR, trace=trace)
    qr = R.ramp_query(c)
    growth = [float(mx[0, 0, qr] - m[0, 0, qr]) for mx, m in trace[1:]]           # the first block starts from -inf
    print(f"{c['name']}: block maximum minus the kept maximum, per block: " + " ".join(f"{g:.2f}" for g in growth))
    assert any(0.5 < g <= R.DEFER_THR for g in growth), growth
    assert sum(g > R.DEFER_THR for g in growth) >= 2, growth
