"""CPU checks of tests/attn_bwd_ref.py (the float64 restatement of csrc/attention_bwd.hip that tests/test_attention_bwd_fp64_gpu.py compares the
kernel with): (a) it equals float64 torch autograd of the masked, dropped softmax attention, (b) a float32 / bf16 emulation of the kernel's
rounding points stays inside the derived bound on every case, (c) each deliberate mutation of the restatement leaves the bound on the case named
for it, i.e. the GPU suite would notice a kernel that is wrong in that way."""
import pytest
import torch

from tests import attn_bwd_ref as R

F64 = torch.float64
CASES = R.ALL + R.FWD_O + [R.LONG]
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def refs():
    """case name -> (inputs, o, reference), computed once and never modified."""
    cache = {}

    def get(c):
        if c["name"] not in cache:
            cache[c["name"]] = R.case_reference(c)
        return cache[c["name"]]
    return get


def _autograd(c, inp, o_for_delta):
    """float64 autograd, per query head, of  sum(dO * (P m) V): with o_for_delta None plain softmax autograd (delta = rowsum(dO * o) of the exact
    o); else the softmax normaliser is held constant and the term -delta * P added, which makes d/dS = P (m dP - delta) for the GIVEN delta."""
    B, Lq, Lk, H, Hkv, D = c["dims"]
    G, sc = H // Hkv, R.f32(c["scale"])
    bi, hi = torch.arange(B) // c["kv_bdiv"], torch.arange(H) // G
    q = inp["q"].to(F64).requires_grad_(True)
    kk = inp["k"].to(F64)[bi][:, :, hi].clone().requires_grad_(True)          # one leaf per (b, query head): gradients stay per query head
    vv = inp["v"].to(F64)[bi][:, :, hi].clone().requires_grad_(True)
    do = inp["do"].to(F64)
    len_k = torch.full((B,), Lk) if inp["k_len"] is None else inp["k_len"].long()[bi].clamp(max=Lk)
    ak, aq = torch.arange(Lk).view(1, 1, 1, Lk), torch.arange(Lq).view(1, 1, Lq, 1)
    allowed = (ak < len_k.view(B, 1, 1, 1)).expand(B, 1, Lq, Lk)
    if c["causal"]:
        allowed = allowed & (ak <= aq + (len_k - Lq).view(B, 1, 1, 1))
    rowok = allowed.any(-1, keepdim=True)
    s = torch.einsum("bqhd,bkhd->bhqk", q, kk) * sc
    s = torch.where(rowok, s.masked_fill(~allowed, float("-inf")), torch.zeros_like(s))
    m = 1.0
    if c["drop"] is not None:
        p, seed = c["drop"]
        m = R.drop_keep(B, H, Lq, Lk, p, seed).to(F64) * R.f32(1.0 / (1.0 - p))
    if o_for_delta is None:
        P = torch.softmax(s, -1) * rowok
        loss = (torch.einsum("bhqk,bkhd->bqhd", P * m, vv) * do).sum()
    else:
        P = torch.exp(s - torch.logsumexp(s, -1, keepdim=True).detach()) * rowok
        delta = (do * o_for_delta.to(F64)).sum(-1).permute(0, 2, 1)[..., None]
        loss = (torch.einsum("bhqk,bkhd->bqhd", P * m, vv) * do).sum() - (delta * P).sum()
    loss.backward()
    sel = lambda t: R.select_rows(t, len_k, c["kv_row0"], Lq)                  # noqa: E731
    return {"dq": q.grad, "dk": sel(kk.grad), "dv": sel(vv.grad)}


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_restatement_equals_float64_autograd(c, refs):
    inp, o, ref = refs(c)
    kw = R.ref_kwargs(c)
    kw["k_len"] = inp["k_len"]
    fwd = {n: kw[n] for n in ("scale", "causal", "k_len", "kv_bdiv", "drop")}
    o64 = R.forward_o64(inp["q"], inp["k"], inp["v"], **fwd)
    exact = R.reference(inp["q"], inp["k"], inp["v"], o64, inp["do"], bounds=False, **kw)
    for given, mine in ((o, ref), (None, exact)):
        auto = _autograd(c, inp, given)
        for n in ("dq", "dk", "dv"):
            a, b = auto[n], mine[n][0]
            assert a.shape == b.shape
            assert (a - b).abs().max().item() <= 1e-12 * max(b.abs().max().item(), 1e-300), (n, given is None)
    # the op's zero rows: keys at or past len_k
    B, Lq, Lk = c["dims"][:3]
    if inp["k_len"] is not None:
        for b in range(B):
            lk = min(int(inp["k_len"][b // c["kv_bdiv"]]), Lk)
            r0 = max(0, lk - (c["kv_row0"] if c["kv_row0"] >= 0 else max(0, lk - Lq)))
            assert not ref["dk"][0][b, r0:].any() and not ref["dv"][0][b, r0:].any()
            assert not ref["dk"][1][b, r0:].any() and not ref["dv"][1][b, r0:].any()      # bound 0 there: the GPU check is `== 0`


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_emulated_kernel_rounding_stays_inside_the_bound(c, refs):
    inp, o, ref = refs(c)
    kw = R.ref_kwargs(c)
    kw["k_len"] = inp["k_len"]
    emu = R.emulate(inp["q"], inp["k"], inp["v"], o, inp["do"], **kw)
    worst = {}
    for n in ("dq", "dk", "dv"):
        worst[n], ok = R.ratio(emu[n], *ref[n])
        assert ok, f"{c['name']} {n}: emulation at {worst[n]:.3f} x bound"
    print(f"{c['name']}: emulation worst |err|/bound " + " ".join(f"{n} {w:.3f}" for n, w in worst.items()))


def _by_name(part, pool=None):
    hits = [c for c in (pool or R.ALL) if part in c["name"]]
    assert len(hits) == 1, (part, [c["name"] for c in hits])
    return hits[0]


# mutation -> the case named for it
MUTANTS = [
    ("mask_long", "ragged_row0-3x20x70x2x2x64-klen70_37_0-scale0.3"),        # non-causal: key len_k (planted) becomes visible
    ("mask_short", "dense-2x33x65x2x2x64"),
    ("diag_plus", "causal-1x65x65x2x2x64-causal"),
    ("diag_minus", "causal-1x65x65x2x2x64-causal"),
    ("shift_Lk", "ragged_last-3x4x200x4x2x128-causal-klen200_131_64-row-1-llm"),
    ("no_scale", "dense-1x32x129x3x3x72"),
    ("delta_f64", "dropout-2x33x65x2x2x48-causal-p0.1-scale0.3"),
    ("dv_no_dropscale", "dropout-2x33x65x2x2x48-causal-p0.1-scale0.3"),
    ("drop_idx_lenk", "dropout-1x4x70x4x2x128-klen50-p0.25"),
    ("kv_head_mod", "causal-2x4x130x4x2x128-causal"),
    ("no_bdiv", "layout-4x8x40x2x2x64-bdiv2-scale0.3"),
]


def test_every_mutation_is_listed():
    assert {m for m, _ in MUTANTS} == set(R.MUTATIONS)


@pytest.mark.parametrize("mut,name", MUTANTS, ids=[m for m, _ in MUTANTS])
def test_mutation_leaves_the_bound(mut, name, refs):
    c = next(x for x in R.ALL if x["name"] == name)
    inp, o, ref = refs(c)
    kw = R.ref_kwargs(c)
    kw["k_len"] = inp["k_len"]
    bad = R.reference(inp["q"], inp["k"], inp["v"], o, inp["do"], mut=mut, bounds=False, **kw)
    worst = {n: R.ratio(bad[n][0], *ref[n])[0] for n in ("dq", "dk", "dv")}
    print(f"{mut} on {name}: |mutant - ref| / bound " + " ".join(f"{n} {w:.1f}" for n, w in worst.items()))
    assert max(worst.values()) > 1.0, worst
    if mut == "delta_f64":
        # shows only where a row's weight sits on one key and o is not representable: with dropout o = v / (1 - p) is rounded, and
        # dP m - delta, which cancels for the exact o, is left with the rounding of o. Rows: the last query of each sequence (planted key
        # len_k - 1) and the mid-tile query (planted diagonal), first head of each kv group - and query 0, which sees a single key. On rows
        # with spread weight the difference stays near 0.3 x bound (2^-9 of |dS| against 2^-8 of it).
        err = (bad["dq"][0] - ref["dq"][0]).abs() / ref["dq"][1].clamp_min(1e-300)
        rows = {int(r) for r in (err.amax(-1) > 1.0).nonzero()[:, 1]}
        Lq = c["dims"][1]
        print("delta_f64 rows over the bound:", sorted(rows))
        assert rows & {Lq - 1, R.mid_query(Lq)}
