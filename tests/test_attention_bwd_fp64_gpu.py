"""Attention backward (internnav_amd/csrc/attention_bwd.hip through train_ops.attention_bwd) against the float64 restatement of
tests/attn_bwd_ref.py at its mask, tile and split edges. The reference, the per-element bound (derived from the number formats, limit 1.0) and the
case table live in tests/attn_bwd_ref.py; tests/test_attn_bwd_ref_cpu.py checks them without a GPU (autograd equality, an emulation of the
kernel's rounding points, the ten mutations - the diagonal shifted both ways - that must leave the bound).

Every case hands the kernel an `o` computed by the reference (float64, rounded once to bf16), so a forward error cannot hide a backward one; one
more case per group takes `o` from ops.attention. dq / dk / dv are pre-filled with NaN: rows of keys at or past k_len must come back exactly 0
(their bound is 0), never left as they were. Inputs carry planted edges (attn_bwd_ref.make_inputs): a mask that is off by one key moves the
result by thousands of bounds.

Measured worst |err| / bound per group (MI355X, ROCm 7):
    dense        dq 0.654   dk 0.682   dv 0.701
    causal       dq 0.736   dk 0.912   dv 0.836
    ragged_last  dq 0.736   dk 0.867   dv 0.872
    ragged_row0  dq 0.700   dk 0.736   dv 0.765
    splits       dq 0.593   dk 0.912   dv 0.935
    dropout      dq 0.669   dk 0.855   dv 0.858
    layout       dq 0.669   dk 0.836   dv 0.918
(the float32 / bf16 emulation of tests/test_attn_bwd_ref_cpu.py gives the same figures to three digits: the two bf16 roundings dominate).
With the zero stores of the key pass taken out, exactly the ten cases with a dk / dv row at or past k_len fail (all of ragged_row0, the
k_len [40, 5] case of ragged_last, and the k_len cases of splits, dropout and layout whose k_len is below Lk); the other 36 pass.
"""
import pytest
import torch

from tests import attn_bwd_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
NAN = float("nan")


@pytest.fixture(scope="module")
def T(built_lib):
    from internnav_amd import train_ops

    return train_ops


def _ids(cases):
    return [c["name"] for c in cases]


def _views(c, inp):
    """device views of the inputs in the case's layout (base offsets and strides multiples of 8 elements) and NaN / sentinel-filled outputs.
    Returns (q, k, v, outs dict, guard) - guard() checks that nothing outside the output views was written."""
    B, Lq, Lk, H, Hkv, D = c["dims"]
    Bk = B // c["kv_bdiv"]
    rows = min(Lq, Lk) if c["kv_row0"] < 0 else Lk - c["kv_row0"]
    guard = lambda: None                                                         # noqa: E731
    if c["layout"] == "packed3":            # q / k / v column slices of one [B * L, 3C] projection; gradients into a second, wider buffer
        assert Lq == Lk and H == Hkv and c["kv_row0"] == 0
        Cd = H * D
        qkv = torch.cat([inp[n].reshape(B * Lq, Cd) for n in ("q", "k", "v")], 1).to(DEV)
        q, k, v = (qkv[:, i * Cd:(i + 1) * Cd].view(B, Lq, H, D) for i in range(3))
        sentinel = -7.0
        buf = torch.full((B * Lq + 2, 3 * Cd + 32), sentinel, dtype=BF16, device=DEV)      # guard row above and below, 8 guard columns around each slice
        cols = [8 + i * (Cd + 8) for i in range(3)]
        dq, dk, dv = (buf[1:-1, c0:c0 + Cd].view(B, Lq, H, D) for c0 in cols)
        for t in (dq, dk, dv):
            t.fill_(NAN)

        def guard():
            mask = torch.ones_like(buf, dtype=torch.bool)
            for c0 in cols:
                mask[1:-1, c0:c0 + Cd] = False
            assert torch.equal(buf[mask], torch.full_like(buf[mask], sentinel)), "wrote outside the dq / dk / dv slices"
    elif c["layout"] == "llm":              # sft_llm.py: q and dq in a packed [rows, (H + 2 Hkv) D] projection, k / v the two halves of a KV cache
        W = (H + 2 * Hkv) * D
        qkv = torch.zeros(B * Lq, W, dtype=BF16, device=DEV)
        qkv[:, :H * D] = inp["q"].reshape(B * Lq, H * D).to(DEV)
        q = qkv[:, :H * D].view(B, Lq, H, D)
        cache = torch.zeros(Bk + 1, Lk + 5, 2, Hkv, D, dtype=BF16, device=DEV)
        cache[:Bk, :Lk, 0], cache[:Bk, :Lk, 1] = inp["k"].to(DEV), inp["v"].to(DEV)
        k, v = cache[:Bk, :Lk, 0], cache[:Bk, :Lk, 1]
        dqkv = torch.full((B * Lq, W), NAN, dtype=BF16, device=DEV)
        dq = dqkv[:, :H * D].view(B, Lq, H, D)
        dk, dv = (torch.full((B, rows, H, D), NAN, dtype=BF16, device=DEV) for _ in range(2))

        def guard():
            assert torch.isnan(dqkv[:, H * D:]).all(), "wrote outside the dq columns"
    else:
        q, k, v = (inp[n].to(DEV) for n in ("q", "k", "v"))
        dq = torch.full((B, Lq, H, D), NAN, dtype=BF16, device=DEV)
        dk, dv = (torch.full((B, rows, H, D), NAN, dtype=BF16, device=DEV) for _ in range(2))
    return q, k, v, dict(dq=dq, dk=dk, dv=dv), guard


def _call(T, c, q, k, v, o, do, k_len, outs, salt=None, **over):
    kw = dict(scale=c["scale"], causal=c["causal"], k_len=k_len, kv_bdiv=c["kv_bdiv"], kv_row0=c["kv_row0"], nsplit=c["nsplit"])
    if c["drop"] is not None:
        kw.update(drop_p=c["drop"][0], drop_seed=c["drop"][1], drop_salt=salt)
    kw.update(over)
    res = T.attention_bwd(q, k, v, o, do, dq=outs["dq"], dk=outs.get("dk"), dv=outs.get("dv"), **kw)
    torch.cuda.synchronize()
    return res


def _forward_o(c, q, k, v, k_len, salt=None):
    from internnav_amd import ops

    kw = {} if c["drop"] is None else dict(drop_p=c["drop"][0], drop_seed=c["drop"][1], drop_salt=salt)
    return ops.attention(q, k, v, scale=c["scale"], causal=c["causal"], kv_bdiv=c["kv_bdiv"], k_len=k_len, **kw)


def _check(c, outs, ref, names=("dq", "dk", "dv"), tag=""):
    worst, bad = {}, []
    for n in names:
        worst[n], ok = R.ratio(outs[n].cpu(), *ref[n])
        if not ok:
            bad.append(n)
    print(f"{c['name']}{tag}: worst |err|/bound " + " ".join(f"{n} {w:.3f}" for n, w in worst.items()))
    assert not bad, f"{c['name']}{tag}: {bad} outside the bound (or not exactly 0 where the bound is 0): {worst}"
    return worst


def _run(T, c, fwd_o=False, salted=False):
    """one case: reference o (or the forward kernel's), one backward call, every element of dq / dk / dv against its bound."""
    inp = R.make_inputs(c)
    q, k, v, outs, guard = _views(c, inp)
    do = inp["do"].to(DEV)
    k_len = None if inp["k_len"] is None else inp["k_len"].to(DEV)
    salt = torch.tensor([R.SALT], dtype=torch.int32, device=DEV) if salted else None
    o = _forward_o(c, q, k, v, k_len, salt).cpu() if fwd_o else None
    _, o, ref = R.case_reference(c, inp, o, salt=R.SALT if salted else 0)
    _call(T, c, q, k, v, o.to(DEV), do, k_len, outs, salt=salt)
    guard()
    _check(c, outs, ref, tag=" (salted)" if salted else "")
    return q, k, v, o.to(DEV), do, k_len, outs, ref


def _group(name):
    cases = R.GROUPS[name] + [c for c in R.FWD_O if c["group"] == name]
    return pytest.mark.parametrize("c", cases, ids=_ids(cases))


def _is_fwd(c):
    return c["name"].endswith("-fwd_o")


@_group("dense")
def test_dense(T, c):
    _run(T, c, fwd_o=_is_fwd(c))


@_group("causal")
def test_causal(T, c):
    _run(T, c, fwd_o=_is_fwd(c))


@_group("ragged_last")
def test_ragged_k_len_last_rows(T, c):
    """the sft_llm.py call: causal, ragged k_len, kv_row0 = -1, dq into the packed projection gradient."""
    _run(T, c, fwd_o=_is_fwd(c))


@_group("ragged_row0")
def test_ragged_k_len_from_row0(T, c):
    """dk / dv rows of keys at or past k_len are written as zero (NaN pre-fill), k_len 0 and a sequence that starts past its len_k included."""
    _run(T, c, fwd_o=_is_fwd(c))


@_group("splits")
def test_key_splits(T, c):
    """dq through the statistics + fp32-atomics launches against the bound; dk / dv must not depend on the split: bit-equal to nsplit 1."""
    B, Lq, Lk = c["dims"][:3]
    if c["nsplit"] is None:
        assert Lq <= 32 and Lk >= 512, "the automatic case must reach the split path"
    q, k, v, o, do, k_len, outs, ref = _run(T, c, fwd_o=_is_fwd(c))
    one = {n: torch.full_like(t, NAN) for n, t in outs.items()}
    _call(T, c, q, k, v, o, do, k_len, one, nsplit=1)
    _check(c, one, ref, tag=" (nsplit 1)")
    assert torch.equal(one["dk"], outs["dk"]) and torch.equal(one["dv"], outs["dv"])


@_group("dropout")
@pytest.mark.parametrize("salted", [False, True], ids=["nosalt", "salt"])
def test_dropout(T, c, salted):
    _run(T, c, fwd_o=_is_fwd(c), salted=salted)


@_group("layout")
def test_layouts(T, c):
    """packed column-slice views with guard rows / columns; kv_bdiv 2 (sequences b and b + 1 share k / v, not gradients)."""
    q, k, v, o, do, k_len, outs, ref = _run(T, c, fwd_o=_is_fwd(c))
    if c["kv_bdiv"] > 1:
        assert not torch.equal(outs["dk"][0], outs["dk"][1]) and not torch.equal(outs["dv"][0], outs["dv"][1])


def test_need_dkv_false_same_dq_bits(T):
    c = R.DENSE[0]
    q, k, v, o, do, k_len, outs, ref = _run(T, c)
    only = dict(dq=torch.full_like(outs["dq"], NAN))
    _, dk, dv = _call(T, c, q, k, v, o, do, k_len, only, need_dkv=False)
    assert dk is None and dv is None
    assert torch.equal(only["dq"], outs["dq"])


@pytest.mark.parametrize("dims,kw", [
    ((1, 4, 8, 2, 2, 12), {}),
    ((1, 4, 8, 2, 2, 136), {}),
    ((1, 4, 8, 3, 2, 64), {}),
    ((1, 4, 8, 2, 2, 64), dict(kv_row0=9)),
    ((1, 4, 8, 2, 2, 64), dict(kv_row0=-2)),
    ((1, 4, 8, 2, 2, 64), dict(nsplit=65)),
], ids=["D12", "D136", "H3_Hkv2", "kv_row0_past_Lk", "kv_row0_minus2", "nsplit65"])
def test_refusals(T, dims, kw):
    """rejected by the library's argument checks (before any launch), reported through _lib.check; the outputs are left as they were."""
    from internnav_amd import _lib

    B, Lq, Lk, H, Hkv, D = dims
    q, do, o = (torch.zeros(B, Lq, H, D, dtype=BF16, device=DEV) for _ in range(3))
    k, v = (torch.zeros(B, Lk, Hkv, D, dtype=BF16, device=DEV) for _ in range(2))
    dq = torch.full((B, Lq, H, D), NAN, dtype=BF16, device=DEV)
    with pytest.raises(_lib.EngineError, match="attention_bwd"):
        T.attention_bwd(q, k, v, o, do, dq=dq, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(dq).all()
