"""CPU: every case of tests/tape_cases.py - the ops of internnav_amd/tape.py and the layers of internnav_amd/train_layers.py against float64 autograd -
with the torch stand-ins of tests/_cpu_kernels.py in place of the kernel wrappers. This pins the case table, the references and the bounds without
a GPU: the exact cases are exact here too, the bounded ones hold their kernel bounds (the stand-ins compute in fp32), the layers their bf16-autocast
yardstick. tests/test_tape_ops_fp64_gpu.py runs the same table on the HIP kernels.

The cases whose dW route depends on alignment keep the product's own `train_ops.gemm_dw_ok` (plain Python on shapes, strides and addresses), so
the five-launch fallback is reached on the CPU as well. Cases the stand-ins cannot run carry a reason and are skipped; at most 10 % may be."""
import pytest
import torch

from tests import _cpu_kernels as K
from tests import tape_cases as C

OPS = C.CASES
WORST = {}


def _install(monkeypatch, case):
    from internnav_amd import train_ops

    real_ok = train_ops.gemm_dw_ok
    K.install(monkeypatch)
    if getattr(case, "real_dw_ok", False):
        monkeypatch.setattr(train_ops, "gemm_dw_ok", real_ok)


def test_skip_cap():
    skipped = [c.id for c in OPS + C.LAYERS if getattr(c, "cpu_skip", None)]
    assert len(skipped) <= 0.10 * len(OPS + C.LAYERS), skipped
    assert all(isinstance(c.cpu_skip, str) and c.cpu_skip for c in OPS if c.cpu_skip)
    assert len({c.id for c in OPS + C.LAYERS}) == len(OPS + C.LAYERS)


@pytest.mark.parametrize("case", OPS, ids=[c.id for c in OPS])
def test_op(monkeypatch, case):
    if case.cpu_skip:
        pytest.skip(case.cpu_skip)
    _install(monkeypatch, case)
    w = C.check(case, C.run(case, "cpu"), WORST)
    print(f"{case.id}: worst |err| / bound {w:.3f}")


@pytest.mark.parametrize("fallback,aligned", C.DW_TWINS)
def test_dw_routes_agree_bit_for_bit(monkeypatch, fallback, aligned):
    """the five-launch fallback and gemm_dw on the same exact values: the same dW, db and dX bits."""
    from internnav_amd import train_ops

    taken = []
    real_ok = train_ops.gemm_dw_ok
    K.install(monkeypatch)
    monkeypatch.setattr(train_ops, "gemm_dw_ok", lambda *a: taken.append(real_ok(*a)) or taken[-1])
    a, b = C.run(C.by_id(fallback), "cpu"), C.run(C.by_id(aligned), "cpu")
    assert taken[:2] == [False, True] and all(taken[1:]), f"routes offered (gemm_dw?): {taken}"          # (gemm_dw asks once more itself)
    for k in ("p.w", "p.b", "x.x"):
        assert torch.equal(a[k], b[k]), k


def test_frozen_linear_has_no_gradient_entry_and_no_dw_launch(monkeypatch):
    """a linear whose weight lives in the frozen store: the trainable store has no entry for it and the backward never reaches the dW routes."""
    from internnav_amd import ops, train_ops

    K.install(monkeypatch)
    calls = []
    for mod, name in ((train_ops, "gemm_dw_ok"), (train_ops, "gemm_dw"), (train_ops, "transpose"), (train_ops, "colsum"), (ops, "linear")):
        monkeypatch.setattr(mod, name, (lambda f, n: lambda *a, **kw: calls.append(n) or f(*a, **kw))(getattr(mod, name), name))
    case = C.by_id("linear-frozen")
    got = C.run(case, "cpu")
    store = got["_tape"].store
    assert "w" not in store.index and "b" not in store.index and set(store.index) == {"dummy"} and "p.w" not in got
    assert calls == ["linear", "transpose", "linear"], calls          # forward, W^T for dX, dX: no dW GEMM, no bias column sum
    C.check(case, got)


@pytest.mark.parametrize("case", [c for c in OPS if c.op == "attention"], ids=[c.id for c in OPS if c.op == "attention"])
def test_attention_closed_form_is_autograd(case):
    """attn_bwd_ref's restatement with delta from the float64 o equals float64 autograd: the bound's reference is the derivative."""
    pb = C.built(case)
    a = pb.attn
    b = a.blocks({k: t for k, (t, _) in pb.vars.items()})
    assert C.attention_autograd_gap(b["q"], b["k"], b["v"], a.do.view(a.B, a.Lq, a.H, a.D), a.causal) < 1e-12


@pytest.mark.parametrize("lc", C.LAYERS, ids=[c.id for c in C.LAYERS])
def test_layer(monkeypatch, lc):
    K.install(monkeypatch)
    table = []
    w = C.layer_check(lc, C.layer_run(lc, "cpu"), table)
    print("\n".join(table))
    print(f"{lc.id}: worst engine / bf16-autocast ratio {w:.2f}")


def test_zz_worst_per_op():
    print("worst |err| / bound per op (stand-ins):", {k: round(v, 3) for k, v in sorted(WORST.items())})
    assert all(v <= 1.0 for v in WORST.values())
