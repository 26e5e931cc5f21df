"""CPU: the float64 reference of the SFT-step kernels (tests/train_ops_ref.py) is itself checked - hand-written derivatives against
torch.autograd in float64, AdamW against torch.optim.AdamW + clip_grad_norm_ in float64, the LayerNorm conditioning term of the bound against
fp32 torch - and every stand-in of tests/_cpu_kernels.py is held to the reference with the argument sets the GPU test gives the kernels
(tests/train_ops_cases.py): the CPU half of "stand-in == kernel"."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _cpu_kernels as K
from tests import train_ops_cases as CASES
from tests import train_ops_ref as R

F64 = torch.float64
_TORCH_ACT = {"gelu_erf": F.gelu, "gelu_tanh": lambda t: F.gelu(t, approximate="tanh"), "relu": F.relu, "silu": F.silu, "tanh": torch.tanh}


def _close(a, b, what, rel=1e-12):
    tol = rel * b.abs().max().clamp_min(1e-300)
    assert float((a - b).abs().max()) <= float(tol), f"{what}: {float((a - b).abs().max())} vs tol {float(tol)}"


@pytest.mark.parametrize("act", R.ACTS)
def test_activation_closed_forms_equal_autograd(act):
    x = torch.cat([torch.linspace(-12, 12, 4801, dtype=F64), torch.tensor([-100.0, -50.0, -20.0, 20.0, 50.0, 100.0], dtype=F64)])
    x = x[x != 0] if act == "relu" else x
    xr = x.clone().requires_grad_(True)
    y = _TORCH_ACT[act](xr)
    dy = torch.linspace(-2, 3, x.numel(), dtype=F64)
    (gx,) = torch.autograd.grad(y, xr, dy)
    _close(R.act_value(x, act)[0], y.detach(), f"{act} value")
    _close(R.act_bwd(x, dy, act)[0], gx, f"{act} backward")
    v, vs = R.act_value(x, act)
    s, ss = R.act_slope(x, act)
    assert bool((vs >= v.abs() * (1 - 1e-15)).all()) and bool((ss >= s.abs() * (1 - 1e-15)).all()), "scale is a sum of |terms|: never below |ref|"


def test_glu_closed_form_equals_autograd():
    g = torch.Generator().manual_seed(0)
    a, b, dy = (torch.randn(33, 20, generator=g, dtype=F64) * 3 for _ in range(3))
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ga, gb = torch.autograd.grad(F.silu(ar) * br, (ar, br), dy)
    (da, _), (db, _) = R.glu_bwd(a, b, dy)
    _close(R.glu_fwd(a, b)[0], (F.silu(a) * b), "glu forward")
    _close(da, ga, "glu da")
    _close(db, gb, "glu db")


@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("gamma", [False, True])
def test_norm_backward_closed_form_equals_autograd(rms, gamma):
    g = torch.Generator().manual_seed(1)
    for C in (4, 70, 384):
        x = torch.randn(9, C, generator=g, dtype=F64) * 2 + 0.6
        dy = torch.randn(9, C, generator=g, dtype=F64)
        ga = torch.randn(C, generator=g, dtype=F64) * 0.2 + 1 if gamma else None
        xr = x.clone().requires_grad_(True)
        y = R.norm_fwd(xr, ga, 1e-5, rms)
        (gx,) = torch.autograd.grad(y, xr, dy)
        (dx, _), (xh, _) = R.norm_bwd(x, dy, ga, 1e-5, rms)
        _close(dx, gx, f"norm_bwd C={C}", rel=1e-11)
        if not rms:
            _close(y.detach(), F.layer_norm(x, (C,), ga, None, 1e-5), "norm forward == F.layer_norm")
            _close(xh, F.layer_norm(x, (C,), None, None, 1e-5), "xhat")


def test_masked_mse_closed_form_equals_autograd():
    g = torch.Generator().manual_seed(2)
    nseq, T, D = 6, 8, 3
    pred = torch.randn(nseq * T, D, generator=g, dtype=F64)
    tgt = torch.randn(nseq * T, D, generator=g)
    mask = torch.tensor([1, 0.5, 0, 1, 0, 0.25])
    pr = pred.clone().requires_grad_(True)
    loss = (F.mse_loss(pr, tgt.double(), reduction="none").view(nseq, T, D) * mask.double()[:, None, None]).sum() / mask.double().sum() / (T * D)
    (gp,) = torch.autograd.grad(loss * 0.3, pr)
    (l, _), (dp, _) = R.mse_masked(pred, tgt, mask, T, loss_scale=R.f32(0.3))
    _close(l, loss.detach().view(1), "loss")
    _close(dp, gp * (R.f32(0.3) / 0.3), "dpred", rel=1e-11)
    (l0, _), (dp0, _) = R.mse_masked(pred, tgt, torch.zeros(nseq), T)
    assert float(l0) == 0.0 and not dp0.any(), "an all-masked batch: loss 0, dpred 0"


@pytest.mark.parametrize("max_norm,gscale", [(1.0, 1.0), (1.0, 0.125), (0.0, 0.5)])
def test_adamw_restatement_equals_torch_float64(max_norm, gscale):
    g = torch.Generator().manual_seed(3)
    n = 2048
    # the restatement takes the hyper-parameters as the fp32 values of the C-ABI: values that fp32 holds exactly make the two the same formula
    hp = dict(lr=2.0 ** -7, beta1=0.875, beta2=1 - 2.0 ** -10, eps=2.0 ** -27, wd=2.0 ** -6)
    p0 = torch.randn(n, generator=g, dtype=F64)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=hp["wd"])
    p, m, v = p0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for step in range(1, 4):
        grad = torch.randn(n, generator=g, dtype=F64) * (3.0 if step == 2 else 0.01) / gscale
        ref.grad = grad * gscale
        tn = torch.nn.utils.clip_grad_norm_([ref], max_norm) if max_norm > 0 else None
        opt.step()
        r = R.adamw(p, grad, m, v, step=step, sumsq=float(grad.pow(2).sum()), max_norm=max_norm, grad_scale=gscale, **hp)
        p, m, v = r["p"], r["m"], r["v"]
        _close(p, ref.detach(), f"p after step {step}")
        if tn is not None:
            assert abs(r["norm"] - float(tn)) <= 1e-12 * float(tn)


@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("C", [8, 384, 3584, 4096, 5120])
@pytest.mark.parametrize("shift,spread", [(0.6, 2.0), (64.0, 1.0)])
def test_norm_backward_bound_model_holds_for_fp32_torch(rms, C, shift, spread):
    """the bound the GPU test applies to the kernel (k = 16) is met, with margin, by plain fp32 torch autograd - including LayerNorm at
    mean = 64 x spread, where the model without the |x|max * rstd term of `scale` is missed."""
    g = torch.Generator().manual_seed(C)
    x = torch.randn(16, C, generator=g) * spread + shift
    dy, ga = torch.randn(16, C, generator=g), torch.randn(C, generator=g) * 0.2 + 1
    xr = x.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(R.norm_fwd(xr, ga, 1e-5, rms), xr, dy)
    (dx, scale), _ = R.norm_bwd(x, dy, ga, 1e-5, rms)
    ratio = float(((gx.double() - dx).abs() / (R.U * math.sqrt(C) * scale)).max())
    assert ratio <= 4.0, f"fp32 torch misses the model by {ratio}"


@pytest.mark.parametrize("g", [1, 32, 33, 2048, 2049, 4096, 4097, 8192, 8193, 95000])
def test_colsum_chunks_cover_the_group(g):
    from internnav_amd import train_ops as T

    n = T.colsum_chunks(g)
    chunk = g if g <= 32 else 32 if g <= 2048 else 64 if g <= 4096 else 128 if g <= 8192 else 256
    assert n * chunk >= g > (n - 1) * chunk and n <= max(64, (g + 255) // 256)


def _ids(cs):
    return [c["id"] for c in cs]


_ALL_CASES = [c for name, fn in CASES.ALL.items() for c in fn("cpu")] + [CASES.colsum_big_case("cpu")]


@pytest.mark.parametrize("c", _ALL_CASES, ids=_ids(_ALL_CASES))
def test_stand_in_within_the_fp32_bound_of_the_reference(c):
    """covers the four points where stand-in and kernel used to differ: all-masked MSE, a tab that does not divide rows, x_bcast, scale = 0."""
    CASES.run_case(K.TRAIN_OPS, c)


def test_case_list_holds_the_four_contract_points():
    ids = " ".join(_ids(_ALL_CASES))
    for needle in ("-zero-", "tab32-rows80", "colsum-x_bcast", "colsum-scale0"):
        assert needle in ids, needle


@pytest.mark.parametrize("var", CASES.ADAMW_VARIANTS, ids=[v["id"] for v in CASES.ADAMW_VARIANTS])
def test_adamw_stand_in_within_the_bound(var):
    CASES.adamw_run(K.adamw, K.sumsq_parts, "cpu", var, n=4096 + 777, steps=4)
