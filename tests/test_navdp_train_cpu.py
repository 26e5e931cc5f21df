"""CPU: the NavDPNet training step (internnav_amd/navdp_train.py) without a GPU.
  * the fp32 restatement of tests/navdp_train_ref.py against the reference-executed fixture tests/golden/navdp_train.pt
    (tools/make_golden_navdp_train.py): loss terms, per-tensor gradient norms, stored gradient slices;
  * the trainer's host-side parameter plan (trainable / frozen / untouched, decay group) against the reference's module tree;
  * the mg goal-slot table against the reference's `b % 27` rule;
  * the WIRING of the tape (every forward op and backward closure) with the torch stand-ins of tests/_cpu_kernels.py against autograd
    of the restatement, at a reduced depth / memory size;
  * the cosine schedule."""
import math
from pathlib import Path

import pytest
import torch

from internnav_amd import navdp_train as NT
from internnav_amd import synthetic as S
from tests import _cpu_kernels as K
from tests import navdp_train_ref as O

GOLD = Path(__file__).resolve().parent / "golden" / "navdp_train.pt"


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, weights_only=False)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


@pytest.mark.parametrize("pc", [4, 7])
def test_oracle_matches_reference_fixture(gold, pc):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    g = gold["pixel_channel"][pc]
    cfg = S.NAVDPNET_CFG
    sd = S.navdpnet_train_state_dict(seed=gold["weight_seed"], pixel_channel=pc)
    batch = O.synthetic_batch(gold["B"], gold["batch_seed"], pc, cfg)
    draws = O.synthetic_draws(gold["B"], gold["draw_seed"], cfg)
    terms, grads = O.oracle_grads(sd, batch, draws, cfg)
    for k in O.LOSS_TERMS:
        assert _rel(terms[k], g["terms"][k]) <= 1e-5, (k, terms[k], g["terms"][k])
    assert set(grads) == set(g["grad_norms"]), "the oracle and the reference differ in which tensors get a gradient"
    scale = max(g["grad_norms"].values())
    worst = max(((k, abs(grads[k].norm().item() - n) / max(n, 1e-6 * scale)) for k, n in g["grad_norms"].items()), key=lambda t: t[1])
    assert worst[1] <= 1e-4, worst
    for k, ref in g["grad_slices"].items():
        got = grads[k].flatten()[: ref.numel()]
        assert ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item() <= 1e-4, k


@pytest.mark.parametrize("pc", [4, 7])
def test_param_plan_matches_reference(gold, pc):
    g = gold["pixel_channel"][pc]
    keys = list(S.navdpnet_train_spec(S.NAVDPNET_CFG, pc).keys())
    assert set(keys) == set(g["keys"])
    plan = NT.param_plan(keys)
    trainable = {k for k, v in plan.items() if v == "trainable"}
    assert trainable == set(g["requires_grad"]) - set(g["no_grad"])
    assert {k for k, v in plan.items() if v == "untouched"} == set(g["no_grad"]) == {
        p + "mask_token" for p in ("rgbd_encoder.depth_model.", "image_encoder.imagegoal_encoder.", "pixel_encoder.pixelgoal_encoder.")}
    frozen = {k for k, v in plan.items() if v == "frozen"}
    assert frozen == set(keys) - set(g["requires_grad"]) and all(k.startswith("rgbd_encoder.rgb_model.") for k in frozen)
    assert "rgbd_encoder.rgb_model.patch_embed.proj.weight" in frozen
    decay = NT.decay_names(keys)
    # the reference's list also names the unregistered (None) q/k/v_proj_weight slots of nn.MultiheadAttention: no tensor behind them
    assert len(decay) == len(set(decay)) and set(decay) == set(g["decay"]) & set(keys)
    with pytest.raises(NotImplementedError, match="finetune"):
        NT.param_plan(keys, finetune=True)


def test_goal_slot_table_is_the_reference_rule():
    for B in range(1, 65):
        t = NT.goal_slot_table(B)
        assert torch.equal(t, O.goal_slots(B)), B
        for b in range(B):
            assert [int(v) for v in t[b]] == [(b % 27) // 3 ** j % 3 for j in range(3)]


def test_cosine_schedule():
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=1e-4)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(s) / 10))))
    for s in range(12):
        assert abs(NT.cosine_lr(1e-4, s, 10) - opt.param_groups[0]["lr"]) < 1e-12, s
        opt.step()
        sched.step()
    assert NT.cosine_lr(1e-4, 5, None) == 1e-4


def _patchify_any(img, out, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), ps=14):
    """CPU stand-in of ops.patchify for every channel count (tests/_cpu_kernels.py covers C = 1 / 3)."""
    n, H, W, C = img.shape
    if C in (1, 3):
        return K.patchify(img, out, mean, std, ps)
    p = img.float().permute(0, 3, 1, 2).unfold(2, ps, ps).unfold(3, ps, ps)
    p = p.permute(0, 2, 3, 1, 4, 5).reshape(n * (H // ps) * (W // ps), C * ps * ps)
    out.zero_()
    out[:, : p.shape[1]] = p.to(out.dtype)
    return out


@pytest.mark.parametrize("pc", [4, 7])
def test_tape_wiring(monkeypatch, pc):
    from internnav_amd import ops

    K.install(monkeypatch)
    monkeypatch.setattr(ops, "patchify", _patchify_any)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cfg = dict(S.NAVDPNET_CFG, memory_size=1, temporal_depth=2)
    B = 2
    sd = S.navdpnet_train_state_dict(seed=1, cfg=cfg, pixel_channel=pc)
    batch = O.synthetic_batch(B, 3, pc, cfg)
    draws = O.synthetic_draws(B, 4, cfg)
    terms, ref = O.oracle_grads(sd, batch, draws, cfg)
    head = NT.NavDPNetTrainHead(sd, "cpu", cfg)
    got = head.loss_and_grads(batch, draws)
    for k in O.LOSS_TERMS:
        assert _rel(got[k].item(), terms[k]) < 1e-2, (k, got[k].item(), terms[k])
    assert set(head.P.index) == set(ref), "the tape trains a different set of tensors than autograd"
    scale = max(v.norm().item() for v in ref.values())
    worst = ("", 0.0)
    for k, r in ref.items():
        gk = head.P.grad(k).view_as(r)
        if r.norm().item() < 1e-6 * scale:
            assert gk.norm().item() < 1e-4 * scale, k
            continue
        e = ((gk - r).norm() / r.norm()).item()
        worst = max(worst, (k, e), key=lambda t: t[1])
    assert worst[1] < 4e-2, worst          # bf16 activations between the stand-in ops, like the engine
    # gradient accumulation: loss_scale scales every gradient, the reported loss terms are unscaled
    full = head.P.g32.clone()
    head.P.zero_grad()
    half = head.loss_and_grads(batch, draws, loss_scale=0.5)
    assert abs(half["loss"].item() - got["loss"].item()) < 1e-6
    assert ((head.P.g32 - 0.5 * full).norm() / full.norm()).item() < 1e-5
