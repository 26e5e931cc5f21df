"""CPU checks of NavDPNet's image-, pixel- and mixed-goal inference: the fp32 restatement (tests/navdp_goal_ref.py) against the fixture
written from the reference's own NavDPNet, the host plan of a mixed call, the goal towers a checkpoint yields, and what reaches
ina_goal_slots. No GPU: engines are built on the CPU device (construction launches nothing) and the library is stood in for."""
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from internnav_amd import _lib, ops
from internnav_amd import synthetic as S
from internnav_amd.navdp import GOAL_IMAGE, GOAL_NONE, GOAL_PIXEL, GOAL_POINT, NavDPNet, goal_plan
from internnav_amd.vit_s import KPAD, DinoV2Encoder, VitWorkspace, patch_kpad
from tests import navdp_goal_ref as O

GOLD = Path(__file__).resolve().parent / "golden" / "navdpnet_goals.pt"
CFG = S.NAVDPNET_CFG


def _gold():
    return torch.load(GOLD, weights_only=True)


def _rel(a, b):
    return (a.float() - b.float()).abs().max().item() / max(b.float().abs().max().item(), 1e-30)


@pytest.mark.parametrize("kind,pc", [("image", 4), ("pixel", 4), ("pixel", 7)])
def test_restatement_matches_reference_fixture(kind, pc):
    gold = _gold()
    g = gold["image"] if kind == "image" else gold["pixel"][pc]
    B = gold["B"]
    assert g["oracle_max_rel_diff"] < 1e-4
    sd = S.navdpnet_train_state_dict(seed=gold["weight_seed"], pixel_channel=pc)
    inp = S.navdpnet_inputs(B, seed=gold["input_seed"])
    goal = S.navdpnet_goal_inputs(B, seed=gold["input_seed"], pixel_channel=pc)["goal_" + kind]
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    with torch.no_grad():
        e = O.goal_embed(sd, kind, goal)
        neg, pos, fin, cr = O.navdpnet_goal(sd, e, inp["images"], inp["depths"], inp["x_init"], inp["step_noise"], CFG, return_all=True)
    for name, mine in (("goal_embed", e), ("negative", neg), ("positive", pos), ("oracle_final", fin), ("oracle_critic", cr)):
        assert _rel(mine, g[name]) < 1e-4, name


def test_goal_differs_between_kinds_in_fixture():
    """the fixture is not degenerate: the goal moves the trajectories (image vs pixel goal on the same frames and noise)."""
    gold = _gold()
    assert (gold["image"]["oracle_final"] - gold["pixel"][4]["oracle_final"]).abs().max().item() > 1e-2
    assert (gold["pixel"][4]["goal_embed"] - gold["pixel"][7]["goal_embed"]).abs().max().item() > 1e-2


def test_mixed_plan_index_maps():
    kind = [GOAL_NONE, GOAL_PIXEL, GOAL_IMAGE, GOAL_POINT, GOAL_IMAGE, GOAL_PIXEL, GOAL_POINT]
    img = torch.zeros(2, 224, 224, 6)
    pix = torch.zeros(2, 224, 224, 4)
    plan = goal_plan(kind, torch.zeros(7, 3), img, pix, pixel_channel=4)
    assert plan.B == 7 and (plan.n_point, plan.n_image, plan.n_pixel) == (2, 2, 2)
    assert plan.kind.dtype == plan.row.dtype == torch.int32
    assert plan.kind.tolist() == kind
    # image / pixel rows: rank among the envs of that kind; point rows: the env itself for a [B, 3] goal_point
    assert plan.row.tolist() == [0, 0, 0, 3, 1, 1, 6]
    compact = goal_plan(kind, torch.zeros(2, 3), img, pix, pixel_channel=4)
    assert compact.row.tolist() == [0, 0, 0, 0, 1, 1, 1]
    single = goal_plan(torch.full((3,), GOAL_IMAGE), goal_image=torch.zeros(3, 224, 224, 6), pixel_channel=None)
    assert single.row.tolist() == [0, 1, 2] and (single.n_point, single.n_image, single.n_pixel) == (0, 3, 0)


@pytest.mark.parametrize("args,match", [
    (dict(goal_kind=[0, 4]), "values must be"),
    (dict(goal_kind=torch.tensor([0.0, 1.0])), "integer"),
    (dict(goal_kind=[]), "non-empty"),
    (dict(goal_kind=[1, 0]), "goal_point is None"),
    (dict(goal_kind=[1, 1, 0], goal_point=torch.zeros(1, 3)), r"\[B, 3\]"),
    (dict(goal_kind=[0, 0], goal_point=torch.zeros(2, 3)), "no env has goal kind 1"),
    (dict(goal_kind=[2, 0, 2], goal_image=torch.zeros(3, 224, 224, 6)), r"must be \[2, 224, 224, 6\]"),
    (dict(goal_kind=[2], goal_image=torch.zeros(1, 224, 224, 3)), r"must be \[1, 224, 224, 6\]"),
    (dict(goal_kind=[3, 3], goal_pixel=torch.zeros(2, 224, 224, 7), pixel_channel=4), r"must be \[2, 224, 224, 4\]"),
    (dict(goal_kind=[3], goal_pixel=torch.zeros(1, 224, 224, 4), pixel_channel=None), "needs a pixel-goal encoder"),
    (dict(goal_kind=[0], goal_image=torch.zeros(1, 224, 224, 6)), "no env has goal kind 2"),
])
def test_mixed_plan_validation(args, match):
    args = dict(args)
    args.setdefault("pixel_channel", 4)
    with pytest.raises(ValueError, match=match):
        goal_plan(**args)


@pytest.mark.parametrize("pc", [4, 7])
def test_pixel_channel_and_tower_widths_from_weights(pc):
    net = NavDPNet(S.navdpnet_train_state_dict(seed=1, pixel_channel=pc), CFG, "cpu", max_envs=2)
    assert net.pixel_channel == pc
    assert sorted(net.goal_towers) == ["image", "pixel"] and not net.missing_goal_keys
    assert net.goal_towers["image"].vit.kpad == 1176 and net.goal_towers["pixel"].vit.kpad == patch_kpad(pc) == {4: 784, 7: 1376}[pc]
    # the shared im2col buffer holds either the RGB frames or the widest goal sub-batch
    assert net.vit_ws.patches.numel() >= max(2 * CFG["memory_size"] * 256 * KPAD, 2 * 256 * patch_kpad(pc))
    assert net.rgb.kpad == net.depth_vit.kpad == KPAD


def test_point_only_checkpoint_refuses_image_and_pixel_goals():
    net = NavDPNet(S.navdpnet_state_dict(seed=0), CFG, "cpu", max_envs=2)
    assert net.goal_towers == {} and net.pixel_channel is None
    inp = S.navdpnet_inputs(2, seed=0)
    goals = S.navdpnet_goal_inputs(2, seed=0, pixel_channel=4)
    rest = (inp["images"], inp["depths"], inp["x_init"], inp["step_noise"])
    with pytest.raises(KeyError, match=r"no image-goal encoder: \d+ parameters are missing, e.g. \['image_encoder\.imagegoal_encoder\."):
        net.predict_imagegoal_batch_action_vel(goals["goal_image"], *rest)
    with pytest.raises(KeyError, match=r"no pixel-goal encoder: \d+ parameters are missing, e.g. \['pixel_encoder\.pixelgoal_encoder\."):
        net.predict_pixelgoal_batch_action_vel(goals["goal_pixel"], *rest)
    with pytest.raises(KeyError, match="image_encoder.project_layer.weight|imagegoal_encoder"):
        net.predict_mixedgoal_batch_action_vel(torch.tensor([1, 2]), goal_point=torch.zeros(2, 3), goal_image=goals["goal_image"][:1],
                                               input_images=inp["images"], input_depths=inp["depths"], x_init=inp["x_init"],
                                               step_noise=inp["step_noise"])


def test_partial_goal_tower_is_refused():
    sd = S.navdpnet_train_state_dict(seed=0, pixel_channel=4)
    del sd["pixel_encoder.project_layer.bias"]
    with pytest.raises(KeyError, match="part of the pixel-goal encoder"):
        NavDPNet(sd, CFG, "cpu", max_envs=1)


@pytest.mark.parametrize("cin", [1, 3, 4, 6, 7])
def test_patch_embed_width_follows_the_conv_weight(cin):
    """K = max(C, 3) * 196 padded to a multiple of 8 (train_layers.DinoTrain's rule); C = 3 keeps the padded weight it had (592 columns, 4 zeros)."""
    spec = S.dinov2_vits_spec("")
    spec["patch_embed.proj.weight"] = ((384, cin, 14, 14), "w")
    sd = S.materialize(spec, seed=2)
    enc = DinoV2Encoder(sd, "", "cpu")
    conv = sd["patch_embed.proj.weight"]
    assert enc.channels == cin and enc.kpad == (max(cin, 3) * 196 + 7) // 8 * 8
    assert enc.w_patch.shape == (384, enc.kpad) and enc.w_patch.dtype == torch.bfloat16
    assert torch.equal(enc.w_patch[:, : cin * 196], conv.float().reshape(384, -1).to(torch.bfloat16))
    assert not enc.w_patch[:, cin * 196:].float().any()
    if cin == 3:
        old = F.pad(conv.float().reshape(384, 588), (0, KPAD - 588)).to(torch.bfloat16)
        assert torch.equal(enc.w_patch, old)


def test_vit_workspace_patch_capacity():
    assert VitWorkspace(2, "cpu").patches.numel() == 2 * 256 * KPAD
    assert VitWorkspace(2, "cpu", patch_numel=2 * 256 * 1376).patches.numel() == 2 * 256 * 1376


class _Recorder:
    def __init__(self):
        self.calls = []

    def ina_goal_slots(self, *args):
        self.calls.append(args)
        return 0


def test_goal_slots_arguments_reach_the_library(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    B, L, D = 4, 132, 384
    cond = torch.empty(B * L, D, dtype=torch.bfloat16)
    plan = torch.tensor([0, 1, 2, 3, 0, 0, 0, 0], dtype=torch.int32)
    pos = torch.zeros(L, D)
    embed = torch.empty(B, D)
    pt = (torch.zeros(1, 3), torch.zeros(D, 3), torch.zeros(D))
    tok = torch.zeros(2 * 256, 384)
    img = (tok[:256], torch.zeros(D, 384), torch.zeros(D), 256)
    pix = (tok[256:], torch.zeros(D, 384), torch.zeros(D), 256)
    ops.goal_slots(cond, L, plan[:B], plan[B:], pos=pos, embed=embed, point=pt, image=img, pixel=pix)
    a = rec.calls[-1]
    assert len(a) == len(_lib.SYMBOLS["ina_goal_slots"][1])
    Y, ldy, ydt, L_, slot0, nslots, P, B_, D_, kind, row, emb = a[:12]
    assert (Y, ldy, ydt, L_, slot0, nslots, P, B_, D_) == (cond.data_ptr(), D, 0, L, 1, 3, pos.data_ptr(), B, D)
    assert (kind, row, emb) == (plan.data_ptr(), plan[B:].data_ptr(), embed.data_ptr())
    assert a[12:16] == (pt[0].data_ptr(), 1, pt[1].data_ptr(), pt[2].data_ptr())
    assert a[16:20] == (tok.data_ptr(), 1, img[1].data_ptr(), img[2].data_ptr())
    assert a[20:24] == (tok[256:].data_ptr(), 1, pix[1].data_ptr(), pix[2].data_ptr())
    assert a[24:26] == (256, 384)
    ops.goal_slots(cond, L, plan[:B], plan[B:], pos=pos)            # no goal inputs at all: zero rows everywhere
    a = rec.calls[-1]
    assert a[13] == a[17] == a[21] == 0 and a[12] is None and a[16] is None and a[20] is None
