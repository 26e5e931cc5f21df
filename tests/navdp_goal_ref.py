"""TEST INFRASTRUCTURE: fp32 restatement of NavDPNet inference with an image, pixel or point goal, composed from the oracle's pieces:
the goal towers of tests/navdp_train_ref.py (`_goal_tower`: ImageGoalBackbone / PixelGoalBackbone.forward), oracle.navdp's
`navdpnet_predict_noise` / `navdpnet_predict_critic`, and the loop of oracle.navdp.navdpnet_pointgoal with the goal embedding passed in -
the reference's predict_pointgoal_batch_action_vel (navdp_policy.py:302-321) with goal_embed = the tower's output. Pinned by
tests/golden/navdpnet_goals.pt (written by tools/make_golden_navdp_goals.py from the reference's own NavDPNet)."""
from __future__ import annotations

import torch

from oracle.navdp import navdpnet_predict_critic, navdpnet_predict_noise, rgbd_backbone
from oracle.nn_ref import linear
from oracle.schedulers import DDPMScheduler
from tests.navdp_train_ref import _goal_tower

KINDS = ("image", "pixel")


def goal_embed(sd, kind: str, goal: torch.Tensor) -> torch.Tensor:
    """f32 [B, D]: point_encoder(goal [B, 3]), image_encoder(goal [B,224,224,6]) or pixel_encoder(goal [B,224,224,C])."""
    if kind == "point":
        return linear(goal.float(), sd, "point_encoder")
    return _goal_tower(goal, sd, f"{kind}_encoder.")


def navdpnet_goal(sd, goal: torch.Tensor, images, depths, x_init, step_noise, cfg, return_all=False):
    """the sampler / critic / ranking of navdpnet_pointgoal, per env, with the goal embedding goal [B, D] (zeros: the no-goal call).
    Returns negative / positive [B,8,T,3] (+ final samples [B,S,T,3] and critic values [B,S])."""
    B = images.shape[0]
    K = cfg["num_train_timesteps"]
    sch = DDPMScheduler(num_train_timesteps=K)
    sch.set_timesteps(K)
    rgbd = rgbd_backbone(images, depths, sd)
    g = goal.float().unsqueeze(1)
    neg, pos, finals, critics = [], [], [], []
    for b in range(B):
        x = x_init[b].float()
        for i, t in enumerate(sch.timesteps.tolist()):
            eps = navdpnet_predict_noise(sd, x, t, g[b:b + 1], rgbd[b:b + 1], cfg)
            x = sch.step(eps, t, x, noise=step_noise[i, b].float()).prev_sample
        c = navdpnet_predict_critic(sd, x, rgbd[b:b + 1], cfg)
        traj = torch.cumsum(x / 4.0, dim=1)
        neg.append(traj[c.argsort()[0:8]])
        pos.append(traj[(-c).argsort()[0:8]])
        finals.append(x)
        critics.append(c)
    out = (torch.stack(neg), torch.stack(pos))
    if return_all:
        out = out + (torch.stack(finals), torch.stack(critics))
    return out
