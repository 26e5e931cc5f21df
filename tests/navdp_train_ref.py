"""TEST INFRASTRUCTURE: fp32 autograd restatement of one NavDPNet training step (NavDPNet.forward, navdp_policy.py:187-273, and
NavDPTrainer.compute_loss, navdp_trainer.py:80-101), composed from the oracle's functions (oracle/navdp.py, oracle/dinov2.py,
oracle/nn_ref.py). `tests/golden/navdp_train.pt` (written by tools/make_golden_navdp_train.py from the reference's own modules) pins it;
the GPU tests compare the HIP trainer against it. Dropout is off (the eval-mode gradient), the two `sample_noise` draws are inputs."""
from __future__ import annotations

from typing import Dict

import torch

from oracle import dinov2
from oracle.navdp import _decoder, rgbd_backbone
from oracle.nn_ref import causal_mask, layer_norm, linear, sinusoidal_pos_emb
from oracle.schedulers import DDPMScheduler

LOSS_TERMS = ("loss", "ng_action_loss", "mg_action_loss", "critic_loss", "aux_loss")


def goal_slots(B: int) -> torch.Tensor:
    """navdp_policy.py:222-232, as the reference writes it: slot j of sample b takes candidate (b % 27 // 3^j) % 3 (0 point, 1 image,
    2 pixel)."""
    pattern = torch.arange(B) % 27
    return torch.stack([pattern % 3, (pattern // 3) % 3, (pattern // 9) % 3], dim=1)


def _goal_tower(img, sd, p):
    """ImageGoalBackbone / PixelGoalBackbone.forward (navdp_backbone.py:340-346, 391-397): raw channels, mean over the patch tokens,
    project_layer."""
    x = img.float().permute(0, 3, 1, 2)
    tower = p + ("imagegoal_encoder." if p.startswith("image") else "pixelgoal_encoder.")
    return linear(dinov2.forward_tokens(x, sd, tower).mean(dim=1), sd, p + "project_layer")


def navdpnet_train_loss(sd: Dict[str, torch.Tensor], batch: Dict[str, torch.Tensor], draws: Dict[str, torch.Tensor], cfg) -> Dict[str, torch.Tensor]:
    """batch: the navdp_collate_fn dict (navdp_lerobot_dataset.py:573-586); draws: ng_noise / mg_noise [B, T, 3], ng_t / mg_t int [B].
    Returns the five loss terms of compute_loss (+ the heads' outputs) as fp32 autograd values."""
    D, M, H = cfg["token_dim"], cfg["memory_size"], cfg["heads"]
    depth = cfg["temporal_depth"]
    pg = batch["batch_pg"].float()
    labels, augments = batch["batch_labels"].float(), batch["batch_augments"].float()
    B, Tn = labels.shape[:2]
    sch = DDPMScheduler(num_train_timesteps=cfg["num_train_timesteps"])

    def sample(noise, t):                       # sample_noise (navdp_policy.py:148-157) with injected draws
        a = sch.alphas_cumprod[t.long()].view(B, 1, 1)
        noisy = a.sqrt() * labels + (1 - a).sqrt() * noise.float()
        return sinusoidal_pos_emb(t.long().float(), D).unsqueeze(1), linear(noisy, sd, "input_embed")

    ng_te, ng_x = sample(draws["ng_noise"], draws["ng_t"])
    mg_te, mg_x = sample(draws["mg_noise"], draws["mg_t"])
    sd_rgb = {k: (v.detach() if ".rgb_model." in k else v) for k, v in sd.items()}          # finetune=False: RGB tokens detached
    rgbd = rgbd_backbone(batch["batch_rgb"], batch["batch_depth"].unsqueeze(1), sd_rgb)      # [B, M*16, D]
    point = linear(pg, sd, "point_encoder").unsqueeze(1)
    nogoal = torch.zeros_like(point)
    image = _goal_tower(batch["batch_ig"], sd, "image_encoder.").unsqueeze(1)
    pixel = _goal_tower(batch["batch_tg"], sd, "pixel_encoder.").unsqueeze(1)
    image_aux = linear(image[:, 0], sd, "image_aux_head")
    pixel_aux = linear(pixel[:, 0], sd, "pixel_aux_head")
    label_embed = linear(labels, sd, "input_embed").detach()
    augment_embed = linear(augments, sd, "input_embed").detach()
    cpe = sd["cond_pos_embed.position_embedding.weight"][: 4 + M * 16]
    ng_cond = torch.cat([ng_te, nogoal, nogoal, nogoal, rgbd], dim=1) + cpe
    cand = torch.stack([point, image, pixel], dim=0)                                         # [3, B, 1, D]
    sel, ar = goal_slots(B), torch.arange(B)
    mg_cond = torch.cat([mg_te, cand[sel[:, 0], ar], cand[sel[:, 1], ar], cand[sel[:, 2], ar], rgbd], dim=1) + cpe
    ope = sd["out_pos_embed.position_embedding.weight"][:Tn]
    cmask = causal_mask(Tn)
    mmask = torch.zeros(Tn, 4 + M * 16)
    mmask[:, 0:4] = float("-inf")

    def head(x):
        return layer_norm(x, sd, "layernorm", 1e-5)
    pred_ng = linear(head(_decoder(ng_x + ope, ng_cond, sd, depth, H, tgt_mask=cmask)), sd, "action_head")
    pred_mg = linear(head(_decoder(mg_x + ope, mg_cond, sd, depth, H, tgt_mask=cmask)), sd, "action_head")
    cr_label = linear(head(_decoder(label_embed + ope, ng_cond, sd, depth, H, memory_mask=mmask)).mean(dim=1), sd, "critic_head")[:, 0]
    cr_aug = linear(head(_decoder(augment_embed + ope, ng_cond, sd, depth, H, memory_mask=mmask)).mean(dim=1), sd, "critic_head")[:, 0]
    # NavDPTrainer.compute_loss (navdp_trainer.py:80-101)
    ng_loss = (pred_ng - draws["ng_noise"].float()).square().mean()
    mg_loss = (pred_mg - draws["mg_noise"].float()).square().mean()
    aux_loss = 0.5 * (pg - image_aux).square().mean() + 0.5 * (pg - pixel_aux).square().mean()
    critic_loss = (cr_label - batch["batch_label_critic"].float()).square().mean() + (cr_aug - batch["batch_augment_critic"].float()).square().mean()
    loss = 0.8 * (0.5 * mg_loss + 0.5 * ng_loss) + 0.2 * critic_loss + 0.5 * aux_loss
    return dict(loss=loss, ng_action_loss=ng_loss, mg_action_loss=mg_loss, critic_loss=critic_loss, aux_loss=aux_loss,
                pred_ng=pred_ng, pred_mg=pred_mg, critic=cr_label, augment=cr_aug, image_aux=image_aux, pixel_aux=pixel_aux)


def oracle_grads(sd: Dict[str, torch.Tensor], batch, draws, cfg):
    """(loss terms as floats, {name: fp32 gradient}) of the composed step; tensors that get no gradient are absent."""
    leaves = {k: v.detach().float().clone().requires_grad_(".rgb_model." not in k) for k, v in sd.items()}
    out = navdpnet_train_loss(leaves, batch, draws, cfg)
    out["loss"].backward()
    terms = {k: out[k].item() for k in LOSS_TERMS}
    return terms, {k: v.grad for k, v in leaves.items() if v.grad is not None}


def synthetic_batch(B: int, seed: int, pixel_channel: int, cfg) -> Dict[str, torch.Tensor]:
    """seeded navdp_collate_fn batch at the collate shapes: images 0..1, depth in metres, trajectories, critic labels."""
    g = torch.Generator().manual_seed(seed)
    M, Tn = cfg["memory_size"], cfg["predict_size"]
    return dict(batch_pg=torch.randn(B, 3, generator=g) * torch.tensor([3.0, 3.0, 0.5]),
                batch_ig=torch.rand(B, 224, 224, 6, generator=g),
                batch_tg=torch.cat([(torch.rand(B, 224, 224, 1, generator=g) > 0.9).float(),
                                    torch.rand(B, 224, 224, pixel_channel - 1, generator=g)], dim=-1),
                batch_rgb=torch.rand(B, M, 224, 224, 3, generator=g),
                batch_depth=torch.rand(B, 224, 224, 1, generator=g) * 5.0,
                batch_labels=torch.cumsum(torch.randn(B, Tn, 3, generator=g) * 0.1, dim=1),
                batch_augments=torch.cumsum(torch.randn(B, Tn, 3, generator=g) * 0.1, dim=1),
                batch_label_critic=torch.randn(B, generator=g),
                batch_augment_critic=torch.randn(B, generator=g))


def synthetic_draws(B: int, seed: int, cfg) -> Dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    Tn, K = cfg["predict_size"], cfg["num_train_timesteps"]
    return dict(ng_noise=torch.randn(B, Tn, 3, generator=g), ng_t=torch.randint(0, K, (B,), generator=g),
                mg_noise=torch.randn(B, Tn, 3, generator=g), mg_t=torch.randint(0, K, (B,), generator=g))
