"""Training step of the standalone NavDPNet (BASELINE config #2) on the gfx950 kernels: NavDPTrainer parity.

What the reference does (internnav/trainer/navdp_trainer.py:80-101 with NavDPNet.forward, navdp_policy.py:187-273, launched by
scripts/train/base_train/train.py with model_name='navdp'): per navdp_collate_fn micro-batch, the RGB-D memory tokens (frozen RGB ViT-S,
trainable depth ViT-S, 2-layer post-LN former), the image-goal / pixel-goal ViT-S encoders (6- and pixel_channel-channel patch embeds,
mean over the patch tokens), the point-goal Linear, two DDPM noise draws (ng: no goal, mg: goal slots by the `b % 27` pattern), four passes
of the 16-layer pre-LN decoder (ng / mg causal; the two critic passes over the label / augment trajectories with the 4 time / goal slots of
the ng condition hidden), the action / critic / aux heads and the weighted MSE sum; then adamw_torch (lr 1e-4, cosine to 0, no warmup,
clip 1.0, weight decay 0 unless set - with HF's no-decay group for LayerNorm parameters and biases).

This module is that step on the define-by-run tape of `tape.py` and the layers of `train_layers.py` (the kernels of libinternnav_amd.so; torch for allocation, views, index
tables and RNG draws only). The passes that share weights are batched: ng and mg are 2B causal sequences of one decoder run, the two critic
passes 2B sequences of another, whose memory is the ng condition from row 4 on (the reference's -inf memory mask on slots 0..3) tiled twice.

Differences from the reference's execution: bf16 GEMM / attention operands against its fp32 training (fp32 master weights, gradients, Adam
moments, residual streams and accumulation); dropout masks come from the tape's counter hash (the same distribution, other draws); the RGB
ViT-S runs without a tape (frozen, finetune=False - finetune=True is refused).
"""
from __future__ import annotations

import math
import re
from typing import Dict, Iterable, List, Optional

import torch

from . import train_ops as T
from .tape import F32, ParamStore, Tape, Var
from .train_layers import (RESNET_MEAN, RESNET_STD, DinoTrain, ddpm_add_noise, ddpm_alphas_cumprod, decoder_layer_prenorm, rgbd_former,
                           sinusoidal_pos_emb)
from .synthetic import NAVDPNET_CFG

IDENTITY = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
LOSS_TERMS = ("loss", "ng_action_loss", "mg_action_loss", "critic_loss", "aux_loss")
_LAYERNORM_PARAM = re.compile(r"(^|\.)(norm\d*|layernorm)\.(weight|bias)$")


# ---------------------------------------------------------------------------------------------------------------- host-side plan
def param_plan(keys: Iterable[str], finetune: bool = False) -> Dict[str, str]:
    """name -> 'trainable' | 'frozen' | 'untouched' for the NavDPNet state-dict keys. frozen: the RGB ViT-S (requires_grad=False when
    finetune=False, navdp_policy.py:93-96); untouched: the DINOv2 `mask_token`s of the trained towers - they require a gradient but are
    never read by get_intermediate_layers, so torch.optim.AdamW skips them (no update, no decay)."""
    if finetune:
        raise NotImplementedError("NavDPNet with finetune=True (a trainable RGB ViT-S) is not supported by this trainer; train with finetune=False")
    plan = {}
    for k in keys:
        if k.startswith("rgbd_encoder.rgb_model."):
            plan[k] = "frozen"
        elif k.endswith("mask_token"):
            plan[k] = "untouched"
        else:
            plan[k] = "trainable"
    return plan


def decay_names(keys: Iterable[str]) -> List[str]:
    """the decay group of internnav/trainer/base.py:48-66 (get_parameter_names(model, [nn.LayerNorm]) minus names containing 'bias'):
    in NavDPNet every LayerNorm module is named norm, norm<i> or layernorm."""
    return [k for k in keys if not _LAYERNORM_PARAM.search(k) and "bias" not in k]


def goal_slot_table(B: int) -> torch.Tensor:
    """int64 [B, 3]: the candidate (0 point, 1 image, 2 pixel goal) of goal slot j of sample b, (b % 27 // 3^j) % 3
    (navdp_policy.py:222-232)."""
    b = torch.arange(B) % 27
    return torch.stack([b // 3 ** j % 3 for j in range(3)], dim=1)


def cosine_lr(lr: float, step: int, total_steps: Optional[int]) -> float:
    """HF get_cosine_schedule_with_warmup(0 warmup steps): lr * 0.5 * (1 + cos(pi * step / total_steps)) for the step-th update
    (0-based); total_steps None = constant lr."""
    if not total_steps:
        return lr
    return lr * max(0.0, 0.5 * (1.0 + math.cos(math.pi * step / total_steps)))


# ---------------------------------------------------------------------------------------------------------------- tape helpers
def _critic_memory(tape: Tape, cond: Var, B: int, Lc: int, first: int) -> Var:
    """rows first..Lc-1 of the B ng condition sequences (the first B*Lc rows of cond), tiled for the label and the augment pass:
    [2B * (Lc - first), C]. The reference's memory mask (-inf on slots 0..first-1, navdp_policy.py:130-131) as a K/V view."""
    Cd = cond.v.shape[1]
    Lm = Lc - first
    src = cond.v[: B * Lc].view(B, Lc, Cd)[:, first:]
    y = Var(src.unsqueeze(0).expand(2, B, Lm, Cd).reshape(2 * B * Lm, Cd), req=cond.req)

    def bwd():
        if y.g is None:
            return
        g = torch.zeros(cond.v.shape, dtype=F32, device=cond.v.device)
        g[: B * Lc].view(B, Lc, Cd)[:, first:] = y.g.float().view(2, B, Lm, Cd).sum(0)
        tape.accumulate(cond, g)
    tape.nodes.append(bwd)
    return y


# ---------------------------------------------------------------------------------------------------------------- the loss
class NavDPNetTrainHead:
    """Loss + gradients of NavDPNet.forward + NavDPTrainer.compute_loss for one micro-batch. Parameters: a flat trainable store (decay
    group first, then the no-decay group), a frozen store (the RGB ViT-S) and the untouched `mask_token`s held on the host."""

    def __init__(self, sd: Dict[str, torch.Tensor], device, cfg=NAVDPNET_CFG, pixel_channel: Optional[int] = None, dropout: float = 0.0,
                 finetune: bool = False):
        plan = param_plan(sd.keys(), finetune)
        if pixel_channel is None:
            pixel_channel = int(sd["pixel_encoder.pixelgoal_encoder.patch_embed.proj.weight"].shape[1])
        assert pixel_channel in (4, 7), f"pixel_channel {pixel_channel}: the reference uses 4 (train config) or 7 (dataset default)"
        self.keys = list(sd.keys())
        self.plan = plan
        decay = set(decay_names(self.keys))
        trainable = [k for k in self.keys if plan[k] == "trainable"]
        order = [k for k in trainable if k in decay] + [k for k in trainable if k not in decay]
        self.P = ParamStore({k: sd[k] for k in order}, device)
        n_decay = sum(1 for k in trainable if k in decay)
        self.decay_end = self.P.index[order[n_decay]][0] if n_decay < len(order) else self.P.numel      # flat [0, decay_end) decays
        self.F = ParamStore({k: sd[k] for k in self.keys if plan[k] == "frozen"}, device, trainable=False)
        self.untouched = {k: sd[k].detach().float().cpu().clone() for k in self.keys if plan[k] == "untouched"}
        self.device, self.cfg, self.dropout, self.pixel_channel = device, cfg, dropout, pixel_channel
        self.rgb = DinoTrain("rgbd_encoder.rgb_model.", device, mean=RESNET_MEAN, std=RESNET_STD)       # fp32 constants, navdp_backbone.py:233-234
        self.depth = DinoTrain("rgbd_encoder.depth_model.", device, mean=IDENTITY[0], std=IDENTITY[1], channels=1)
        self.image = DinoTrain("image_encoder.imagegoal_encoder.", device, mean=IDENTITY[0], std=IDENTITY[1], channels=6)
        self.pixel = DinoTrain("pixel_encoder.pixelgoal_encoder.", device, mean=IDENTITY[0], std=IDENTITY[1], channels=pixel_channel)
        self.acp = ddpm_alphas_cumprod(cfg["num_train_timesteps"]).to(device)

    def _goal(self, tape: Tape, dino: DinoTrain, img: torch.Tensor, p: str) -> Var:
        """ImageGoalBackbone / PixelGoalBackbone.forward: mean over the 256 patch tokens, project_layer -> f32 [B, D]."""
        tok = dino.forward(tape, img.to(device=self.device, dtype=F32).contiguous())
        return tape.linear(tape.mean_tokens(tok, dino.L), p + "project_layer.weight", p + "project_layer.bias", out_dtype=F32)

    def loss_and_grads(self, batch: Dict[str, torch.Tensor], draws: Dict[str, torch.Tensor], seed: int = 0,
                       loss_scale: float = 1.0) -> Dict[str, torch.Tensor]:
        """batch: the navdp_collate_fn dict; draws: ng_noise / mg_noise f32 [B, T, 3], ng_t / mg_t int [B] (the two sample_noise draws).
        Gradients (times loss_scale) are ACCUMULATED into the store; returns the five loss terms of compute_loss as f32 [1] device tensors."""
        P, dev, cfg = self.P, self.device, self.cfg
        D, H, M, Tn = cfg["token_dim"], cfg["heads"], cfg["memory_size"], cfg["predict_size"]
        Lm, Lc, Lf = M * 16, M * 16 + 4, (M + 1) * 256
        labels = batch["batch_labels"].to(device=dev, dtype=F32)
        B = labels.shape[0]
        assert labels.shape[1] == Tn and batch["batch_rgb"].shape[1] == M, "batch shapes do not match the model config"
        tape = Tape(P, self.F, drop_p=self.dropout, seed=seed)
        ones = torch.ones(B, dtype=F32, device=dev)
        pg = batch["batch_pg"].to(device=dev, dtype=F32).contiguous()

        # ---- rgbd_encoder (navdp_backbone.py:248-286): frozen RGB tokens, trainable depth tokens, former_net, project_layer
        rgb = self.rgb.forward(tape, batch["batch_rgb"].to(dev).reshape(B * M, *batch["batch_rgb"].shape[2:]))
        dep = self.depth.forward(tape, batch["batch_depth"].to(device=dev, dtype=F32).reshape(B, 224, 224, 1))
        rgbd = rgbd_former(tape, tape.cat_tokens([(rgb, M * 256), (dep, 256)], B), B, Lf, Lm, "former_pe.position_embedding.weight",
                           "former_query.position_embedding.weight")                                            # bf16 [B*Lm, D]

        # ---- goal embeddings and aux heads (Linear(D, 3) on a goal embedding, 0.25-weighted MSE against the point goal)
        point = tape.small_linear(pg, "point_encoder")                                                           # f32 [B, D]
        image = self._goal(tape, self.image, batch["batch_ig"], "image_encoder.")
        pixel = self._goal(tape, self.pixel, batch["batch_tg"], "pixel_encoder.")
        l_img, = tape.mse_head(image, "image_aux_head", pg, ones, 1, 0.25 * loss_scale)
        l_pix, = tape.mse_head(pixel, "pixel_aux_head", pg, ones, 1, 0.25 * loss_scale)

        # ---- conditions of the 2B noise passes [ng b = 0..B-1 | mg b = 0..B-1]: [time, 3 goal slots, rgbd] + cond_pos_embed, self.drop
        gi = (goal_slot_table(B) * B + torch.arange(B)[:, None]).reshape(-1).to(dev)                            # rows of [point; image; pixel]
        cand = torch.cat([point.v, image.v, pixel.v])
        ts = torch.cat([draws["ng_t"], draws["mg_t"]]).to(dev).long()
        head = torch.zeros(2 * B, 4, D, dtype=F32, device=dev)
        head[:, 0] = sinusoidal_pos_emb(ts, D)
        head[B:, 1:] = cand[gi].view(B, 3, D)
        hd = Var(head.view(2 * B * 4, D))

        def bwd_goals():
            if hd.g is None:
                return
            g = torch.zeros(3 * B, D, dtype=F32, device=dev)
            g.index_add_(0, gi, hd.g.float().view(2 * B, 4, D)[B:, 1:].reshape(3 * B, D))
            for i, var in enumerate((point, image, pixel)):
                tape.accumulate(var, g[i * B:(i + 1) * B].clone())
        tape.nodes.append(bwd_goals)
        cond = tape.cat_tokens([(hd, 4), (tape.repeat_seq(rgbd, 1, B * Lm, 2), Lm)], 2 * B)         # the rgbd block once per noise pass
        cond = tape.dropout(tape.add_table(cond, "cond_pos_embed.position_embedding.weight", Lc))                  # f32 [2B*Lc, D]

        # ---- action embeddings [ng | mg | label | augment] (label / augment: input_embed detached), + out_pos_embed, self.drop
        lab = labels.reshape(B, Tn, 3)
        aug = batch["batch_augments"].to(device=dev, dtype=F32).reshape(B, Tn, 3)
        noise = torch.cat([draws["ng_noise"], draws["mg_noise"]]).to(device=dev, dtype=F32).reshape(2 * B, Tn, 3)
        noisy = ddpm_add_noise(self.acp, ts, lab.repeat(2, 1, 1), noise)
        acts = torch.cat([noisy, lab, aug]).reshape(4 * B * Tn, 3).contiguous()
        tab = P.w32("out_pos_embed.position_embedding.weight")[:Tn].contiguous()
        x = Var(T.small_linear(acts, P.w32("input_embed.weight"), P.w32("input_embed.bias"), tab=tab))         # f32 [4B*Tn, D]

        def bwd_embed():
            dy = x.g
            if dy is None:
                return
            dy = dy.float().contiguous()
            n = 2 * B * Tn
            tape.small_linear_grad("input_embed", acts[:n], dy[:n])                  # the label / augment rows are detached
            T.colsum(dy.view(4 * B, Tn * D), out=P.grad("out_pos_embed.position_embedding.weight").view(-1, D)[:Tn].view(1, -1), accumulate=True)
        tape.nodes.append(bwd_embed)
        x = tape.dropout(x)

        # ---- the 16-layer decoder: 2B causal noise sequences, 2B critic sequences over the ng condition rows 4..
        y = tape.rows(x, 0, 2 * B * Tn)
        z = tape.rows(x, 2 * B * Tn, 4 * B * Tn)
        mem_cr = _critic_memory(tape, cond, B, Lc, 4)
        for i in range(cfg["temporal_depth"]):
            y = decoder_layer_prenorm(tape, y, cond, f"decoder.layers.{i}", 2 * B, Tn, Lc, H, D, causal=True)
        for i in range(cfg["temporal_depth"]):
            z = decoder_layer_prenorm(tape, z, mem_cr, f"decoder.layers.{i}", 2 * B, Tn, Lm, H, D, causal=False)

        # ---- heads and losses (navdp_trainer.py:80-101)
        pred = tape.norm(y, "layernorm.weight", "layernorm.bias", 1e-5)                                        # bf16 [2B*Tn, D]
        l_ng, l_mg = tape.mse_head(pred, "action_head", noise.reshape(2 * B * Tn, 3), ones, Tn, 0.4 * loss_scale, blocks=2)

        pc = tape.norm(z, "layernorm.weight", "layernorm.bias", 1e-5, out_dtype=F32)
        pooled = tape.mean_tokens(pc, Tn)                                                                       # f32 [2B, D]
        ct = torch.cat([batch["batch_label_critic"], batch["batch_augment_critic"]]).to(device=dev, dtype=F32).view(2 * B, 1)
        l_cl, l_ca = tape.mse_head(pooled, "critic_head", ct, ones, 1, 0.2 * loss_scale, blocks=2)                 # label | augment

        self.last_dropout_sites = dict(tape.sites)
        tape.backward()
        ng_cr = l_cl + l_ca
        aux = 0.5 * (l_img + l_pix)
        loss = 0.8 * (0.5 * l_mg + 0.5 * l_ng) + 0.2 * ng_cr + 0.5 * aux
        return dict(loss=loss, ng_action_loss=l_ng, mg_action_loss=l_mg, critic_loss=ng_cr, aux_loss=aux)


# ---------------------------------------------------------------------------------------------------------------- the trainer
class NavDPNetTrainer:
    """NavDPTrainer on one device: forward_backward(collate batch) accumulates the gradient of compute_loss, optimizer_step() applies
    adamw_torch with the reference's schedule, clip and decay groups. Data-parallel ranks and hipGraph capture are not part of it."""

    def __init__(self, sd: Dict[str, torch.Tensor], device="cuda:0", cfg=NAVDPNET_CFG, pixel_channel: Optional[int] = None, lr: float = 1e-4,
                 total_steps: Optional[int] = None, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: float = 1.0,
                 dropout: float = 0.1, seed: int = 0, finetune: bool = False):
        """sd: a full NavDPNet state dict (the reference's key names; synthetic.navdpnet_train_state_dict). total_steps: length of the
        cosine schedule (HF max_steps; None = constant lr). dropout: p of every dropout site (the reference's il.dropout, 0.1); 0 gives
        the eval-mode gradient. seed: the noise / time-step generator and the dropout masks."""
        self.head = NavDPNetTrainHead(sd, device, cfg, pixel_channel, dropout, finetune)
        self.P = self.head.P
        self.device, self.cfg, self.seed = device, cfg, seed
        self.lr, self.total_steps, self.weight_decay = lr, total_steps, weight_decay
        self.betas, self.eps, self.max_grad_norm = betas, eps, max_grad_norm
        self.gen = torch.Generator().manual_seed(seed)
        self.step_idx, self.micro_idx = 0, 0
        self.norm = torch.zeros(1, dtype=F32, device=device)

    def draw(self, B: int) -> Dict[str, torch.Tensor]:
        """the two sample_noise draws of one micro-batch (navdp_policy.py:148-157): eps ~ N(0, 1) [B, T, 3], t ~ U{0..K-1} [B]."""
        Tn, K = self.cfg["predict_size"], self.cfg["num_train_timesteps"]
        out = {}
        for p in ("ng", "mg"):
            out[p + "_noise"] = torch.randn(B, Tn, 3, generator=self.gen)
            out[p + "_t"] = torch.randint(0, K, (B,), generator=self.gen)
        return out

    def forward_backward(self, batch: Dict[str, torch.Tensor], draws: Optional[Dict[str, torch.Tensor]] = None,
                         loss_scale: float = 1.0) -> Dict[str, torch.Tensor]:
        """one micro-batch: the loss terms (f32 [1] device tensors: loss, ng_action_loss, mg_action_loss, critic_loss, aux_loss); its gradient
        (times loss_scale, e.g. 1 / accumulation steps) is added to the store. draws: injected noise / time steps (tests)."""
        if draws is None:
            draws = self.draw(batch["batch_labels"].shape[0])
        seed = (self.seed * 1000003 + self.micro_idx) & 0x7FFFFFFF
        self.micro_idx += 1
        return self.head.loss_and_grads(batch, draws, seed=seed, loss_scale=loss_scale)

    def current_lr(self) -> float:
        return cosine_lr(self.lr, self.step_idx, self.total_steps)

    def optimizer_step(self) -> torch.Tensor:
        """clip_grad_norm_(max_grad_norm) over all trainable tensors + torch.optim.AdamW with the decay / no-decay groups, one global norm;
        gradients are zeroed. Returns the pre-clip gradient norm (f32 [1] device tensor)."""
        self.P.adamw_step(self.current_lr(), self.betas, self.eps, self.weight_decay, self.max_grad_norm, norm_out=self.norm,
                          decay_end=self.head.decay_end)
        self.step_idx += 1
        return self.norm

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """every NavDPNet tensor under the reference's names (fp32, CPU): loads into NavDPNet.load_state_dict(strict=True) and into
        the engine's navdp.NavDPNet."""
        out = {}
        for k in self.head.keys:
            if k in self.P.index:
                out[k] = self.P.w32(k).detach().cpu().clone()
            elif k in self.head.F.index:
                out[k] = self.head.F.w32(k).detach().cpu().clone()
            else:
                out[k] = self.head.untouched[k].clone()
        return out

    def checkpoint(self) -> dict:
        """resume point: master weights + Adam moments of the trainable store, step / micro-step counters, generator state."""
        return dict(store=self.P.checkpoint(), step_idx=self.step_idx, micro_idx=self.micro_idx, rng=self.gen.get_state(),
                    pixel_channel=self.head.pixel_channel)

    def save_checkpoint(self, path: str):
        torch.save(self.checkpoint(), path)

    def load_checkpoint(self, ck):
        """ck: a checkpoint() dict or a path written by save_checkpoint."""
        if isinstance(ck, str):
            ck = torch.load(ck, map_location="cpu", weights_only=True)
        if int(ck["pixel_channel"]) != self.head.pixel_channel:
            raise ValueError(f"checkpoint of a pixel_channel={ck['pixel_channel']} model, trainer built for {self.head.pixel_channel}")
        self.P.load_checkpoint(ck["store"])
        self.step_idx, self.micro_idx = int(ck["step_idx"]), int(ck["micro_idx"])
        self.gen.set_state(ck["rng"])
