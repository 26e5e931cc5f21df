"""Write tests/golden/navdp_train.pt by executing the reference's own NavDPNet training forward + loss + autograd on CPU.

Run where the reference tree is available (the same place as `python -m oracle.make_golden`):  python tools/make_golden_navdp_train.py

For pixel_channel 4 (the train config's value) and 7 (the dataset default) the reference NavDPNet is built through
`oracle.ref_loader` exactly as `oracle.make_golden.gold_navdpnet` builds it, loaded strictly with
`synthetic.navdpnet_train_state_dict`, run in eval() (dropout off) on a seeded B = 3 navdp_collate_fn batch with the two
`sample_noise` draws injected (torch.randn / torch.randint answer from the seeded draws while forward runs), and the loss of
NavDPTrainer.compute_loss (navdp_trainer.py:80-101: the method itself imports psutil / transformers and synchronises CUDA, so its
formula is restated here) is back-propagated. Stored: the seeds, the five loss terms, the gradient norm of every parameter, the first
SLICE elements of the gradients of a chosen subset, the reference's state-dict keys, the parameters that require a gradient and the
decay-group names of its optimiser (internnav/trainer/base.py:48-66: HF get_parameter_names(model, [nn.LayerNorm]) minus 'bias').
The fp32 restatement of tests/navdp_train_ref.py is evaluated on the same inputs and its largest relative deviation is recorded.
"""
from __future__ import annotations

import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from internnav_amd import synthetic as S  # noqa: E402
from oracle import ref_loader as R  # noqa: E402
from oracle.make_golden import _load_strict  # noqa: E402
from tests import navdp_train_ref as O  # noqa: E402

OUT = ROOT / "tests" / "golden" / "navdp_train.pt"
B, WEIGHT_SEED, BATCH_SEED, DRAW_SEED = 3, 5, 11, 13
SLICE = 1024
GRAD_SUBSET = ("image_encoder.project_layer.weight", "image_encoder.project_layer.bias", "pixel_encoder.project_layer.weight",
               "pixel_encoder.project_layer.bias", "image_aux_head.weight", "image_aux_head.bias", "pixel_aux_head.weight",
               "pixel_aux_head.bias", "critic_head.weight", "critic_head.bias", "action_head.weight", "action_head.bias",
               "input_embed.weight", "input_embed.bias", "point_encoder.weight", "point_encoder.bias", "out_pos_embed.position_embedding.weight",
               "cond_pos_embed.position_embedding.weight", "layernorm.weight", "rgbd_encoder.project_layer.weight",
               "image_encoder.imagegoal_encoder.patch_embed.proj.weight", "pixel_encoder.pixelgoal_encoder.patch_embed.proj.weight",
               "rgbd_encoder.depth_model.patch_embed.proj.weight") + tuple(
    f"decoder.layers.7.{n}" for n in ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "multihead_attn.in_proj_weight",
                                      "multihead_attn.in_proj_bias", "multihead_attn.out_proj.bias", "linear1.weight", "linear2.bias", "norm1.weight",
                                      "norm2.bias", "norm3.weight"))


def parameter_names(model, forbidden) -> list:
    """transformers.trainer_pt_utils.get_parameter_names: names of the parameters not inside a `forbidden` module."""
    out = []
    for name, child in model.named_children():
        out += [f"{name}.{n}" for n in parameter_names(child, forbidden) if not isinstance(child, tuple(forbidden))]
    out += list(model._parameters.keys())
    return out


def build(pixel_channel: int):
    torch_load = torch.load
    torch.load = lambda *a, **k: {}
    try:
        npm = R.navdp_policy_module()
        cfg = S.NAVDPNET_CFG
        il = dict(image_size=224, memory_size=cfg["memory_size"], predict_size=cfg["predict_size"], pixel_channel=pixel_channel,
                  temporal_depth=cfg["temporal_depth"], heads=cfg["heads"], channels=3, dropout=0.1,
                  token_dim=cfg["token_dim"], scratch=False, finetune=False)
        net = npm.NavDPNet(npm.NavDPModelConfig(model_cfg={"model": {}, "local_rank": 0, "il": il}))
    finally:
        torch.load = torch_load
    sd = S.navdpnet_train_state_dict(seed=WEIGHT_SEED, pixel_channel=pixel_channel)
    net = _load_strict(net, sd)                              # every reference parameter has a synthetic counterpart
    net._device = torch.device("cpu")
    net.cond_critic_mask = net.cond_critic_mask.float()
    return net, sd


def run(pixel_channel: int) -> dict:
    cfg = S.NAVDPNET_CFG
    net, sd = build(pixel_channel)
    batch = O.synthetic_batch(B, BATCH_SEED, pixel_channel, cfg)
    draws = O.synthetic_draws(B, DRAW_SEED, cfg)
    queue_n = [draws["ng_noise"], draws["mg_noise"]]
    queue_t = [draws["ng_t"], draws["mg_t"]]
    randn, randint = torch.randn, torch.randint
    torch.randn = lambda *a, **k: queue_n.pop(0).clone()
    torch.randint = lambda *a, **k: queue_t.pop(0).clone()
    try:
        outs = net(batch["batch_pg"], batch["batch_ig"], batch["batch_tg"], batch["batch_rgb"], batch["batch_depth"], batch["batch_labels"],
                   batch["batch_augments"])
    finally:
        torch.randn, torch.randint = randn, randint
    assert not queue_n and not queue_t, "sample_noise did not consume both draws"
    pred_ng, pred_mg, cr, aug, ng_noise, mg_noise, img_aux, pix_aux = outs
    pg = batch["batch_pg"]
    # NavDPTrainer.compute_loss, navdp_trainer.py:80-101
    ng_loss = (pred_ng - ng_noise).square().mean()
    mg_loss = (pred_mg - mg_noise).square().mean()
    aux_loss = 0.5 * (pg - img_aux).square().mean() + 0.5 * (pg - pix_aux).square().mean()
    critic_loss = (cr - batch["batch_label_critic"]).square().mean() + (aug - batch["batch_augment_critic"]).square().mean()
    loss = 0.8 * (0.5 * mg_loss + 0.5 * ng_loss) + 0.2 * critic_loss + 0.5 * aux_loss
    loss.backward()
    params = dict(net.named_parameters())
    terms = dict(loss=loss.item(), ng_action_loss=ng_loss.item(), mg_action_loss=mg_loss.item(), critic_loss=critic_loss.item(),
                 aux_loss=aux_loss.item())
    norms = {k: p.grad.norm().item() for k, p in params.items() if p.grad is not None}
    slices = {k: params[k].grad.detach().flatten()[:SLICE].clone() for k in GRAD_SUBSET}
    decay = [n for n in parameter_names(net, [torch.nn.LayerNorm]) if "bias" not in n]
    # the oracle restatement on the same inputs
    o_terms, o_grads = O.oracle_grads(sd, batch, draws, cfg)
    dev = max(abs(o_terms[k] - terms[k]) / abs(terms[k]) for k in terms)
    gdev = max(abs(o_grads[k].norm().item() - norms[k]) / max(norms[k], 1e-30) for k in norms)
    print(f"pixel_channel {pixel_channel}: loss {terms['loss']:.6f}; oracle max rel dev: terms {dev:.2e}, grad norms {gdev:.2e}")
    return dict(terms=terms, grad_norms=norms, grad_slices=slices, keys=list(net.state_dict().keys()),
                requires_grad=[k for k, p in params.items() if p.requires_grad], no_grad=[k for k, p in params.items() if p.requires_grad and p.grad is None],
                decay=decay, oracle_terms_max_rel_dev=dev, oracle_grad_norm_max_rel_dev=gdev)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    out = dict(B=B, weight_seed=WEIGHT_SEED, batch_seed=BATCH_SEED, draw_seed=DRAW_SEED, slice=SLICE, pixel_channel={})
    for pc in (4, 7):
        out["pixel_channel"][pc] = run(pc)
    torch.save(out, OUT)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
