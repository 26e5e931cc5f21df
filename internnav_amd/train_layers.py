"""Model pieces shared by the training heads (sft.py, navdp_train.py), built from the ops of tape.py: the DINOv2 ViT-S tower with
gradients, the nn.Transformer encoder / decoder layers (post-LN and pre-LN), the RGB-D former of the two NavDP heads, and the host-side
sinusoid tables, DDPM schedule, noising and frame mask they use.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import ops
from . import train_ops as T
from .tape import BF, F32, Tape, Var

RESNET_MEAN, RESNET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---------------------------------------------------------------------------------------------------------------- DINOv2 ViT-S
class DinoTrain:
    """DinoVisionTransformer.get_intermediate_layers(x)[0] with gradients (dinov2.py:298-322, block.py:82-107 - the training branch
    equals the eval branch at drop_path 0); patch-embed conv = GEMM on im2col rows, bicubic pos-embed resampling = sparse row mix."""

    D, DEPTH, HEADS, PATCH = 384, 12, 6, 14

    def __init__(self, prefix: str, device, img_size: int = 224, mean=RESNET_MEAN, std=RESNET_STD, channels: int = 3):
        """mean / std: input normalisation fused into the im2col kernel; channels = 1: a depth map replicated to 3 channels
        (navdp_backbone.py:274-279); channels = 4 / 6 / 7: a C-channel patch-embed conv (the goal encoders of NavDPNet,
        navdp_backbone.py:316-412), identity normalisation only. Parameters are looked up on the tape (trainable or frozen store)."""
        assert channels in (1, 3, 4, 6, 7), f"DinoTrain: {channels} input channels"
        assert channels <= 3 or (tuple(mean) == (0.0, 0.0, 0.0) and tuple(std) == (1.0, 1.0, 1.0)), "C > 3 takes no normalisation"
        self.p, self.mean, self.std, self.channels = prefix, mean, std, channels
        self.K = max(channels, 3) * self.PATCH * self.PATCH        # im2col columns of the conv weight [384, max(C, 3), 14, 14]
        self.KPAD = (self.K + 7) // 8 * 8                          # 592 for C = 1 / 3
        g = img_size // self.PATCH
        self.L = g * g
        # the interpolation is linear in pos_embed: recover its sparse matrix once by resampling an identity basis on the host
        import torch.nn.functional as Fn
        n_src = 37
        w0 = g + 0.1
        eye = torch.eye(n_src * n_src, dtype=torch.float32).view(n_src * n_src, 1, n_src, n_src)
        A = Fn.interpolate(eye, scale_factor=(w0 / n_src, w0 / n_src), mode="bicubic", antialias=False)    # [1369, 1, g, g]
        A = A.view(n_src * n_src, self.L).t().contiguous()                                                  # [L, 1369]
        self.fwd_idx, self.fwd_coef = self._ell(A, device)
        self.bwd_idx, self.bwd_coef = self._ell(A.t().contiguous(), device)

    @staticmethod
    def _ell(A: torch.Tensor, device):
        nz = (A != 0)
        taps = int(nz.sum(1).max().item())
        idx = torch.full((A.shape[0], taps), -1, dtype=torch.int32)
        coef = torch.zeros(A.shape[0], taps, dtype=torch.float32)
        for r in range(A.shape[0]):
            c = nz[r].nonzero().flatten()
            idx[r, :c.numel()] = c.to(torch.int32)
            coef[r, :c.numel()] = A[r, c]
        return idx.to(device), coef.to(device)

    def forward(self, tape: Tape, frames: torch.Tensor) -> Var:
        """frames [n, 224, 224, C] -> Var [n * 256, 384] f32 patch tokens after the final LayerNorm (cls dropped)."""
        P, p, D, L = tape.P, self.p, self.D, self.L
        n = frames.shape[0]
        dev = frames.device
        Tt = L + 1
        assert frames.shape[-1] == self.channels
        patches = torch.empty(n * L, self.KPAD, dtype=BF, device=dev)
        ops.patchify(frames.contiguous(), patches, self.mean, self.std, self.PATCH)
        wname = p + "patch_embed.proj.weight"
        train = P.trains(wname)
        wpad = torch.zeros(D, self.KPAD, dtype=BF, device=dev)
        wpad[:, :self.K] = P.w16(wname).view(D, self.K)
        pos_src = P.w32(p + "pos_embed").view(-1, D)                                   # [1370, 384]
        pos = T.sparse_rows(pos_src[1:].contiguous(), self.fwd_idx, self.fwd_coef)     # [L, 384] f32
        x = torch.empty(n, Tt, D, dtype=F32, device=dev)
        ops.linear(patches.view(n, L, self.KPAD), wpad, bias=P.w32(p + "patch_embed.proj.bias"), residual=pos, out=x[:, 1:, :], batched=True)
        x[:, 0, :] = P.w32(p + "cls_token").view(1, D) + pos_src[:1]
        xv = x_embed = Var(x.view(n * Tt, D), req=train)

        def bwd_embed():
            dx = x_embed.g
            if dx is None:
                return
            d3 = dx.view(n, Tt, D)
            dtok = tape.bf16(d3[:, 1:, :].reshape(n * L, D))
            gw = torch.zeros(D, self.KPAD, dtype=F32, device=dev)
            ops.linear(T.transpose(dtok), T.transpose(patches), out=gw, residual=gw)
            P.grad(wname).view(D, self.K).add_(gw[:, :self.K])
            T.colsum(dtok, out=P.grad(p + "patch_embed.proj.bias"), accumulate=True)
            dpos_all = T.colsum(d3.reshape(n, Tt * D)).view(Tt, D)                     # summed over the frames
            gpos = P.grad(p + "pos_embed").view(-1, D)
            gpos[:1] += dpos_all[:1]
            P.grad(p + "cls_token").view(1, D).add_(dpos_all[:1])
            T.sparse_rows(dpos_all[1:].contiguous(), self.bwd_idx, self.bwd_coef, out=gpos[1:], accumulate=True)
        if train:
            tape.nodes.append(bwd_embed)

        for i in range(self.DEPTH):
            b = f"{p}blocks.{i}"
            h = tape.norm(xv, b + ".norm1.weight", b + ".norm1.bias", 1e-6)
            qkv = tape.linear(h, b + ".attn.qkv.weight", b + ".attn.qkv.bias")
            att = tape.attention((qkv, 0), (qkv, D), (qkv, 2 * D), n, Tt, Tt, self.HEADS, D // self.HEADS)
            y = tape.linear(att, b + ".attn.proj.weight", b + ".attn.proj.bias")
            xv = tape.col_scale(y, b + ".ls1.gamma", base=xv)
            h = tape.norm(xv, b + ".norm2.weight", b + ".norm2.bias", 1e-6)
            h = tape.act(tape.linear(h, b + ".mlp.fc1.weight", b + ".mlp.fc1.bias"), "gelu_erf")
            y = tape.linear(h, b + ".mlp.fc2.weight", b + ".mlp.fc2.bias")
            xv = tape.col_scale(y, b + ".ls2.gamma", base=xv)
        # fp32 tokens: the consumers add a positional table before their first GEMM rounds to bf16 (one rounding, as bf16-autocast PyTorch)
        out = tape.norm(xv, p + "norm.weight", p + "norm.bias", 1e-6, out_dtype=F32)
        # drop the cls token
        tok = Var(out.v.view(n, Tt, D)[:, 1:, :].reshape(n * L, D), req=out.req)

        def bwd_drop():
            if tok.g is None:
                return
            g = torch.zeros(n, Tt, D, dtype=tok.g.dtype, device=dev)
            g[:, 1:, :] = tok.g.view(n, L, D)
            tape.accumulate(out, g.view(n * Tt, D))
        tape.nodes.append(bwd_drop)
        return tok


# ---------------------------------------------------------------------------------------------------------------- nn.Transformer layers
def _mha(tape: Tape, xq: Var, xkv: Var, p: str, B: int, Lq: int, Lk: int, H: int, d: int, residual: Optional[Var] = None,
         causal: bool = False, attn_dropout: bool = True) -> Var:
    """nn.MultiheadAttention(batch_first=True): packed in_proj, SDPA (+ attention-probability dropout when the tape trains with dropout),
    out_proj, then the surrounding layer's dropout + residual (fp32 sum; fused into the out_proj epilogue when there is no dropout).
    attn_dropout=False: a module built WITHOUT dropout (nn.MultiheadAttention's default 0.0, e.g. TokenCompressor.cross_attention,
    encoder/navdp_backbone.py:77) - the nn.Transformer layers pass their own p to their attention modules, that one does not."""
    w, b = p + ".in_proj_weight", p + ".in_proj_bias"
    if xq is xkv:
        qkv = tape.linear(xq, w, b)
        att = tape.attention((qkv, 0), (qkv, d), (qkv, 2 * d), B, Lq, Lk, H, d // H, causal=causal, dropout=attn_dropout)
    else:
        qp = tape.linear(xq, w, b, rows=(0, d))
        kvp = tape.linear(xkv, w, b, rows=(d, 3 * d))
        att = tape.attention((qp, 0), (kvp, 0), (kvp, d), B, Lq, Lk, H, d // H, causal=causal, dropout=attn_dropout)
    if residual is None or tape.drop_p <= 0.0:
        return tape.linear(att, p + ".out_proj.weight", p + ".out_proj.bias", residual=residual, out_dtype=F32 if residual is not None else None)
    return tape.add(residual, tape.dropout(tape.linear(att, p + ".out_proj.weight", p + ".out_proj.bias")))


def _ffn(tape: Tape, x: Var, p: str, act: str, residual: Var) -> Var:
    """linear2(dropout(act(linear1 x))) -> dropout -> + residual (torch/nn/modules/transformer.py _ff_block + dropout2 / dropout3)."""
    h = tape.dropout(tape.act(tape.linear(x, p + ".linear1.weight", p + ".linear1.bias"), act))
    if tape.drop_p <= 0.0:
        return tape.linear(h, p + ".linear2.weight", p + ".linear2.bias", residual=residual, out_dtype=F32)
    return tape.add(residual, tape.dropout(tape.linear(h, p + ".linear2.weight", p + ".linear2.bias")))


def encoder_layer(tape: Tape, x: Var, p: str, B: int, L: int, H: int, d: int) -> Var:
    """nn.TransformerEncoderLayer(batch_first=True, norm_first=False, activation=relu); dropout sites follow tape.drop_p. The post-LN
    stream stays fp32 between the sub-layers (the LayerNorm output is the next residual base; bf16-autocast PyTorch keeps it in fp32 too)."""
    x = tape.norm(_mha(tape, x, x, p + ".self_attn", B, L, L, H, d, residual=x), p + ".norm1.weight", p + ".norm1.bias", 1e-5, out_dtype=F32)
    return tape.norm(_ffn(tape, x, p, "relu", x), p + ".norm2.weight", p + ".norm2.bias", 1e-5, out_dtype=F32)


def decoder_layer(tape: Tape, x: Var, mem: Var, p: str, B: int, Lq: int, Lm: int, H: int, d: int) -> Var:
    """nn.TransformerDecoderLayer(batch_first=True, norm_first=False, activation=relu), no masks; dropout sites follow tape.drop_p.
    fp32 post-LN stream as in encoder_layer (round 4: a bf16 stream here put the RGB-D condition tokens 1.4x further from fp32 than
    bf16-autocast PyTorch, and every one of the 16 decoder layers re-reads them)."""
    x = tape.norm(_mha(tape, x, x, p + ".self_attn", B, Lq, Lq, H, d, residual=x), p + ".norm1.weight", p + ".norm1.bias", 1e-5, out_dtype=F32)
    x = tape.norm(_mha(tape, x, mem, p + ".multihead_attn", B, Lq, Lm, H, d, residual=x), p + ".norm2.weight", p + ".norm2.bias", 1e-5, out_dtype=F32)
    return tape.norm(_ffn(tape, x, p, "relu", x), p + ".norm3.weight", p + ".norm3.bias", 1e-5, out_dtype=F32)


def decoder_layer_prenorm(tape: Tape, x: Var, mem: Var, p: str, B: int, Lq: int, Lm: int, H: int, d: int, causal: bool) -> Var:
    """nn.TransformerDecoderLayer(batch_first=True, norm_first=True, activation='gelu'), causal tgt_mask, no memory mask; dropout sites
    follow tape.drop_p; x is the fp32 residual stream."""
    h = tape.norm(x, p + ".norm1.weight", p + ".norm1.bias", 1e-5)
    x = _mha(tape, h, h, p + ".self_attn", B, Lq, Lq, H, d, residual=x, causal=causal)
    h = tape.norm(x, p + ".norm2.weight", p + ".norm2.bias", 1e-5)
    x = _mha(tape, h, mem, p + ".multihead_attn", B, Lq, Lm, H, d, residual=x)
    h = tape.norm(x, p + ".norm3.weight", p + ".norm3.bias", 1e-5)
    return _ffn(tape, h, p, "gelu_erf", x)


def rgbd_former(tape: Tape, tok: Var, n: int, Lf: int, Lm: int, pe_name: str, query_name: str, prefix: str = "rgbd_encoder.") -> Var:
    """the former of the NavDP RGB-D backbones (navdp_backbone.py:248-286): n sequences of Lf RGB | depth patch tokens + the `pe_name`
    table -> Lm learned queries (`query_name`) through two post-LN decoder layers -> project_layer, bf16 [n*Lm, token_dim]."""
    P = tape.P
    tok = tape.add_table(tok, prefix + pe_name, Lf)
    q = tape.broadcast_param(P.w32(prefix + query_name), [P.grad(prefix + query_name)], n)
    for i in range(2):
        q = decoder_layer(tape, q, tok, f"{prefix}former_net.layers.{i}", n, Lm, Lf, 8, 384)
    return tape.linear(q, prefix + "project_layer.weight", prefix + "project_layer.bias")


# ---------------------------------------------------------------------------------------------------------------- host-side tables, noise, masks
def timestep_embedding(t: torch.Tensor, dim: int = 256) -> torch.Tensor:
    """diffusers Timesteps(256, flip_sin_to_cos=True, downscale_freq_shift=0): [cos | sin] of t * 10000^(-i/128)."""
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=F32, device=t.device) / half)
    a = t[:, None].float() * freqs[None]
    return torch.cat([torch.cos(a), torch.sin(a)], dim=-1)


def sinusoidal_positions(Tn: int, dim: int, device) -> torch.Tensor:
    """SinusoidalPositionalEncoding(dim)(arange(T)) (internvla_n1_arch.py:50-73)."""
    half = dim // 2
    exponent = -torch.arange(half, dtype=F32, device=device) * (torch.log(torch.tensor(10000.0)) / half)
    freqs = torch.arange(Tn, dtype=F32, device=device).unsqueeze(-1) * exponent.exp()
    return torch.cat([torch.sin(freqs), torch.cos(freqs)], dim=-1).contiguous()


def ddpm_alphas_cumprod(num_train_timesteps: int) -> torch.Tensor:
    """diffusers DDPMScheduler(beta_schedule='squaredcos_cap_v2'): betas_for_alpha_bar (cosine, max_beta 0.999) -> cumprod(1 - beta), fp32."""
    def alpha_bar(t):
        return math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2
    betas = [min(1 - alpha_bar((i + 1) / num_train_timesteps) / alpha_bar(i / num_train_timesteps), 0.999) for i in range(num_train_timesteps)]
    return torch.cumprod(1.0 - torch.tensor(betas, dtype=F32), dim=0)


def sinusoidal_pos_emb(x: torch.Tensor, dim: int) -> torch.Tensor:
    """SinusoidalPosEmb (navdp_backbone.py:9-21)."""
    half = dim // 2
    e = torch.exp(torch.arange(half, dtype=F32, device=x.device) * -(math.log(10000) / (half - 1)))
    e = x[:, None].float() * e[None, :]
    return torch.cat((e.sin(), e.cos()), dim=-1)


def ddpm_add_noise(acp: torch.Tensor, ts: torch.Tensor, x: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
    """DDPMScheduler.add_noise: sqrt(acp[t]) * x + sqrt(1 - acp[t]) * noise per sequence; acp f32 [K], ts int64 [n], x / noise [n, T, 3]."""
    a = acp[ts].view(-1, 1, 1)
    return a.sqrt() * x + (1 - a).sqrt() * noise


def frame_mask(Tn: int, video_frame_num: torch.Tensor, dev) -> torch.Tensor:
    """f32 [B*Tn]: 1 for the sub-goal frames a sample really has (t < video_frame_num[b]), 0 for its padding."""
    return (torch.arange(Tn, device=dev)[None, :] < video_frame_num.to(dev)[:, None]).to(F32).reshape(-1).contiguous()
