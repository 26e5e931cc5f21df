"""InternVLA-N1 System-2 (Qwen2.5-VL vision tower + 7B LLM + latent trajectory queries) on the gfx950 op library.

Drop-in for the model surface the reference's callers use:
    model.generate(input_ids, pixel_values, image_grid_thw, max_new_tokens, do_sample=False).sequences
    model.generate_latents(output_ids, pixel_values, image_grid_thw) -> [B, N_QUERY, 3584]
(/root/reference/internnav/model/basemodel/internvla_n1/internvla_n1.py:58-220, 320-347; call sites
internvla_n1_policy.py:169-191, habitat_vln_evaluator.py:418-448), batched over environments (the reference is batch 1).

Arithmetic = transformers Qwen2.5-VL (un-vendored dependency of the reference; restated and pinned in oracle/qwen_vl.py):
  vision: patch-embed GEMM (K = 1176), window permutation, 32 x {RMSNorm, qkv+bias GEMM, 2-D rope, varlen window / per-image
          attention (16 heads x 80), proj GEMM + residual, RMSNorm, SwiGLU GEMM pair + bias}, merger (RMSNorm, 5120->5120 GELU ->3584)
  text:   embedding gather, image-embed scatter, latent_queries rows, m-rope tables from 3-D position ids, 28 x {RMSNorm,
          fused q|k|v GEMM + bias, m-rope, KV-cache append, causal GQA attention (28q / 4kv x 128), o_proj + residual, RMSNorm,
          SwiGLU GEMM pair + residual}, final RMSNorm, lm_head on the LAST position only, greedy argmax on the device.
Work the reference wastes and this engine removes without changing results (SURVEY.md 7 "hard parts"):
  * lm_head on every prompt position (internvla_n1.py:220) -> last position only (the only row generate() reads);
  * generate_latents re-runs ViT + the whole prompt (internvla_n1.py:330-344) -> the N_QUERY latent tokens run against the KV
    cache left by generate(): causal attention makes the prefix K/V identical;
  * per-token host syncs of HF generate -> a fixed number of decode steps on the device, EOS handled after the fact.

HBM layout (B sequences of S tokens, cache capacity S_max, H = 3584):
  x f32 [B*S, H] residual stream | h, att bf16 [B*S, H] | qkv bf16 [B*S, 4608] = q(28x128) | k(4x128) | v(4x128)
  ff bf16 [B*S, 18944] | kv[l] bf16 [B*S_max, 1024] = k | v per cached token | cos/sin f32 [B*S, 128] m-rope tables
  vision: xv f32 [Np, 1280] | hv/attv bf16 [Np, 1280] | qkvv bf16 [Np, 3840] | ffv bf16 [Np, 3456] (3420 zero-padded) | emb bf16 [Np/4, H]
"""
from __future__ import annotations

import weakref
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .runtime import CapacityError
from .s2_select import Selection


# ---------------------------------------------------------------------------------------------------- host index logic (integers only)
def vision_window_permutation(grids: Sequence[Tuple[int, int, int]], merge: int = 2, window: int = 112, patch: int = 14):
    """Window order of the merged 2x2 cells and the window boundaries in patch units (transformers get_window_index)."""
    win = window // merge // patch
    idx_all, cu, base = [], [0], 0
    for t, h, w in grids:
        gh, gw = h // merge, w // merge
        idx = np.arange(t * gh * gw).reshape(t, gh, gw)
        ph, pw = win - gh % win, win - gw % win
        nh, nw = (gh + ph) // win, (gw + pw) // win
        pad = np.pad(idx, ((0, 0), (0, ph), (0, pw)), constant_values=-100)
        pad = pad.reshape(t, nh, win, nw, win).transpose(0, 1, 3, 2, 4).reshape(t, nh * nw, win * win)
        lens = (pad != -100).sum(-1).reshape(-1)
        flat = pad.reshape(-1)
        idx_all.append(flat[flat != -100] + base)
        for n in lens.tolist():
            if n:
                cu.append(cu[-1] + n * merge * merge)
        base += t * gh * gw
    return np.concatenate(idx_all), np.asarray(cu, dtype=np.int32)


def vision_rope_tables(grids, hd: int = 80, merge: int = 2):
    """cos/sin [Np, hd] of the 2-D vision rope in pixel_values (block-major) order (transformers rot_pos_emb)."""
    out = []
    for t, h, w in grids:
        hp = np.broadcast_to(np.arange(h)[:, None], (h, w)).reshape(h // merge, merge, w // merge, merge).transpose(0, 2, 1, 3).reshape(-1)
        wp = np.broadcast_to(np.arange(w)[None, :], (h, w)).reshape(h // merge, merge, w // merge, merge).transpose(0, 2, 1, 3).reshape(-1)
        out.append(np.tile(np.stack([hp, wp], -1), (t, 1)))
    pos = torch.from_numpy(np.concatenate(out)).float()
    dim = hd // 2
    inv = 1.0 / (10000.0 ** (torch.arange(0, dim, 2, dtype=torch.float32) / dim))
    rot = (pos.unsqueeze(-1) * inv).flatten(1)
    emb = torch.cat((rot, rot), dim=-1)
    return emb.cos(), emb.sin()


def rope_index(input_ids: np.ndarray, grids, image_token_id: int, vision_start_id: int, merge: int = 2):
    """3-D (t,h,w) position ids of get_rope_index_25 (reference internnav/dataset/rope2d.py:69-158) for still images, no padding."""
    B, S = input_ids.shape
    pos = np.zeros((3, B, S), dtype=np.int64)
    deltas = np.zeros(B, dtype=np.int64)
    img = 0
    for b in range(B):
        toks = input_ids[b]
        starts = np.nonzero((toks[:-1] == vision_start_id) & (toks[1:] == image_token_id))[0]
        chunks, st, nxt = [], 0, 0
        for s0 in starts:
            ed = int(s0) + 1
            t, h, w = grids[img]
            img += 1
            gh, gw = h // merge, w // merge
            text_len = ed - st
            chunks.append(np.broadcast_to(np.arange(text_len)[None], (3, text_len)) + nxt)
            ti = np.zeros(t * gh * gw, dtype=np.int64)
            hi = np.broadcast_to(np.arange(gh)[None, :, None], (t, gh, gw)).reshape(-1)
            wi = np.broadcast_to(np.arange(gw)[None, None, :], (t, gh, gw)).reshape(-1)
            vis = np.stack([ti, hi, wi]) + text_len + nxt
            chunks.append(vis)
            nxt = int(vis.max()) + 1
            st = ed + t * gh * gw
        if st < S:
            chunks.append(np.broadcast_to(np.arange(S - st)[None], (3, S - st)) + nxt)
        p = np.concatenate(chunks, axis=1)
        pos[:, b] = p
        deltas[b] = int(p.max()) + 1 - S
    return pos, deltas


# a GEMM of at most this many rows runs the weight-streaming kernels (csrc/gemm.hip, ina_plan_gemm: kernel 32 for M <= 64), which round
# differently from the tiled prefill kernels: a prefill stays bit-equal to a longer one only while its run rectangle keeps MORE rows
SKINNY_GEMM_MAX_ROWS = 64
# causal attention with fewer than this many query (or key) rows per sequence runs the narrow kernel instead of the wide one that a full
# prefill of a real prompt runs (csrc/attention_wide.hip, ina_attention_wide_contract): K/V and hidden states then differ in the last bits
ATTN_WIDE_MIN_ROWS = 128


def kv_image_cut(ids: np.ndarray, n: int, image_token_id: int) -> int:
    """n cut back to the first token of the image it would split (a cached prefix holds whole images or none of an image)."""
    while 0 < n < ids.shape[0] and ids[n - 1] == image_token_id and ids[n] == image_token_id:
        n -= 1
    return n


def kv_reuse_lengths(ids: np.ndarray, seq_lens, cached_ids: Sequence[Optional[np.ndarray]], image_token_id: int) -> np.ndarray:
    """per sequence of a (right-padded) batch ids [B, S]: how many leading prompt tokens to take from a cache holding the K/V of
    cached_ids[b] (None: nothing cached). The longest common prefix, at least one real token left to run, cut back to the start of an
    image it would split; then, if the run rectangle (S - min over the batch) would be narrower than ATTN_WIDE_MIN_ROWS or keep
    SKINNY_GEMM_MAX_ROWS rows or fewer in all, the shortest reuse is cut back until it is not (bit-equality with a full prefill)."""
    B, S = ids.shape
    lens = np.asarray(seq_lens, dtype=np.int64).reshape(B)
    pl = np.zeros(B, dtype=np.int64)
    for b in range(B):
        c = cached_ids[b]
        if c is None or len(c) == 0:
            continue
        m = min(len(c), int(lens[b]) - 1)
        diff = np.nonzero(ids[b, :m] != np.asarray(c[:m]))[0]
        n = int(diff[0]) if diff.size else m
        pl[b] = kv_image_cut(ids[b], n, image_token_id)
    need = max(ATTN_WIDE_MIN_ROWS, SKINNY_GEMM_MAX_ROWS // B + 1)   # rectangle width of the kernels a full prefill runs
    if pl.any() and S - int(pl.min()) < need:
        b = int(np.argmin(pl))
        pl[b] = kv_image_cut(ids[b], max(0, min(int(pl[b]), S - need)), image_token_id)
    return pl


def kv_reuse_fit(pl: np.ndarray, S: int, tail: int, s_max: int) -> Tuple[np.ndarray, int]:
    """drop the reuse of the rows with the longest prefixes until the run rectangle (every row's suffix starts behind ITS prefix, plus the
    answer and the latent queries: tail) fits a cache of s_max positions -> (prefix lengths, number of rows dropped)."""
    pl = np.asarray(pl, dtype=np.int64).copy()
    dropped = 0
    while pl.any() and int(pl.max()) + S - int(pl.min()) + tail > s_max:
        pl[int(np.argmax(pl))] = 0
        dropped += 1
    return pl, dropped


def eos_ids(eos) -> Tuple[int, ...]:
    """eos_token_id as HF takes it - an int or a list of ints, any of which ends a row - as a non-empty tuple"""
    out = tuple(int(e) for e in (eos if isinstance(eos, (list, tuple)) else [eos]))
    assert out, "eos_token_id: an int or a non-empty list"
    return out


def _ids_np(input_ids) -> np.ndarray:
    """token ids (a tensor on any device, or anything array-like) as int64 on the host"""
    return (input_ids.cpu().numpy() if isinstance(input_ids, torch.Tensor) else np.asarray(input_ids)).astype(np.int64)


def _grid_list(image_grid_thw) -> List[Tuple[int, int, int]]:
    """image_grid_thw (a tensor [n_images, 3], or None for a call without images) as a list of (t, h, w)"""
    return [tuple(int(v) for v in g) for g in (image_grid_thw.tolist() if image_grid_thw is not None else [])]


def _prompt_lens(B: int, S: int, lens) -> np.ndarray:
    """real tokens per prompt of a batch of B prompts padded to S: lens [B], or None when every prompt fills the rectangle"""
    return np.full(B, S, dtype=np.int64) if lens is None else np.asarray(lens, dtype=np.int64).reshape(B)


def prompt_images(ids: np.ndarray, ntok: Sequence[int], image_token_id: int):
    """(sequence, first token, last token) of every image of a batch, in prompt order: image k fills the next ntok[k] image tokens of its sequence"""
    k = 0
    for b in range(ids.shape[0]):
        ipos = np.nonzero(ids[b] == image_token_id)[0]
        cum = 0
        while cum < ipos.size:
            assert k < len(ntok), "image count of the prompts and image_grid_thw disagree"
            yield b, int(ipos[cum]), int(ipos[cum + ntok[k] - 1])
            cum += ntok[k]
            k += 1


class EngineKVCache:
    """K/V of the PROMPT rows of each sequence of a System-2 call, per row bf16 [layers, n_b, kv_w] with the token ids (int64, CPU) they
    cover: what `generate(return_dict_in_generate=True, use_cache=True).past_key_values` returns and `generate(past_key_values=...)`
    takes back. The subset of HF's `Cache` its callers use: get_seq_length, crop, row selection, copy.deepcopy.
    Unlike HF's cache it does not hold the decoded answer: the decode passes run the weight-streaming GEMMs, which round differently
    from the tiled prefill, so the next call prefills the answer with the rest of its new tokens (a handful of rows).
    A fresh handle is a VIEW of the engine's cache slots (no copy). It is materialised into tensors of its own - one ina_kv_copy launch for
    every live handle concerned - when deepcopy / materialize() is called, or just before the engine would overwrite its rows."""

    def __init__(self, token_ids: Sequence[Optional[torch.Tensor]], kv: Optional[Sequence[Optional[torch.Tensor]]] = None, engine=None,
                 views: Optional[Sequence[Optional[Tuple[int, int]]]] = None):
        n = len(token_ids)
        self.token_ids = [None if t is None else torch.as_tensor(t).detach().to("cpu", torch.int64).reshape(-1) for t in token_ids]
        self.kv = list(kv) if kv is not None else [None] * n
        self._views = list(views) if views is not None else [None] * n     # per row: (slot, generation) while the rows live in a cache slot
        assert len(self.kv) == len(self._views) == n
        for b in range(n):
            if self.get_seq_length(b) == 0:
                self.kv[b], self._views[b] = None, None
            else:
                assert (self.kv[b] is None) != (self._views[b] is None), "a row is either a view of a cache slot or holds its own K/V"
                assert self.kv[b] is None or self.kv[b].shape[1] == self.get_seq_length(b)
        self._engine = engine if any(v is not None for v in self._views) else None
        if self._engine is not None:
            self._engine._kv_views.add(self)

    def __len__(self) -> int:
        return len(self.token_ids)

    @property
    def batch_size(self) -> int:
        return len(self.token_ids)

    def get_seq_length(self, row: int = 0) -> int:
        t = self.token_ids[row]
        return 0 if t is None else int(t.numel())

    @property
    def is_view(self) -> bool:
        return any(v is not None for v in self._views)

    def crop(self, max_length: int) -> "EngineKVCache":
        """keep the first max_length tokens of every row (HF: a negative value removes that many from the end)."""
        for b in range(len(self)):
            n = self.get_seq_length(b)
            m = n + max_length if max_length < 0 else max_length
            if n == 0 or n <= m:
                continue
            m = max(m, 0)
            self.token_ids[b] = self.token_ids[b][:m]
            if self.kv[b] is not None:
                self.kv[b] = self.kv[b][:, :m]
            if m == 0:
                self.token_ids[b], self.kv[b], self._views[b] = None, None, None
        return self

    def select(self, rows: Sequence[int]) -> "EngineKVCache":
        """a handle over the given rows (views stay views of the same slots; tensors are shared, never written in place)."""
        rows = [int(r) for r in rows]
        return EngineKVCache([self.token_ids[r] for r in rows], [self.kv[r] for r in rows], self._engine, [self._views[r] for r in rows])

    def batch_select_indices(self, indices) -> None:
        """HF name: keep the given rows, in place."""
        o = self.select(torch.as_tensor(indices).reshape(-1).tolist())
        self.token_ids, self.kv, self._views = o.token_ids, o.kv, o._views
        if self._engine is not None and self.is_view:
            self._engine._kv_views.add(self)

    def materialize(self) -> "EngineKVCache":
        if self._engine is not None and self.is_view:
            self._engine.materialize_kv([(self, b) for b in range(len(self)) if self._views[b] is not None])
        return self

    def __deepcopy__(self, memo):
        kv = [None if t is None else t.clone() for t in self.kv]
        c = EngineKVCache([None if t is None else t.clone() for t in self.token_ids], kv, self._engine, list(self._views))
        c.materialize()                                          # straight from the cache slots: this handle stays a view
        return c


W8_DECODER_KEYS = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
                   "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight")


def w8_roundtrip_state_dict(sd, cfg: dict) -> dict:
    """the checkpoint an engine built with w8_decode=True computes: q / k / v / o / gate / up / down of every decoder layer and lm_head replaced
    by their e4m3 * 2^e round trip (ops.w8_quantize of the bf16 weight: the scale is per output row, so fusing or interleaving rows afterwards
    changes nothing); every other tensor is passed through. For tests, and for evaluating the quantised model elsewhere."""
    names = {f"model.layers.{i}.{k}" for i in range(cfg["t_layers"]) for k in W8_DECODER_KEYS} | {"lm_head.weight"}
    out = {}
    for k in sd.keys():
        v = sd[k]
        out[k] = ops.w8_quantize(v.to(torch.bfloat16).contiguous())[2].to(v.dtype) if k in names else v
    return out


def mx4_roundtrip_state_dict(sd, cfg: dict) -> dict:
    """the checkpoint an engine built with mx4_decode=True computes: q / k / v / o / gate / up / down of every decoder layer replaced by
    their MXFP4 round trip (ops.mx4_quantize of the bf16 weight: the blocks run along K inside one output row, so fusing or interleaving rows
    afterwards changes nothing) and lm_head by its e4m3 * 2^e round trip (ops.w8_quantize); every other tensor is passed through. For tests,
    and for evaluating the quantised model elsewhere."""
    names = {f"model.layers.{i}.{k}" for i in range(cfg["t_layers"]) for k in W8_DECODER_KEYS}
    out = {}
    for k in sd.keys():
        v = sd[k]
        if k in names:
            out[k] = ops.mx4_quantize(v.to(torch.bfloat16).contiguous())[2].to(v.dtype)
        elif k == "lm_head.weight":
            out[k] = ops.w8_quantize(v.to(torch.bfloat16).contiguous())[2].to(v.dtype)
        else:
            out[k] = v
    return out


def _interleave16(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    n, k = a.shape
    return torch.stack([a.view(n // 16, 16, k), b.view(n // 16, 16, k)], dim=1).reshape(2 * n, k).contiguous()


def _pad_rows(t: torch.Tensor, n: int) -> torch.Tensor:
    return t if t.shape[0] == n else torch.cat([t, t.new_zeros((n - t.shape[0],) + tuple(t.shape[1:]))], 0)


class QwenVLEngine:
    """weights: mapping key -> tensor (a state dict, or a lazy provider that materialises tensors on the device)."""

    def __init__(self, weights, cfg: dict, device="cuda:0", max_seqs: int = 16, max_seq_len: int = 1024, max_patches: int = 16 * 3136,
                 frag_weights: Optional[bool] = None, w8_decode: bool = False, token_logprobs: bool = False, max_decode: int = 128,
                 mx4_decode: bool = False):
        """token_logprobs (opt-in, fixed for the engine's life: captured graphs and cached models are of one setting): every greedy selection
        also writes the log-probability and the top-2 margin of the chosen token (ops.logprob_rows IN PLACE of the argmax launch: same launch
        count, same tokens) into per-step device buffers for up to max_decode answer tokens; read them with `last_logprobs`."""
        if w8_decode and mx4_decode:
            raise ValueError("w8_decode and mx4_decode are two roundings of the same weights: choose one")
        dev = torch.device(device)
        bf, f32 = torch.bfloat16, torch.float32
        self.cfg, self.device = cfg, dev
        self.B_max, self.S_max, self.Np_max = max_seqs, max_seq_len, max_patches
        self.fuse_decode_norm = True   # decode passes: RMSNorm fused into the q|k|v and gate|up weight-streaming GEMMs
        # prefill of >= 2 plain prompts (no cached prefix / embeddings) as two half batches on two streams (fork / join inside the launch
        # sequence, graph capturable): every op of the tower and of the decoder stack works on row ranges, so the halves use disjoint
        # slices of the same buffers and cache slots and the results are the same; the tails of one half's GEMM launches (tile
        # quantisation over 256 CUs) are filled by the other half's workgroups (119.6 -> 115.5 ms at 7 prompts, profiles/r03q_*)
        self.split_prefill = True
        self.split_serial = False     # True: the two half micro-batches of split_prefill on ONE stream (per-launch event timing, bench.py)
        self._side = None
        self.fuse_decode_rope = True   # single-token passes: rotary embedding + KV-cache append inside the attention launch instead of a launch of their own
        self.tap = None   # debug / parity hook: tap(kind, index, residual_stream) after every ViT block ("vit") and decoder layer ("llm"); eager runs only
        D, I = cfg["v_hidden"], cfg["v_inter"]
        Ip = (I + 63) // 64 * 64   # SwiGLU width padded with zero rows/cols: GLU tiles need N % 32 == 0, the LDS-DMA GEMM K % 64 == 0
        self.vD, self.vI, self.vH, self.vhd = D, Ip, cfg["v_heads"], D // cfg["v_heads"]
        H, TI = cfg["t_hidden"], cfg["t_inter"]
        self.H, self.TI, self.nh, self.nkv = H, TI, cfg["t_heads"], cfg["t_kv_heads"]
        self.hd = H // self.nh
        self.qkv_w = (self.nh + 2 * self.nkv) * self.hd
        self.kv_w = 2 * self.nkv * self.hd
        W = weights

        def w(k):
            return W[k].to(device=dev, dtype=bf).contiguous()

        def f(k):
            return W[k].to(device=dev, dtype=f32).contiguous()

        # ---- vision tower
        self.v_patch = W["visual.patch_embed.proj.weight"].to(device=dev, dtype=bf).reshape(D, -1).contiguous()
        self.v_blocks = []
        for i in range(cfg["v_depth"]):
            b = f"visual.blocks.{i}."
            gw_, uw = _pad_rows(W[b + "mlp.gate_proj.weight"].to(dev).float(), Ip), _pad_rows(W[b + "mlp.up_proj.weight"].to(dev).float(), Ip)
            gb, ub = _pad_rows(W[b + "mlp.gate_proj.bias"].to(dev).float(), Ip), _pad_rows(W[b + "mlp.up_proj.bias"].to(dev).float(), Ip)
            dw = W[b + "mlp.down_proj.weight"].to(dev).float()
            dw = torch.cat([dw, dw.new_zeros(D, Ip - I)], 1) if Ip != I else dw
            self.v_blocks.append(dict(
                n1=f(b + "norm1.weight"), n2=f(b + "norm2.weight"), qkv_w=w(b + "attn.qkv.weight"), qkv_b=f(b + "attn.qkv.bias"),
                proj_w=w(b + "attn.proj.weight"), proj_b=f(b + "attn.proj.bias"),
                gu_w=_interleave16(gw_, uw).to(bf), gu_b=_interleave16(gb[:, None], ub[:, None]).reshape(-1).contiguous(),
                down_w=dw.to(bf).contiguous(), down_b=f(b + "mlp.down_proj.bias"), full=i in cfg["v_fullatt"]))
        self.m_ln = f("visual.merger.ln_q.weight")
        self.m0 = (w("visual.merger.mlp.0.weight"), f("visual.merger.mlp.0.bias"))
        self.m2 = (w("visual.merger.mlp.2.weight"), f("visual.merger.mlp.2.bias"))
        Np = max_patches
        self.pv_perm = torch.empty(Np, 1176, dtype=bf, device=dev)
        self.xv = torch.empty(Np, D, dtype=f32, device=dev)
        self.hv = torch.empty(Np, D, dtype=bf, device=dev)
        self.attv = torch.empty(Np, D, dtype=bf, device=dev)
        self.qkvv = torch.empty(Np, 3 * D, dtype=bf, device=dev)
        self.ffv = torch.empty(Np, Ip, dtype=bf, device=dev)
        self.mh = torch.empty(Np // 4, 4 * D, dtype=bf, device=dev)
        self.emb = torch.empty(Np // 4, cfg["v_out"], dtype=bf, device=dev)
        self.emb_tok = torch.empty(Np // 4, cfg["v_out"], dtype=bf, device=dev)   # the same rows in image-token order (what a per-frame cache keeps)
        self.v_cos = torch.empty(Np, self.vhd, dtype=f32, device=dev)
        self.v_sin = torch.empty(Np, self.vhd, dtype=f32, device=dev)
        # ---- text model
        self.embed = w("model.embed_tokens.weight")
        self.layers = []
        for i in range(cfg["t_layers"]):
            b = f"model.layers.{i}."
            qkvw = torch.cat([W[b + "self_attn.q_proj.weight"].to(dev), W[b + "self_attn.k_proj.weight"].to(dev), W[b + "self_attn.v_proj.weight"].to(dev)], 0)
            qkvb = torch.cat([W[b + "self_attn.q_proj.bias"].to(dev), W[b + "self_attn.k_proj.bias"].to(dev), W[b + "self_attn.v_proj.bias"].to(dev)], 0)
            self.layers.append(dict(
                n1=f(b + "input_layernorm.weight"), n2=f(b + "post_attention_layernorm.weight"),
                qkv_w=qkvw.to(bf).contiguous(), qkv_b=qkvb.to(f32).contiguous(), o_w=w(b + "self_attn.o_proj.weight"),
                gu_w=_interleave16(W[b + "mlp.gate_proj.weight"].to(dev), W[b + "mlp.up_proj.weight"].to(dev)).to(bf),
                down_w=w(b + "mlp.down_proj.weight"),
                kv=torch.empty(max_seqs * max_seq_len, self.kv_w, dtype=bf, device=dev)))
        # the three wide decoder weights a second time in MFMA fragment order (ops.gemm_preshuffle, + 12 GB at the 7B geometry): the prefill GEMMs
        # that run the four-wave 256 x 256 tile then fetch their B fragments straight from global memory into registers (tile config 40,
        # gemm_w4.hip: half the LDS-DMA pieces and fragment reads per stage; bit-equal); the single-token passes keep streaming the row-major copy
        self.frag_weights = torch.device(dev).type == "cuda" if frag_weights is None else bool(frag_weights)
        self.norm_w = f("model.norm.weight")
        self.lm_head = w("lm_head.weight")
        # w8_decode: the decoder projections and lm_head rounded to e4m3 * 2^e per output row (ops.w8_quantize). The bf16 tensors then hold the
        # dequantised values - the model every pass computes - and the GEMMs of at most SKINNY_GEMM_MAX_ROWS rows stream the fp8 bytes instead
        # (ops.linear_w8: half the weight bytes, the same bits as the bf16 weight-streaming kernels on the dequantised weights)
        # mx4_decode: the same for the decoder projections in MXFP4 (ops.mx4_quantize: e2m1 elements, an e8m0 scale per 32 k; ops.linear_mx4
        # streams 0.27 of the bf16 bytes, same bits on the dequantised weights); lm_head, the most sensitive layer, goes the e4m3 way
        self.w8_decode = False
        self.mx4_decode = False
        self.lm_head8 = None
        if w8_decode:
            self.refresh_w8_weights()          # (rebuilds the fragment-ordered copies from the dequantised weights)
        elif mx4_decode:
            self.refresh_mx4_weights()         # (likewise)
        elif self.frag_weights:
            self.refresh_frag_weights()
        self.latent_q = W["model.latent_queries"].to(device=dev, dtype=bf).reshape(-1, H).contiguous()
        rows = max_seqs * max_seq_len
        self.x_in = torch.empty(rows, H, dtype=bf, device=dev)
        self.x = torch.empty(rows, H, dtype=f32, device=dev)
        self.h = torch.empty(rows, H, dtype=bf, device=dev)
        self.att = torch.empty(rows, H, dtype=bf, device=dev)
        self.qkv = torch.empty(rows, self.qkv_w, dtype=bf, device=dev)
        self.ff = torch.empty(rows, TI, dtype=bf, device=dev)
        self.cos = torch.empty(rows, self.hd, dtype=f32, device=dev)
        self.sin = torch.empty(rows, self.hd, dtype=f32, device=dev)
        self.hl = torch.empty(max_seqs * 8, H, dtype=bf, device=dev)
        self.xl = torch.empty(max_seqs, H, dtype=f32, device=dev)
        self.logits = torch.empty(max_seqs, cfg["vocab"], dtype=f32, device=dev)
        self.next_tok = torch.empty(max_seqs, dtype=torch.int32, device=dev)
        # repetition penalty (generation_config.json, HF RepetitionPenaltyLogitsProcessor): per sequence the bitmap of the tokens seen so far
        # (token t = bit t & 31 of word t >> 5; rows of a multiple of 4 words). Only a call with a penalty != 1 ever touches it.
        self.seen = torch.zeros(max_seqs, ((cfg["vocab"] + 31) // 32 + 3) // 4 * 4, dtype=torch.uint32, device=dev)
        # token_logprobs: log-probability / top-2 margin of answer token j of sequence b at [b, j]. Stored step-major, so the column a step's
        # launch writes is one contiguous row at an address fixed per step (capturable); tok_logprob / tok_margin are the [B_max, max_decode] views
        self.token_logprobs, self.max_decode = bool(token_logprobs), int(max_decode)
        self._lp_steps = self._mg_steps = self.tok_logprob = self.tok_margin = None      # (no buffer at all without the setting)
        self._smp_lp = None      # sampling (prefill(sampling=)): log-probability of the draws, step-major f32 [max_decode, max_seqs], allocated by the first sampling call
        # shared-prompt sampling (prefill(sampling=dict(share_prefix=True))): row-count-sized twins of logits / next_tok / seen / xl / hl / _smp_lp
        # and the per-layer answer tails, allocated by the first such call (`_shared_buffers`)
        self._shared = None
        self._beam = None        # beam search (prefill(beam=)): the second tail set, the beam tables and the histories, allocated by the first beam call
        # constrained decoding (plan(constraint=)): the rows' automaton states, int32 [2, max_seqs] - step `col` reads row col & 1 and writes the
        # other (ops.automaton_mask_rows needs distinct buffers). Allocated by the first constrained call; the shared-prompt twins carry their own.
        self._cstate = None
        # logits-processor rules (plan(logit_rules=)): the rows' token histories, int32 [max_seqs, max_seq_len + max_decode] - prompt, then answer
        # (ops.logit_rules_rows). Allocated by the first call that carries rules; the shared-prompt twins carry their own.
        self._rhist = None
        if self.token_logprobs:
            self._lp_steps, self._mg_steps = (torch.zeros(self.max_decode, max_seqs, dtype=f32, device=dev) for _ in range(2))
            self.tok_logprob, self.tok_margin = self._lp_steps.t(), self._mg_steps.t()
        half = self.hd // 2
        self.inv_freq = (1.0 / (cfg["rope_theta"] ** (torch.arange(0, self.hd, 2, dtype=f32) / self.hd))).to(dev)
        axis = np.concatenate([np.full(16, 0), np.full(24, 1), np.full(24, 2)]).astype(np.int32)  # mrope_section [16, 24, 24]
        assert axis.size == half
        self.axis_of = torch.from_numpy(axis).to(dev)
        self._kv_reset_tracking()

    def _kv_reset_tracking(self):
        self._kv_views = weakref.WeakSet()                       # live EngineKVCache handles with rows still in this engine's cache slots
        self._slot_gen = np.zeros(self.B_max, dtype=np.int64)    # bumped when a slot is rewritten from row 0: views of older generations are gone
        self._kv_base = None                                     # int64 [layers] device table of the layers' cache addresses (ina_kv_copy)

    _BUFFERS = ("pv_perm", "xv", "hv", "attv", "qkvv", "ffv", "mh", "emb", "emb_tok", "v_cos", "v_sin", "x_in", "x", "h", "att", "qkv", "ff", "cos", "sin",
                "hl", "xl", "logits", "next_tok", "seen")

    def twin(self) -> "QwenVLEngine":
        """a second engine over the SAME weight tensors (nothing is copied; `latent_q` stays one shared parameter) with its own activation
        buffers and KV cache: two calls can then be in flight on two streams - the SFT trainer prefills the frozen prefix of micro-batch
        i + 1 in the twin while micro-batch i's latent-query rows still read this engine's cache (trainer.prefetch)."""
        import copy

        t = copy.copy(self)
        for n in self._BUFFERS:
            setattr(t, n, torch.empty_like(getattr(self, n)))
        if self.token_logprobs:
            t._lp_steps, t._mg_steps = torch.zeros_like(self._lp_steps), torch.zeros_like(self._mg_steps)
            t.tok_logprob, t.tok_margin = t._lp_steps.t(), t._mg_steps.t()
        t.layers = [dict(L, kv=torch.empty_like(L["kv"])) for L in self.layers]
        t._side = None
        t._shared = None
        t._beam = None
        t._cstate = None
        t._rhist = None
        t._kv_reset_tracking()
        return t

    # ------------------------------------------------------------------------------------------------ vision tower
    def plan_vision(self, grids: List[Tuple[int, int, int]]) -> dict:
        """host side of the vision tower for a list of image grids: window permutation, cu_seqlens, rope tables (uploaded once)."""
        dev, hd = self.device, self.vhd
        win_idx, cu_win = vision_window_permutation(grids, 2, self.cfg["v_window"], self.cfg["v_patch"])
        perm = (win_idx[:, None] * 4 + np.arange(4)[None]).reshape(-1).astype(np.int32)
        cu_full = np.concatenate([[0], np.cumsum([t * h * w for t, h, w in grids])]).astype(np.int32)
        cos, sin = vision_rope_tables(grids, hd)
        Np = int(cu_full[-1])
        if Np > self.Np_max:
            raise CapacityError(f"{Np} image patches exceed the engine's max_patches={self.Np_max}")
        return dict(Np=Np, perm=torch.from_numpy(perm).to(dev), cos=cos[perm].contiguous().to(dev), sin=sin[perm].contiguous().to(dev),
                    cu_win=torch.from_numpy(cu_win).to(dev), cu_full=torch.from_numpy(cu_full).to(dev),
                    max_win=int(np.diff(cu_win).max()), max_full=int(np.diff(cu_full).max()), inv=np.argsort(win_idx).astype(np.int32))

    def run_vision(self, vp: dict, pixel_values: torch.Tensor) -> torch.Tensor:
        """launch sequence of the vision tower (graph capturable): pixel_values bf16 [Np, 1176] -> embeds bf16 [Np/4, 3584], WINDOW order."""
        D, Hh, hd, Np = self.vD, self.vH, self.vhd, vp["Np"]
        assert pixel_values.shape[0] == Np and pixel_values.dtype == torch.bfloat16
        p0 = vp.get("p0", 0)                                      # first patch row of this launch sequence in the engine's buffers (split prefill)
        xp, x, h, att, qkv, ff = (t[p0:p0 + Np] for t in (self.pv_perm, self.xv, self.hv, self.attv, self.qkvv, self.ffv))
        ops.gather_rows(pixel_values, xp, src=vp["perm"])
        ops.linear(xp, self.v_patch, out=x)
        q3 = qkv.view(Np, 3, Hh, hd)
        for bi, blk in enumerate(self.v_blocks):
            ops.norm(x, blk["n1"], None, eps=1e-6, rms=True, out=h)
            ops.linear(h, blk["qkv_w"], bias=blk["qkv_b"], out=qkv)
            ops.rope(qkv, vp["cos"], vp["sin"], heads=2 * Hh, D=hd, col0=0, rows=Np)
            cu, mx = (vp["cu_full"], vp["max_full"]) if blk["full"] else (vp["cu_win"], vp["max_win"])
            ops.attention(q3[:, 0], q3[:, 1], q3[:, 2], cu_q=cu, cu_k=cu, max_q=mx, max_k=mx, out=att.view(Np, Hh, hd))
            ops.linear(att, blk["proj_w"], bias=blk["proj_b"], residual=x, out=x)
            ops.norm(x, blk["n2"], None, eps=1e-6, rms=True, out=h)
            ops.linear(h, blk["gu_w"], bias=blk["gu_b"], act="silu", glu=True, out=ff)
            ops.linear(ff, blk["down_w"], bias=blk["down_b"], residual=x, out=x)
            if self.tap is not None:
                self.tap("vit", bi, x)
        ops.norm(x, self.m_ln, None, eps=1e-6, rms=True, out=h)
        mh, emb = self.mh[p0 // 4: (p0 + Np) // 4], self.emb[p0 // 4: (p0 + Np) // 4]
        ops.linear(h.view(Np // 4, 4 * D), self.m0[0], bias=self.m0[1], act="gelu", out=mh)
        ops.linear(mh, self.m2[0], bias=self.m2[1], out=emb)
        return emb

    def vision(self, pixel_values: torch.Tensor, grids: List[Tuple[int, int, int]]):
        """pixel_values bf16 [Np, 1176] (HF processor patch layout) -> (embeds in WINDOW order, inv) with inv[k] = embed row of the
        k-th image token in sequence order."""
        vp = self.plan_vision(grids)
        return self.run_vision(vp, pixel_values), vp["inv"]

    def refresh_frag_weights(self):
        """(re)build the fragment-ordered copies of the wide decoder weights from the row-major ones - at load, and after anything that
        replaces or updates a layer weight in place (checkpoint reload, LoRA merge): the copies are not views"""
        self.frag_weights = True
        for L in self.layers:
            for k in ("qkv_w", "gu_w", "down_w"):
                n_, k_ = L[k].shape
                if n_ % 16 == 0 and k_ % 32 == 0:
                    L[k + "f"] = ops.gemm_preshuffle(L[k], out=L.get(k + "f"))
                else:
                    L[k + "f"] = None

    def drop_frag_weights(self):
        """release the fragment-ordered copies (12 GB at the 7B geometry): the prefill GEMMs fall back to tile config 39 / 18, same bits"""
        self.frag_weights = False
        for L in self.layers:
            for k in ("qkv_wf", "gu_wf", "down_wf"):
                L.pop(k, None)

    W8_LAYER_WEIGHTS = ("qkv_w", "o_w", "gu_w", "down_w")

    def refresh_w8_weights(self):
        """(re)quantise q|k|v, o, gate|up, down of every decoder layer and lm_head to e4m3 with a power-of-two scale per output row - at load
        (w8_decode=True), and after anything that replaces or updates one of these weights in place. The bf16 tensors are overwritten IN PLACE
        with the dequantised values (twins and the prefill keep reading them; quantising them again changes nothing), the packed fp8 bytes
        and the exponents are kept beside them (+ 7 GB at the 7B geometry) and the fragment-ordered copies are rebuilt. Vision tower,
        embeddings, norms and biases are untouched."""
        if self.mx4_decode:
            raise ValueError("refresh_w8_weights on an mx4_decode engine: drop_mx4_weights() first (the weights would be rounded twice)")
        for L in self.layers:
            for k in self.W8_LAYER_WEIGHTS:
                w8, e, wd = ops.w8_quantize(L[k])
                L[k].copy_(wd)
                L[k + "8"] = (w8, e)
        w8, e, wd = ops.w8_quantize(self.lm_head)
        self.lm_head.copy_(wd)
        self.lm_head8 = (w8, e)
        self.w8_decode = True
        if self.frag_weights:
            self.refresh_frag_weights()

    def drop_w8_weights(self):
        """release the fp8 copies: the single-token passes stream the (dequantised) bf16 weights again - the same model, the same bits"""
        self.w8_decode = False
        self.lm_head8 = None
        for L in self.layers:
            for k in self.W8_LAYER_WEIGHTS:
                L.pop(k + "8", None)

    def refresh_mx4_weights(self):
        """(re)quantise q|k|v, o, gate|up, down of every decoder layer to MXFP4 (e2m1 elements, one e8m0 scale per 32 consecutive k) and
        lm_head to e4m3 with a power-of-two scale per output row - at load (mx4_decode=True), and after anything that replaces or updates
        one of these weights in place. The fused / interleaved tensors are quantised as they stand: a block lies inside one output row, so
        the rounding commutes with every permutation of rows. The bf16 tensors are overwritten IN PLACE with the dequantised values (twins
        and the prefill keep reading them; quantising them again changes nothing), the packed bytes and scales are kept beside them (+ 3.5 GB
        and + 0.55 GB for lm_head at the 7B geometry) and the fragment-ordered copies are rebuilt. Vision tower, embeddings, norms and
        biases are untouched."""
        if self.w8_decode:
            raise ValueError("refresh_mx4_weights on a w8_decode engine: drop_w8_weights() first (the weights would be rounded twice)")
        for L in self.layers:
            for k in self.W8_LAYER_WEIGHTS:
                w4, sc, wd = ops.mx4_quantize(L[k])
                L[k].copy_(wd)
                L[k + "4"] = (w4, sc)
        w8, e, wd = ops.w8_quantize(self.lm_head)
        self.lm_head.copy_(wd)
        self.lm_head8 = (w8, e)
        self.mx4_decode = True
        if self.frag_weights:
            self.refresh_frag_weights()

    def drop_mx4_weights(self):
        """release the MXFP4 copies and lm_head's fp8 copy: the single-token passes stream the (dequantised) bf16 weights again - the same
        model, the same bits"""
        self.mx4_decode = False
        self.lm_head8 = None
        for L in self.layers:
            for k in self.W8_LAYER_WEIGHTS:
                L.pop(k + "4", None)

    def _linear(self, x, L: dict, k: str, quant, **kw):
        """one decoder projection: the quantised weight stream this pass uses (quant "8": fp8, "4": MXFP4; same bits as the bf16 kernels on
        the dequantised weights), else (None / False) the bf16 kernels"""
        if quant:
            kw.pop("w_frag", None)
            if quant == "4":
                return ops.linear_mx4(x, *L[k + "4"], **kw)
            return ops.linear_w8(x, *L[k + "8"], **kw)
        return ops.linear(x, L[k], **kw)

    def _lm_head(self, h: torch.Tensor, out: torch.Tensor):
        """lm_head on the rows of h: the fp8 weight stream on a w8_decode / mx4_decode engine, like every other weight-streaming GEMM"""
        if (self.w8_decode or self.mx4_decode) and h.shape[0] <= SKINNY_GEMM_MAX_ROWS:
            ops.linear_w8(h, *self.lm_head8, out=out)
        else:
            ops.linear(h, self.lm_head, out=out)                  # (152064 columns: one wave per 16-column tile owns all of K)

    def _i32(self, v) -> torch.Tensor:
        """a host-built index table on the device, int32"""
        return torch.from_numpy(np.ascontiguousarray(v).astype(np.int32)).to(self.device)

    # ------------------------------------------------------------------------------------------------ text model
    def _phase(self, B: int, S: int, pos3: np.ndarray, cache_pos0, k_len: Optional[np.ndarray] = None, b0: int = 0) -> dict:
        """host side of one pass of the decoder stack over B x S new tokens: 3-D position ids, cache rows, key lengths.
        b0: first cache slot / sequence of the pass (a half batch of the split prefill runs sequences b0 .. b0 + B on buffer rows b0 * S ..)."""
        dev = self.device
        pos0 = np.broadcast_to(np.asarray(cache_pos0, dtype=np.int64).reshape(-1, 1), (B, 1))
        rows = ((b0 + np.arange(B))[:, None] * self.S_max + pos0 + np.arange(S)[None]).reshape(-1).astype(np.int32)
        if int(pos0.max()) + S > self.S_max:
            raise CapacityError(f"KV cache capacity exceeded: {int(pos0.max()) + S} tokens > max_seq_len={self.S_max}")
        ph = dict(B=B, S=S, pos=torch.from_numpy(np.ascontiguousarray(np.broadcast_to(pos3, (3, B, S)).reshape(3, B * S)).astype(np.int32)).to(dev),
                  rows=torch.from_numpy(rows).to(dev), Lk=int(pos0.max()) + S, k_len=None, b0=b0, r0=b0 * S)
        if k_len is not None:
            ph["k_len"] = torch.from_numpy(np.asarray(k_len, dtype=np.int32)).to(dev)
        # the new tokens of every sequence are its LAST S keys (what the attention launch assumes when it appends them itself, ina_attn_args.rope_cos)
        ph["new_are_last"] = bool(np.all((np.asarray(k_len).reshape(-1) if k_len is not None else ph["Lk"]) == pos0[:, 0] + S))
        ph["w0"] = pos0[:, 0].copy()                              # first cache row each sequence writes (live KV handles, _kv_evict)
        return ph

    def _layers(self, ph: dict):
        """28 decoder layers over the phase's rows (x_in holds their bf16 input embeddings); K/V land at ph['rows'] of the cache."""
        H, nh, nkv, hd, Smax = self.H, self.nh, self.nkv, self.hd, self.S_max
        B, S = ph["B"], ph["S"]
        rows, r0, b0 = B * S, ph.get("r0", 0), ph.get("b0", 0)
        if self._kv_views and "w0" in ph:
            self._kv_evict({b0 + i: int(w) for i, w in enumerate(ph["w0"])})
        x, h, att, qkv, ff, x_in, cos, sin = (t[r0:r0 + rows] for t in (self.x, self.h, self.att, self.qkv, self.ff, self.x_in, self.cos, self.sin))
        ops.mrope_table(ph["pos"], self.inv_freq, self.axis_of, cos, sin)
        q4 = qkv[:, : nh * hd].view(B, S, nh, hd)
        # single-token decode passes (<= 16 rows): the two RMSNorms of a layer run inside the weight-streaming GEMMs that consume them
        # (ina_gemm_bf16 norm_gamma) and the rotary embedding + KV-cache append of the new token inside the attention launch
        # (ina_attn_args.rope_cos): 5 launches per layer - q|k|v, attention, o, gate|up, down - in a chain that is launch / latency bound
        single = rows <= 16 and self.tap is None
        fused_norm = single and self.fuse_decode_norm
        # suffix pass (ph["prefix"], `_suffix_phase`): B pairs x S candidate tokens behind prompts that stay in their cache slots - rope without
        # the cache append, ops.attention_prefix in place of ops.attention; nothing of the cache is written
        pfx = ph.get("prefix")
        if pfx is not None:
            k4 = qkv[:, nh * hd:(nh + nkv) * hd].view(B, S, nkv, hd)
            v4 = qkv[:, (nh + nkv) * hd:].view(B, S, nkv, hd)
        # shared-prompt decode pass (ph["shared"], `_shared_phase`): one row per returned sequence; k|v of the new token go to the row's own tail
        # (the same rope launch, another destination), ops.attention_shared reads the prompt in place; nothing of the cache is written
        shr = ph.get("shared")
        fuse_rope = pfx is None and shr is None and single and self.fuse_decode_rope and ph.get("new_are_last", False) and ops.attention_rope_ok(S, ph["Lk"], nh, nkv, hd)
        if fuse_rope:
            kn4 = qkv[:, nh * hd:(nh + nkv) * hd].view(B, S, nkv, hd)
            vn4 = qkv[:, (nh + nkv) * hd:].view(B, S, nkv, hd)
        # w8_decode: every GEMM of this pass that would run the bf16 weight-streaming kernels reads the fp8 copy instead
        # (mx4_decode: the MXFP4 copy)
        quant = ("8" if self.w8_decode else "4" if self.mx4_decode else None) if rows <= SKINNY_GEMM_MAX_ROWS else None
        for li, L in enumerate(self.layers):
            src = x_in if li == 0 else x
            wf = (lambda k, L=L: L.get(k)) if (self.frag_weights and rows > SKINNY_GEMM_MAX_ROWS) else (lambda k: None)
            if fused_norm:
                self._linear(src, L, "qkv_w", quant, bias=L["qkv_b"], out=qkv, prenorm=(L["n1"], 1e-6))
            else:
                ops.norm(src, L["n1"], None, eps=1e-6, rms=True, out=h)
                self._linear(h, L, "qkv_w", quant, bias=L["qkv_b"], out=qkv, w_frag=wf("qkv_wf"))
            if pfx is not None:
                ops.rope(qkv, cos, sin, heads=nh + nkv, D=hd, col0=0, rows=rows)      # q and k in place: no cache append
                kvc = L["kv"].view(self.B_max, Smax, 2, nkv, hd)
                tl = pfx.get("tail")
                if tl is None:
                    ops.attention_prefix(q4, k4, v4, kvc[:, :, 0], kvc[:, :, 1], pfx["slot"], pfx["pfx_len"], pfx["suf_len"],
                                         out=att.view(B, S, nh, hd), max_pfx=pfx["max_pfx"])
                else:                                                 # the pairs' own answer K/V: rows of the shared-prompt tails, read in place
                    t5 = tl["tails"][li][: tl["rows"] * tl["T"]].view(tl["rows"], tl["T"], 2, nkv, hd)
                    ops.attention_prefix_tail(q4, k4, v4, kvc[:, :, 0], kvc[:, :, 1], pfx["slot"], pfx["pfx_len"], pfx["suf_len"], t5[:, :, 0],
                                              t5[:, :, 1], tl["tail_row"], tl["tail_len"], out=att.view(B, S, nh, hd), max_pfx=pfx["max_pfx"],
                                              max_tail=tl["max_tail"])
            elif shr is not None:
                tail = shr["tails"][li]
                ops.rope(qkv, cos, sin, heads=nh + nkv, D=hd, col0=0, rows=rows, kv_out=tail, kv_dst=shr["kv_dst"], kv_head0=nh, v_heads=nkv)
                kvc = L["kv"].view(self.B_max, Smax, 2, nkv, hd)
                t5 = tail[: rows * shr["T"]].view(rows, shr["T"], 2, nkv, hd)
                ops.attention_shared(qkv[:, : nh * hd].view(rows, nh, hd), t5[:, :, 0], t5[:, :, 1], kvc[:, :, 0], kvc[:, :, 1], shr["tile_rows"],
                                     shr["tile_slot"], shr["tile_pfx"], shr["tail_len"], out=att.view(rows, nh, hd), max_pfx=shr["max_pfx"])
            else:
                if not fuse_rope:
                    # m-rope on q (in place) and k, and the KV-cache append (rotated k | v -> cache row of every token) in ONE launch
                    ops.rope(qkv, cos, sin, heads=nh + nkv, D=hd, col0=0, rows=rows, kv_out=L["kv"], kv_dst=ph["rows"], kv_head0=nh, v_heads=nkv)
                kv4 = L["kv"].view(self.B_max, Smax, 2, nkv, hd)[b0:b0 + B, : ph["Lk"]]
                ops.attention(q4, kv4[:, :, 0], kv4[:, :, 1], causal=True, out=att.view(B, S, nh, hd), k_len=ph["k_len"],
                              rope=(cos, sin, kn4, vn4) if fuse_rope else None)
            self._linear(att, L, "o_w", quant, residual=src, out=x)
            if fused_norm:
                self._linear(x, L, "gu_w", quant, act="silu", glu=True, out=ff, prenorm=(L["n2"], 1e-6))
            else:
                ops.norm(x, L["n2"], None, eps=1e-6, rms=True, out=h)
                self._linear(h, L, "gu_w", quant, act="silu", glu=True, out=ff, w_frag=wf("gu_wf"))
            self._linear(ff, L, "down_w", quant, residual=x, out=x, w_frag=wf("down_wf"))
            if self.tap is not None:
                self.tap("llm", li, x)

    def _suffix_phase(self, slot, next_pos, pfx_len, suf_len, m: int, tail_row=None, tail_len=None) -> dict:
        """host side of a suffix pass (`suffix_pass`, `latents_behind`): P pairs x m tokens; pair p continues the prompt in cache slot slot[p]
        (pfx_len[p] cached tokens, next text position next_pos[p]) with suf_len[p] <= m tokens of its own. Positions are next_pos + i on all
        three m-rope axes - what a decode would give the same tokens. tail_row / tail_len (together, optional): between its slot's rows and
        its own tokens pair p also sees the first tail_len[p] rows of row tail_row[p] of the shared-prompt tails (ops.attention_prefix_tail)."""
        slot, pfx_len, suf_len = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (slot, pfx_len, suf_len))
        P = slot.size
        assert P >= 1 and pfx_len.size == P and suf_len.size == P and np.asarray(next_pos).size == P
        if not 1 <= m <= ops.ATTN_PREFIX_MAX_ROWS:
            raise ValueError(f"a suffix pass runs 1 .. {ops.ATTN_PREFIX_MAX_ROWS} tokens per pair, got {m}")
        if P * m > self.x.shape[0]:
            raise CapacityError(f"suffix pass of {P} x {m} tokens exceeds the engine's {self.x.shape[0]} buffer rows")
        assert int(slot.min()) >= 0 and int(slot.max()) < self.B_max and int(pfx_len.min()) >= 0 and int(pfx_len.max()) <= self.S_max
        assert int(suf_len.min()) >= 0 and int(suf_len.max()) <= m
        pos = (np.asarray(next_pos, dtype=np.int64).reshape(-1, 1) + np.arange(m)[None]).reshape(1, P * m)
        prefix = dict(slot=self._i32(slot), pfx_len=self._i32(pfx_len), suf_len=self._i32(suf_len), max_pfx=int(pfx_len.max()))
        if tail_row is not None:
            bufs = self._shared
            tail_row, tail_len = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (tail_row, tail_len))
            assert bufs is not None and tail_row.size == P and tail_len.size == P
            assert int(tail_row.min()) >= 0 and int(tail_row.max()) < bufs.rows and int(tail_len.min()) >= 0 and int(tail_len.max()) <= bufs.T
            prefix["tail"] = dict(tails=bufs.tails, rows=bufs.rows, T=bufs.T, tail_row=self._i32(tail_row), tail_len=self._i32(tail_len), max_tail=int(tail_len.max()))
        return dict(B=P, S=m, pos=self._i32(np.broadcast_to(pos, (3, P * m))), b0=0, r0=0, prefix=prefix)

    def suffix_pass(self, state: dict, prompt_of, tokens, suf_len) -> torch.Tensor:
        """teacher-forced continuation of prefilled prompts WITHOUT touching their cache slots: pair p runs tokens[p, :suf_len[p]] (int [P, m],
        right-padded) behind prompt prompt_of[p] of `state` (what `prefill` returned). -> x f32 [P * m, H] (a view of the engine's residual
        buffer: row p * m + i is the last hidden state at suffix position i; the prompts' own rows in that buffer are overwritten)."""
        tokens = np.asarray(tokens, dtype=np.int64)
        P, m = tokens.shape
        prompt_of = np.asarray(prompt_of, dtype=np.int64).reshape(-1)
        assert prompt_of.size == P and int(prompt_of.min()) >= 0 and int(prompt_of.max()) < state["B"]
        pl = _prompt_lens(state["B"], state["S"], state.get("lens"))
        ph = self._suffix_phase(prompt_of, np.asarray(state["next_pos"])[prompt_of], pl[prompt_of], suf_len, m)
        ops.gather_rows(self.embed, self.x_in, src=self._i32(tokens.reshape(-1)), rows=P * m)
        self._layers(ph)
        return self.x[: P * m]

    def _last_logits(self, B: int, S: int, row_in_seq, rows_idx: Optional[torch.Tensor] = None):
        """the plain greedy first selection (`s2_select.Selection.first` without options): final RMSNorm + lm_head on ONE row per sequence of
        x rows B x S, argmax on the device -> next_tok[:B]"""
        Selection(self, {}).first(B, S, row_in_seq, rows_idx)

    def last_logprobs(self, state: dict):
        """(logprob, margin) f32 [B, n] device views: one value per answer token selected so far from `state` (what `prefill` returned and
        `decode` advanced, or a plan after `run_decode`: all n_decode positions). logprob = log_softmax of the repetition-penalised logits at
        the chosen token (HF compute_transition_scores(normalize_logits=True) on processed scores), margin = its distance to the runner-up.
        Views of the engine's buffers: the next call overwrites them."""
        if not self.token_logprobs:
            raise RuntimeError("this engine was built without token_logprobs=True (QwenVLEngine(..., token_logprobs=True) / "
                               "model_settings['token_logprobs'] / from_pretrained(token_logprobs=True))")
        n = int(state["n_sel"]) if "n_sel" in state else int(state.get("n_decode", 0))
        return self.tok_logprob[: state["B"], :n], self.tok_margin[: state["B"], :n]

    def last_sample_logprobs(self, state: dict) -> torch.Tensor:
        """f32 [rows, n] device view: log q of every token drawn so far from a sampling `state` (rows = B * num_return_sequences), the
        log-softmax of HF's processed scores (penalty, temperature, top-k, top-p) at the draw. A view: the next sampling call overwrites it."""
        assert "sampling" in state, "not a sampling state (prefill(..., sampling=...))"
        return state["select"].bufs._smp_lp.t()[: state["B"], : int(state.get("n_sel", 0))]

    def _replicate(self, state: dict, K: int):
        """`state` becomes the decode state of B * K rows, prompt-major (HF's repeat_interleave): next_pos / lens / cur replicated"""
        state["B"] *= K
        state["next_pos"] = np.repeat(np.asarray(state["next_pos"]), K)
        if state.get("lens") is not None:
            state["lens"] = np.repeat(np.asarray(state["lens"], dtype=np.int64), K)
            state["cur"] = state["lens"].copy()
        state["fan"] = K

    def _fan_out(self, state: dict, K: int):
        """num_return_sequences = K behind ONE prefill: the prompt rows of cache slot b go to slots b * K + c (ina_kv_copy, out to temporary
        tensors and back in - source slots are destinations too: two launches for the whole batch), and `state` becomes the decode state of
        B * K rows (`_replicate`). The seen rows were replicated in front of the
        first draw, which marks them per returned sequence."""
        B = state["B"]
        n = _prompt_lens(B, state["S"], state.get("lens"))
        self._kv_evict({slot: 0 for slot in range(B * K)})
        tmp = [torch.empty(len(self.layers), int(n[b]), self.kv_w, dtype=torch.bfloat16, device=self.device) for b in range(B)]
        self._kv_copy([(tmp[b], b, int(n[b])) for b in range(B)], to_engine=False)
        self._kv_copy([(tmp[b], b * K + c, int(n[b])) for b in range(B) for c in range(K)], to_engine=True)
        self._replicate(state, K)

    def _shared_buffers(self, rows: int, T: int) -> SimpleNamespace:
        """the buffers of the shared-prompt sampling path, sized by its ROW count (returned sequences), not by max_seqs: twins of logits /
        next_tok / seen / xl / hl / _smp_lp (what a selection touches, `s2_select.Selection.bufs`) and per layer a tail [rows * T, 2 * Hkv * hd]
        in the cache's row format (row r keeps the k|v of its answer token t at tail row r * T + t). Allocated by the first shared call, grown
        only when a later call needs more rows or a longer answer (T <= max_decode); an engine that never takes the path allocates nothing."""
        sh = self._shared
        if sh is not None and sh.rows >= rows and sh.T >= T:
            return sh
        rows, T = max(rows, sh.rows if sh else 0), max(T, sh.T if sh else 0)
        self._shared = sh = None                                  # (the old set goes before the new one comes)
        dev, bf, f32 = self.device, torch.bfloat16, torch.float32
        self._shared = SimpleNamespace(
            rows=rows, T=T, logits=torch.empty(rows, self.cfg["vocab"], dtype=f32, device=dev), next_tok=torch.empty(rows, dtype=torch.int32, device=dev),
            seen=torch.zeros(rows, self.seen.shape[1], dtype=torch.uint32, device=dev), xl=torch.empty(rows, self.H, dtype=f32, device=dev),
            hl=torch.empty(rows, self.H, dtype=bf, device=dev), _smp_lp=torch.zeros(T, rows, dtype=f32, device=dev), _cstate=None, _rhist=None,
            tails=[torch.empty(rows * T, self.kv_w, dtype=bf, device=dev) for _ in self.layers])
        return self._shared

    def _share_out(self, state: dict, K: int):
        """num_return_sequences = K behind ONE prefill WITHOUT a cache slot per returned sequence (sampling spec share_prefix): `state` becomes
        the decode state of B * K rows (`_replicate`); row b * K + c keeps
        reading prompt b in cache slot b (pfx_len = the prompt's length) and appends its own answer tokens to its tail (tail_len = 0 here).
        Host work only: the tile table of ops.attention_shared (rows of one prompt share a tile) and its per-tile slot / length."""
        B = state["B"]
        n = _prompt_lens(B, state["S"], state.get("lens"))
        prompt_of = np.repeat(np.arange(B), K)
        tiles, owner = ops.attention_shared_plan(prompt_of, self.nh // self.nkv)
        state["shared"] = dict(slot=prompt_of, pfx_len=n[prompt_of], tail_len=0, tile_rows=self._i32(tiles), tile_slot=self._i32(owner),
                               tile_pfx=self._i32(n[owner]), max_pfx=int(n.max()))
        self._replicate(state, K)

    def _shared_phase(self, state: dict) -> dict:
        """host side of one single-token pass of the shared-prompt path: every row runs its pending token at text position next_pos, appends
        its k|v at tail row tail_len (all rows advance together) and attends its prompt + tail_len + 1 tail rows"""
        sh, bufs, R = state["shared"], self._shared, state["B"]
        t = int(sh["tail_len"])
        assert t < bufs.T and R <= bufs.rows, (t, bufs.T, R, bufs.rows)
        pos = np.broadcast_to(np.asarray(state["next_pos"], dtype=np.int64).reshape(1, R), (3, R))
        return dict(B=R, S=1, pos=self._i32(pos), b0=0, r0=0,
                    shared=dict(tails=sh.get("tails", bufs.tails), T=bufs.T, kv_dst=self._i32(np.arange(R) * bufs.T + t), tail_len=self._i32(np.full(R, t + 1)),
                                tile_rows=sh["tile_rows"], tile_slot=sh["tile_slot"], tile_pfx=sh["tile_pfx"], max_pfx=sh["max_pfx"]))

    def _beam_buffers(self, rows: int, T: int) -> SimpleNamespace:
        """the buffers of the beam path beside the shared-prompt twins (`_shared_buffers(rows, T)`, whose logits / next_tok / xl / hl, seen set and
        tails are set 0 here): a second tail set and a second seen set (every step re-parents the rows from the current set into the other,
        ops.beam_reorder, with the layers' base addresses in device tables), the automaton states (what the mask wrote | gathered by parent),
        the candidate lists, the running scores / parents / token histories and transition scores (ping-pong) and the finished sets.
        Allocated by the first beam call, again when the twins were regrown; an engine that never takes the path allocates nothing."""
        sh = self._shared_buffers(rows, T)
        bm = self._beam
        if bm is not None and bm.sh is sh:
            return bm
        self._beam = bm = None
        dev, R, Tt = self.device, sh.rows, sh.T
        z = lambda *shape, dt=torch.int32: torch.zeros(*shape, dtype=dt, device=dev)      # noqa: E731
        f32 = torch.float32
        tails2 = [torch.empty_like(t) for t in sh.tails]
        base = torch.tensor([[t.data_ptr() for t in sh.tails], [t.data_ptr() for t in tails2]], dtype=torch.int64, device=dev)
        self._beam = SimpleNamespace(
            sh=sh, tails=[sh.tails, tails2], base=base, seen=[sh.seen, torch.zeros_like(sh.seen)], cstate=z(2, R),
            cand_score=z(R * ops.BEAM_MAX_CANDIDATES, dt=f32), cand_tok=z(R * ops.BEAM_MAX_CANDIDATES), run_score=z(R, dt=f32), parent=z(R),
            hist=z(2, R, Tt), ts=z(2, R, Tt, dt=f32), fin_tok=z(R, Tt), fin_ts=z(R, Tt, dt=f32), fin_score=z(R, dt=f32), fin_len=z(R), fin_flag=z(R),
            heur=z(R), done=z(R))
        return self._beam

    def _beam_view(self, beam: dict, R: int) -> SimpleNamespace:
        """the state ops.beam_step works on: the first R rows (R // K prompts) of the beam buffers; next_tok is the twins' (the next pass embeds it)"""
        bm, K = self._beam, beam["K"]
        return SimpleNamespace(K=K, eos=beam["eos_t"], run_score=bm.run_score[:R], next_tok=bm.sh.next_tok[:R], parent=bm.parent[:R],
                               hist=[bm.hist[0, :R], bm.hist[1, :R]], ts=[bm.ts[0, :R], bm.ts[1, :R]], fin_tok=bm.fin_tok[:R], fin_ts=bm.fin_ts[:R],
                               fin_score=bm.fin_score[:R], fin_len=bm.fin_len[:R], fin_flag=bm.fin_flag[:R], heur=bm.heur[: R // K], done=bm.done[: R // K])

    def _beam_state(self, spec: dict, B: int) -> dict:
        """validated copy of a beam spec (`prefill`); every capacity error is raised here, before anything is launched"""
        K, T = int(spec["K"]), int(spec["max_new_tokens"])
        eos = tuple(int(e) for e in spec.get("eos", ()))
        lp, early = float(spec.get("length_penalty", 1.0)), spec.get("early_stopping", False)
        if K < 2 or T < 1 or not np.isfinite(lp) or not any(early is v for v in (False, True)) and early != "never":
            raise ValueError(f"beam spec: K={K} (>= 2), max_new_tokens={T} (>= 1), length_penalty={lp} (finite), early_stopping={early!r} (False, True, 'never')")
        if self.hd != 128 or self.nh // self.nkv > ops.ATTN_SHARED_MAX_GROUP:
            raise ValueError(f"beam search needs head dim 128 and at most {ops.ATTN_SHARED_MAX_GROUP} query heads per KV head (ops.attention_shared), "
                             f"this model has {self.hd} and {self.nh // self.nkv}")
        M = max(2, 1 + len(eos)) * K
        if K > 8 or len(eos) > 3 or M > ops.BEAM_MAX_CANDIDATES or M > self.cfg["vocab"]:
            raise CapacityError(f"num_beams={K} with {len(eos)} EOS ids: at most 8 beams and 3 EOS ids ({ops.BEAM_MAX_CANDIDATES} candidates per prompt)")
        if B > self.B_max or B * K > min(SKINNY_GEMM_MAX_ROWS, self.x.shape[0]):
            raise CapacityError(f"{B} prompts x {K} beams exceed max_seqs={self.B_max} prompts or {min(SKINNY_GEMM_MAX_ROWS, self.x.shape[0])} rows "
                                "(the single-token passes stay on the weight-streaming kernels)")
        if T > self.max_decode:
            raise CapacityError(f"max_new_tokens={T} exceeds the engine's max_decode={self.max_decode}")
        self._beam_buffers(B * K, T)
        eos_t = torch.tensor(eos, dtype=torch.int32, device=self.device) if eos else None
        return dict(K=K, M=M, eos=eos, eos_t=eos_t, max_new_tokens=T, length_penalty=lp, early_stopping=early, flip=0)

    def beam_results(self, state: dict) -> SimpleNamespace:
        """the finished sets of a beam state after `decode`, on the host, [B, K, ...] best first: tokens int64 [B, K, T], token_scores f32 (the
        hypotheses' per-token transition scores), scores f32 / lengths int64 / finished bool [B, K], done bool [B], and the running rows' tokens /
        scores / parents of the last step (what the step-by-step tests read)"""
        bm, K, R = self._beam, state["beam"]["K"], state["B"]
        B, n, h = R // K, int(state.get("n_sel", 0)), state.get("n_sel", 0) & 1        # (step j wrote history half 1 - (j & 1))
        c = lambda t: t.cpu()                                                            # noqa: E731
        return SimpleNamespace(tokens=c(bm.fin_tok[:R]).long().view(B, K, -1), token_scores=c(bm.fin_ts[:R]).view(B, K, -1), scores=c(bm.fin_score[:R]).view(B, K),
                               lengths=c(bm.fin_len[:R]).long().view(B, K), finished=c(bm.fin_flag[:R]).bool().view(B, K), done=c(bm.done[:B]).bool(),
                               heur=c(bm.heur[:B]).bool(), run_tokens=c(bm.hist[h, :R, :n]).long().view(B, K, n), run_token_scores=c(bm.ts[h, :R, :n]).view(B, K, n),
                               run_scores=c(bm.run_score[:R]).view(B, K), parents=c(bm.parent[:R]).long().view(B, K) - torch.arange(B).view(B, 1) * K)

    def beam_done(self, state: dict) -> torch.Tensor:
        """bool [B] on the host: which prompts of a beam state are done (the one read `generate` makes per decode chunk)"""
        return self._beam.done[: state["B"] // state["beam"]["K"]].cpu().bool()

    # ---- plan / run: all host work up front, then a pure launch sequence (hipGraph capturable)
    def plan(self, input_ids, image_grid_thw, n_decode: int = 0, with_latents: bool = False, cached_embeds: Optional[list] = None,
             prefix_len=0, repetition_penalty: float = 1.0, seq_lens=None, constraint=None, logit_rules=None) -> dict:
        """Host-side plan of one S2 call for B equal-length prompts: embedding / scatter indices, vision plan, position ids and cache
        rows of the prefill, of every decode step and of the latent-query pass (fixed-length answers of n_decode tokens).
        cached_embeds: one entry per image (prompt order over the batch), None = run the vision tower on it, else its merged embeddings
        bf16 [h*w/4, H] in token order from an earlier call (per-frame ViT cache, SURVEY.md 8f-1: the tower attends per image, so a
        frame's embeddings do not depend on what else is in the batch). pixel_values then holds the patches of the fresh images only.
        prefix_len (prefix-KV reuse, SURVEY.md 7 / DESIGN 8.5): the first prefix_len tokens of EVERY sequence are not run - their K/V of
        all layers are already in the cache slots of this batch (`import_prefix_kv`, from an earlier call whose prompt started with the
        same tokens: system prompt + instruction + first history frame between the System-2 calls of an episode). With a causal mask
        the K/V of a token depend on the tokens before it only, so the suffix sees exactly what a full prefill would have cached.
        Images whose tokens lie inside the prefix are not encoded (pixel_values holds the patches of the other images); the prefix
        must end on an image boundary. prefix_len may be an int or one value per sequence (0 = nothing cached for that sequence): the
        call then runs a right-padded rectangle of max(S - prefix_len) tokens per sequence behind each sequence's own prefix.
        repetition_penalty (generation_config.json; HF RepetitionPenaltyLogitsProcessor): != 1.0 makes every greedy selection of the decode
        run over the penalised logits of the tokens seen so far - the WHOLE prompt (image placeholders and tokens whose K/V came from a
        cache included; seq_lens [B] real tokens of right-padded prompts) plus the answer. The plan then uploads the full ids [B, S] and the
        lengths; with 1.0 nothing is uploaded and the launch sequence is the plain one.
        constraint (a constrain.TokenAutomaton over this vocabulary; None = unconstrained, nothing allocated, every launch what it was):
        every selection of run_decode / decode runs behind ops.automaton_mask_rows (`s2_select.Selection`). The tables are uploaded and the state
        buffers allocated HERE, so the launch sequence stays capturable.
        logit_rules (a logit_rules.CompiledRules made for THIS call - its vocabulary, one prompt length per sequence, max_new_tokens >= n_decode;
        None = no rules, nothing allocated, every launch what it was): every selection of run_decode / decode runs behind
        ops.logit_rules_rows (`s2_select.Selection`). The tables and the full ids [B, S] are uploaded and the histories allocated HERE; P["rules_key"]
        is the rule set's identity (a cache of captured graphs keys on it beside the prompt geometry). ValueError for another vocabulary or
        other prompt lengths, CapacityError when prompt + answer exceed the history rows (max_seq_len + max_decode tokens)."""
        cfg, dev = self.cfg, self.device
        if constraint is not None:
            if getattr(constraint, "vocab", None) != cfg["vocab"]:
                raise ValueError(f"constraint: an automaton over {getattr(constraint, 'vocab', None)} tokens, this model has {cfg['vocab']}")
            constraint.to(dev)
        pen = float(repetition_penalty)
        if not (np.isfinite(pen) and pen > 0.0):
            raise ValueError(f"repetition_penalty={repetition_penalty!r}: HF requires a strictly positive float")
        ids = _ids_np(input_ids)
        B, S = ids.shape
        if B > self.B_max or S > self.S_max:
            raise CapacityError(f"System-2 batch of {B} x {S} tokens exceeds the engine's max_seqs={self.B_max} / max_seq_len={self.S_max}")
        if self.token_logprobs and n_decode > self.max_decode:      # here, not inside run_decode: that may run under a graph capture
            raise CapacityError(f"n_decode={n_decode} answer tokens exceed the engine's max_decode={self.max_decode} log-probability columns")
        pl = np.broadcast_to(np.asarray(prefix_len, dtype=np.int64).reshape(-1), (B,)).copy()
        assert int(pl.min()) >= 0 and int(pl.max()) < S, f"prefix_len={pl.tolist()} must leave at least one token of the {S}-token prompts to run"
        # the planned decode / latent passes read every sequence's first token at row S_run - 1 of its rectangle: only uniform prefixes put
        # the last real token there (ragged prefixes decode through the eager `decode()`, which carries per-sequence row indices) - ADVICE r3
        assert (n_decode == 0 and not with_latents) or int(pl.min()) == int(pl.max()), \
            f"plan(n_decode={n_decode}, with_latents={with_latents}) needs ONE prefix length for all sequences, got {pl.tolist()}: use prefill() + decode()"
        grids = grids_all = _grid_list(image_grid_thw)
        Sr = S - int(pl.min())                                    # tokens per sequence this call runs (rectangle width)
        run = np.zeros((B, Sr), dtype=np.int64)                   # row b = ids[b, pl[b]:] right-padded
        for b in range(B):
            run[b, : S - pl[b]] = ids[b, pl[b]:]
        flat = run.reshape(-1)
        P = dict(B=B, S=S, S_run=Sr, prefix_len=pl, n_decode=n_decode, ids=self._i32(flat), vision=None, cached=[], fresh_tokens=[])
        lens = _prompt_lens(B, S, seq_lens)
        if pen != 1.0:
            assert int(lens.min()) >= 1 and int(lens.max()) <= S
            P["rep_penalty"] = pen
            P["rep_ids"] = self._i32(ids)
            P["rep_lens"] = self._i32(lens)
        if constraint is not None:
            P["constraint"] = constraint
        if logit_rules is not None:
            if logit_rules.vocab != cfg["vocab"] or logit_rules.len0.tolist() != lens.tolist():
                raise ValueError(f"logit_rules: compiled for {logit_rules.vocab} tokens and prompt lengths {logit_rules.len0.tolist()}, this call has "
                                 f"{cfg['vocab']} and {lens.tolist()}")
            if int(lens.max()) + max(int(n_decode), 1) > self.S_max + self.max_decode:
                raise CapacityError(f"logit_rules: prompt of {int(lens.max())} tokens + {n_decode} answer tokens exceed the "
                                    f"{self.S_max + self.max_decode} tokens of a history row (max_seq_len + max_decode)")
            P["rules"] = dict(tabs=logit_rules.to(dev), ids=P["rep_ids"] if "rep_ids" in P else self._i32(ids))
            P["rules_key"] = logit_rules.key
        img_pos = np.nonzero(flat == cfg["image_token_id"])[0].astype(np.int32)
        if grids:
            ntok_all = [t * h * w // 4 for t, h, w in grids]
            # images inside the prefix: their tokens are cached K/V, nothing of them is needed (neither pixels nor embeddings)
            imgs = list(prompt_images(ids, ntok_all, cfg["image_token_id"]))
            assert len(imgs) == len(grids), "image count of the prompts and image_grid_thw disagree"
            for b, first, last in imgs:
                assert last < pl[b] or first >= pl[b], "the cached prefix must end on an image boundary"
            img_seq = [b for b, _, _ in imgs]
            keep = [k for k, (b, _, last) in enumerate(imgs) if last >= pl[b]]
            P["images_run"] = keep
            cached_all = list(cached_embeds) if cached_embeds is not None else [None] * len(grids)
            assert len(cached_all) == len(grids)
            grids = [grids_all[k] for k in keep]
            cached_embeds = [cached_all[k] for k in keep]
            ntok = [ntok_all[k] for k in keep]
            assert img_pos.size == sum(ntok), f"Image features and image tokens do not match: tokens: {img_pos.size}, features {sum(ntok)}"
            off = np.concatenate([[0], np.cumsum(ntok)])
            cached = list(cached_embeds)
            fresh = [k for k, c in enumerate(cached) if c is None]
            if fresh:
                vp = self.plan_vision([grids[k] for k in fresh])
                dst = np.concatenate([img_pos[off[k]:off[k + 1]] for k in fresh])
                P["vision"], P["img_src"], P["img_dst"] = vp, torch.from_numpy(vp["inv"]).to(dev), torch.from_numpy(dst).to(dev)
                P["_split_info"] = (img_seq, ntok, off, img_pos) if (len(fresh) == len(grids_all) and int(pl.max()) == 0) else None
                o = 0
                for k in fresh:
                    P["fresh_tokens"].append((keep[k], o, o + ntok[k]))      # rows of emb_tok that hold image keep[k] (index over ALL images) after run_prefill
                    o += ntok[k]
            for k, c in enumerate(cached):
                if c is not None:
                    assert c.shape == (ntok[k], self.H) and c.dtype == torch.bfloat16, f"cached embeds of image {k}: {tuple(c.shape)} vs grid {grids[k]}"
                    P["cached"].append((c, torch.from_numpy(img_pos[off[k]:off[k + 1]]).to(dev)))
        traj_pos = np.nonzero(flat == cfg["traj_token_id"])[0].astype(np.int32)
        if traj_pos.size:
            nq = self.latent_q.shape[0]
            P["traj_src"] = torch.from_numpy((np.arange(traj_pos.size) % nq).astype(np.int32)).to(dev)
            P["traj_dst"] = torch.from_numpy(traj_pos).to(dev)
        pos3, _ = rope_index(ids, grids_all, cfg["image_token_id"], cfg["vision_start_id"])
        if int(pl.max()) == 0:
            P["prefill"] = self._phase(B, Sr, pos3, 0)
            info = P.pop("_split_info", None)
            if self.split_prefill and B >= 2 and info is not None:
                # two half batches (sequences [0, Ba) and [Ba, B)) with their own vision plans: same buffers, disjoint row ranges
                img_seq, ntok, off, img_pos = info
                P["split"] = []
                Ba = (B + 1) // 2
                for b0, b1 in ((0, Ba), (Ba, B)):
                    ks = [k for k in range(len(grids_all)) if b0 <= img_seq[k] < b1]
                    if not ks or ks != list(range(ks[0], ks[-1] + 1)):
                        P.pop("split")
                        break
                    vp = self.plan_vision([grids_all[k] for k in ks])
                    vp["p0"] = int(sum(t * h * w for t, h, w in grids_all[: ks[0]]))
                    P["split"].append(dict(vision=vp, img_src=torch.from_numpy(vp["inv"]).to(dev), tok0=int(off[ks[0]]), n_tok=int(off[ks[-1] + 1] - off[ks[0]]),
                                           img_dst=torch.from_numpy(np.concatenate([img_pos[off[k]:off[k + 1]] for k in ks])).to(dev),
                                           prefill=self._phase(b1 - b0, Sr, pos3[:, b0:b1], 0, b0=b0)))
        P.pop("_split_info", None)
        if int(pl.max()) != 0:
            pos_run = np.zeros((3, B, Sr), dtype=np.int64)
            for b in range(B):
                n = S - pl[b]
                pos_run[:, b, :n] = pos3[:, b, pl[b]:]
                pos_run[:, b, n:] = pos3[:, b, -1:]                # pad rows: any position (never attended by real tokens, causal)
            uniform = bool((pl == pl[0]).all())
            # per-sequence prefixes: query i of sequence b sees keys <= pl[b] + i (the kernels align the causal mask to each k_len)
            P["prefill"] = self._phase(B, Sr, pos_run, pl, k_len=None if uniform else pl + Sr)
        nxt = pos3[:, :, -1].max(axis=0) + 1                      # text position of the first generated token, per sequence
        P["next_pos"] = nxt
        P["decode"] = [self._phase(B, 1, (nxt + j)[None, :, None], S + j) for j in range(max(n_decode - 1, 0))]
        if with_latents:
            nq = self.latent_q.shape[0]
            cur = S + max(n_decode - 1, 0)                        # cached tokens after the decode steps
            m = 1 if n_decode > 0 else 0                          # the last sampled token has no K/V yet
            p = (nxt + (cur - S))[None, :, None] + np.arange(m + nq)[None, None, :]
            P["latents"] = self._phase(B, m + nq, p, cur)
            P["lat_m"] = m
        P["select"] = Selection(self, P)                          # (allocates the automaton states / histories of a constrained / ruled call)
        return P

    def run_prefill(self, P: dict, pixel_values: Optional[torch.Tensor]):
        if self._kv_views:                                        # live KV handles on rows this prefill writes: ONE export launch for all
            self._kv_evict({b: int(w) for b, w in enumerate(P["prefill"]["w0"])})
        ops.gather_rows(self.embed, self.x_in, src=P["ids"])
        if self.split_prefill and P.get("split") and self.tap is None:
            if "traj_src" in P:
                ops.gather_rows(self.latent_q, self.x_in, src=P["traj_src"], dst=P["traj_dst"])
            main = torch.cuda.current_stream()
            if self._side is None:
                self._side = torch.cuda.Stream(device=self.device)
            self._side.wait_stream(main)

            def half(s):
                vp = s["vision"]
                emb = self.run_vision(vp, pixel_values[vp["p0"]: vp["p0"] + vp["Np"]])
                tok = self.emb_tok[s["tok0"]: s["tok0"] + s["n_tok"]]
                ops.gather_rows(emb, tok, src=s["img_src"])                   # window order -> image-token order (kept for the frame cache)
                ops.gather_rows(tok, self.x_in, dst=s["img_dst"])
                self._layers(s["prefill"])

            # both halves' GEMMs run beside each other: tiles are picked without the quantisation charge (ops.shared_tail; decoder chain of
            # 3 + 3 envs 61.8 vs 64.2 ms, 4 + 3 envs 73.4 vs 74.5 ms, vision chain 28.0 vs 28.7 ms: profiles/r03x_native_chain_partitions.log)
            with ops.shared_tail():
                if self.split_serial:        # profiling: the SAME launches (half batches, shared-tail tile selection) back to back on one stream
                    half(P["split"][1])
                else:
                    with torch.cuda.stream(self._side):
                        half(P["split"][1])
                half(P["split"][0])
            main.wait_stream(self._side)
            return
        if P["vision"] is not None:
            emb = self.run_vision(P["vision"], pixel_values)
            n = P["img_src"].shape[0]
            ops.gather_rows(emb, self.emb_tok[:n], src=P["img_src"])          # window order -> image-token order (kept for the frame cache)
            ops.gather_rows(self.emb_tok[:n], self.x_in, dst=P["img_dst"])
        for c, dst in P["cached"]:
            ops.gather_rows(c, self.x_in, dst=dst)
        if "traj_src" in P:
            ops.gather_rows(self.latent_q, self.x_in, src=P["traj_src"], dst=P["traj_dst"])
        self._layers(P["prefill"])

    def fresh_image_embeds(self, P: dict) -> Dict[int, torch.Tensor]:
        """image index -> a copy of its merged embeddings bf16 [h*w/4, H] (token order) as computed by the last run_prefill(P):
        what a caller stores in its per-frame cache and hands back through plan(..., cached_embeds=...)."""
        return {k: self.emb_tok[a:b].clone() for k, a, b in P["fresh_tokens"]}

    def run_decode(self, P: dict, tokens_out: torch.Tensor, j0: int = 0, j1: Optional[int] = None):
        """n_decode greedy tokens: the first from the prompt's last position, then n_decode - 1 single-token passes.
        [j0, j1): the tokens this call produces (default: all) - the chain can be issued (and captured) in pieces, e.g. to let another stream
        start between two passes; the pieces hand over through the engine's buffers (next token, KV cache) only."""
        B, S, n = P["B"], P["S_run"], P["n_decode"]               # rows of x: the tokens this call ran (all of them without a cached prefix)
        j1 = n if j1 is None else min(j1, n)
        if n == 0 or j0 >= j1:
            return
        sel = P["select"]
        if j0 == 0:
            sel.first(B, S, S - 1)
        for j in range(j0, j1):
            self._decode_step(sel, B, tokens_out[:, j], None if j == n - 1 else lambda: P["decode"][j], j + 1)      # (a callable: `decode` must make its phase inside the step)

    def _decode_step(self, sel: Selection, B: int, out: torch.Tensor, phase, col: int, shared: Optional[dict] = None):
        """one step of `run_decode` / `decode`: emit the B tokens the last selection chose into `out`, then - unless they are the call's last
        (phase None) - embed them, run the single-token pass and select answer column `col`. phase: a callable that gives the pass's phase;
        it is called behind `sel.reparent`, which turns the tails a beam state's phase reads (shared = state["shared"])."""
        out.copy_(sel.next_tok[:B])
        if phase is None:
            return
        sel.reparent(B, shared)
        ops.gather_rows(self.embed, self.x_in, src=sel.next_tok[:B], rows=B)
        self._layers(phase())
        sel.step(B, col)

    def _latent_pass(self, R: int, m: int, ph: dict, tail: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the N_QUERY latent queries of R rows, each behind m tail rows, as the pass `ph` over R x (m + N_QUERY) rows of x_in; the query
        rows go through the final RMSNorm -> out bf16 [R, N_QUERY, H]. tail int32 [R * m]: the tail tokens, embedded here (None with
        m > 0: the caller has placed their embeddings itself)."""
        nq, H = self.latent_q.shape[0], self.H
        x3 = self.x_in[: R * (m + nq)].view(R, m + nq, H)
        if tail is not None:
            tmp = self.hl[: R * m]
            ops.gather_rows(self.embed, tmp, src=tail, rows=R * m)
            x3[:, :m].copy_(tmp.view(R, m, H))
        x3[:, m:].copy_(self.latent_q.view(1, nq, H).expand(R, nq, H))
        self._layers(ph)
        out = torch.empty(R, nq, H, dtype=torch.bfloat16, device=self.device) if out is None else out
        ops.norm(self.x[: R * (m + nq)], self.norm_w, None, eps=1e-6, rms=True, out=out.view(R * nq, H), rows=R * nq, in_map=(nq, m + nq, m))
        return out

    def run_latents(self, P: dict, out: torch.Tensor):
        """N_QUERY latent queries (behind the last sampled token) against the KV cache -> out bf16 [B, N_QUERY, H]."""
        self._latent_pass(P["B"], P["lat_m"], P["latents"], self.next_tok[: P["B"]] if P["lat_m"] else None, out)

    def run_s2(self, P: dict, pixel_values, tokens_out: torch.Tensor, latents_out: Optional[torch.Tensor]):
        """whole System-2 call as one launch sequence: ViT + prefill + n_decode greedy tokens (+ latent queries)."""
        self.run_prefill(P, pixel_values)
        self.run_decode(P, tokens_out)
        if latents_out is not None:
            self.run_latents(P, latents_out)

    # ---- prefix-KV reuse: the K/V of a prompt prefix leave / re-enter the batch's cache slots (device copies, no arithmetic)
    def images_in_prefix(self, input_ids, image_grid_thw, prefix_len) -> List[bool]:
        """per image of the batch (prompt order): do all of its tokens lie inside its sequence's cached prefix?"""
        ids = _ids_np(input_ids)
        pl = np.broadcast_to(np.asarray(prefix_len, dtype=np.int64).reshape(-1), (ids.shape[0],))
        ntok = [t * h * w // 4 for t, h, w in _grid_list(image_grid_thw)]
        return [last < pl[b] for b, _, last in prompt_images(ids, ntok, self.cfg["image_token_id"])]

    def export_prefix_kv(self, seq: int, n_tokens: int) -> torch.Tensor:
        """K/V of the first n_tokens cached tokens of batch slot `seq`, all layers: bf16 [layers, n_tokens, 2 * kv_heads * head_dim]
        (a copy: what a caller keeps per environment between the System-2 calls of an episode)."""
        assert 0 <= seq < self.B_max and 0 < n_tokens <= self.S_max
        return torch.stack([L["kv"].view(self.B_max, self.S_max, self.kv_w)[seq, :n_tokens] for L in self.layers])

    def import_prefix_kv_batch(self, kv: torch.Tensor):
        """kv bf16 [m, layers, n, kv_w]: the prefixes of m environments into batch slots 0 .. m-1 (one strided copy per layer)."""
        m, nl, n, w = kv.shape
        assert nl == len(self.layers) and w == self.kv_w and m <= self.B_max and n <= self.S_max and kv.dtype == torch.bfloat16
        if self._kv_views:
            self._kv_evict({b: 0 for b in range(m)})
        for li, L in enumerate(self.layers):
            L["kv"].view(self.B_max, self.S_max, self.kv_w)[:m, :n].copy_(kv[:, li])

    def import_prefix_kv(self, seq: int, kv: torch.Tensor):
        """put an exported prefix back into batch slot `seq` (before plan(..., prefix_len=kv.shape[1]) / prefill(..., prefix_len=))."""
        n = kv.shape[1]
        assert kv.shape == (len(self.layers), n, self.kv_w) and kv.dtype == torch.bfloat16 and n <= self.S_max
        if self._kv_views:
            self._kv_evict({seq: 0})
        for li, L in enumerate(self.layers):
            L["kv"].view(self.B_max, self.S_max, self.kv_w)[seq, :n].copy_(kv[li])

    # ---- KV handles (EngineKVCache): views of cache slots, materialised / imported with ina_kv_copy (one launch per direction)
    def kv_handle(self, token_ids: Sequence[Optional[torch.Tensor]]) -> EngineKVCache:
        """a handle over the first len(token_ids[b]) cached rows of slots 0 .. B-1 (a view: nothing is copied now)."""
        return EngineKVCache(token_ids, None, self, [(b, int(self._slot_gen[b])) for b in range(len(token_ids))])

    def _kv_copy(self, entries, to_engine: bool):
        """entries: (tensor bf16 [layers, n, kv_w] with contiguous rows, slot, n) -> one ina_kv_copy launch over all of them."""
        if not entries:
            return
        nl, w = len(self.layers), self.kv_w
        if self._kv_base is None:
            self._kv_base = torch.tensor([L["kv"].data_ptr() for L in self.layers], dtype=torch.int64, device=self.device)
        tab = np.zeros((len(entries), 4), dtype=np.int64)
        for i, (t, slot, n) in enumerate(entries):
            assert t.dtype == torch.bfloat16 and t.device == self.device and t.dim() == 3 and t.shape[0] == nl and t.shape[2] == w
            assert t.stride(2) == 1 and t.stride(1) == w and 0 < n <= t.shape[1] and 0 <= slot < self.B_max and n <= self.S_max
            assert t.data_ptr() % 16 == 0 and (t.stride(0) * 2) % 16 == 0, "ina_kv_copy moves 16-byte units"
            tab[i] = (t.data_ptr(), t.stride(0) * 2, slot * self.S_max, n)
        ops.kv_copy(self._kv_base, torch.from_numpy(tab).to(self.device), self.B_max * self.S_max, w * 2, int(tab[:, 3].max()), to_engine)

    def materialize_kv(self, rows):
        """rows: (handle, row) pairs that are views of this engine's slots -> each gets K/V tensors of its own (one export launch)."""
        entries, todo = [], []
        for h, b in rows:
            v = h._views[b]
            if v is None or any(h is h2 and b == b2 for h2, b2 in todo):
                continue
            slot, gen = v
            if gen != self._slot_gen[slot]:
                raise RuntimeError(f"EngineKVCache row {b}: cache slot {slot} was rewritten before the handle was materialised")
            n = h.get_seq_length(b)
            t = torch.empty(len(self.layers), n, self.kv_w, dtype=torch.bfloat16, device=self.device)
            entries.append((t, slot, n))
            todo.append((h, b))
        self._kv_copy(entries, to_engine=False)
        for (h, b), (t, _, _) in zip(todo, entries):
            h.kv[b], h._views[b] = t, None
        for h, _ in todo:
            if not h.is_view:
                self._kv_views.discard(h)
                h._engine = None

    def _kv_evict(self, writes: Dict[int, int], extra=()):
        """before rows [writes[slot], ...) of the given slots are written: materialise every live view that covers one of them (plus the
        (handle, row) pairs in `extra`), all in one export launch; a slot written from row 0 starts a new generation."""
        rows = list(extra)
        for h in list(self._kv_views):
            for b, v in enumerate(h._views):
                if v is not None and v[0] in writes and h.get_seq_length(b) > writes[v[0]] and v[1] == self._slot_gen[v[0]]:
                    rows.append((h, b))
        self.materialize_kv(rows)
        for slot, w in writes.items():
            if w == 0:
                self._slot_gen[slot] += 1

    def import_kv(self, sources, prefix_len: np.ndarray):
        """sources[b]: (EngineKVCache, row) or None; prefix_len[b] leading rows of each source go into cache slot b. A source that is
        still a view of slot b itself is already in place; every other one is materialised if need be (one export launch, together
        with the live views these writes would clobber) and copied in (one import launch)."""
        writes, need = {}, []
        for b, src in enumerate(sources):
            n = int(prefix_len[b])
            if src is None or n == 0:
                writes[b] = 0
                continue
            h, r = src
            v = h._views[r]
            in_place = v is not None and h._engine is self and v[0] == b and v[1] == self._slot_gen[b]
            writes[b] = n if in_place else 0
            if not in_place:
                need.append((h, r, b, n))
        self._kv_evict(writes, extra=[(h, r) for h, r, _, _ in need if h._engine is self])
        for h, r, _, _ in need:
            assert h.kv[r] is not None, "past_key_values of another engine: materialize() it first"
        self._kv_copy([(h.kv[r], b, n) for h, r, b, n in need], to_engine=True)

    # ---- eager, stateful API (used by the policy layer: answers have data-dependent lengths)
    def prefill(self, input_ids: torch.Tensor, pixel_values: Optional[torch.Tensor], image_grid_thw, cached_embeds: Optional[list] = None,
                seq_lens=None, prefix_len: int = 0, repetition_penalty: float = 1.0, sampling: Optional[dict] = None, constraint=None,
                beam: Optional[dict] = None, logit_rules=None) -> dict:
        """seq_lens [B] (optional): RAGGED batch - input_ids is right-padded to a common length S and sequence b has seq_lens[b] real
        tokens. Causal attention keeps every real position independent of the padding behind it, so the prefill runs on the padded
        rectangle; the first token is read at each sequence's own last position and the decode / latent passes append at per-sequence
        cache positions with per-sequence key lengths (the pad rows' K/V are never attended and get overwritten).
        sampling (opt-in; None = greedy, the launch sequence it always was): dict(temperature > 0, top_k >= 0 (0 = off), top_p in (0, 1],
        u = f32 [steps, B * K] uniforms in [0, 1) drawn by the caller (row j serves answer token j), K = num_return_sequences, default 1).
        `decode` then draws every token with ops.sample_rows in place of the argmax launch (HF do_sample=True: penalty, temperature, top-k,
        top-p, multinomial) and keeps the draws' log-probabilities in a buffer of its own, allocated here on the first sampling call - an
        engine without token_logprobs=True samples as well (`last_sample_logprobs`). K > 1: the B prompts are prefilled once (images encoded
        once), the K first tokens of prompt b are drawn from its ONE logits row, its cache rows are replicated into slots b * K + c
        (`_fan_out`) and decoding continues with B * K rows, prompt-major; B * K > max_seqs raises CapacityError before anything is launched.
        share_prefix=True in the dict (opt-in, any K >= 1): no fan-out - the prompts stay in their B slots, which nothing writes after the
        prefill; row b * K + c appends the k|v of its answer tokens to a small tail of its own and ops.attention_shared reads prompt b in
        place (`_share_out`). The selection runs on row-count-sized twins of the max_seqs-sized buffers (`_shared_buffers`, allocated by the
        first such call). Capacity: B <= max_seqs and B * K <= SKINNY_GEMM_MAX_ROWS, else CapacityError before anything is launched.
        plan() / run_decode (the graph path) stay greedy.
        constraint: as in `plan` - greedy and sampled decoding alike; each returned sequence keeps an automaton state of its own.
        beam (opt-in; None = every launch what it was; not combined with sampling): dict(K = num_beams >= 2, max_new_tokens, eos = the EOS ids,
        length_penalty = 1.0, early_stopping = False | True | "never") - transformers' beam search on the shared-prompt route: the prompts stay
        in their B slots, the K hypotheses of prompt b are rows b * K .. b * K + K - 1 with tails of their own, and `decode` runs per step
        ops.beam_reorder (tails, seen sets and automaton states re-parented into the other set of a pair), the single-token pass, the
        automaton mask, ops.beam_topm_rows and ops.beam_step - no host round trip between the steps. The repetition penalty acts on the
        LOG-PROBABILITIES (HF runs its processors behind the log-softmax in beam search; the greedy and sampled paths penalise logits); with
        a constraint the scores are log-probabilities over the ALLOWED tokens (masked in front of the log-softmax, unlike HF's
        prefix_allowed_tokens_fn under beams, which masks behind it and does not renormalise). Capacity: B <= max_seqs, B * K <= 64, K <= 8,
        at most 3 EOS ids, max_new_tokens <= max_decode - CapacityError before anything is launched. Read the result with `beam_results`.
        logit_rules: as in `plan` - greedy and sampled decoding alike; each returned sequence keeps a history of its own. With beam= it raises
        NotImplementedError before anything is launched (HF applies the processors to log-probabilities there, and the histories would have
        to be re-parented)."""
        if beam is not None and logit_rules is not None:
            raise NotImplementedError("beam search (num_beams > 1) with logit rules (sequence_bias, no_repeat_ngram_size, bad_words_ids, min_length, "
                                      "min_new_tokens, forced_eos_token_id, suppress_tokens, begin_suppress_tokens) is not implemented")
        if beam is not None:
            assert sampling is None, "beam search does not sample (beam sampling is not implemented)"
            beam = self._beam_state(beam, input_ids.shape[0])
        if sampling is not None:
            sampling = self._sampling_state(sampling, input_ids.shape[0])
        P = self.plan(input_ids, image_grid_thw, cached_embeds=cached_embeds, prefix_len=prefix_len, repetition_penalty=repetition_penalty,
                      seq_lens=seq_lens, constraint=constraint, logit_rules=logit_rules)
        if sampling is not None or beam is not None:
            P["select"] = Selection(self, P, sampling, beam)          # (its state buffers, before any launch)
        self.run_prefill(P, pixel_values)
        st = self.prefill_state(P, input_ids, image_grid_thw, seq_lens)
        if sampling is not None:
            st["sampling"] = sampling
        if beam is not None:
            st["beam"] = beam
        return st

    def _sampling_state(self, spec: dict, B: int) -> dict:
        """validated copy of a sampling spec (`prefill`); allocates the sampling log-probability buffer on the first call"""
        K = int(spec.get("K", 1))
        T, top_k, top_p, u = float(spec["temperature"]), int(spec.get("top_k", 0) or 0), float(spec.get("top_p", 1.0)), spec["u"]
        if K < 1 or not (np.isfinite(T) and T > 0.0) or top_k < 0 or not 0.0 < top_p <= 1.0:
            raise ValueError(f"sampling spec: temperature={T} (> 0), top_k={top_k} (>= 0), top_p={top_p} (in (0, 1]), K={K} (>= 1)")
        share = bool(spec.get("share_prefix", False))
        if share:
            if self.hd != 128 or self.nh // self.nkv > ops.ATTN_SHARED_MAX_GROUP:
                raise ValueError(f"sampling spec: share_prefix needs head dim 128 and at most {ops.ATTN_SHARED_MAX_GROUP} query heads per KV head "
                                 f"(ops.attention_shared), this model has {self.hd} and {self.nh // self.nkv}")
            if B > self.B_max or B * K > min(SKINNY_GEMM_MAX_ROWS, self.x.shape[0]):
                raise CapacityError(f"{B} prompts x {K} returned sequences behind shared prompts exceed max_seqs={self.B_max} prompts or "
                                    f"{min(SKINNY_GEMM_MAX_ROWS, self.x.shape[0])} rows (the single-token passes stay on the weight-streaming kernels)")
        elif B * K > self.B_max:
            raise CapacityError(f"{B} prompts x {K} returned sequences exceed the engine's max_seqs={self.B_max}")
        if not (u.dtype == torch.float32 and u.dim() == 2 and u.shape[1] == B * K and u.is_contiguous() and u.device == self.device):
            raise ValueError(f"sampling spec: u must be a contiguous f32 [steps, {B * K}] tensor on {self.device}")
        if u.shape[0] > self.max_decode:
            raise CapacityError(f"{u.shape[0]} sampling steps exceed the engine's max_decode={self.max_decode} log-probability columns")
        if share:
            self._shared_buffers(B * K, int(u.shape[0]))
            return dict(temperature=T, top_k=top_k, top_p=top_p, u=u, K=K, share_prefix=True)
        if self._smp_lp is None:
            self._smp_lp = torch.zeros(self.max_decode, self.B_max, dtype=torch.float32, device=self.device)
        return dict(temperature=T, top_k=top_k, top_p=top_p, u=u, K=K)

    def prefill_state(self, P: dict, input_ids, image_grid_thw, seq_lens=None) -> dict:
        """the host-side state `prefill` returns for a plan that has been run (decode / latent passes continue from it): a function of the
        prompt GEOMETRY only (lengths, image-token positions), not of the token values - a captured prefill can be replayed on new tokens
        and pixels of the same geometry and continue from a copy of this state (trainer: graphed frozen prefix)."""
        st = dict(B=P["B"], S=P["S"], S_run=P["S_run"], next_pos=P["next_pos"].copy(), plan=P, select=P["select"])
        if seq_lens is not None:
            lens = np.asarray(seq_lens, dtype=np.int64)
            assert lens.shape == (P["B"],) and int(lens.max()) <= P["S"] and int(lens.min()) >= 1
            if bool((lens != P["S"]).any()):
                assert bool((lens > P["prefix_len"]).all()), "every sequence must have tokens behind its cached prefix"
                pos3, _ = rope_index(_ids_np(input_ids), _grid_list(image_grid_thw), self.cfg["image_token_id"], self.cfg["vision_start_id"])
                st["next_pos"] = np.asarray([int(pos3[:, b, : lens[b]].max()) + 1 for b in range(P["B"])], dtype=np.int64)
                st["lens"] = lens
        return st

    def decode(self, state: dict, n_steps: int) -> torch.Tensor:
        """n greedy steps after prefill (or after a previous decode); returns int32 [B, n] generated tokens (device). The last
        returned token is sampled but not yet run through the layers (its K/V are not cached).
        A beam state (`prefill(beam=)`): the same convention over the B * K running rows - n selections on the first call, n - 1 on a later
        one, each later selection behind ops.beam_reorder and one pass; the returned tokens are the running rows' (a hypothesis is read from
        `beam_results`, never from them). Prompts that are done keep decoding harmlessly; `beam_results(state).done` says when to stop."""
        B, S = state["B"], state["S"]
        Sr = state.get("S_run", S)                                # rows per sequence in x (prompt minus a cached prefix)
        sel = state["select"]
        n = _prompt_lens(B, S, state.get("lens"))
        sel.check_chunk(state.get("n_sel", 1) + n_steps - 1, int(n.max()))      # the last answer token of this chunk: refused before anything is launched
        K = sel.K if "cur" not in state else 1                                 # > 1: this call makes the first draw and fans the batch out
        out = torch.empty(B * K, n_steps, dtype=torch.int32, device=self.device)
        if "cur" not in state:
            # each sequence's last real row in its run rectangle: one row index serves all unless the prompts or their prefixes are ragged
            last = n - state["plan"]["prefix_len"] - 1
            if bool((last == Sr - 1).all()):
                sel.first(B, Sr, Sr - 1)
            else:
                sel.first(B, Sr, rows_idx=self._i32(np.arange(B) * Sr + last))
            state["cur"] = S if state.get("lens") is None else n.copy()
            state["n_sel"] = 1                                    # selections made so far = answer tokens with a log-probability column
            if "beam" in state:                                   # what `latents_after` continues: the prompts as the prefill left them
                state["beam"]["prompts"] = dict(B=B, next_pos=np.asarray(state["next_pos"]).copy(), lens=n.copy())
            if sel.shared:
                self._share_out(state, K)
            elif K > 1:
                self._fan_out(state, K)
            B = state["B"]
        def phase():
            if sel.shared:
                return self._shared_phase(state)
            cur = state["cur"]
            return self._phase(B, 1, state["next_pos"][None, :, None], cur, k_len=cur + 1 if np.ndim(cur) else None)      # (ragged batch: per-sequence cache positions)

        for j in range(n_steps):
            self._decode_step(sel, B, out[:, j], None if j == n_steps - 1 else phase, state["n_sel"], state.get("shared"))
            if j == n_steps - 1:
                break
            if sel.shared:
                state["shared"]["tail_len"] += 1
            state["n_sel"] += 1
            state["cur"] = state["cur"] + 1
            state["next_pos"] = state["next_pos"] + 1
        return out

    def latents(self, state: dict, tail_tokens: Optional[torch.Tensor], seq_lens: Optional[np.ndarray] = None) -> torch.Tensor:
        """N_QUERY latent trajectory queries against the cached prefix (generate_latents without the re-run).
        tail_tokens int32 [B, m]: tokens to run in front of the queries because their K/V are not cached yet (the last sampled
        token). seq_lens [B]: number of cached tokens to keep per sequence (prompt + answer up to where it ended); the m + N_QUERY
        new tokens are placed right behind them, K/V cached beyond that point (post-EOS decode steps) are ignored / overwritten."""
        B, nq = state["B"], self.latent_q.shape[0]
        m = 0 if tail_tokens is None else tail_tokens.shape[1]
        cur = state.get("cur", state.get("lens", state["S"]))
        keep = cur if seq_lens is None else np.asarray(seq_lens, dtype=np.int64)      # (ragged batch: everything cached so far, per sequence)
        start_pos = state["next_pos"] - (cur - keep)                  # text positions advance by one per cached token
        p = start_pos[None, :, None] + np.arange(m + nq)[None, None, :]
        ph = self._phase(B, m + nq, p, keep, k_len=None if np.ndim(keep) == 0 else keep + m + nq)
        return self._latent_pass(B, m, ph, tail_tokens.reshape(-1).contiguous() if m else None)

    def latents_behind(self, state: dict, rows, last_tokens, keep_len) -> torch.Tensor:
        """N_QUERY latent trajectory queries behind SELECTED rows of a sampling state (`prefill(sampling=)` + `decode`), without re-running
        their prompts and without writing anything the state lives in: no cache row, no tail row, no seen set - the call can be repeated, and
        run again for other rows. rows int [P] (rows of the state, prompt-major; a row may be named twice); keep_len int [P]: the cached tokens
        of each row to keep = its prompt + the kept answer tokens but the last; last_tokens int [P]: that last kept answer token, whose K/V
        need not be cached (the last draw's are not). Pair p runs 1 + N_QUERY rows - the embedding of last_tokens[p], then latent_q - as a
        suffix pass (`_suffix_phase`) at text positions next_pos[row] - (cur[row] - keep_len[p]) + i, what `latents` gives a greedy row:
          shared-prompt state   slot = the row's prompt, pfx_len = the prompt's length, tail row = the row, tail_len = keep_len - prompt length;
          one slot per row      slot = the row, pfx_len = keep_len, no tail (fan-out, or one returned sequence per prompt).
        -> bf16 [P, N_QUERY, H] through the final RMSNorm. CapacityError before any launch if P * (1 + N_QUERY) exceeds the buffer rows."""
        m = 1 + self.latent_q.shape[0]
        rows, keep = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (rows, keep_len))
        last = np.asarray(last_tokens.cpu() if isinstance(last_tokens, torch.Tensor) else last_tokens, dtype=np.int64).reshape(-1)
        P = rows.size
        assert "sampling" in state and "cur" in state, "latents_behind continues a sampling state after its first decode"
        assert P >= 1 and keep.size == P and last.size == P and int(rows.min()) >= 0 and int(rows.max()) < state["B"]
        if P * m > self.x.shape[0]:
            raise CapacityError(f"latent queries behind {P} rows x {m} tokens exceed the engine's {self.x.shape[0]} buffer rows")
        cur = np.broadcast_to(np.asarray(state["cur"], dtype=np.int64), (state["B"],))[rows]
        start = np.asarray(state["next_pos"], dtype=np.int64)[rows] - (cur - keep)
        sh = state.get("shared")
        if sh is not None:
            pl = np.asarray(sh["pfx_len"], dtype=np.int64)[rows]
            assert bool((keep >= pl).all()) and bool((keep - pl <= int(sh["tail_len"])).all()), "keep_len outside what the rows' tails hold"
            ph = self._suffix_phase(np.asarray(sh["slot"])[rows], start, pl, np.full(P, m), m, tail_row=rows, tail_len=keep - pl)
        else:
            assert bool((keep >= 1).all()) and bool((keep <= cur).all()), "keep_len outside what the rows' cache slots hold"
            ph = self._suffix_phase(rows, start, keep, np.full(P, m), m)
        ops.gather_rows(self.embed, self.x_in, src=self._i32(last), dst=self._i32(np.arange(P) * m), rows=P)      # straight to each pair's tail row
        return self._latent_pass(P, 1, ph)

    def latents_after(self, state: dict, prompt_of, answers) -> torch.Tensor:
        """N_QUERY latent trajectory queries behind finished hypotheses of a beam state, which keep no tail: pair p runs answers[p] (its answer
        tokens, EOS included where it ended) and then latent_q as ONE suffix pass behind prompt prompt_of[p] in its cache slot, which beam
        search never writes (`_suffix_phase`, ops.attention_prefix). Nothing is written: the call can be repeated. -> bf16 [P, N_QUERY, H]
        through the final RMSNorm. ValueError if an answer + N_QUERY exceeds the rows of a suffix pass, CapacityError if the pass exceeds the
        engine's buffer rows - both before any launch."""
        nq, H = self.latent_q.shape[0], self.H
        pr = state["beam"]["prompts"]
        prompt_of = np.asarray(prompt_of, dtype=np.int64).reshape(-1)
        P = prompt_of.size
        alen = np.asarray([len(a) for a in answers], dtype=np.int64)
        assert P >= 1 and alen.size == P and int(alen.min()) >= 1 and int(prompt_of.min()) >= 0 and int(prompt_of.max()) < pr["B"]
        m = int(alen.max()) + nq
        ph = self._suffix_phase(prompt_of, pr["next_pos"][prompt_of], pr["lens"][prompt_of], alen + nq, m)      # (raises before any launch)
        toks = np.zeros((P, m), dtype=np.int32)
        for p, a in enumerate(answers):
            toks[p, : alen[p]] = np.asarray(a, dtype=np.int32)
        qrows = (np.arange(P)[:, None] * m + alen[:, None] + np.arange(nq)[None]).reshape(-1)
        ops.gather_rows(self.embed, self.x_in, src=self._i32(toks.reshape(-1)), rows=P * m)
        self.x_in[: P * m].index_copy_(0, torch.from_numpy(qrows).to(self.device), self.latent_q.repeat(P, 1))
        self._layers(ph)
        tmp = torch.empty(P * nq, H, dtype=self.x.dtype, device=self.device)
        ops.gather_rows(self.x[: P * m], tmp, src=self._i32(qrows))
        out = torch.empty(P, nq, H, dtype=torch.bfloat16, device=self.device)
        ops.norm(tmp, self.norm_w, None, eps=1e-6, rms=True, out=out.view(P * nq, H), rows=P * nq)
        return out

    # ------------------------------------------------------------------------------------------------ HF-style surface
    def generate(self, input_ids, pixel_values=None, image_grid_thw=None, max_new_tokens: int = 8, eos_token_id=None,
                 repetition_penalty: float = 1.0, constraint=None, logit_rules=None, **_):
        """greedy generate: returns sequences int64 [B, S + n] (a row that reached EOS keeps EOS), n = max_new_tokens.
        eos_token_id: an int or a list (any member ends a row; the row is filled with the first); repetition_penalty, constraint and
        logit_rules (a CompiledRules for this call) as in `plan`."""
        state = self.prefill(input_ids, pixel_values, image_grid_thw, repetition_penalty=repetition_penalty, constraint=constraint,
                             logit_rules=logit_rules)
        toks = self.decode(state, max_new_tokens).cpu().long()
        eos_all = eos_ids(self.cfg["eos_token_id"] if eos_token_id is None else eos_token_id)
        eos = eos_all[0]
        for b in range(toks.shape[0]):
            hit = torch.isin(toks[b], torch.tensor(eos_all)).nonzero()
            if hit.numel():
                toks[b, int(hit[0]) + 1:] = eos
        self._state = state
        return torch.cat([input_ids.cpu().long(), toks], dim=1)

    def generate_latents(self, output_ids, pixel_values=None, image_grid_thw=None, cached_embeds: Optional[list] = None):
        """reference signature (internvla_n1.py:320): full prefill over output_ids + N_QUERY latent queries (no cache reuse)."""
        cfg = self.cfg
        nq = self.latent_q.shape[0]
        ids = torch.cat([output_ids.cpu().long(), torch.full((output_ids.shape[0], nq), cfg["traj_token_id"], dtype=torch.long)], dim=1)
        P = self.plan(ids, image_grid_thw, cached_embeds=cached_embeds)
        self.run_prefill(P, pixel_values)
        B, S = P["B"], P["S"]
        out = torch.empty(B, nq, self.H, dtype=torch.bfloat16, device=self.device)
        ops.norm(self.x[: B * S], self.norm_w, None, eps=1e-6, rms=True, out=out.view(B * nq, self.H), rows=B * nq, in_map=(nq, S, S - nq))
        return out
