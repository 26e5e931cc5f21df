"""Drop-in model / policy surface of InternVLA-N1 on the MI355X engines.

Mirrors, with the same names, arguments and return types, what the reference's callers use:
  * `InternVLAN1ForCausalLM`  <- internnav/model/basemodel/internvla_n1/internvla_n1.py:39 : `.eval()`, `.device`,
        `.generate(**inputs, max_new_tokens, do_sample=False, ...).sequences`, `.generate_latents(output_ids, pixel_values,
        image_grid_thw)`, `.generate_traj(traj_latents, images_dp, depths_dp)`
        (call sites habitat_vln_evaluator.py:418-459, internvla_n1_policy.py:169-203, internvla_n1_agent_realworld.py:221-256)
  * `InternVLAN1Net`          <- internnav/model/basemodel/internvla_n1/internvla_n1_policy.py:26 : `reset`, `step_no_infer`,
        `s2_step`, `s1_step_latent`
  * host post-processing `traj_to_actions`, `chunk_token`, `split_and_clean`, `S1Output`, `S2Output`, `S2Input`
        <- internnav/model/utils/vln_utils.py:19-175 (numpy / python; stays on the host in the reference too).
The tokenizer / image processor (a1 in SURVEY.md 8a: HF `AutoProcessor`, third-party, host side) is injected; the kernel
boundary starts at `input_ids` / `pixel_values` / `image_grid_thw`.

Unlike the reference (one env per call) every method here also accepts a batch of environments; batch-1 calls keep the
reference's exact shapes (e.g. generate_traj returns [32*B, T, 3]).
"""
from __future__ import annotations

import copy
import itertools
import re
from collections import OrderedDict
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import logit_rules, ops, synthetic
from .navdp import NavDPPolicyDAT
from .nextdit import NextDiTSystem1
from .qwen_vl import ATTN_WIDE_MIN_ROWS, SKINNY_GEMM_MAX_ROWS, EngineKVCache, QwenVLEngine, eos_ids, kv_reuse_fit, kv_reuse_lengths
from .runtime import CapacityError  # noqa: F401  (re-exported)


# ------------------------------------------------------------------------------------------------------ vln_utils mirror
def split_and_clean(text: str) -> List[str]:
    """vln_utils.py:19-33: split on <image>, drop newlines / empty parts."""
    out = []
    for part in re.split(r"(<image>)", text):
        if part == "<image>":
            out.append(part)
        else:
            c = part.replace("\n", "").strip()
            if c:
                out.append(c)
    return out


def chunk_token(dp_actions) -> List[int]:
    """vln_utils.py:36-60: per-waypoint discretisation (0 stop, 1 forward, 2 left, 3 right)."""
    out = []
    for xyyaw in dp_actions:
        x, yaw = float(xyyaw[0]), float(xyyaw[-1])
        if x < 0.05 and abs(yaw) < 0.05:
            out.append(0)
        elif abs(x / 0.25) >= abs(yaw * 12 / np.pi):
            out.append(1)
        else:
            out.append(3 if yaw < 0 else 2)
    return out


def traj_to_actions(dp_actions, use_discrate_action: bool = True):
    """vln_utils.py:63-136. dp_actions [S, T, 3] (x4-scaled increments): un-normalise IN PLACE (the reference mutates its input,
    :129), cumulative sum, mean over the S samples, greedy pure-pursuit discretisation (0.25 m steps, 15 degree turns, lookahead 4)."""
    dp_actions[:, :, :2] /= 4.0
    d = dp_actions.float().cpu().numpy() if isinstance(dp_actions, torch.Tensor) else np.asarray(dp_actions, dtype=np.float64)
    B, T = d.shape[:2]
    xy = np.zeros((B, T + 1, 2))
    xy[:, 1:] = np.cumsum(d[:, :, :2], axis=1)
    trajectory = xy.mean(axis=0)
    if not use_discrate_action:
        return trajectory
    actions: List[int] = []
    yaw, pos, goal = 0.0, trajectory[0], trajectory[-1]
    turn = np.deg2rad(15)

    def norm_angle(a):
        return (a + np.pi) % (2 * np.pi) - np.pi

    while np.linalg.norm(pos - goal) > 0.2:
        nearest = int(np.argmin(np.linalg.norm(trajectory - pos, axis=1)))
        target = trajectory[min(nearest + 4, len(trajectory) - 1)]
        tdir = target - pos
        if np.linalg.norm(tdir) < 1e-6:
            break
        n_turns = int(round(norm_angle(np.arctan2(tdir[1], tdir[0]) - yaw) / turn))
        if n_turns > 0:
            actions += [2] * n_turns
        elif n_turns < 0:
            actions += [3] * (-n_turns)
        yaw = norm_angle(yaw + n_turns * turn)
        nxt = pos + 0.25 * np.array([np.cos(yaw), np.sin(yaw)])
        if np.linalg.norm(nxt - goal) > np.linalg.norm(pos - goal):
            break
        actions.append(1)
        pos = nxt
    return actions


@dataclass
class S2Input:
    idx: Optional[int] = -1
    instruction: Optional[str] = None
    rgb: Optional[np.ndarray] = None
    depth: Optional[np.ndarray] = None
    pose: Optional[Any] = None
    look_down: Optional[bool] = False
    should_infer: Optional[bool] = False


@dataclass
class S2Output:
    idx: Optional[int] = -1
    is_infering: Optional[bool] = False
    output_action: Optional[Any] = None
    output_trajectory: Optional[np.ndarray] = None
    output_pixel: Optional[np.ndarray] = None
    output_latent: Optional[torch.Tensor] = None
    rgb_memory: Optional[np.ndarray] = None
    depth_memory: Optional[np.ndarray] = None
    # model_settings['token_logprobs'] only (else None): log-probability of the decoded answer (sum over its tokens, EOS included) and the
    # smallest top-2 margin among them (how close the answer came to being another one). Fields only: no policy decision reads them.
    answer_logprob: Optional[float] = None
    answer_min_margin: Optional[float] = None

    def validate(self) -> bool:
        return sum(x is not None for x in (self.output_action, self.output_pixel, self.output_latent)) > 0 and self.idx >= 0


@dataclass
class S1Output:
    idx: Optional[List[int]] = None
    vis_image: Optional[np.ndarray] = None


# ------------------------------------------------------------------------------------------------------ model facade
def smart_resize(height: int, width: int, factor: int = 28, min_pixels: int = 56 * 56, max_pixels: int = 14 * 14 * 4 * 1280):
    """transformers image_processing_qwen2_vl.smart_resize (the processor's target size; restated in preprocess.py for the device path)."""
    import math

    h_bar, w_bar = round(height / factor) * factor, round(width / factor) * factor
    if h_bar * w_bar > max_pixels:
        beta = math.sqrt((height * width) / max_pixels)
        h_bar, w_bar = max(factor, math.floor(height / beta / factor) * factor), max(factor, math.floor(width / beta / factor) * factor)
    elif h_bar * w_bar < min_pixels:
        beta = math.sqrt(min_pixels / (height * width))
        h_bar, w_bar = math.ceil(height * beta / factor) * factor, math.ceil(width * beta / factor) * factor
    return h_bar, w_bar


def s2_capacity(num_history: int = 8, resize_w: int = 384, resize_h: int = 384, cam_w: int = 640, cam_h: int = 480,
                text_tokens: int = 512, max_new_tokens: int = 128, n_query: int = 4):
    """(max_seq_len, max_patches_per_seq) of the longest System-2 prompt the reference's callers can build: num_history history frames
    + the current frame at the resized size, + one look-down frame fed UN-resized at camera size (internvla_n1_policy.py:113-116,140),
    the chat text, the answer and the latent queries. Default harness settings: 9 x 196 + 391 image tokens + text = 2.8 K tokens."""
    rh, rw = smart_resize(resize_h, resize_w)
    ch, cw = smart_resize(cam_h, cam_w)
    p_hist, p_cam = (rh // 14) * (rw // 14), (ch // 14) * (cw // 14)
    patches = (num_history + 1) * p_hist + p_cam
    seq = patches // 4 + 2 * (num_history + 2) + text_tokens + max_new_tokens + n_query
    return (seq + 127) // 128 * 128, patches


def qwen_cfg_from_hf(cfgj: dict) -> dict:
    """engine configuration from a checkpoint's config.json (Qwen2.5-VL layout of transformers 4.51: text keys at the top level;
    newer exports nest them under text_config) - defaults are the Qwen2.5-VL-7B values InternVLA-N1 ships with."""
    t = dict(cfgj)
    t.update(cfgj.get("text_config") or {})
    v = cfgj.get("vision_config") or {}
    d = synthetic.QWEN_N1_CFG
    rope = t.get("rope_theta") or (t.get("rope_parameters") or {}).get("rope_theta") or d["rope_theta"]
    eos = t.get("eos_token_id", d["eos_token_id"])
    return dict(
        v_hidden=v.get("hidden_size", d["v_hidden"]), v_heads=v.get("num_heads", d["v_heads"]), v_inter=v.get("intermediate_size", d["v_inter"]),
        v_depth=v.get("depth", d["v_depth"]), v_fullatt=tuple(v.get("fullatt_block_indexes", d["v_fullatt"])), v_window=v.get("window_size", d["v_window"]),
        v_patch=v.get("patch_size", d["v_patch"]), v_out=v.get("out_hidden_size", d["v_out"]),
        t_hidden=t.get("hidden_size", d["t_hidden"]), t_inter=t.get("intermediate_size", d["t_inter"]), t_heads=t.get("num_attention_heads", d["t_heads"]),
        t_kv_heads=t.get("num_key_value_heads", d["t_kv_heads"]), t_layers=t.get("num_hidden_layers", d["t_layers"]), vocab=t.get("vocab_size", d["vocab"]),
        rope_theta=float(rope), n_query=cfgj.get("n_query", d["n_query"]),
        image_token_id=cfgj.get("image_token_id", d["image_token_id"]), traj_token_id=cfgj.get("traj_token_id", d["traj_token_id"]),
        vision_start_id=cfgj.get("vision_start_token_id", d["vision_start_id"]), vision_end_id=cfgj.get("vision_end_token_id", d["vision_end_id"]),
        eos_token_id=int(eos[0] if isinstance(eos, (list, tuple)) else eos))


# generation_config.json keys that change what greedy generate() returns and that the engine does not implement -> the value that leaves
# HF's behaviour unchanged (a key set to anything else is refused at load: never differ silently)
_GEN_REFUSED = {
    "no_repeat_ngram_size": lambda v: not v or v <= 0, "encoder_repetition_penalty": lambda v: v is None or float(v) == 1.0,
    "bad_words_ids": lambda v: not v, "suppress_tokens": lambda v: not v, "begin_suppress_tokens": lambda v: not v,
    "forced_bos_token_id": lambda v: v is None, "forced_eos_token_id": lambda v: v is None, "min_length": lambda v: not v or v <= 0,
    "min_new_tokens": lambda v: not v or v <= 0, "sequence_bias": lambda v: not v, "num_beams": lambda v: v is None or v <= 1,
    "penalty_alpha": lambda v: v is None, "exponential_decay_length_penalty": lambda v: v is None, "renormalize_logits": lambda v: not v}


def generation_config_from_hf(raw: Optional[dict], default_eos, ignore: bool = False, rules_from_file: bool = False) -> SimpleNamespace:
    """what `generate(do_sample=False)` honours of a checkpoint's generation_config.json (HF starts from that file and overrides only the
    keys it is passed): `repetition_penalty` (default 1.0) and `eos_token_id` (an int or a list; default: config.json's) -> a namespace with
    repetition_penalty, eos_token_id (tuple) and the raw dict. raw None = no file: penalty 1.0, EOS of config.json.
    Sampling-only keys (do_sample, temperature, top_k, top_p, min_p, typical_p) are ignored by greedy decoding, as HF ignores them under
    do_sample=False; the namespace carries the file's do_sample / temperature / top_k / top_p (None = not set) for generate(do_sample=True)
    (`sampling_spec`, which is also where min_p / typical_p / epsilon_cutoff / eta_cutoff are refused - at generate() time, not here).
    A key that changes greedy output and is not implemented raises NotImplementedError naming it, unless `ignore`.
    rules_from_file (default False: today's refusal; generation_rules="file" of the model sets it): the eight logits-processor keys of
    `logit_rules.KEYS` are then not refused but returned as `rules` (the keys the file switches on, values as they stand; {} otherwise) -
    the model's default rule set of generate()."""
    raw = dict(raw or {})
    bad = sorted(k for k, ok in _GEN_REFUSED.items() if k in raw and not ok(raw[k]) and not (rules_from_file and k in logit_rules.KEYS))
    if bad and not ignore:
        raise NotImplementedError(
            f"generation_config.json sets {', '.join(f'{k}={raw[k]!r}' for k in bad)}: greedy decoding with these is not implemented, and ignoring "
            "them would decode other tokens than transformers does (model_settings['ignore_generation_config']=True loads anyway)")
    pen = raw.get("repetition_penalty")
    pen = 1.0 if pen is None else float(pen)
    if not (np.isfinite(pen) and pen > 0.0):
        raise ValueError(f"generation_config.json: repetition_penalty={raw.get('repetition_penalty')!r} is not a strictly positive float")
    eos = raw.get("eos_token_id")
    # the file's sampling keys as they stand (None = not in the file): read only by generate(do_sample=True) (`sampling_spec`), never by greedy
    rules = {k: raw[k] for k in logit_rules.KEYS if rules_from_file and k in raw and not _GEN_REFUSED[k](raw[k])}
    return SimpleNamespace(repetition_penalty=pen, eos_token_id=eos_ids(default_eos if eos is None else eos), raw=raw, rules=rules,
                           do_sample=raw.get("do_sample"), temperature=raw.get("temperature"), top_k=raw.get("top_k"), top_p=raw.get("top_p"))


# sampling keys that are not implemented: key -> is this value HF's "off"?
_SAMPLING_REFUSED = {"min_p": lambda v: v is None, "typical_p": lambda v: v is None or float(v) == 1.0,
                     "epsilon_cutoff": lambda v: v is None or float(v) == 0.0, "eta_cutoff": lambda v: v is None or float(v) == 0.0}


def sampling_spec(gen_cfg: SimpleNamespace, do_sample: bool, temperature=None, top_k=None, top_p=None, num_return_sequences: Optional[int] = None,
                  extra: Optional[dict] = None) -> Optional[SimpleNamespace]:
    """what generate() samples with, resolved as HF resolves it (host only): None under do_sample=False (the file's sampling keys and the
    sampling kwargs are ignored, as HF ignores them), else a namespace temperature / top_k (0 = off) / top_p / K = num_return_sequences.
    A None argument takes generation_config.json's value; without one HF's defaults apply: temperature 1.0, top_k 50, top_p 1.0.
    ValueError (as HF): num_return_sequences > 1 without do_sample; a temperature that is not a strictly positive finite float; top_k < 0;
    top_p outside (0, 1]. NotImplementedError naming the key: min_p, typical_p, epsilon_cutoff or eta_cutoff set to something other than
    off, in the kwargs (`extra`) or the file - at generate() time, never at load."""
    K = 1 if num_return_sequences is None else int(num_return_sequences)
    if K < 1:
        raise ValueError(f"num_return_sequences={num_return_sequences!r} must be >= 1")
    if not do_sample:
        if K > 1:
            raise ValueError(f"num_return_sequences={K} > 1 needs do_sample=True: greedy decoding returns one sequence per prompt (as HF)")
        return None
    extra = extra or {}
    for k, off in _SAMPLING_REFUSED.items():
        v = extra[k] if extra.get(k) is not None else gen_cfg.raw.get(k)
        if not off(v):
            raise NotImplementedError(f"generate(do_sample=True): {k}={v!r} is set ({'argument' if extra.get(k) is not None else 'generation_config.json'}) "
                                      "and is not implemented; sampling without it would draw from another distribution than transformers does")
    pick = lambda arg, name, default: arg if arg is not None else (default if getattr(gen_cfg, name, None) is None else getattr(gen_cfg, name))      # noqa: E731
    T, tk, tp = float(pick(temperature, "temperature", 1.0)), int(pick(top_k, "top_k", 50) or 0), float(pick(top_p, "top_p", 1.0))
    if not (np.isfinite(T) and T > 0.0):
        raise ValueError(f"do_sample=True: temperature={T!r} has to be a strictly positive float (use do_sample=False for greedy decoding)")
    if tk < 0:
        raise ValueError(f"do_sample=True: top_k={tk!r} has to be >= 0 (0 = off)")
    if not 0.0 < tp <= 1.0:
        raise ValueError(f"do_sample=True: top_p={tp!r} has to be in (0, 1] (1 = off)")
    return SimpleNamespace(temperature=T, top_k=tk, top_p=tp, K=K)


BEAM_MAX_BEAMS = 8         # num_beams and EOS ids of the beam path: max(2, 1 + n_eos) * num_beams candidates per prompt stay within the 32 of
BEAM_MAX_EOS = 3           # ops.beam_topm_rows


def beam_spec(num_beams=None, num_return_sequences: Optional[int] = None, length_penalty: float = 1.0, early_stopping=False,
              do_sample: bool = False, share_prefix: Optional[bool] = None, extra: Optional[dict] = None) -> Optional[SimpleNamespace]:
    """what generate(num_beams=K) searches with, resolved as HF resolves it (host only): None for num_beams None or 1 (today's paths), else a
    namespace K = num_beams / n = num_return_sequences (default 1) / length_penalty / early_stopping (False, True or "never").
    ValueError (as HF): num_beams < 1; num_return_sequences > num_beams; a length_penalty that is not finite; early_stopping outside
    {False, True, "never"}; share_prefix=False passed explicitly (the beams of a prompt always share its one cache slot).
    NotImplementedError naming the key: do_sample=True with beams (beam sampling), num_beam_groups > 1, a diversity_penalty other than 0,
    constraints / force_words_ids (`extra` = generate's remaining kwargs). Beam search is opt-in by ARGUMENT only: a generation_config.json
    that sets num_beams > 1 stays refused at load (`generation_config_from_hf`)."""
    if num_beams is None:
        return None
    K = int(num_beams)
    if K < 1:
        raise ValueError(f"num_beams={num_beams!r} must be >= 1")
    if K == 1:
        return None
    extra = extra or {}
    if do_sample:
        raise NotImplementedError("generate(num_beams > 1, do_sample=True): beam sampling is not implemented (do_sample=False searches, "
                                  "num_beams=1 samples)")
    for k, off in (("num_beam_groups", lambda v: v is None or int(v) == 1), ("diversity_penalty", lambda v: v is None or float(v) == 0.0),
                   ("constraints", lambda v: v is None), ("force_words_ids", lambda v: v is None)):
        if not off(extra.get(k)):
            raise NotImplementedError(f"generate(num_beams > 1): {k}={extra[k]!r} is not implemented (group / diverse / lexically constrained "
                                      "beam search); constraint= takes a constrain.TokenAutomaton")
    n = 1 if num_return_sequences is None else int(num_return_sequences)
    if n < 1:
        raise ValueError(f"num_return_sequences={num_return_sequences!r} must be >= 1")
    if n > K:
        raise ValueError(f"num_return_sequences={n} has to be smaller or equal to num_beams={K} (as HF)")
    lp = float(length_penalty)
    if not np.isfinite(lp):
        raise ValueError(f"length_penalty={length_penalty!r} has to be a finite float")
    if not any(early_stopping is v for v in (False, True)) and early_stopping != "never":
        raise ValueError(f"early_stopping={early_stopping!r} must be a boolean or 'never' (as HF)")
    if share_prefix is not None and not share_prefix:
        raise ValueError("share_prefix=False with num_beams > 1: the beams of a prompt are decoded behind its one cache slot, there is no other path")
    return SimpleNamespace(K=K, n=n, length_penalty=lp, early_stopping=early_stopping)


SCORE_SLAB_ROWS = 256      # rows of the fp32 [rows, vocab] logit buffer of score_answers (156 MB at 152064 tokens), allocated on first use


def answer_logprob_summary(token_logprobs: torch.Tensor, token_margins: torch.Tensor, lengths) -> SimpleNamespace:
    """the log-probability outputs of generate(): per-token values [B, n] of the emitted tokens and lengths [B] (tokens of each row up to and
    including its first EOS) -> token_logprobs / token_margins with 0.0 at the positions behind it (a NaN there is dropped, one inside the
    answer is kept), sequences_logprob [B] = the sum over the answer, answer_lengths int64 [B] = the lengths, on the device."""
    lens = torch.as_tensor(np.asarray(lengths, dtype=np.int64), device=token_logprobs.device)
    keep = torch.arange(token_logprobs.shape[1], device=token_logprobs.device)[None, :] < lens[:, None]
    lp = torch.where(keep, token_logprobs.float(), torch.zeros((), device=token_logprobs.device))
    mg = torch.where(keep, token_margins.float(), torch.zeros((), device=token_logprobs.device))
    return SimpleNamespace(token_logprobs=lp, token_margins=mg, sequences_logprob=lp.sum(dim=1), answer_lengths=lens)


def answer_confidences(res) -> List[Tuple[float, float]]:
    """(answer_logprob, answer_min_margin) of every row of a generate(output_logprobs=True) result as Python floats: the sum of the answer's
    token log-probabilities and the smallest top-2 margin among its tokens. ONE device-to-host copy for the whole batch."""
    mg = res.token_margins
    keep = torch.arange(mg.shape[1], device=mg.device)[None, :] < res.answer_lengths[:, None]
    low = torch.where(keep, mg, torch.full((), float("inf"), device=mg.device)).min(dim=1).values if mg.shape[1] else torch.full_like(res.sequences_logprob, float("inf"))
    both = torch.stack([res.sequences_logprob, low]).cpu().tolist()
    return list(zip(both[0], both[1]))


def score_row_plan(prompt_lens, answer_lens, slab_rows: int = SCORE_SLAB_ROWS):
    """host plan of score_answers: sequence q = prompt_lens[q] prompt tokens followed by answer_lens[q] answer tokens, right-padded to the
    longest. Answer token i of sequence q is predicted by the hidden row at position prompt_lens[q] - 1 + i of that sequence.
    -> (S, rows int32 [R] = absolute rows q * S + position in sequence-major order, offsets int64 [Q + 1] of each sequence's rows in that order,
    slabs = [(r0, r1), ...] consecutive row ranges of at most slab_rows rows)."""
    pl, al = np.asarray(prompt_lens, dtype=np.int64).reshape(-1), np.asarray(answer_lens, dtype=np.int64).reshape(-1)
    assert pl.shape == al.shape and pl.size > 0 and int(pl.min()) >= 1 and int(al.min()) >= 0 and slab_rows >= 1
    S = int((pl + al).max())
    off = np.concatenate([[0], np.cumsum(al)])
    rows = np.concatenate([q * S + pl[q] - 1 + np.arange(al[q]) for q in range(pl.size)] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    R = int(off[-1])
    return S, rows, off, [(r0, min(r0 + slab_rows, R)) for r0 in range(0, R, slab_rows)]


SCORE_SUFFIX_MAX_ROWS = 64  # candidate tokens a suffix pass runs per pair (ops.ATTN_PREFIX_MAX_ROWS): candidates of up to 65 tokens


def score_prefix_plan(prompt_lens, answer_lens_per_prompt, max_rows: int, slab_rows: int = SCORE_SLAB_ROWS) -> dict:
    """host plan of score_answers(share_prefix=True) for ONE group of prompts prefilled together (prompt b in cache slot b, right-padded to
    S = the longest): answer_lens_per_prompt[b] = the token counts of prompt b's candidates. Pairs are numbered prompt-major.
    Token 0 of a candidate is predicted by its prompt's last hidden row b * S + prompt_lens[b] - 1 (one gathered row per pair: the source index
    repeats). Tokens 1 .. n - 1 are predicted by a suffix pass over the candidate's tokens 0 .. n - 2: pairs with n >= 2 are cut, in order, into
    passes of P pairs x m rows (m = the longest of the pass, at most SCORE_SUFFIX_MAX_ROWS) with P * m <= max_rows; row j * m + i of a pass
    predicts token i + 1 of its j-th pair. ->
      S, pairs [(b, c)], off int64 [pairs + 1] (token i of pair q is value off[q] + i of the group's flat result), total = off[-1],
      first_rows int32 / first_dst int64 / first_pair int64 [F] and first_slabs, the pairs with n >= 1,
      passes: dicts of pair int64 [P], prompt int64 [P], m, suf_len int64 [P], rows int32 [R], dst int64 [R], slabs.
    slabs = consecutive ranges of at most slab_rows gathered rows (one lm_head GEMM each)."""
    pl = np.asarray(prompt_lens, dtype=np.int64).reshape(-1)
    assert pl.size > 0 and len(answer_lens_per_prompt) == pl.size and int(pl.min()) >= 1 and slab_rows >= 1
    pairs = [(b, c) for b in range(pl.size) for c in range(len(answer_lens_per_prompt[b]))]
    al = np.asarray([int(answer_lens_per_prompt[b][c]) for b, c in pairs], dtype=np.int64)
    assert al.size == 0 or int(al.min()) >= 0
    if al.size and int(al.max()) - 1 > SCORE_SUFFIX_MAX_ROWS:
        raise ValueError(f"a candidate of {int(al.max())} tokens exceeds the {SCORE_SUFFIX_MAX_ROWS + 1} tokens score_answers(share_prefix=True) "
                         "scores behind a shared prompt: score it with share_prefix=False (one prefill per pair)")
    longest = int(al.max()) if al.size else 0
    assert max_rows >= max(1, longest - 1), f"max_rows={max_rows} cannot hold the {longest - 1} suffix rows of the longest candidate"
    S = int(pl.max())
    off = np.concatenate([[0], np.cumsum(al)]).astype(np.int64)
    slabs = lambda R: [(r0, min(r0 + slab_rows, R)) for r0 in range(0, R, slab_rows)]
    first = np.asarray([q for q in range(al.size) if al[q] >= 1], dtype=np.int64)
    pb = np.asarray([b for b, _ in pairs], dtype=np.int64)
    plan = dict(S=S, pairs=pairs, off=off, total=int(off[-1]), first_pair=first, first_rows=(pb[first] * S + pl[pb[first]] - 1).astype(np.int32),
                first_dst=off[first], first_slabs=slabs(first.size), passes=[])
    cur = []

    def close():
        if not cur:
            return
        q = np.asarray(cur, dtype=np.int64)
        sl = al[q] - 1
        m = int(sl.max())
        rows = np.concatenate([j * m + np.arange(sl[j]) for j in range(q.size)]).astype(np.int32)
        dst = np.concatenate([off[q[j]] + 1 + np.arange(sl[j]) for j in range(q.size)]).astype(np.int64)
        plan["passes"].append(dict(pair=q, prompt=pb[q], m=m, suf_len=sl, rows=rows, dst=dst, slabs=slabs(rows.size)))
        cur.clear()

    m_cur = 0
    for q in range(al.size):
        if al[q] < 2:
            continue
        m_new = max(m_cur, int(al[q]) - 1)
        if cur and (len(cur) + 1) * m_new > max_rows:
            close()
            m_new = int(al[q]) - 1
        cur.append(q)
        m_cur = m_new
    close()
    return plan


class InternVLAN1ForCausalLM:
    """HF-style model object backed by the HIP engines (no nn.Module, no CPU fallback)."""

    def __init__(self, weights, qwen_cfg: dict, system1: str = "nextdit_async", s1_cfg: Optional[dict] = None,
                 device="cuda:0", max_envs: int = 16, max_seq_len: Optional[int] = None, max_patches: Optional[int] = None,
                 max_s2_seqs: Optional[int] = None, num_history: int = 8, resize_w: int = 384, resize_h: int = 384,
                 cam_w: int = 640, cam_h: int = 480, w8_decode: bool = False, generation_config: Optional[dict] = None,
                 ignore_generation_config: bool = False, token_logprobs: bool = False, max_decode: int = 128,
                 mx4_decode: bool = False, generation_rules=None):
        """generation_rules (opt-in; None = none): the model's default logits-processor rules of every generate() - a dict of
        `logit_rules.KEYS` (sequence_bias, no_repeat_ngram_size, bad_words_ids, min_length, min_new_tokens, forced_eos_token_id,
        suppress_tokens, begin_suppress_tokens; validated here), or "file": the values generation_config.json sets, which are otherwise
        refused at load. generate()'s arguments override them key by key.
        Engine capacity defaults to the longest prompt the reference's harness can build for (num_history, resize, camera size):
        see `s2_capacity`; exceeding it raises `CapacityError` (never a silent STOP).
        token_logprobs (opt-in): the System-2 engine keeps the log-probability and top-2 margin of every greedy token
        (generate(output_logprobs=True)) for answers of up to max_decode tokens (generate() refuses a larger max_new_tokens on such a model);
        off, the launch sequence is the plain one."""
        self.device = torch.device(device)
        # the checkpoint's generation_config.json (None: no such file): generate() starts from it, as HF's does
        self.generation_config = generation_config_from_hf(generation_config, qwen_cfg["eos_token_id"], ignore=ignore_generation_config,
                                                           rules_from_file=generation_rules == "file")
        if not (generation_rules is None or generation_rules == "file" or isinstance(generation_rules, dict)):
            raise ValueError(f"generation_rules={generation_rules!r}: None, a dict of {', '.join(logit_rules.KEYS)}, or 'file'")
        self.generation_rules = logit_rules.normalize(self.generation_config.rules if generation_rules == "file" else generation_rules, qwen_cfg["vocab"])
        if system1 not in ("nextdit_async", "navdp_async", "nextdit", "navdp"):
            # the four System-1 types of generate_traj (internvla_n1.py:359-441): 'nextdit' [+ 'async'] and 'navdp' [+ 'async']
            raise NotImplementedError(f"system1={system1!r}: known types are 'nextdit_async' (DualVLN), 'navdp_async', 'nextdit', 'navdp'")
        self.config = SimpleNamespace(system1=system1, n_query=qwen_cfg["n_query"], hidden_size=qwen_cfg["t_hidden"],
                                      image_token_id=qwen_cfg["image_token_id"])
        n_s2 = max_s2_seqs or max_envs   # System-2 runs on micro-batches of the envs whose plan expired (agent / bench schedule)
        cap_seq, cap_patches = s2_capacity(num_history, resize_w, resize_h, cam_w, cam_h, n_query=qwen_cfg["n_query"])
        self.qwen = QwenVLEngine(weights, qwen_cfg, device, max_seqs=n_s2, max_seq_len=max_seq_len or cap_seq,
                                 max_patches=max_patches or n_s2 * cap_patches, w8_decode=w8_decode, token_logprobs=token_logprobs, max_decode=max_decode,
                                 mx4_decode=mx4_decode)
        self._score_logits = None       # fp32 [<= SCORE_SLAB_ROWS, vocab] of score_answers, allocated on first use
        self.last_score = dict(prompt_prefills=0, images_encoded=0, suffix_rows=0, suffix_passes=0)      # counters of the last score_answers call
        if "nextdit" in system1:
            # the DiT's geometry (width, depth, heads, FFN width) is not in config.json - NextDiTCrossAttnConfig is constructed in code
            # (internvla_n1_arch.py:127-131) and its FFN width depends on the diffusers release (synthetic.lumina_ffn_width): read it off
            # the checkpoint's tensor shapes
            s1w = _Prefixed(weights, "model.")
            self.s1 = NextDiTSystem1(s1w, s1_cfg or synthetic.n1_nextdit_cfg_from_weights(s1w), device, max_envs, use_async="async" in system1)
        else:
            self.s1 = NavDPPolicyDAT(_Prefixed(weights, "model.navdp."), s1_cfg or synthetic.N1_NAVDP_CFG, device, max_envs, use_async="async" in system1)
        self._noise_gen = torch.Generator(device=self.device).manual_seed(0)
        self._sample_gen = torch.Generator(device="cpu").manual_seed(0)      # default source of generate(do_sample=True)'s uniforms: advances per call
        self.kv_reuse_rows = 0          # prompt rows generate(past_key_values=...) took from caches instead of prefilling them (cumulative)
        self.kv_reuse_fallbacks = 0     # rows that had to run without their cache: the run rectangle would not fit the engine (cumulative)
        self.last_kv_reuse = dict(rows=0, fallbacks=0)

    # ---- construction
    @classmethod
    def from_pretrained(cls, path, torch_dtype=torch.bfloat16, attn_implementation: str = "flash_attention_2", device_map=None, **kw):
        """reference call: InternVLAN1ForCausalLM.from_pretrained(path, torch_dtype=bf16, attn_implementation=..., device_map={"": dev}).
        Loads every *.safetensors shard under `path` (HF checkpoint layout, the reference's parameter names); config.json supplies the
        Qwen2.5-VL dimensions / token ids, system1 and n_query (InternVLAN1ModelConfig fields, internvla_n1.py:22-29);
        generation_config.json, when present, supplies repetition_penalty and eos_token_id of generate() (`model.generation_config`,
        `generation_config_from_hf`: unimplemented keys that change greedy output raise NotImplementedError unless
        ignore_generation_config=True is passed)."""
        import json
        from pathlib import Path

        from safetensors import safe_open

        p = Path(path)
        files = sorted(p.glob("*.safetensors"))
        if not files:
            raise FileNotFoundError(f"no *.safetensors under {p}: InternVLA-N1 checkpoints are HF safetensors shards")
        cfgj = json.loads((p / "config.json").read_text()) if (p / "config.json").exists() else {}
        device = (device_map or {"": "cuda:0"})[""]
        genj = json.loads((p / "generation_config.json").read_text()) if (p / "generation_config.json").exists() else None
        # only the refusal check, before any weight is read (the EOS default is a placeholder): __init__ builds the namespace the model keeps
        generation_config_from_hf(genj, 0, ignore=bool(kw.get("ignore_generation_config", False)), rules_from_file=kw.get("generation_rules") == "file")
        weights = _ShardedCheckpoint(files)
        system1 = cfgj.get("system1", "nextdit_async")
        s1_cfg = None
        if "nextdit" in system1:
            probe = "model.traj_dit.model.layers.0.feed_forward.linear_1.weight"
            if probe not in weights:
                raise KeyError(f"checkpoint {p} has no {probe}: not an InternVLA-N1 '{system1}' checkpoint")
            s1_cfg = synthetic.n1_nextdit_cfg_from_weights(_Prefixed(weights, "model."))
        spec = synthetic.n1_full_spec(qwen_cfg_from_hf(cfgj), system1, s1_cfg=s1_cfg)
        missing = [k for k in spec if k not in weights]
        if missing:
            raise KeyError(f"checkpoint {p} lacks {len(missing)} parameters the engines need, e.g. {missing[:4]}")
        bad = [(k, weights.shape_of(k), shp) for k, (shp, _) in spec.items() if k.startswith("model.traj_dit.") and tuple(weights.shape_of(k)) != tuple(shp)]
        if bad:
            raise ValueError(f"checkpoint {p}: {len(bad)} NextDiT tensors do not have the shapes its own geometry implies, e.g. {bad[:3]}")
        return cls(weights, qwen_cfg_from_hf(cfgj), system1=system1, s1_cfg=s1_cfg, device=device, generation_config=genj, **kw)

    def eval(self):
        return self

    def get_n_query(self):
        return self.config.n_query

    def get_system1_type(self):
        return self.config.system1

    # ---- System 2
    def generate(self, input_ids=None, pixel_values=None, image_grid_thw=None, attention_mask=None, max_new_tokens: int = 128,
                 do_sample: bool = False, use_cache: bool = True, past_key_values=None, return_dict_in_generate: bool = False,
                 decode_chunk: int = 8, eos_token_id=None, cached_image_embeds: Optional[list] = None, prefix_kv: Optional[list] = None,
                 export_prefix: Optional[list] = None, repetition_penalty: Optional[float] = None, output_logprobs: bool = False,
                 temperature: Optional[float] = None, top_k: Optional[int] = None, top_p: Optional[float] = None,
                 num_return_sequences: Optional[int] = None, generator: Optional[torch.Generator] = None, seed: Optional[int] = None,
                 share_prefix: Optional[bool] = None, constraint=None, num_beams: Optional[int] = None, length_penalty: float = 1.0,
                 early_stopping=False, sequence_bias=None, no_repeat_ngram_size: Optional[int] = None, bad_words_ids=None,
                 min_length: Optional[int] = None, min_new_tokens: Optional[int] = None, forced_eos_token_id=None, suppress_tokens=None,
                 begin_suppress_tokens=None, **kw):
        """greedy decoding by default (do_sample=False is the only mode the reference uses, internvla_n1_policy.py:169-176). Decodes in chunks of
        `decode_chunk` device-side steps and stops once every sequence has emitted EOS. Sequences are right-filled with EOS.
        repetition_penalty / eos_token_id: None = the checkpoint's generation_config.json (`self.generation_config`; without that file 1.0
        and config.json's EOS), an explicit value overrides it as HF kwargs do. The penalty acts on every greedy step over prompt + answer
        so far (HF RepetitionPenaltyLogitsProcessor; for a ragged batch over each row's real tokens); eos_token_id may be a list, any
        member ends a row and rows are right-filled with the first.
        cached_image_embeds (extension, per-frame ViT cache): one entry per image of the batch, None = encode it (its patches are in
        pixel_values), else the embeddings an earlier call returned through `last_image_embeds()`.
        prefix_kv (extension, prefix-KV reuse): one entry per sequence - None, or the K/V bf16 [layers, P, 1024] of the sequence's first P
        prompt tokens as an earlier call exported them (the prompt must start with the same P tokens: system prompt + instruction +
        first history frame between the System-2 calls of an episode). Those tokens are not run and their images not encoded;
        pixel_values may still hold every image's patches (the cached images' rows are skipped). Exact: causal attention.
        export_prefix: one entry per sequence - 0, or the number of leading prompt tokens whose K/V to keep (`last_prefix_kv()`).
        past_key_values: an EngineKVCache with one row per sequence, or a list of one-row EngineKVCache / None per sequence, from earlier
        calls (`return_dict_in_generate=True`). Each sequence takes the K/V of the longest common prefix of its prompt and the cached
        token ids (cut back to an image boundary and so that the suffix still runs the kernels of a full prefill: exact). The caller vouches
        that cached images are the same images (only token ids are compared). pixel_values may hold every image or only the others.
        With return_dict_in_generate and use_cache the result carries `.past_key_values`: an EngineKVCache of every sequence's PROMPT
        rows (not the answer: see EngineKVCache).
        output_logprobs (with return_dict_in_generate; needs a model built with token_logprobs=True): the result also carries
        `.token_logprobs` f32 [B, n] - per answer token the log-softmax of the PROCESSED scores (after the repetition penalty) at that token,
        what HF's compute_transition_scores(sequences, scores, normalize_logits=True) returns -, `.token_margins` [B, n] (distance of the
        chosen logit to the runner-up), `.sequences_logprob` [B] (the sum up to and including EOS) and `.answer_lengths` int64 [B] (tokens of
        each answer up to and including its first EOS: the positions the sum runs over); positions behind a row's first EOS hold 0.0. output_scores / output_logits stay swallowed: no [B, vocab] tensor is returned.
        do_sample=True (opt-in; greedy launches what it always launched): HF's multinomial sampling - repetition penalty, temperature, top-k,
        top-p in HF's processor order, then the draw - in one device launch per step in place of the argmax (ops.sample_rows).
        temperature / top_k / top_p: None = generation_config.json's value, without the file HF's defaults 1.0 / 50 / 1.0 (`sampling_spec`,
        which also names the refusals). The uniforms come from `generator` (a CPU torch.Generator), else from a fresh generator seeded
        `seed`, else from the model's own CPU generator (seeded 0 at construction, advancing per call): the same seed gives the same
        sequences. num_return_sequences=K: every prompt is prefilled ONCE (its images encoded once), its K first tokens are drawn from the
        one logits row and its cache rows are replicated into K slots; `sequences` is [B * K, S + n], prompt-major like HF's
        repeat_interleave; B * K beyond the engine's max_seqs raises CapacityError before anything is launched. With K > 1 the result
        carries past_key_values=None, export_prefix is refused (ValueError), and generate_latents on the returned B * K rows (rows= the
        chosen ones) continues the cached state of those rows without re-running their prompts. output_logprobs under sampling works on every model
        (token_logprobs=True is not needed: the sampling path keeps its own buffer): token_logprobs = log q of each draw, the log-softmax
        of HF's processed scores (after penalty, temperature, top-k, top-p); token_margins is not defined for a draw and is NaN inside
        the answer (0.0 behind EOS, like every masked position); answer_confidences' margin of a sampled row is NaN accordingly.
        share_prefix=True (opt-in, needs do_sample=True, any num_return_sequences K >= 1; without it every launch is what it was): the K
        answers of a prompt are decoded behind the prompt's ONE cache slot - no replication into K slots, the attention of the single-token
        passes (ops.attention_shared) reads the prompt in place and every returned sequence keeps only its own answer tokens' K/V in a small
        tail. Capacity then reads B <= max_seqs and B * K <= 64 (SKINNY_GEMM_MAX_ROWS: the passes stay on the weight-streaming kernels),
        max_new_tokens <= max_decode; CapacityError before anything is launched. The tokens are not bit-equal to the fan-out path's (another
        attention kernel: an equally valid rounding). Everything else is as with K > 1 above, for every K: EOS handling, answer_lengths,
        output_logprobs, seed= / generator=, decode_chunk, past_key_values=None in the result, export_prefix refused, generate_latents(rows=)
        continues the chosen rows behind prompt slot + tail. The prompts' cache slots hold exactly what the prefill wrote when the call returns.
        constraint (opt-in; None = every launch what it was): a constrain.TokenAutomaton over the model's vocabulary - what HF users reach
        for prefix_allowed_tokens_fn for, as tables on the device. One short launch in front of every selection (ops.automaton_mask_rows)
        advances each row's state by the token it just got and sets the logits of the tokens its state does not allow to -inf; greedy,
        do_sample (num_return_sequences / share_prefix: a state per returned sequence), output_logprobs (the log-softmax over the ALLOWED
        tokens: HF's processed scores) and past_key_values work as without it. At most 256 states and 256 token classes. An answer that
        max_new_tokens cuts before an accepting state is returned as it is. score_answers is NOT constrained and not renormalised.
        num_beams=K > 1 (opt-in BY ARGUMENT only; None or 1 = the paths above, launch for launch): transformers' beam search
        (GenerationMixin._beam_search; tests/beam_ref.py restates its rules) - the K most probable answers of every prompt, deterministic and
        distinct, decoded behind the prompt's ONE cache slot like share_prefix sampling, with three more launches per step and no host round
        trip inside a decode_chunk (`QwenVLEngine.prefill(beam=)`). num_return_sequences=n <= K (default 1), length_penalty (default 1.0) and
        early_stopping (False, True or "never") mean what they mean in HF; repetition_penalty, eos_token_id (at most 3 ids) and constraint
        work as everywhere. `sequences` is [B * n, S + T], prompt-major, best first, right-filled with the first EOS id; with
        return_dict_in_generate the result also carries sequences_scores f32 [B * n] (sum of log-probabilities / length ** length_penalty),
        answer_lengths, valid bool [B * n] (a finished hypothesis with a score above -inf; an invalid row is filled with EOS and scores -inf)
        and, with output_logprobs=True (any model), token_logprobs [B * n, T]: the hypothesis's per-token transition scores, 0.0 behind its
        end - their sum / length ** length_penalty is the score. past_key_values is None and export_prefix is refused, as with K > 1 sampling;
        generate_latents(rows=) on the returned rows runs answer + latent queries as one suffix pass behind the untouched prompt slot.
        Capacity: B <= max_seqs, B * K <= 64, K <= 8, max_new_tokens <= max_decode; CapacityError before anything is launched.
        Two documented differences from HF: (1) the repetition penalty acts on log-probabilities here as in HF's beam search, which is NOT what
        the greedy and sampled paths do (they penalise logits, as HF does there); with constraint= the banned logits are -inf BEFORE the
        log-softmax, so a score is the log-probability over the allowed tokens, renormalised per step - HF's prefix_allowed_tokens_fn under
        beams masks behind the softmax and does not renormalise; a hypothesis that had to take a banned token stays at -inf and is not valid.
        (2) a generation_config.json that sets num_beams > 1 stays refused at load: the agent's captured plan() / run_decode chain is greedy.
        Refused (as HF / NotImplementedError naming the key): `beam_spec`.
        sequence_bias, no_repeat_ngram_size, bad_words_ids, min_length, min_new_tokens, forced_eos_token_id, suppress_tokens,
        begin_suppress_tokens (opt-in; None = the model's `generation_rules`, without them every launch what it was): transformers' logits
        processors of these names, in `_get_logits_processor`'s order, compiled per call to tables on the device (`logit_rules.compile_rules`:
        this call's EOS ids, each row's REAL prompt length, max_new_tokens) and applied by one launch in front of every selection
        (ops.logit_rules_rows) - greedy, output_logprobs (the log-softmax over the processed scores), do_sample with num_return_sequences /
        share_prefix (a history per returned sequence), constraint= (forced_eos_token_id wins over the automaton), past_key_values and
        decode_chunk alike. A row's history is its own prompt tokens (cached prefix and image placeholders included, padding not) + its
        answer: in a ragged batch that is what a batch-1 HF call on the row sees, where HF on a left-padded batch would count and match the
        pad tokens too. ValueError as HF's validators raise it (`logit_rules.normalize`); with num_beams > 1 NotImplementedError before
        anything is launched. score_answers and generate_latents apply no rules."""
        rule_spec = logit_rules.merge(getattr(self, "generation_rules", None), dict(
            sequence_bias=sequence_bias, no_repeat_ngram_size=no_repeat_ngram_size, bad_words_ids=bad_words_ids, min_length=min_length,
            min_new_tokens=min_new_tokens, forced_eos_token_id=forced_eos_token_id, suppress_tokens=suppress_tokens,
            begin_suppress_tokens=begin_suppress_tokens))
        if rule_spec:                                            # (without a key the engine is not even looked at here)
            rule_spec = logit_rules.normalize(rule_spec, self.qwen.cfg["vocab"])
        if rule_spec and num_beams is not None and int(num_beams) > 1:
            raise NotImplementedError(f"generate(num_beams > 1) with logit rules ({', '.join(rule_spec)}): beam search applies HF's processors to "
                                      "log-probabilities and re-parents the histories; not implemented")
        if constraint is not None and getattr(constraint, "vocab", None) != self.qwen.cfg["vocab"]:
            raise ValueError(f"constraint: an automaton over {getattr(constraint, 'vocab', None)} tokens, this model has {self.qwen.cfg['vocab']}")
        bms = beam_spec(num_beams, num_return_sequences, length_penalty, early_stopping, do_sample, share_prefix, kw)
        share_prefix = bool(share_prefix) and bms is None
        smp = sampling_spec(self.generation_config, do_sample, temperature, top_k, top_p, None if bms is not None else num_return_sequences, kw)
        if bms is not None:                                      # every refusal of the beam path before anything is launched
            n_eos = len(self.generation_config.eos_token_id if eos_token_id is None else eos_ids(eos_token_id))
            if export_prefix is not None and any(export_prefix):
                raise ValueError("export_prefix is not supported with num_beams > 1: export the prefix from a call with one sequence per prompt")
            if input_ids.shape[0] > self.qwen.B_max or input_ids.shape[0] * bms.K > SKINNY_GEMM_MAX_ROWS:
                raise CapacityError(f"{input_ids.shape[0]} prompts x num_beams={bms.K} exceed the engine's max_seqs={self.qwen.B_max} prompts or the "
                                    f"{SKINNY_GEMM_MAX_ROWS} rows of a single-token pass")
            if bms.K > BEAM_MAX_BEAMS or n_eos > BEAM_MAX_EOS:
                raise CapacityError(f"num_beams={bms.K} with {n_eos} EOS ids: the beam path takes at most {BEAM_MAX_BEAMS} beams and {BEAM_MAX_EOS} EOS ids")
            if max_new_tokens > self.qwen.max_decode:
                raise CapacityError(f"max_new_tokens={max_new_tokens} exceeds the engine's max_decode={self.qwen.max_decode}: build the model with a "
                                    "larger max_decode (from_pretrained(..., max_decode=N))")
        if share_prefix and smp is None:
            raise ValueError("share_prefix=True needs do_sample=True: greedy decoding returns one sequence per prompt and has nothing to share")
        if smp is not None:
            if (smp.K > 1 or share_prefix) and export_prefix is not None and any(export_prefix):
                raise ValueError("export_prefix is not supported with num_return_sequences > 1 or share_prefix=True: export the prefix from a call "
                                 "with one sequence per prompt")
            if share_prefix:
                if input_ids.shape[0] > self.qwen.B_max or input_ids.shape[0] * smp.K > SKINNY_GEMM_MAX_ROWS:
                    raise CapacityError(f"{input_ids.shape[0]} prompts x num_return_sequences={smp.K} behind shared prompts exceed the engine's "
                                        f"max_seqs={self.qwen.B_max} prompts or the {SKINNY_GEMM_MAX_ROWS} rows of a single-token pass")
            elif input_ids.shape[0] * smp.K > self.qwen.B_max:
                raise CapacityError(f"{input_ids.shape[0]} prompts x num_return_sequences={smp.K} exceed the engine's max_seqs={self.qwen.B_max}")
            if max_new_tokens > self.qwen.max_decode:
                raise CapacityError(f"max_new_tokens={max_new_tokens} exceeds the max_decode={self.qwen.max_decode} log-probability columns of the "
                                    "sampling path: build the model with a larger max_decode (from_pretrained(..., max_decode=N))")
        if output_logprobs and smp is None and bms is None and not self.qwen.token_logprobs:
            raise ValueError("generate(output_logprobs=True) needs the engine setting token_logprobs: build the model with "
                             "token_logprobs=True (from_pretrained(..., token_logprobs=True) / model_settings['token_logprobs'] = True)")
        if self.qwen.token_logprobs and max_new_tokens > self.qwen.max_decode:
            raise CapacityError(f"max_new_tokens={max_new_tokens} exceeds the max_decode={self.qwen.max_decode} log-probability columns of this "
                                "token_logprobs model: build it with a larger max_decode (from_pretrained(..., max_decode=N))")
        eos_all = self.generation_config.eos_token_id if eos_token_id is None else eos_ids(eos_token_id)
        eos, eos_t = eos_all[0], torch.tensor(eos_all, dtype=torch.long)
        penalty = self.generation_config.repetition_penalty if repetition_penalty is None else float(repetition_penalty)
        pv = pixel_values.to(self.device, torch.bfloat16) if pixel_values is not None and pixel_values.numel() else None
        B, S = input_ids.shape
        # ragged batch (extension; the reference is batch 1): prompts RIGHT-padded to a common length, real lengths from attention_mask
        plens = np.full(B, S, dtype=np.int64) if attention_mask is None else np.asarray(attention_mask.cpu().long().sum(1), dtype=np.int64)
        if attention_mask is not None:
            am = attention_mask.cpu().long()
            assert bool((am[:, 1:] <= am[:, :-1]).all()), "ragged System-2 batches are right-padded (mask = 1...1 0...0)"
        rules = logit_rules.compile_rules(rule_spec, self.qwen.cfg["vocab"], eos_all, plens, max_new_tokens) if rule_spec else None
        pl = 0
        self._gen = None                                       # the cache slots (and tails) are rewritten from here on: nothing older may be continued
        self.last_kv_reuse = dict(rows=0, fallbacks=0)
        if past_key_values is not None:
            assert prefix_kv is None, "past_key_values and prefix_kv are two forms of the same reuse: pass one"
            pl, pv = self._import_past(input_ids, plens, pv, image_grid_thw, past_key_values, cached_image_embeds,
                                       max_new_tokens + self.qwen.latent_q.shape[0])
        elif prefix_kv is not None and any(k is not None for k in prefix_kv):
            assert len(prefix_kv) == B and cached_image_embeds is None, "prefix_kv: one entry per sequence (not combined with cached_image_embeds)"
            pl = np.asarray([0 if k is None else int(k.shape[1]) for k in prefix_kv], dtype=np.int64)
            if int(pl.max()) + S - int(pl.min()) + max_new_tokens + self.qwen.latent_q.shape[0] > self.qwen.S_max:
                # prefixes of different lengths widen the rectangle the engine runs (every sequence's rows start behind ITS prefix): if that
                # no longer fits the cache, run this call without the prefix caches - same results, only the saving is lost
                prefix_kv, pl = [None] * B, np.zeros(B, dtype=np.int64)
            for b, k in enumerate(prefix_kv):
                if k is not None:
                    self.qwen.import_prefix_kv(b, k)
            # drop the patch rows of the images whose tokens are cached K/V
            skip = self.qwen.images_in_prefix(input_ids, image_grid_thw, pl)
            if pv is not None and any(skip):
                n_rows = [int(t * h * w) for t, h, w in image_grid_thw.tolist()]
                assert pv.shape[0] == sum(n_rows), "prefix_kv: pixel_values must hold the patches of every image of the batch"
                off = np.concatenate([[0], np.cumsum(n_rows)])
                keep = [pv[off[i]:off[i + 1]] for i, s in enumerate(skip) if not s]
                pv = torch.cat(keep, 0) if keep else None
        state = self.qwen.prefill(input_ids, pv, image_grid_thw, cached_embeds=cached_image_embeds, seq_lens=plens if attention_mask is not None else None,
                                  prefix_len=pl, **({} if penalty == 1.0 else {"repetition_penalty": penalty}), **self._sampling_kw(smp, B, max_new_tokens, generator, seed, share_prefix),
                                  **({} if constraint is None else {"constraint": constraint}),
                                  **({} if rules is None else {"logit_rules": rules}),
                                  **({} if bms is None else {"beam": dict(K=bms.K, max_new_tokens=max_new_tokens, eos=eos_all, length_penalty=bms.length_penalty,
                                                                          early_stopping=bms.early_stopping)}))
        self._prefix_out = {}
        if export_prefix is not None:
            for b, n in enumerate(export_prefix):
                if n:
                    self._prefix_out[b] = self.qwen.export_prefix_kv(b, int(n))
        self._fresh = self.qwen.fresh_image_embeds(state["plan"]) if cached_image_embeds is not None else {}
        if bms is not None:
            return self._finish_beams(state, bms, input_ids, plens, max_new_tokens, decode_chunk, eos, return_dict_in_generate, output_logprobs)
        chunks, n = [], 0
        while n < max_new_tokens:
            k = min(decode_chunk, max_new_tokens - n)
            t = self.qwen.decode(state, k + 1 if n else k)  # later chunks re-emit the pending token first
            t = t[:, 1:] if n else t
            chunks.append(t.cpu().long())
            n += k
            if bool(torch.isin(torch.cat(chunks, dim=1), eos_t).any(dim=1).all()):
                break
        toks = torch.cat(chunks, dim=1)
        lens = []
        for b in range(toks.shape[0]):
            hit = torch.isin(toks[b], eos_t).nonzero()
            e = int(hit[0]) + 1 if hit.numel() else toks.shape[1]
            toks[b, e:] = eos
            lens.append(e)
        K = 1 if smp is None else smp.K
        fanned = K > 1 or share_prefix                            # the cached state is of B * K rows (or, shared, of rows without a slot)
        ids_cpu = input_ids.cpu().long()
        if K > 1:                                                 # rows are prompt-major from here on: row b * K + c = prompt b, sequence c
            plens, ids_cpu = np.repeat(plens, K), ids_cpu.repeat_interleave(K, dim=0)
        # what generate_latents continues: the greedy state (and the sampled one of one sequence per prompt in its own slot) through
        # qwen.latents, which appends to the cache; a fanned state - B * K rows, or rows without a slot - through qwen.latents_behind, which
        # writes nothing and runs only the rows it is asked for
        self._gen = dict(state=state, tokens=toks, lens=np.asarray(lens), prompt_lens=plens, fanned=fanned,
                         path="shared" if share_prefix else "fan" if fanned else None)
        # every row = its own prompt, then its answer, right-filled with EOS to the common width S + n
        seqs = torch.full((B * K, S + toks.shape[1]), eos, dtype=torch.long)
        for b in range(B * K):
            L = int(plens[b])
            seqs[b, :L] = ids_cpu[b, :L]
            seqs[b, L:L + toks.shape[1]] = toks[b]
        seqs = seqs.to(self.device)
        if not return_dict_in_generate:
            return seqs
        lp_out = {}
        if output_logprobs and smp is not None:
            lp = self.qwen.last_sample_logprobs(state)         # one column per draw
            assert lp.shape == toks.shape, (lp.shape, toks.shape)
            lp_out = vars(answer_logprob_summary(lp, torch.full_like(lp, float("nan")), lens))
        elif output_logprobs:
            lp, mg = self.qwen.last_logprobs(state)            # one column per selection = per emitted token, chunked or not
            assert lp.shape[1] == toks.shape[1], (lp.shape, toks.shape)
            lp_out = vars(answer_logprob_summary(lp, mg, lens))
        # a prefill narrower than ATTN_WIDE_MIN_ROWS, or of SKINNY_GEMM_MAX_ROWS rows or fewer, ran other kernels than a full prefill of
        # a real prompt: only the rows it took from a cache are exact
        exact = int(state["S_run"]) >= ATTN_WIDE_MIN_ROWS and B * int(state["S_run"]) > SKINNY_GEMM_MAX_ROWS
        keep = plens if exact else np.broadcast_to(np.asarray(pl, dtype=np.int64), (B,))
        pkv = self.qwen.kv_handle([ids_cpu[b, : int(keep[b])] for b in range(B)]) if use_cache and not fanned else None
        return SimpleNamespace(sequences=seqs, past_key_values=pkv, **lp_out)

    def _finish_beams(self, state, bms, input_ids, plens, max_new_tokens: int, decode_chunk: int, eos: int, as_dict: bool, with_logprobs: bool):
        """the decode loop and the outputs of generate(num_beams=K): chunks of device-side steps, ONE host read (the prompts' done flags) per chunk"""
        n = 0
        while n < max_new_tokens:
            k = min(decode_chunk, max_new_tokens - n)
            self.qwen.decode(state, k + 1 if n else k)           # later chunks re-emit the pending tokens first
            n += k
            if bool(self.qwen.beam_done(state).all()):
                break
        res = self.qwen.beam_results(state)
        B, S = input_ids.shape
        K, nr = bms.K, bms.n
        valid = (res.finished & (res.scores > -float("inf")))[:, :nr].reshape(-1)
        lens = torch.where(valid, res.lengths[:, :nr].reshape(-1), torch.zeros((), dtype=torch.long))
        scores = torch.where(valid, res.scores[:, :nr].reshape(-1), torch.full((), -float("inf")))
        T = max(1, int(lens.max()))
        cols = torch.arange(T).view(1, T)
        inside = cols < lens.view(-1, 1)
        toks = torch.where(inside, res.tokens[:, :nr, :T].reshape(B * nr, T), torch.full((), eos, dtype=torch.long))
        ids_cpu = input_ids.cpu().long().repeat_interleave(nr, dim=0)
        pl = np.repeat(plens, nr)
        seqs = torch.full((B * nr, S + T), eos, dtype=torch.long)
        for r in range(B * nr):
            L = int(pl[r])
            seqs[r, :L] = ids_cpu[r, :L]
            seqs[r, L:L + T] = toks[r]
        # what generate_latents continues: the prompts' slots, which the search never wrote (qwen.latents_after)
        self._gen = dict(state=state, tokens=toks, lens=lens.numpy(), prompt_lens=pl, fanned=True, path="beam", prompt_of=np.repeat(np.arange(B), nr))
        seqs = seqs.to(self.device)
        if not as_dict:
            return seqs
        out = dict(sequences=seqs, past_key_values=None, sequences_scores=scores.to(self.device), answer_lengths=lens.to(self.device), valid=valid.to(self.device))
        if with_logprobs:
            out["token_logprobs"] = torch.where(inside, res.token_scores[:, :nr, :T].reshape(B * nr, T), torch.zeros(())).to(self.device)
        return SimpleNamespace(**out)

    def _sampling_kw(self, smp, B: int, max_new_tokens: int, generator, seed, share_prefix: bool = False) -> dict:
        """the engine's sampling spec of one generate() call ({} = greedy): the uniforms of every step and returned sequence, drawn HERE on
        the host (one f32 [max_new_tokens, B * K] table, one copy to the device) - no random number is generated in a kernel"""
        if smp is None:
            return {}
        if generator is not None:
            assert isinstance(generator, torch.Generator) and generator.device.type == "cpu", "generator: a CPU torch.Generator"
        gen = generator if generator is not None else (torch.Generator(device="cpu").manual_seed(int(seed)) if seed is not None else self._sample_gen)
        u = torch.rand(max_new_tokens, B * smp.K, generator=gen, dtype=torch.float32).to(self.device)
        # (share_prefix travels beside the spec: `sampling_spec`'s namespace is HF's sampling parameters only)
        return {"sampling": dict(temperature=smp.temperature, top_k=smp.top_k, top_p=smp.top_p, u=u, K=smp.K, **({"share_prefix": True} if share_prefix else {}))}

    def score_answers(self, input_ids, answers, pixel_values=None, image_grid_thw=None, attention_mask=None, share_prefix: bool = False,
                      max_suffix_rows: Optional[int] = None) -> SimpleNamespace:
        """Teacher-forced scoring of caller-supplied answers: how likely is each candidate given its prompt?
        input_ids int [B, S] (right-padded with attention_mask, as generate() takes them), answers: per prompt a list of candidate token-id
        lists (append EOS to a candidate to have EOS scored). -> token_logprobs: per prompt, per candidate an f32 tensor [len] with
        log P(token i | prompt, tokens < i); lengths (the same nesting, ints); sequences_logprob: per prompt an f32 tensor [candidates] of
        the sums (device tensors).
        The log-softmax runs over the RAW logits: NO repetition penalty is applied (under teacher forcing the seen set would differ at every
        position; generate()'s token_logprobs are after the penalty - the two agree at penalty 1.0). Works without token_logprobs=True.
        Nor is an answer constraint (generate(constraint=)) applied: the scores are over the whole vocabulary, not renormalised over the
        tokens an automaton would allow, and a candidate the automaton rejects is scored like any other.
        Every (prompt, candidate) pair is one right-padded sequence of a normal prefill (images are encoded per pair: a prompt with four
        candidates runs the vision tower on its images four times), in groups of at most the engine's max_seqs pairs; the hidden rows that
        predict answer tokens are gathered, normed and run through lm_head into an fp32 [<= 256, vocab] buffer, and ops.logprob_rows reads the
        target tokens' log-probabilities off it.
        share_prefix=True (opt-in; the default path is unchanged): every prompt is prefilled ONCE (groups of at most max_seqs prompts, its images
        encoded once), token 0 of each of its candidates is read off the prompt's last hidden row, and only the candidates' own tokens
        0 .. n - 2 run through the stack as a suffix pass whose attention (ops.attention_prefix) reads the prompt's K/V in place in its cache
        slot. Same result object; the values differ from the default path's by kernel rounding (other GEMM tiles, another attention kernel).
        Candidates of more than 65 tokens raise ValueError (use the default path). max_suffix_rows: rows of one suffix pass (default: the
        engine's row buffers).
        `last_score` = dict(prompt_prefills, images_encoded, suffix_rows, suffix_passes) of the last call, either path."""
        q = self.qwen
        self._gen = None                                       # the cache slots are rewritten: generate_latents() must not continue an older generate()
        ids_cpu = input_ids.cpu().long()
        B, S0 = ids_cpu.shape
        assert len(answers) == B, "answers: one list of candidates per prompt"
        plens = np.full(B, S0, dtype=np.int64) if attention_mask is None else np.asarray(attention_mask.cpu().long().sum(1), dtype=np.int64)
        grids = image_grid_thw.tolist() if image_grid_thw is not None else []
        img_of = [[] for _ in range(B)]                        # images of each prompt (prompt order) and their patch rows in pixel_values
        k = 0
        for b in range(B):
            left = int((ids_cpu[b, : plens[b]] == q.cfg["image_token_id"]).sum())
            while left > 0:
                t, h, w = (int(v) for v in grids[k])
                img_of[b].append(k)
                left -= t * h * w // 4
                k += 1
            assert left == 0, "image tokens and image_grid_thw disagree"
        p_off = np.concatenate([[0], np.cumsum([int(t * h * w) for t, h, w in grids])]).astype(np.int64)
        pv_all = pixel_values.to(self.device, torch.bfloat16) if pixel_values is not None and pixel_values.numel() else None
        pairs = [(b, [int(t) for t in cand]) for b in range(B) for cand in answers[b]]
        vocab = q.cfg["vocab"]
        for b, cand in pairs:
            assert all(0 <= t < vocab for t in cand), "answer token outside the vocabulary"
        if share_prefix:
            longest = max((len(c) for _, c in pairs), default=0)
            if longest - 1 > SCORE_SUFFIX_MAX_ROWS:             # before any launch
                raise ValueError(f"score_answers(share_prefix=True) scores candidates of at most {SCORE_SUFFIX_MAX_ROWS + 1} tokens, got one of "
                                 f"{longest}: score it with share_prefix=False (the per-pair path, one prefill per candidate)")
            return self._score_shared_prefix(ids_cpu, plens, answers, pv_all, image_grid_thw, img_of, p_off, max_suffix_rows)
        self.last_score = dict(prompt_prefills=0, images_encoded=0, suffix_rows=0, suffix_passes=0)
        out_lp = {}
        for g0 in range(0, len(pairs), q.B_max):
            grp = pairs[g0:g0 + q.B_max]
            pl, al = np.asarray([plens[b] for b, _ in grp]), np.asarray([len(c) for _, c in grp])
            S, rows, off, slabs = score_row_plan(pl, al)
            ids = torch.zeros(len(grp), S, dtype=torch.long)
            for r, (b, cand) in enumerate(grp):
                ids[r, : pl[r]] = ids_cpu[b, : pl[r]]
                ids[r, pl[r]: pl[r] + al[r]] = torch.tensor(cand, dtype=torch.long)
            imgs = [k for b, _ in grp for k in img_of[b]]
            pv = torch.cat([pv_all[p_off[k]:p_off[k + 1]] for k in imgs], 0) if imgs else None
            grid = image_grid_thw[imgs] if imgs else None
            q.prefill(ids, pv, grid, seq_lens=pl + al)
            self.last_score["prompt_prefills"] += len(grp)
            self.last_score["images_encoded"] += len(imgs)
            R = int(off[-1])
            if R == 0:
                continue
            lp = torch.empty(R, dtype=torch.float32, device=self.device)
            self._score_rows(q.x[: len(grp) * S], rows, slabs, [t for _, c in grp for t in c], lp)
            for r in range(len(grp)):
                out_lp[g0 + r] = lp[off[r]:off[r + 1]]
        res_lp, res_len, res_sum, i = [], [], [], 0
        for b in range(B):
            n = len(answers[b])
            per = [out_lp.get(i + c, torch.empty(0, dtype=torch.float32, device=self.device)) for c in range(n)]
            res_lp.append(per)
            res_len.append([int(t.numel()) for t in per])
            res_sum.append(torch.stack([t.sum() for t in per]) if per else torch.empty(0, dtype=torch.float32, device=self.device))
            i += n
        return SimpleNamespace(token_logprobs=res_lp, lengths=res_len, sequences_logprob=res_sum)

    def _score_rows(self, x_rows: torch.Tensor, rows: np.ndarray, slabs, targets, lp: torch.Tensor):
        """gather rows of the residual stream, final norm, lm_head and the target tokens' log-probabilities, one slab at a time -> lp [len(rows)]"""
        q, vocab = self.qwen, self.qwen.cfg["vocab"]
        if self._score_logits is None:
            self._score_logits = torch.empty(SCORE_SLAB_ROWS, vocab, dtype=torch.float32, device=self.device)
            self._score_x = torch.empty(SCORE_SLAB_ROWS, q.H, dtype=torch.float32, device=self.device)
            self._score_h = torch.empty(SCORE_SLAB_ROWS, q.H, dtype=torch.bfloat16, device=self.device)
        rows_d = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(self.device)
        tgt = torch.tensor(targets, dtype=torch.int32, device=self.device)
        tok = torch.empty(len(targets), dtype=torch.int32, device=self.device)
        for r0, r1 in slabs:
            m = r1 - r0
            x, h, logits = self._score_x[:m], self._score_h[:m], self._score_logits[:m]
            ops.gather_rows(x_rows, x, src=rows_d[r0:r1])
            ops.norm(x, q.norm_w, None, eps=1e-6, rms=True, out=h, rows=m)
            ops.linear(h, q.lm_head, out=logits)
            ops.logprob_rows(logits, tok[r0:r1], lp[r0:r1], target=tgt[r0:r1])

    def _score_shared_prefix(self, ids_cpu, plens, answers, pv_all, image_grid_thw, img_of, p_off, max_suffix_rows) -> SimpleNamespace:
        """score_answers(share_prefix=True): see there. Per group of prompts: one prefill, the first tokens off the prompts' last rows (before
        the suffix pass reuses the residual buffer), then the suffix passes of `score_prefix_plan`."""
        q = self.qwen
        B = ids_cpu.shape[0]
        max_rows = int(q.x.shape[0]) if max_suffix_rows is None else int(max_suffix_rows)
        assert 1 <= max_rows <= q.x.shape[0], f"max_suffix_rows={max_rows} outside [1, {q.x.shape[0]}]"
        self.last_score = dict(prompt_prefills=0, images_encoded=0, suffix_rows=0, suffix_passes=0)
        empty = torch.empty(0, dtype=torch.float32, device=self.device)
        res_lp, res_len, res_sum = [], [], []
        for b0 in range(0, B, q.B_max):
            grp = list(range(b0, min(b0 + q.B_max, B)))
            pl = np.asarray([plens[b] for b in grp], dtype=np.int64)
            cands = [[[int(t) for t in c] for c in answers[b]] for b in grp]
            plan = score_prefix_plan(pl, [[len(c) for c in cs] for cs in cands], max_rows)
            S = plan["S"]
            ids = torch.zeros(len(grp), S, dtype=torch.long)
            for r, b in enumerate(grp):
                ids[r, : pl[r]] = ids_cpu[b, : pl[r]]
            imgs = [k for b in grp for k in img_of[b]]
            pv = torch.cat([pv_all[p_off[k]:p_off[k + 1]] for k in imgs], 0) if imgs else None
            state = q.prefill(ids, pv, image_grid_thw[imgs] if imgs else None, seq_lens=pl)
            self.last_score["prompt_prefills"] += len(grp)
            self.last_score["images_encoded"] += len(imgs)
            cand_of = [cands[r][c] for r, c in plan["pairs"]]
            lp = torch.empty(plan["total"], dtype=torch.float32, device=self.device)
            if plan["first_pair"].size:
                first = torch.empty(plan["first_pair"].size, dtype=torch.float32, device=self.device)
                self._score_rows(q.x[: len(grp) * S], plan["first_rows"], plan["first_slabs"], [cand_of[p][0] for p in plan["first_pair"]], first)
                lp[torch.from_numpy(plan["first_dst"]).to(self.device)] = first
            for ps in plan["passes"]:
                P, m = ps["pair"].size, ps["m"]
                toks = np.zeros((P, m), dtype=np.int64)
                for j, p in enumerate(ps["pair"]):
                    toks[j, : ps["suf_len"][j]] = cand_of[p][:-1]
                x = q.suffix_pass(state, ps["prompt"], toks, ps["suf_len"])
                part = torch.empty(ps["rows"].size, dtype=torch.float32, device=self.device)
                self._score_rows(x, ps["rows"], ps["slabs"], [t for p in ps["pair"] for t in cand_of[p][1:]], part)
                lp[torch.from_numpy(ps["dst"]).to(self.device)] = part
                self.last_score["suffix_rows"] += P * m
                self.last_score["suffix_passes"] += 1
            off, k = plan["off"], 0
            for r in range(len(grp)):
                per = [lp[off[k + c]:off[k + c + 1]] if off[k + c + 1] > off[k + c] else empty for c in range(len(cands[r]))]
                k += len(cands[r])
                res_lp.append(per)
                res_len.append([int(t.numel()) for t in per])
                res_sum.append(torch.stack([t.sum() for t in per]) if per else empty)
        return SimpleNamespace(token_logprobs=res_lp, lengths=res_len, sequences_logprob=res_sum)

    def _import_past(self, input_ids, plens, pv, image_grid_thw, past, cached_image_embeds, tail):
        """generate(past_key_values=...): reused prompt lengths per sequence, the cached rows put into the batch's cache slots, and
        pixel_values without the patches of the images inside the reused prefixes."""
        B = input_ids.shape[0]
        if isinstance(past, EngineKVCache):
            assert len(past) == B, f"past_key_values holds {len(past)} rows for a batch of {B}"
            src = [(past, b) for b in range(B)]
        else:
            assert len(past) == B, "past_key_values: one EngineKVCache (or None) per sequence"
            src = []
            for c in past:
                assert c is None or (isinstance(c, EngineKVCache) and len(c) == 1), "past_key_values: one-row EngineKVCache per sequence"
                src.append(None if c is None else (c, 0))
        ids = input_ids.cpu().numpy().astype(np.int64)
        pl = kv_reuse_lengths(ids, plens, [None if s is None else s[0].token_ids[s[1]] for s in src], self.qwen.cfg["image_token_id"])
        pl, dropped = kv_reuse_fit(pl, ids.shape[1], tail, self.qwen.S_max)
        self.kv_reuse_fallbacks += dropped
        self.kv_reuse_rows += int(pl.sum())
        self.last_kv_reuse = dict(rows=int(pl.sum()), fallbacks=dropped)
        if not pl.any():
            return 0, pv
        self.qwen.import_kv([s if n else None for s, n in zip(src, pl.tolist())], pl)
        skip = self.qwen.images_in_prefix(input_ids, image_grid_thw, pl)
        if pv is not None and any(skip):
            n_rows = [int(t * h * w) for t, h, w in image_grid_thw.tolist()]
            enc = [True] * len(n_rows) if cached_image_embeds is None else [c is None for c in cached_image_embeds]
            if pv.shape[0] == sum(r for r, e in zip(n_rows, enc) if e):     # patches of every image to encode: drop the reused ones
                off = np.concatenate([[0], np.cumsum([r if e else 0 for r, e in zip(n_rows, enc)])])
                keep = [pv[off[i]:off[i + 1]] for i in range(len(n_rows)) if enc[i] and not skip[i]]
                pv = torch.cat(keep, 0) if keep else None
            else:
                assert pv.shape[0] == sum(r for r, e, k in zip(n_rows, enc, skip) if e and not k), \
                    "past_key_values: pixel_values must hold the patches of every image to encode, or of those behind the reused prefixes"
        return pl, pv

    def last_prefix_kv(self) -> Dict[int, torch.Tensor]:
        """sequence index of the last generate() call -> the prefix K/V it was asked to export (`export_prefix`)."""
        return getattr(self, "_prefix_out", {})

    def last_image_embeds(self) -> Dict[int, torch.Tensor]:
        """image index (position in the last generate() call's image list) -> merged embeddings bf16 [tokens, 3584] of every image that
        call encoded; only filled when generate() was given `cached_image_embeds` (i.e. by callers that keep a frame cache)."""
        return getattr(self, "_fresh", {})

    def generate_latents(self, output_ids, pixel_values, image_grid_thw, cached_image_embeds: Optional[list] = None, rows=None):
        """[B, N_QUERY, 3584] hidden states of the latent trajectory queries (internvla_n1.py:320-347). When called right after
        generate() on its own output (the reference's only usage, internvla_n1_policy.py:191) the KV cache is reused: the queries
        are placed behind each sequence's last kept token; otherwise the full prompt is re-run.
        rows (extension for the batched agent): the batch rows whose answer was a pixel goal - only their latents are returned
        ([len(rows), N_QUERY, 3584]); the pass itself streams the weights once whatever the number of rows.
        After a SAMPLED generate() with num_return_sequences > 1 or share_prefix=True (output_ids = its B * K prompt-major rows, rows indexes
        them, None = all) the state that call left is continued too, and ONLY the requested rows run: 1 + N_QUERY rows each behind the prompt
        in its cache slot and the row's own answer K/V (its slot on the fan-out path, its tail on the shared-prefix path), read in place
        (`QwenVLEngine.latents_behind`, ops.attention_prefix_tail) - no ViT, no prefill, nothing written, so the call can be repeated and
        made for other rows. The requested rows' answers must equal the tokens generate() returned (up to the common width); anything
        else - other tokens, another row count, a score_answers() call in between - takes the re-run path, as before.
        After generate(num_beams=K) (output_ids = its B * num_return_sequences rows): a finished hypothesis keeps no tail, but its prompt's
        cache slot is untouched - the requested rows run their answer tokens and then the latent queries as ONE suffix pass behind that slot
        (`QwenVLEngine.latents_after`, ops.attention_prefix; no ViT, no prefill, nothing written, repeatable). An answer of more than
        64 - N_QUERY tokens, an invalid row or other token ids take the re-run path; a pass beyond the buffer rows raises CapacityError."""
        g = getattr(self, "_gen", None)
        if g is not None and g.get("fanned") and output_ids.shape[0] == g["tokens"].shape[0]:
            pl, lens, toks = g["prompt_lens"], g["lens"], g["tokens"]
            sel = list(range(toks.shape[0])) if rows is None else [int(r) for r in rows]
            oc = output_ids.cpu().long()
            nt = toks.shape[1]
            same = sel and all(0 <= r < toks.shape[0] and int(pl[r]) + nt <= oc.shape[1] and torch.equal(oc[r, int(pl[r]):int(pl[r]) + nt], toks[r]) for r in sel)
            if g.get("path") == "beam":
                # a finished hypothesis keeps no tail: answer + latent queries run as ONE suffix pass behind the prompt's untouched slot
                nq = self.qwen.latent_q.shape[0]
                if same and all(1 <= int(lens[r]) and int(lens[r]) + nq <= ops.ATTN_PREFIX_MAX_ROWS for r in sel):
                    return self.qwen.latents_after(g["state"], [int(g["prompt_of"][r]) for r in sel], [toks[r, : int(lens[r])].tolist() for r in sel])
            elif same:
                return self.qwen.latents_behind(g["state"], sel, [int(toks[r, lens[r] - 1]) for r in sel], [int(pl[r] + lens[r] - 1) for r in sel])
        if rows is not None:
            return self.generate_latents(output_ids, pixel_values, image_grid_thw, cached_image_embeds)[torch.as_tensor(list(rows), dtype=torch.long, device=self.device)]
        if g is not None and not g.get("fanned") and output_ids.shape[0] == g["tokens"].shape[0]:
            pl, lens, toks = g["prompt_lens"], g["lens"], g["tokens"]
            oc = output_ids.cpu().long()
            nt = toks.shape[1]
            if all(int(pl[b]) + nt <= oc.shape[1] and torch.equal(oc[b, int(pl[b]):int(pl[b]) + nt], toks[b]) for b in range(toks.shape[0])):
                last = torch.stack([toks[b, lens[b] - 1] for b in range(toks.shape[0])]).to(self.device, torch.int32).view(-1, 1)
                return self.qwen.latents(g["state"], last.contiguous(), seq_lens=pl + lens - 1)
        pv = pixel_values.to(self.device, torch.bfloat16) if pixel_values is not None and pixel_values.numel() else None
        self._gen = None                                       # the re-run rewrites the cache slots: what generate() left is gone
        return self.qwen.generate_latents(output_ids, pv, image_grid_thw, cached_embeds=cached_image_embeds)

    # ---- System 1
    def generate_traj(self, traj_latents, images_dp, depths_dp=None, predict_step_nums: int = 32, guidance_scale: float = 1.0,
                      num_inference_steps: int = 10, num_sample_trajs: int = 32, noise: Optional[dict] = None):
        """[32*B, T, 3] sampled trajectories (internvla_n1.py:349-441). `noise` = dict(x_init[, step_noise]) makes the sampler
        reproducible / checkable; by default it is drawn on the device like the reference's randn_tensor / torch.randn."""
        B = traj_latents.shape[0]
        s1 = self.s1
        S, T = s1.S, s1.T
        x_init = noise["x_init"] if noise else torch.randn(B, S, T, 3, device=self.device, generator=self._noise_gen)
        lat = traj_latents.to(self.device, torch.bfloat16)
        if isinstance(s1, NextDiTSystem1):
            assert num_inference_steps == s1.cfg["num_inference_steps"] and predict_step_nums == T and num_sample_trajs == S
            # without 'async' the images are not part of the condition (internvla_n1.py:382-383): whatever the caller passes is ignored
            img = images_dp.to(self.device) if (s1.use_async and torch.is_tensor(images_dp)) else None
            out = s1.generate_traj(lat, img, x_init, guidance_scale=guidance_scale)
        else:
            K = s1.cfg["num_train_timesteps"]
            sn = noise["step_noise"] if noise else torch.randn(K, B, S, T, 3, device=self.device, generator=self._noise_gen)
            if s1.use_async:
                out = s1.predict_pointgoal_action_async(lat, images_dp.to(self.device), depths_dp.to(self.device), x_init, sn)
            else:                                       # internvla_n1.py:438-439: predict_pointgoal_action(traj_latents) - no images
                out = s1.predict_pointgoal_action(lat, x_init, sn)
        return out.reshape(B * S, T, 3).clone()


class _Prefixed:
    """view of a weight mapping under a key prefix (checkpoints carry the System-1 modules under `model.`)."""

    def __init__(self, base, prefix):
        self.base, self.prefix = base, prefix

    def __getitem__(self, k):
        return self.base[self.prefix + k]

    def get(self, k, default=None):
        try:
            return self.base[self.prefix + k]
        except KeyError:
            return default

    def __contains__(self, k):
        return (self.prefix + k) in self.base

    def shape_of(self, k):
        b = self.base
        return tuple(b.shape_of(self.prefix + k)) if hasattr(b, "shape_of") else tuple(b[self.prefix + k].shape)


class _ShardedCheckpoint:
    """key -> tensor over a list of safetensors shards, read lazily (one tensor on the host at a time: the engines repack and upload
    each parameter as they read it, so a 16 GB checkpoint never sits in host memory twice)."""

    def __init__(self, files):
        from safetensors import safe_open

        self._where = {}
        for f in files:
            with safe_open(str(f), framework="pt", device="cpu") as sf:
                for k in sf.keys():
                    self._where[k] = str(f)

    def __contains__(self, k):
        return k in self._where

    def keys(self):
        return self._where.keys()

    def __getitem__(self, k):
        from safetensors import safe_open

        with safe_open(self._where[k], framework="pt", device="cpu") as sf:
            return sf.get_tensor(k)

    def shape_of(self, k):
        """tensor shape from the shard header (no tensor data is read)."""
        from safetensors import safe_open

        with safe_open(self._where[k], framework="pt", device="cpu") as sf:
            return tuple(sf.get_slice(k).get_shape())


# ------------------------------------------------------------------------------------------------------ policy wrapper
class InternVLAN1ModelConfig:
    """`InternVLAN1ModelConfig` as the agent layer uses it (internvla_n1_agent.py:40-43: `policy_config(model_cfg={'model': ModelCfg.model_dump()})`):
    a holder of `model_cfg`; the HF PretrainedConfig machinery of the reference's class (internvla_n1.py:22-29) is not needed here."""
    model_type = "internvla_n1"

    def __init__(self, model_cfg: Optional[dict] = None, **kwargs):
        self.model_cfg = model_cfg or {"model": {}}
        for k, v in kwargs.items():
            setattr(self, k, v)


class InternVLAN1Net:
    """`InternVLAN1Net` of the reference (internvla_n1_policy.py:26-215) for ONE environment's episode state; the batched agent
    (internnav_amd/agent.py) holds one instance per env that share a single model and batches their model calls."""

    PROMPT = ("You are an autonomous navigation assistant. Your task is to <instruction>. Where should you go next to stay on track? "
              "Please output the next waypoint's coordinates in the image. Please output STOP when you have successfully completed the task.")
    CONJUNCTION = "you can see "
    ACTIONS2IDX = OrderedDict({"STOP": [0], "↑": [1], "←": [2], "→": [3], "↓": [5]})

    _shared: Dict[Any, Any] = {}   # (model_path, device) -> (model, processor): one set of engines per GPU process, shared by all envs

    def __init__(self, config=None, processor=None, num_history: int = 8, resize_w: int = 384, resize_h: int = 384,
                 continuous_traj: bool = True, frame_preprocessor=None, model: Optional[InternVLAN1ForCausalLM] = None,
                 vit_cache: bool = False, prefix_cache: bool = False, kv_reuse: bool = False, repetition_penalty: Optional[float] = None,
                 answer_constraint=None):
        """Two ways in, both ending in (model, processor, episode state):
          * the reference's: `InternVLAN1Net(config=InternVLAN1ModelConfig(model_cfg={'model': model_settings}))`
            (internvla_n1_agent.py:39-43, internvla_n1_policy.py:29-48) - loads the checkpoint at model_settings['model_path'] on
            model_settings['device'] with `InternVLAN1ForCausalLM.from_pretrained`, and the HF tokenizer / processor from the same
            path (a1 stays on the host); engines are sized from num_history / resize / camera size / env_num;
          * `InternVLAN1Net(model, processor, ...)` with an already-built model (tests, bench, the batched agent's per-env states).
        frame_preprocessor: an internnav_amd.preprocess.FramePreprocessor - the PIL resizes and the HF image processor then run on
        the device from raw uint8 frames (bit-exact with the host path); the processor is only used for the chat template and
        its tokenizer."""
        if model is None and config is not None and not hasattr(config, "model_cfg"):
            model, config = config, None                      # legacy positional form: InternVLAN1Net(model, processor, ...)
        if model is None:
            ms = dict(config.model_cfg["model"])
            num_history, resize_w, resize_h = ms.get("num_history", num_history), ms.get("resize_w", resize_w), ms.get("resize_h", resize_h)
            continuous_traj = ms.get("continuous_traj", continuous_traj)
            model, processor = self._load(ms)
            if frame_preprocessor is None and ms.get("device_preprocess", False):
                from .preprocess import FramePreprocessor

                frame_preprocessor = FramePreprocessor(model.device, resize_w=resize_w, resize_h=resize_h)
        self.model_config = SimpleNamespace(num_history=num_history, resize_w=resize_w, resize_h=resize_h, continuous_traj=continuous_traj)
        self.model, self.processor, self.pre = model, processor, frame_preprocessor
        # per-frame ViT cache (needs the device pre-processor): the embeddings of the frames of the previous System-2
        # call are kept, so the look-down turn (which re-sends every image of the turn before, internvla_n1_policy.py:140-147) and
        # re-sampled history frames (frame 0 is in every np.linspace sample) skip the vision tower. Exact: the tower attends per image.
        self.vit_cache = bool(vit_cache or (config is not None and dict(config.model_cfg["model"]).get("vit_cache", False))) and frame_preprocessor is not None
        # prefix-KV reuse (model_settings['prefix_cache']): every System-2 prompt of an episode after the first starts with the same tokens -
        # chat template, instruction, "These are your historical observations:" and history frame 0 (np.linspace always samples it,
        # internvla_n1_policy.py:125-133); the look-down turn repeats the whole previous prompt. Their K/V of all 28 layers are kept per env
        # (17 MB for 296 tokens) and handed back to generate(): those tokens are not prefilled, frame 0 is not encoded. Exact (causal mask).
        # KV reuse (model_settings['kv_reuse']): the EngineKVCache of this env's last System-2 call is kept with the identity of every image in
        # it, and the next call takes the longest prefix on which token ids AND images agree - the whole previous prompt for the look-down
        # turn, template + instruction + every leading history frame the np.linspace sample repeats otherwise. Works with vit_cache and
        # supersedes prefix_cache. Exact (causal mask; EngineKVCache / kv_reuse_lengths keep the prefill bit-equal).
        self.kv_reuse = bool(kv_reuse or (config is not None and dict(config.model_cfg["model"]).get("kv_reuse", False))) \
            and hasattr(getattr(model, "qwen", None), "kv_handle")
        self.prefix_cache = bool(prefix_cache or (config is not None and dict(config.model_cfg["model"]).get("prefix_cache", False))) \
            and hasattr(getattr(model, "qwen", None), "export_prefix_kv") and not self.vit_cache and not self.kv_reuse
        # model_settings['repetition_penalty'] (None: the checkpoint's generation_config.json): passed to every System-2 generate() of this env,
        # by s2_step and by the batched agent alike
        self.repetition_penalty = dict(config.model_cfg["model"]).get("repetition_penalty", repetition_penalty) if config is not None else repetition_penalty
        # model_settings['answer_constraint'] (a constrain.TokenAutomaton, e.g. TokenAutomaton.navigation_answers over the tokenizer's byte
        # vocabulary; None = unconstrained): passed to every System-2 generate() of this env, by s2_step and by the batched agent alike, so
        # an answer always parses - no retry of the whole System-2 call for a malformed one
        self.answer_constraint = dict(config.model_cfg["model"]).get("answer_constraint", answer_constraint) if config is not None else answer_constraint
        self.tokenizer = getattr(processor, "tokenizer", None)
        self.num_history, self.resize_w, self.resize_h, self.continuous_traj = num_history, resize_w, resize_h, continuous_traj
        self.device = model.device
        self.reset()

    @classmethod
    def _load(cls, ms: dict):
        """model + processor for a model_settings dict, loaded once per (checkpoint, device) and shared afterwards."""
        key = (str(ms["model_path"]), str(ms.get("device", "cuda:0")), bool(ms.get("w8_decode", False)), bool(ms.get("ignore_generation_config", False)),
               bool(ms.get("token_logprobs", False)), bool(ms.get("mx4_decode", False)), repr(ms.get("generation_rules")))
        if key not in cls._shared:
            n_env = int(ms.get("env_num", 1) or 1)
            model = InternVLAN1ForCausalLM.from_pretrained(
                ms["model_path"], torch_dtype=torch.bfloat16, attn_implementation="flash_attention_2", device_map={"": ms.get("device", "cuda:0")},
                max_envs=max(n_env, int(ms.get("max_envs", 1))), max_s2_seqs=ms.get("max_s2_seqs"), num_history=ms.get("num_history", 8),
                resize_w=ms.get("resize_w", 384), resize_h=ms.get("resize_h", 384), cam_w=ms.get("width", 640), cam_h=ms.get("height", 480),
                w8_decode=bool(ms.get("w8_decode", False)),      # System-2 single-token passes on FP8 weights (QwenVLEngine(w8_decode=True))
                ignore_generation_config=bool(ms.get("ignore_generation_config", False)),
                generation_rules=ms.get("generation_rules"),     # default logits-processor rules of every System-2 generate() (dict, or "file")
                mx4_decode=bool(ms.get("mx4_decode", False)),    # ... on MXFP4 weights (QwenVLEngine(mx4_decode=True)); not both
                token_logprobs=bool(ms.get("token_logprobs", False)))   # per-token log-probabilities of System-2 answers (S2Output.answer_logprob)
            cls._shared[key] = (model.eval(), cls.load_processor(ms["model_path"]))
        return cls._shared[key]

    @staticmethod
    def load_processor(model_path):
        """the HF processor + tokenizer of the checkpoint, exactly as the reference loads them (internvla_n1_policy.py:40-43):
        third-party host-side pre-processing."""
        from transformers import AutoProcessor, AutoTokenizer

        processor = AutoProcessor.from_pretrained(model_path)
        processor.tokenizer = AutoTokenizer.from_pretrained(model_path, use_fast=True)
        processor.tokenizer.padding_side = "left"
        return processor

    def spawn(self) -> "InternVLAN1Net":
        """a fresh episode state on the same model / processor (the batched agent keeps one per environment)."""
        return InternVLAN1Net(processor=self.processor, num_history=self.num_history, resize_w=self.resize_w, resize_h=self.resize_h,
                              continuous_traj=self.continuous_traj, frame_preprocessor=self.pre, model=self.model, vit_cache=self.vit_cache,
                              prefix_cache=self.prefix_cache, kv_reuse=self.kv_reuse, repetition_penalty=self.repetition_penalty,
                              answer_constraint=self.answer_constraint)

    def eval(self):
        return self

    def reset(self):
        self.rgb_list, self.depth_list, self.pose_list = [], [], []
        self.episode_idx = 0
        self.conversation_history = []
        self.llm_output = ""
        self.input_images = []
        self.input_keys = []          # frame identity of every input image: index into rgb_list, or "look_down"
        self._emb_cache = {}          # frame key -> (embeds bf16 [tokens, H], grid) of the frames of the last System-2 call
        self._prefix = None           # (token ids of the cached prompt prefix, K/V bf16 [layers, P, 1024]) of this episode
        self.image_keys = []          # identity of every input image: index into rgb_list, or ("look_down", call number) - unique per call
        self._s2_calls = 0
        self._kv = None               # (EngineKVCache of the last System-2 prompt, its image_keys) - kv_reuse

    def parse_actions(self, output: str) -> List[int]:
        regex = re.compile("|".join(re.escape(a) for a in self.ACTIONS2IDX))
        return list(itertools.chain.from_iterable(self.ACTIONS2IDX[m] for m in regex.findall(output)))

    def _to_image(self, rgb, resize: bool):
        if self.pre is not None:   # device path: uint8 [H, W, 3] tensors instead of PIL images
            frame = torch.from_numpy(np.ascontiguousarray(np.asarray(rgb)[..., :3], dtype=np.uint8)).to(self.pre.device)
            return self.pre.resize(frame[None], self.resize_w, self.resize_h)[0] if resize else frame
        from PIL import Image

        image = Image.fromarray(rgb).convert("RGB")
        return image.resize((self.resize_w, self.resize_h)) if resize else image

    def step_no_infer(self, rgb, depth, pose):
        self.rgb_list.append(self._to_image(rgb, True))
        self.episode_idx += 1

    def build_s2_inputs(self, rgb, instruction: str, look_down: bool = False):
        """steps 1-2 of s2_step (internvla_n1_policy.py:110-165): history sampling, prompt, chat template, processor call."""
        image = self._to_image(rgb, not look_down)
        if not look_down:
            self.rgb_list.append(image)
            self.conversation_history = []
            text = self.PROMPT.replace("<instruction>.", instruction)
            if self.episode_idx == 0:
                history_id = []
            else:
                history_id = np.unique(np.linspace(0, self.episode_idx - 1, self.num_history, dtype=np.int32)).tolist()
                text += f" These are your historical observations: {('<image>' + chr(10)) * len(history_id)}."
            self.input_images = [self.rgb_list[i] for i in sorted(history_id)] + self.rgb_list[-1:]
            self.input_keys = sorted(history_id) + [len(self.rgb_list) - 1]
            self.image_keys = list(self.input_keys)
            img_id = 0
            self.episode_idx += 1
        else:
            self.input_images.append(image)
            self.input_keys = list(self.input_keys) + ["look_down"]
            self.image_keys = list(self.image_keys) + [("look_down", self._s2_calls)]
            img_id = -1
            assert self.llm_output != "", "Last llm_output should not be empty when look down"
            text = ""
            self.conversation_history.append({"role": "assistant", "content": [{"type": "text", "text": self.llm_output}]})
        self._s2_calls += 1
        text += f" {self.CONJUNCTION}<image>."
        content = []
        for part in split_and_clean(text):
            if part == "<image>":
                content.append({"type": "image", "image": self.input_images[img_id]})
                img_id += 1
            else:
                content.append({"type": "text", "text": part})
        self.conversation_history.append({"role": "user", "content": content})
        chat = self.processor.apply_chat_template(self.conversation_history, tokenize=False, add_generation_prompt=True)
        if self.pre is None:
            return self.processor(text=[chat], images=self.input_images, return_tensors="pt")
        # device pre-processing: pixel_values / grid from the raw frames; the text side restates Qwen2VLProcessor.__call__ - every
        # image placeholder is expanded to grid.prod() / merge^2 image tokens before tokenisation
        cached = None
        if self.vit_cache:
            hit = [self._emb_cache.get(k) if k != "look_down" else None for k in self.input_keys]
            cached = [h[0] if h is not None else None for h in hit]
            fresh = [im for im, h in zip(self.input_images, hit) if h is None]
            if fresh:
                pixel_values, fgrid = self.pre.processor_pixel_values(fresh)
            else:
                pixel_values, fgrid = torch.empty(0, 1176, dtype=torch.bfloat16, device=self.pre.device), torch.empty(0, 3, dtype=torch.int64)
            it = iter(fgrid.tolist())
            grid = torch.tensor([h[1] if h is not None else next(it) for h in hit], dtype=torch.int64)
        else:
            pixel_values, grid = self.pre.processor_pixel_values(self.input_images)
        tok = getattr(self.processor, "image_token", "<|image_pad|>")
        merge2 = self.pre.merge ** 2
        parts = chat.split(tok)
        assert len(parts) == len(self.input_images) + 1, "chat template and image list disagree on the number of images"
        expanded = parts[0]
        for g, rest in zip(grid.tolist(), parts[1:]):
            expanded += tok * (g[0] * g[1] * g[2] // merge2) + rest
        enc = self.processor.tokenizer([expanded], return_tensors="pt")
        out = {"input_ids": enc["input_ids"], "pixel_values": pixel_values, "image_grid_thw": grid}
        if cached is not None:
            out["cached_image_embeds"] = cached
        return out

    def prefix_request(self, inputs) -> Tuple[Optional[torch.Tensor], int]:
        """(prefix K/V to hand to generate() or None, number of leading tokens to export after the call or 0) for the prompt in `inputs`.
        The reusable prefix ends with the <|vision_end|> of the first image when that image is episode frame 0."""
        if not self.prefix_cache or not self.input_keys or self.input_keys[0] != 0:
            return None, 0
        ids = inputs["input_ids"][0]
        ve = (ids == self.model.qwen.cfg["vision_end_id"]).nonzero()
        if ve.numel() == 0:
            return None, 0
        P = int(ve[0]) + 1
        if P >= ids.shape[0]:
            return None, 0
        if self._prefix is not None and self._prefix[0].shape[0] == P and torch.equal(self._prefix[0], ids[:P].cpu()):
            return self._prefix[1], 0
        return None, P

    def kv_request(self, inputs) -> Optional[EngineKVCache]:
        """kv_reuse: the last call's cache, cropped to the prefix on which the images agree too (the engine compares token ids only, and
        every image has the same image-token ids), or None."""
        if not self.kv_reuse or self._kv is None:
            return None
        cache, keys = self._kv
        ids = inputs["input_ids"][0].cpu()
        img = self.model.qwen.cfg["image_token_id"]
        n = min(cache.get_seq_length(0), int(ids.shape[0]))
        old = cache.token_ids[0][:n]
        diff = (ids[:n] != old).nonzero()
        n = int(diff[0]) if diff.numel() else n
        if n == 0:
            return None
        starts = ((ids[:n] == img) & torch.cat([torch.ones(1, dtype=torch.bool), ids[: n - 1] != img])).nonzero().reshape(-1).tolist()
        for j, st in enumerate(starts):           # the j-th image of both prompts begins at st (the tokens before it are equal)
            if j >= len(keys) or j >= len(self.image_keys) or keys[j] != self.image_keys[j]:
                n = st
                break
        if n == 0:
            return None
        return cache.crop(n)

    def store_kv(self, inputs, cache: Optional[EngineKVCache]):
        self._kv = None if cache is None or not self.kv_reuse else (cache, list(self.image_keys))

    def store_prefix(self, inputs, kv: torch.Tensor):
        self._prefix = (inputs["input_ids"][0, : kv.shape[1]].cpu().clone(), kv)

    def update_frame_cache(self, inputs, fresh: Dict[int, torch.Tensor]):
        """keep the embeddings of exactly the frames of this call (bounded: <= num_history + 2 frames of 196 - 391 tokens)."""
        if not self.vit_cache:
            return
        grids = inputs["image_grid_thw"].tolist()
        new = {}
        for k, key in enumerate(self.input_keys):
            if key == "look_down":
                continue
            c = inputs["cached_image_embeds"][k]
            e = c if c is not None else fresh.get(k)
            if e is not None:
                new[key] = (e, grids[k])
        self._emb_cache = new

    def finish_s2(self, inputs, output_ids, latents_fn, confidence=None) -> S2Output:
        """steps 3-4 of s2_step (internvla_n1_policy.py:177-197): decode text, pixel goal -> latents, else discrete actions.
        confidence: (answer_logprob, answer_min_margin) of this row when the model keeps token log-probabilities, else None."""
        self.llm_output = self.processor.tokenizer.decode(output_ids[0][inputs["input_ids"].shape[1]:], skip_special_tokens=True)
        out = S2Output()
        if confidence is not None:
            out.answer_logprob, out.answer_min_margin = confidence
        if re.search(r"\d", self.llm_output):
            coord = [int(c) for c in re.findall(r"\d+", self.llm_output)]
            out.output_pixel = np.array([int(coord[1]), int(coord[0])])   # a one-number answer raises IndexError like the reference (:187) -> the agent's retry path
            out.output_latent = latents_fn()      # the batched agent passes a marker here and fills the latents of all pixel-goal rows in one call
        else:
            out.output_action = self.parse_actions(self.llm_output)
            if not out.output_action:
                # neither a pixel goal nor a single action token: the reference's agent would index an empty list in its main thread
                # (internvla_n1_agent.py:282, an uncaught IndexError); here it is an S2 failure like any other -> retry once, then STOP
                raise ValueError(f"System-2 answer holds neither a pixel goal nor an action: {self.llm_output!r}")
        return out

    def s2_step(self, rgb, depth, pose, instruction, intrinsic, look_down: bool = False) -> S2Output:
        inputs = self.build_s2_inputs(rgb, instruction, look_down)
        extra = {"cached_image_embeds": inputs["cached_image_embeds"]} if "cached_image_embeds" in inputs else {}
        kv, want = self.prefix_request(inputs)
        if kv is not None or want:
            extra.update(prefix_kv=[kv], export_prefix=[want])
        past = None
        if self.kv_reuse:
            past, self._kv = self.kv_request(inputs), None    # dropped until this call succeeds (S2 failure / retry path)
            past = [past] if past is not None else None
        if self.repetition_penalty is not None:
            extra["repetition_penalty"] = float(self.repetition_penalty)
        if self.answer_constraint is not None:
            extra["constraint"] = self.answer_constraint
        want_lp =bool(getattr(getattr(self.model, "qwen", None), "token_logprobs", False))
        if want_lp:
            extra["output_logprobs"] = True
        res = self.model.generate(input_ids=inputs["input_ids"], pixel_values=inputs["pixel_values"], image_grid_thw=inputs["image_grid_thw"],
                                  max_new_tokens=128, do_sample=False, use_cache=True, past_key_values=past, return_dict_in_generate=True, **extra)
        ids = res.sequences
        conf = answer_confidences(res)[0] if want_lp else None
        if self.kv_reuse:
            self.store_kv(inputs, res.past_key_values)
        del res
        if "cached_image_embeds" in extra:
            self.update_frame_cache(inputs, self.model.last_image_embeds())
        if want:
            self.store_prefix(inputs, self.model.last_prefix_kv()[0])
        extra = {k: v for k, v in extra.items() if k == "cached_image_embeds"}
        try:
            return self.finish_s2(inputs, ids, lambda: self.model.generate_latents(ids, inputs["pixel_values"], inputs["image_grid_thw"], **extra),
                                  **({"confidence": conf} if want_lp else {}))
        except Exception:
            self._kv = None
            raise

    def s1_step_latent(self, rgb, depth, latent) -> S1Output:
        dp_actions = self.model.generate_traj(traj_latents=latent, images_dp=rgb, depths_dp=depth)
        return self.actions_from_traj(dp_actions)

    def actions_from_traj(self, dp_actions) -> S1Output:
        if self.continuous_traj:
            action_list = traj_to_actions(dp_actions)
        else:
            action_list = chunk_token(dp_actions[np.random.choice(dp_actions.shape[0])])
        return S1Output(idx=[x for x in action_list if x != 0][:4])

    def actions_from_traj_batch(self, dp_actions, n_env: int) -> List[S1Output]:
        """`actions_from_traj` of n_env envs at once, on the device: dp_actions is generate_traj's [S * n_env, T, 3] (f32 | bf16, on the GPU); ONE
        ina_traj_actions launch builds the [n_env, 4] int32 action table (kept as `last_action_table`, still on the device - what
        dist.all_gather_actions exchanges) and ONE device-to-host copy of it replaces the copy of the trajectories and the per-env numpy loop.
        Same S1Output per env as actions_from_traj; dp_actions is left as it is (the host function un-normalises its argument in place).
        continuous_traj only: the chunk_token branch draws a sample with numpy's global generator and stays on the host."""
        if not self.continuous_traj:
            raise NotImplementedError("actions_from_traj_batch covers continuous_traj=True only; the chunk_token branch runs on the host (actions_from_traj)")
        from . import ops

        self.last_action_table, _ = ops.traj_actions(dp_actions, n_env, 4)
        return [S1Output(idx=[x for x in row if x != 0]) for row in self.last_action_table.tolist()]
