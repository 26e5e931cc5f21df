"""One scripted System-2 episode through InternVLAN1Net under four reuse settings: rows prefilled, images encoded, ms per call.

Default geometry of the reference's harness: 384 x 384 history frames, a 640 x 480 camera (the look-down frame goes in un-resized),
num_history = 8, the 7B System-2 with synthetic weights drawn on the device. The script: `step_no_infer` frames between System-2 calls,
normal calls, and look-down turns that re-send the previous prompt. The text side is a character-level stand-in tokenizer (the HF
processor is host-side and not what is measured); every answer is the pixel goal "12 34", so each call also runs the latent queries.

    python tools/kv_reuse_episode.py [--settings none,prefix_cache,kv_reuse,kv_reuse+vit_cache] [--calls 10]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from internnav_amd import synthetic  # noqa: E402
from internnav_amd.policy import InternVLAN1ForCausalLM, InternVLAN1Net  # noqa: E402
from internnav_amd.preprocess import FramePreprocessor  # noqa: E402

SETTINGS = {"none": {}, "prefix_cache": {"prefix_cache": True}, "kv_reuse": {"kv_reuse": True},
            "kv_reuse+vit_cache": {"kv_reuse": True, "vit_cache": True}}


class _Tok:
    def __init__(self, cfg):
        self.special = {"<|image_pad|>": cfg["image_token_id"], "<|vision_start|>": cfg["vision_start_id"], "<|vision_end|>": cfg["vision_end_id"]}

    def __call__(self, texts, return_tensors="pt"):
        ids, i, t = [], 0, texts[0]
        while i < len(t):
            for k, v in self.special.items():
                if t.startswith(k, i):
                    ids.append(v)
                    i += len(k)
                    break
            else:
                ids.append(ord(t[i]) % 30000)
                i += 1
        return {"input_ids": torch.tensor([ids])}

    def decode(self, ids, skip_special_tokens=True):
        return "12 34"


class _Proc:
    image_token = "<|image_pad|>"

    def __init__(self, cfg):
        self.tokenizer = _Tok(cfg)

    def apply_chat_template(self, conv, tokenize=False, add_generation_prompt=True):
        return "".join("<|vision_start|><|image_pad|><|vision_end|>" if c["type"] == "image" else c["text"] for m in conv for c in m["content"])


def run(model, pre, proc, flags, frames, calls):
    net = InternVLAN1Net(model, proc, num_history=8, resize_w=384, resize_h=384, frame_preprocessor=pre, **flags)
    rows, imgs, ms, kinds = [], [], [], []
    for f in range(3):
        net.step_no_infer(frames[f], None, None)
    k = 3
    for c in range(calls):
        look_down = c % 2 == 1                                 # every other call is the look-down turn of the call before
        if not look_down:
            for _ in range(3):                                 # the episode moves on between System-2 plans
                net.step_no_infer(frames[k % len(frames)], None, None)
                k += 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        net.s2_step(frames[k % len(frames)], None, None, "walk past the sofa and stop at the kitchen door", None, look_down)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        st = model._gen["state"]
        rows.append(int(st["S_run"]) * int(st["B"]))
        imgs.append(len(st["plan"]["fresh_tokens"]))
        kinds.append("look_down" if look_down else "normal")
        k += 1
    return dict(rows=rows, images=imgs, ms=ms, kind=kinds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default=",".join(SETTINGS))
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    dev = "cuda:0"
    cfg = synthetic.QWEN_N1_CFG
    spec = synthetic.n1_full_spec(cfg, "nextdit_async")
    model = InternVLAN1ForCausalLM(synthetic.LazyDeviceWeights(spec, dev, seed=0), cfg, "nextdit_async", device=dev, max_envs=1)
    pre = FramePreprocessor(dev, resize_w=384, resize_h=384)
    proc = _Proc(cfg)
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(40)]
    run(model, pre, proc, {}, frames, 2)                       # warm-up: allocator, first launches
    out = {}
    print(f"{'setting':>20} | {'kind':>9} | {'rows/call':>9} | {'images/call':>11} | {'ms/call':>8}")
    for name in a.settings.split(","):
        r = run(model, pre, proc, SETTINGS[name], frames, a.calls)
        out[name] = r
        for kind in ("normal", "look_down"):
            sel = [i for i, k in enumerate(r["kind"]) if k == kind and i > 0]   # the episode's first call has nothing to reuse: left out
            if sel:
                print(f"{name:>20} | {kind:>9} | {np.mean([r['rows'][i] for i in sel]):9.0f} | {np.mean([r['images'][i] for i in sel]):11.1f} | "
                      f"{np.median([r['ms'][i] for i in sel]):8.1f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
