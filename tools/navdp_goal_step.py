"""Time NavDPNet inference calls per goal kind on one GPU: B = 64 envs per call, point goal, image goal, pixel goal and a mixed batch
(the four kinds, 16 envs each, interleaved), synthetic weights with both goal towers.

    python tools/navdp_goal_step.py [--batch 64] [--steps 10] [--warmup 3] [--pixel-channel 4]

Prints one JSON line: ms per call of each kind, each kind's overhead over the point-goal call, the library launches of each call
(counted over one extra call with the library's profiler on) and the time of the goal-slot kernel (ina_goal_slots) of the mixed call."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from internnav_amd import runtime, synthetic  # noqa: E402
from internnav_amd.navdp import NavDPNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pixel-channel", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device:", runtime.require_gfx950(), file=sys.stderr)
    cfg = synthetic.NAVDPNET_CFG
    B, pc = a.batch, a.pixel_channel
    net = NavDPNet(synthetic.navdpnet_train_state_dict(seed=0, pixel_channel=pc), cfg, dev, max_envs=B)
    inp = {k: v.to(dev) for k, v in synthetic.navdpnet_inputs(B, seed=0).items()}
    goals = {k: v.to(dev) for k, v in synthetic.navdpnet_goal_inputs(B, seed=0, pixel_channel=pc).items()}
    rest = (inp["images"], inp["depths"], inp["x_init"], inp["step_noise"])
    kinds = torch.arange(B, dtype=torch.int32) % 4
    img, pix = (kinds == 2).nonzero().flatten().to(dev), (kinds == 3).nonzero().flatten().to(dev)
    mixed_img, mixed_pix = goals["goal_image"][img].contiguous(), goals["goal_pixel"][pix].contiguous()
    calls = {
        "point": lambda: net.predict_pointgoal_batch_action_vel(inp["goal"], *rest),
        "image": lambda: net.predict_imagegoal_batch_action_vel(goals["goal_image"], *rest),
        "pixel": lambda: net.predict_pixelgoal_batch_action_vel(goals["goal_pixel"], *rest),
        "mixed": lambda: net.predict_mixedgoal_batch_action_vel(kinds, goal_point=inp["goal"], goal_image=mixed_img, goal_pixel=mixed_pix,
                                                                input_images=inp["images"], input_depths=inp["depths"], x_init=inp["x_init"],
                                                                step_noise=inp["step_noise"]),
    }
    ms, launches, finite = {}, {}, True
    for name, call in calls.items():
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            neg, pos = call()
        torch.cuda.synchronize()
        ms[name] = round((time.perf_counter() - t0) * 1e3 / a.steps, 2)
        finite = finite and bool(torch.isfinite(neg).all() and torch.isfinite(pos).all())
        runtime.prof_enable(True)
        call()
        torch.cuda.synchronize()
        launches[name] = sum(v["launches"] for v in runtime.prof_read().values())
        runtime.prof_enable(False)
    # the goal-slot kernel alone, on the mixed call's inputs (the towers' tokens are in place after the last mixed call)
    from internnav_amd import ops
    from internnav_amd.navdp import goal_plan

    plan = goal_plan(kinds, inp["goal"], mixed_img, mixed_pix, pixel_channel=pc)
    plan_dev = torch.cat([plan.kind, plan.row]).to(dev)
    tok = net.goal_tok
    n_i, n_x = plan.n_image, plan.n_pixel
    ti, tp = net.goal_towers["image"], net.goal_towers["pixel"]

    def slots():
        ops.goal_slots(net.cond[: B * net.Lc], net.Lc, plan_dev[:B], plan_dev[B:], pos=net.cond_pos, embed=net.goal_embed[:B],
                       point=(inp["goal"], net.pt_w, net.pt_b), image=(tok[: n_i * 256], ti.proj_w, ti.proj_b, 256),
                       pixel=(tok[n_i * 256:(n_i + n_x) * 256], tp.proj_w, tp.proj_b, 256))
    for _ in range(3):
        slots()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        slots()
    e1.record()
    torch.cuda.synchronize()
    slot_us = e0.elapsed_time(e1) * 1e3 / 50
    print(json.dumps(dict(workload="navdpnet_goal_calls", batch=B, pixel_channel=pc, steps=a.steps, warmup=a.warmup, ms_per_call=ms,
                          overhead_vs_point_pct={k: round(100.0 * (v / ms["point"] - 1.0), 1) for k, v in ms.items() if k != "point"},
                          launches_per_call=launches, goal_slots_us=round(slot_us, 1), finite=finite)))


if __name__ == "__main__":
    main()
