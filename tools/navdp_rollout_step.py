"""Time a NavDPNet rollout-session step against the full call on one GPU, in one process: B envs, point goal, synthetic weights.

    python tools/navdp_rollout_step.py [--batch 64] [--steps 20] [--warmup 3] [--repeats 3] [--stride 1]

Both are timed eagerly with a device sync per step (wall clock around call + synchronize), `--repeats` times `--steps` steps each,
alternating; the line reports the median per repeat and their spread. The full call is fed a device-resident [B, M, 224, 224, 3] window, so
the upload the session saves the caller is NOT counted in its favour. Also: a captured session step (hipGraph replay), the gather launch
alone (event-timed), and the ring footprint. Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from internnav_amd import ops, runtime, synthetic  # noqa: E402
from internnav_amd.navdp import NavDPNet  # noqa: E402
from internnav_amd.navdp_rollout import NavDPRollout  # noqa: E402


def _median_ms(fn, steps):
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--stride", type=int, default=1)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device:", runtime.require_gfx950(), file=sys.stderr)
    cfg = synthetic.NAVDPNET_CFG
    B = a.batch
    net = NavDPNet(synthetic.navdpnet_state_dict(seed=0), cfg, dev, max_envs=B)
    inp = {k: v.to(dev) for k, v in synthetic.navdpnet_inputs(B, seed=0).items()}
    kinds = torch.ones(B, dtype=torch.int32)
    ses = NavDPRollout(net, B, stride=a.stride)
    frames = inp["images"][:, -1].contiguous()
    rest = dict(depth=inp["depths"], x_init=inp["x_init"], step_noise=inp["step_noise"])

    def full():
        return net.predict_mixedgoal_batch_action_vel(kinds, goal_point=inp["goal"], input_images=inp["images"], input_depths=inp["depths"],
                                                      x_init=inp["x_init"], step_noise=inp["step_noise"])

    def step():
        return ses.step(kinds, goal_point=inp["goal"], rgb=frames, **rest)

    for _ in range(a.warmup):
        full()
        step()
    full_ms, step_ms = [], []
    for _ in range(a.repeats):
        full_ms.append(_median_ms(full, a.steps))
        step_ms.append(_median_ms(step, a.steps))
    neg, pos = step()
    finite = bool(torch.isfinite(neg).all() and torch.isfinite(pos).all())
    graphed = ses.capture(kinds, goal_point=inp["goal"], rgb=frames, **rest)
    graph_ms = _median_ms(lambda: graphed(goal_point=inp["goal"], rgb=frames, **rest), a.steps)
    # the gather launch alone on the session's buffers
    M, nt = net.M, (net.M + 1) * 256
    E = ses.max_envs
    tab = ses.table

    def gather():
        ops.memory_gather(net.former.tokens[: B * nt].view(B, nt, 384), ses.ring, ses.fresh[:B], ses.blank, net.former.pe[: M * 256],
                          tab[2 * E:2 * E + B], tab[3 * E:3 * E + B], tab[4 * E:4 * E + B], stride=a.stride)
    for _ in range(3):
        gather()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(50):
        gather()
    e1.record()
    torch.cuda.synchronize()
    gather_us = e0.elapsed_time(e1) * 1e3 / 50
    moved = B * M * 256 * 384 * 10 + B * 256 * 384 * 4
    r = lambda v: [round(x, 2) for x in v]
    print(json.dumps(dict(workload="navdpnet_rollout_step", batch=B, stride=a.stride, steps=a.steps, warmup=a.warmup, repeats=a.repeats,
                          full_call_ms=r(full_ms), session_step_ms=r(step_ms), full_call_ms_median=round(statistics.median(full_ms), 2),
                          session_step_ms_median=round(statistics.median(step_ms), 2),
                          speedup_pct=round(100.0 * (statistics.median(full_ms) / statistics.median(step_ms) - 1.0), 1),
                          spread_pct=dict(full=round(100.0 * (max(full_ms) - min(full_ms)) / statistics.median(full_ms), 1),
                                          session=round(100.0 * (max(step_ms) - min(step_ms)) / statistics.median(step_ms), 1)),
                          session_graph_replay_ms=round(graph_ms, 2), gather_us=round(gather_us, 1),
                          gather_gbps=round(moved / gather_us / 1e3, 0), ring_mb=round(ses.ring_bytes / 1e6, 1), finite=finite)))


if __name__ == "__main__":
    main()
