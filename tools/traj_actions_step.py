"""Time the end of a policy step - sampled trajectories -> the step's [B, 4] action table - on the host and on the device, in one process.

    python tools/traj_actions_step.py [--batch 64] [--steps 20] [--repeats 3] [--warmup 3]

Input: B envs x [32, 32, 3] seeded trajectories on the GPU (strong / backward / curved / static / slow / tiny drifts in turn), as generate_traj leaves them.
  host path    device-to-host copy of the trajectories, then B x policy.traj_to_actions and the cut to four actions (agent._run_s1 today)
  device path  one ina_traj_actions launch, then the device-to-host copy of the int32 [B, 4] table (model_settings['device_actions'])
Both are wall clock around work that ends on the host with the table in hand; `--repeats` times the median of `--steps` runs, alternating.
The launch alone is timed with device events over 50 back-to-back launches. The two tables must be equal. Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from internnav_amd import ops, runtime  # noqa: E402
from internnav_amd.policy import traj_to_actions  # noqa: E402

S, T = 32, 32


def seeded_trajectories(B: int, seed: int = 0) -> torch.Tensor:
    """f32 [B, 32, 32, 3] x4-scaled increments: mean paths of 0.02 - 3 m, straight, backward or curved, 20 % per-sample noise."""
    rng = np.random.default_rng(seed)
    out = np.empty((B, S, T, 3), np.float32)
    for b in range(B):
        total = (3.0, 2.0, 3.0, 0.02, 0.5, 0.1)[b % 6] * rng.uniform(0.7, 1.3)
        head = math.pi + rng.uniform(-0.4, 0.4) if b % 6 == 1 else rng.uniform(-math.pi, math.pi)
        ang = head + (rng.uniform(-2.5, 2.5) if b % 6 == 2 else 0.0) * np.arange(T) / (T - 1)
        xy = (total / T) * np.stack([np.cos(ang), np.sin(ang)], -1)[None] + rng.normal(0.0, 0.2 * total / T, (S, T, 2))
        out[b, :, :, :2] = 4.0 * xy
        out[b, :, :, 2] = rng.normal(0.0, 0.1, (S, T))
    return torch.from_numpy(out)


def _median_ms(fn, steps):
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    print("device:", runtime.require_gfx950(), file=sys.stderr)
    B = a.batch
    traj = seeded_trajectories(B).reshape(B * S, T, 3).to("cuda:0")       # generate_traj's layout

    def host():
        t = traj.cpu()                                                     # a fresh copy each time: traj_to_actions un-normalises in place
        return [[x for x in traj_to_actions(t[k * S:(k + 1) * S]) if x != 0][:4] for k in range(B)]

    def device():
        return ops.traj_actions(traj, B, 4)[0].cpu()

    for _ in range(a.warmup):
        want, got = host(), device()
    table = [row + [0] * (4 - len(row)) for row in want]
    assert got.tolist() == table, "device table differs from the host path"
    host_ms, dev_ms = [], []
    for _ in range(a.repeats):
        host_ms.append(_median_ms(host, a.steps))
        dev_ms.append(_median_ms(device, a.steps))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kern = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(50):
            ops.traj_actions(traj, B, 4)
        e1.record()
        torch.cuda.synchronize()
        kern.append(e0.elapsed_time(e1) * 1e3 / 50)
    med = statistics.median
    spread = lambda v: round(100.0 * (max(v) - min(v)) / med(v), 1)
    print(json.dumps(dict(workload="traj_actions_step", batch=B, samples=S, horizon=T, steps=a.steps, repeats=a.repeats, warmup=a.warmup,
                          host_path_ms=[round(x, 3) for x in host_ms], device_path_ms=[round(x, 3) for x in dev_ms],
                          host_path_ms_median=round(med(host_ms), 3), device_path_ms_median=round(med(dev_ms), 3),
                          launch_us=[round(x, 1) for x in kern], launch_us_median=round(med(kern), 1),
                          spread_pct=dict(host=spread(host_ms), device=spread(dev_ms), launch=spread(kern)),
                          d2h_bytes=dict(host=B * S * T * 3 * 4, device=B * 4 * 4), tables_equal=True,
                          nonzero_actions=int(sum(len(r) for r in want)))))


if __name__ == "__main__":
    main()
