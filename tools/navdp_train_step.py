"""Time the NavDPNet training step (internnav_amd/navdp_train.py) on one GPU: B = 32 synthetic navdp_collate_fn micro-batches, one
forward_backward + optimizer_step per step, dropout 0.1 as the reference trains.

    python tools/navdp_train_step.py [--batch 32] [--steps 10] [--warmup 3] [--pixel-channel 4]

Prints one JSON line: samples/s, ms per step, the box's calibration (bench.py's 8192^3 bf16 GEMM TF/s), library launches per step (every kernel of libinternnav_amd.so, counted over one extra
step with the library's profiler on; the torch copies / allocations of the tape are not in it) and the step's algorithmic TFLOP
(internnav_amd.flops.navdpnet_train_flops)."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from internnav_amd import flops, runtime, synthetic  # noqa: E402
from internnav_amd.navdp_train import NavDPNetTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pixel-channel", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device:", runtime.require_gfx950(), file=sys.stderr)
    cfg = synthetic.NAVDPNET_CFG
    B, pc = a.batch, a.pixel_channel
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
    from navdp_train_ref import synthetic_batch

    batch = {k: v.to(dev) for k, v in synthetic_batch(B, 0, pc, cfg).items()}
    tr = NavDPNetTrainer(synthetic.navdpnet_train_state_dict(seed=0, pixel_channel=pc), dev, cfg, total_steps=a.warmup + a.steps + 1,
                         dropout=0.1)

    def step():
        terms = tr.forward_backward(batch)
        norm = tr.optimizer_step()
        return terms["loss"], norm

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss, norm = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    runtime.prof_enable(True)
    step()
    torch.cuda.synchronize()
    counts = runtime.prof_read()
    runtime.prof_enable(False)
    launches = sum(v["launches"] for v in counts.values())
    from bench import calibration_gemm

    calib = calibration_gemm(dev)
    fl = flops.navdpnet_train_flops(cfg, B, pc)
    print(json.dumps(dict(workload="navdpnet_train_step", batch=B, pixel_channel=pc, steps=a.steps, warmup=a.warmup, ms_per_step=round(ms, 2),
                          samples_per_s=round(B * 1e3 / ms, 2), launches_per_step=launches, tflop_per_step=round(fl["total"] / 1e12, 3),
                          tflops=round(fl["total"] / 1e12 / (ms / 1e3), 1), calibration=calib, loss=round(loss.item(), 5), grad_norm=round(norm.item(), 5),
                          launches_by_kind={k: v["launches"] for k, v in counts.items() if v["launches"]})))


if __name__ == "__main__":
    main()
