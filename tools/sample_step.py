"""Time the sampling kernel of System-2 decoding against the selections it replaces, and the KV fan-out of num_return_sequences, in one process
on one GPU.

    python tools/sample_step.py [--envs 7] [--prompt 920] [--iters 200] [--repeats 5] [--fan 4] [--fan-tokens 864] [--skip-fan]

1. ops.argmax_rows, ops.logprob_rows and ops.sample_rows at (T 0.7, top-k 50, top-p 0.9), (top-k 0, top-p 0.9) and (top-k 0, top-p 1), all with a
   seen set of --prompt tokens per row, penalty 1.05 and mark, at --envs rows of 152064 fp32 logits: `--iters` launches between two device
   events, the kernels alternating, `--repeats` times, median and all runs. Every launch of a loop reads ANOTHER of 32 copies of the logits
   (4.3 MB each), as in tools/logprob_step.py. The yardstick is logprob_rows in the same run; ratios are printed, not asserted.
2. The KV fan-out of --envs prompts x --fan returned sequences at --fan-tokens prompt tokens and the full depth of the 7B geometry
   (QwenVLEngine._fan_out: one export and one import launch of ina_kv_copy through temporary tensors).
Prints a table and one JSON line."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from internnav_amd import ops, runtime, synthetic  # noqa: E402
from internnav_amd.qwen_vl import QwenVLEngine  # noqa: E402

VOCAB = 152064
SETTINGS = (("sample_50_0.9", 0.7, 50, 0.9), ("sample_0_0.9", 0.7, 0, 0.9), ("sample_0_1", 0.7, 0, 1.0))


def _events_us(fns, iters):
    """us per launch of a loop that calls fns[i % len(fns)]"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(iters):
        fns[i % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def kernel_rows(M, S, iters, repeats, dev):
    g = torch.Generator(device=dev).manual_seed(M)
    copies = 32
    xs = [torch.randn(M, VOCAB, generator=g, device=dev) * 4 for _ in range(copies)]
    ids = torch.randint(0, VOCAB, (M, S), generator=g, device=dev, dtype=torch.int32)
    lens = torch.full((M,), S, dtype=torch.int32, device=dev)
    ldw = ((VOCAB + 31) // 32 + 3) // 4 * 4
    seen0 = torch.zeros(M, ldw, dtype=torch.uint32, device=dev)
    ops.token_seen_set(seen0, ids, lens, VOCAB)
    u = torch.rand(M, generator=g, device=dev)
    tok, nk = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
    lp, mg = torch.empty(M, dtype=torch.float32, device=dev), torch.empty(M, dtype=torch.float32, device=dev)
    loops = {"argmax_rows": [lambda x=x: ops.argmax_rows(x, tok) for x in xs]}
    s_lp = seen0.clone()
    loops["logprob_rows"] = [lambda x=x: ops.logprob_rows(x, tok, lp, mg, seen=s_lp, penalty=1.05, mark=True) for x in xs]
    kept = {}
    for name, T, k, p in SETTINGS:
        s_ = seen0.clone()
        loops[name] = [lambda x=x, s_=s_, T=T, k=k, p=p: ops.sample_rows(x, u, tok, lp, temperature=T, top_k=k, top_p=p, seen=s_, penalty=1.05, mark=True)
                       for x in xs]
        ops.sample_rows(xs[0], u, tok, lp, temperature=T, top_k=k, top_p=p, seen=seen0.clone(), penalty=1.05, mark=True, n_kept=nk)
        kept[name] = nk.tolist()
    for fns in loops.values():
        _events_us(fns, len(fns))
    runs = {name: [] for name in loops}
    for _ in range(repeats):
        for name, fns in loops.items():
            runs[name].append(_events_us(fns, iters))
    med = {name: statistics.median(v) for name, v in runs.items()}
    out = dict(rows=M, n=VOCAB, seen_per_row=S, logits_copies=copies, n_kept_first_copy=kept)
    for name in loops:
        out[name] = dict(us=round(med[name], 2), vs_logprob_rows=round(med[name] / med["logprob_rows"], 3), runs=[round(v, 2) for v in runs[name]])
    return out


def fan_rows(envs, K, S, repeats, dev):
    cfg = synthetic.QWEN_N1_CFG
    eng = QwenVLEngine(synthetic.LazyDeviceWeights(synthetic.qwen_spec(cfg), dev, seed=0), cfg, dev, max_seqs=envs * K, max_seq_len=(S + 63) // 64 * 64,
                       max_patches=64)
    ts = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(repeats + 1):
        st = dict(B=envs, S=S, next_pos=np.full(envs, S, dtype=np.int64))
        torch.cuda.synchronize()
        e0.record()
        eng._fan_out(st, K)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts = ts[1:]                                         # the first run warms the allocator
    gb = 2 * (S * len(eng.layers) * eng.kv_w * 2) * envs * (1 + K) / 1e9      # export: read + write B prompts; import: read + write B * K
    return dict(prompts=envs, K=K, prompt_tokens=S, layers=len(eng.layers), ms=round(statistics.median(ts), 3), runs=[round(v, 3) for v in ts],
                bytes_moved_gb=round(gb, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=7)
    ap.add_argument("--prompt", type=int, default=920)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fan", type=int, default=4)
    ap.add_argument("--fan-tokens", type=int, default=864)
    ap.add_argument("--skip-fan", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device:", runtime.require_gfx950(), file=sys.stderr)
    r = kernel_rows(a.envs, a.prompt, a.iters, a.repeats, dev)
    print(f"selection kernels, {r['rows']} rows x {r['n']} logits, {r['seen_per_row']} seen ids per row ({a.iters} launches x {a.repeats}, median)")
    for name in ("argmax_rows", "logprob_rows") + tuple(s[0] for s in SETTINGS):
        p = r[name]
        print(f"  {name:16s} {p['us']:9.2f} us   {p['vs_logprob_rows']:7.3f} x logprob_rows   runs {p['runs']}")
    print(f"  kept entries per row (first copy): {r['n_kept_first_copy']}")
    out = dict(workload="sample_step", envs=a.envs, iters=a.iters, repeats=a.repeats, kernel=r)
    if not a.skip_fan:
        f = out["fan_out"] = fan_rows(a.envs, a.fan, a.fan_tokens, a.repeats, dev)
        print(f"KV fan-out, {f['prompts']} prompts x {f['K']} at {f['prompt_tokens']} tokens, {f['layers']} layers: {f['ms']} ms   runs {f['runs']}   "
              f"({f['bytes_moved_gb']} GB read + written)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
