"""Time the System-2 single-token passes on FP8 weights (QwenVLEngine w8_decode) against the bf16 weight stream, in one process on one GPU.

    python tools/w8_decode_step.py [--envs 7] [--iters 40] [--repeats 5] [--graph-steps 10] [--skip-graph] [--skip-drift]

1. Per shape at M = --envs rows, in the form the decoder runs it (q|k|v and gate|up with the fused input RMSNorm, o and down with the fp32
   residual, lm_head to fp32): `--iters` launches between two device events, bf16 (ops.linear on the dequantised weights) and fp8
   (ops.linear_w8) alternating, `--repeats` times, median. Every launch of a loop reads ANOTHER copy of the weight, enough copies to exceed
   the 256 MB last-level cache, so the figures are HBM streams. us per launch and TB/s over the algorithmic bytes (2 N K resp. N K + N weight
   bytes + activations + output). Both results are compared bit for bit.
2. The decode + latent-query launch sequence of --envs prompts (4 frames of 28 x 28 patches, 64 instruction tokens, 8 answer tokens) at the full
   depth of the 7B geometry, captured once with the fp8 copies off and once on (ONE engine, the same dequantised model), replayed alternately;
   tokens and latents of the two graphs are compared bit for bit.
3. Drift of the quantised model from the unquantised engine on the QWEN_TEST_CFG prompt: last-position logits and greedy tokens.
Prints a table and one JSON line."""
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
from internnav_amd.qwen_vl import QwenVLEngine  # noqa: E402

H, TI, QKV, VOCAB = 3584, 18944, 4608, 152064
CACHE_BYTES = 768 << 20        # the copies of a weight that a timing loop rotates through hold at least this much (3 x the 256 MB cache)
BF16, F32 = torch.bfloat16, torch.float32


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


def shape_row(name, M, N, K, form, iters, repeats, dev):
    g = torch.Generator(device=dev).manual_seed(N + K)
    w = (torch.randn(N, K, generator=g, device=dev) * K ** -0.5).to(BF16)
    w8, wexp, wd = ops.w8_quantize(w)
    del w
    n16, n8 = max(2, -(-CACHE_BYTES // (2 * N * K))), max(2, -(-CACHE_BYTES // (N * K)))
    wds, w8s = [wd] + [wd.clone() for _ in range(n16 - 1)], [w8] + [w8.clone() for _ in range(n8 - 1)]
    gamma = torch.rand(K, generator=g, device=dev) + 0.5
    x32 = torch.randn(M, K, generator=g, device=dev)
    n_out = N // 2 if form == "gu" else N
    res = torch.randn(M, n_out, generator=g, device=dev)
    if form == "qkv":
        kw = dict(bias=torch.randn(N, generator=g, device=dev), prenorm=(gamma, 1e-6))
        x, odt = x32, BF16
    elif form == "gu":
        kw = dict(act="silu", glu=True, prenorm=(gamma, 1e-6))
        x, odt = x32, BF16
    elif form == "res":
        kw = dict(residual=res)
        x, odt = x32.to(BF16), F32
    else:
        kw = {}
        x, odt = x32.to(BF16), F32
    o16, o8 = torch.empty(M, n_out, dtype=odt, device=dev), torch.empty(M, n_out, dtype=odt, device=dev)
    f16 = [lambda t=t: ops.linear(x, t, out=o16, **kw) for t in wds]
    f8 = [lambda t=t: ops.linear_w8(x, t, wexp, out=o8, **kw) for t in w8s]
    f16[0]()
    f8[0]()
    torch.cuda.synchronize()
    equal = bool(torch.equal(o16, o8))
    _events_us(f16, len(f16))
    _events_us(f8, len(f8))
    t16, t8 = [], []
    for _ in range(repeats):
        t16.append(_events_us(f16, iters))
        t8.append(_events_us(f8, iters))
    a, b = statistics.median(t16), statistics.median(t8)
    act = M * K * (4 if "prenorm" in kw else 2) + M * n_out * (2 if odt == BF16 else 4) * (2 if "residual" in kw else 1)
    by16, by8 = 2 * N * K + act, N * K + N + act
    return dict(shape=name, M=M, N=N, K=K, bf16_us=round(a, 1), w8_us=round(b, 1), bf16_tbps=round(by16 / a / 1e6, 2), w8_tbps=round(by8 / b / 1e6, 2),
                speedup=round(a / b, 3), spread_pct=dict(bf16=round(100 * (max(t16) - min(t16)) / a, 1), w8=round(100 * (max(t8) - min(t8)) / b, 1)),
                bit_equal=equal, copies=dict(bf16=n16, w8=n8))


def graph_rows(envs, steps, repeats, dev):
    cfg = synthetic.QWEN_N1_CFG
    n_img, n_text, n_dec = 4, 64, 8
    inp = synthetic.qwen_inputs(envs, n_img, seed=0, cfg=cfg, n_text=n_text, n_tail=8)
    ids, grid = inp["input_ids"], inp["grid_thw"]
    pv = inp["pixel_values"].to(dev, BF16)
    S = ids.shape[1]
    eng = QwenVLEngine(synthetic.LazyDeviceWeights(synthetic.qwen_spec(cfg), dev, seed=0), cfg, dev, max_seqs=envs,
                       max_seq_len=(S + n_dec + 8 + 63) // 64 * 64, max_patches=pv.shape[0], w8_decode=True)
    P = eng.plan(ids, grid, n_decode=n_dec, with_latents=True)
    eng.run_prefill(P, pv)
    torch.cuda.synchronize()
    out, graphs = {}, {}
    for name, on in (("bf16", False), ("w8", True)):
        eng.w8_decode = on                 # the fp8 copies stay; the bf16 tensors hold the dequantised weights either way: one model
        toks = torch.zeros(envs, n_dec, dtype=torch.int32, device=dev)
        lat = torch.zeros(envs, cfg["n_query"], cfg["t_hidden"], dtype=BF16, device=dev)

        def seq(toks=toks, lat=lat):
            eng.run_decode(P, toks)
            eng.run_latents(P, lat)
        graphs[name] = runtime.GraphedCall(seq, {})
        out[name] = (toks, lat)
    eng.w8_decode = True

    def ms(g):
        ts = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)
    for g in graphs.values():
        g()
    t = {"bf16": [], "w8": []}
    for _ in range(repeats):
        for name in ("bf16", "w8"):
            t[name].append(ms(graphs[name]))
    torch.cuda.synchronize()
    a, b = statistics.median(t["bf16"]), statistics.median(t["w8"])
    equal = bool(torch.equal(out["bf16"][0], out["w8"][0]) and torch.equal(out["bf16"][1], out["w8"][1]))
    w_bytes = sum(L[k].numel() for L in eng.layers for k in eng.W8_LAYER_WEIGHTS) + eng.lm_head.numel()
    e_bytes = sum(L[k].shape[0] for L in eng.layers for k in eng.W8_LAYER_WEIGHTS) + eng.lm_head.shape[0]
    return dict(envs=envs, prompt_tokens=S, passes=f"{n_dec - 1} decode + {n_dec} lm_head + 1 latent-query pass of {envs * (1 + cfg['n_query'])} rows",
                bf16_ms=round(a, 3), w8_ms=round(b, 3), speedup=round(a / b, 3), bf16_runs=[round(v, 3) for v in t["bf16"]], w8_runs=[round(v, 3) for v in t["w8"]],
                bit_equal=equal, w8_extra_gb=round((w_bytes + e_bytes) / 1e9, 2), tokens=out["w8"][0][0].tolist())


def drift(dev):
    cfg = synthetic.QWEN_TEST_CFG
    sd = {k: v.to(dev) for k, v in synthetic.qwen_state_dict(seed=12, cfg=cfg).items()}
    inp = synthetic.qwen_inputs(3, 1, seed=12, cfg=cfg)
    pv = inp["pixel_values"].to(dev, BF16)
    res = {}
    for name, on in (("bf16", False), ("w8", True)):
        eng = QwenVLEngine(sd, cfg, dev, max_seqs=3, max_seq_len=512, max_patches=pv.shape[0], w8_decode=on)
        st = eng.prefill(inp["input_ids"], pv, inp["grid_thw"])
        eng._last_logits(3, st["S_run"], st["S_run"] - 1)
        logits = eng.logits[:3].float().clone()
        res[name] = (logits, eng.decode(st, 8).cpu())
    err = (res["w8"][0] - res["bf16"][0]).abs()
    return dict(prompt="QWEN_TEST_CFG, 3 prompts, seed 12", logits_mean_abs_err=float(err.mean()), logits_max_abs_err=float(err.max()),
                logits_max_abs=float(res["bf16"][0].abs().max()), tokens_bf16=res["bf16"][1].tolist(), tokens_w8=res["w8"][1].tolist(),
                tokens_equal=bool(torch.equal(res["bf16"][1], res["w8"][1])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graph-steps", type=int, default=10)
    ap.add_argument("--skip-graph", action="store_true")
    ap.add_argument("--skip-drift", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device:", runtime.require_gfx950(), file=sys.stderr)
    M = a.envs
    rows = [shape_row(*s, a.iters, a.repeats, dev) for s in (("q|k|v", M, QKV, H, "qkv"), ("o", M, H, H, "res"), ("gate|up", M, 2 * TI, H, "gu"),
                                                             ("down", M, H, TI, "res"), ("lm_head", M, VOCAB, H, "plain"))]
    print(f"{'shape':8s} {'N':>7s} {'K':>6s} {'bf16 us':>9s} {'TB/s':>6s} {'w8 us':>9s} {'TB/s':>6s} {'bf16/w8':>8s}  bits")
    for r in rows:
        print(f"{r['shape']:8s} {r['N']:7d} {r['K']:6d} {r['bf16_us']:9.1f} {r['bf16_tbps']:6.2f} {r['w8_us']:9.1f} {r['w8_tbps']:6.2f} {r['speedup']:8.3f}  "
              f"{'equal' if r['bit_equal'] else 'DIFFER'}   spread % {r['spread_pct']}")
    out = dict(workload="w8_decode_step", envs=M, iters=a.iters, repeats=a.repeats, shapes=rows)
    if not a.skip_graph:
        out["graph"] = graph_rows(M, a.graph_steps, a.repeats, dev)
        gr = out["graph"]
        print(f"decode + latents graph, {M} envs, full depth: bf16 {gr['bf16_ms']} ms  w8 {gr['w8_ms']} ms  bf16/w8 {gr['speedup']}  "
              f"bits {'equal' if gr['bit_equal'] else 'DIFFER'}  (+{gr['w8_extra_gb']} GB)")
    if not a.skip_drift:
        out["drift"] = drift(dev)
        d = out["drift"]
        print(f"drift vs the unquantised engine ({d['prompt']}): logits mean|err| {d['logits_mean_abs_err']:.4e} max|err| {d['logits_max_abs_err']:.4e} "
              f"(max|logit| {d['logits_max_abs']:.3f}); tokens equal {d['tokens_equal']}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
