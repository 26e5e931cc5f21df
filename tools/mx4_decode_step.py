"""Time the System-2 single-token passes on MXFP4 weights (QwenVLEngine mx4_decode) against the bf16 and the fp8 weight streams, in one process
on one GPU.

    python tools/mx4_decode_step.py [--envs 7] [--iters 40] [--repeats 5] [--graph-steps 10] [--skip-graph] [--skip-drift] [--out FILE]

1. Per shape at M = --envs rows, in the form the decoder runs it (q|k|v and gate|up with the fused input RMSNorm, o and down with the fp32
   residual, lm_head to fp32; lm_head stays fp8 in the engine and is listed for reference): `--iters` launches between two device events,
   bf16 (ops.linear on the MXFP4-dequantised weights), fp8 (ops.linear_w8 on e4m3 copies of the same tensors: a yardstick for time, another
   rounding) and MXFP4 (ops.linear_mx4) alternating, `--repeats` times, median and spread. Every launch of a loop reads ANOTHER copy of the
   weight, enough copies to exceed the 256 MB last-level cache, so the figures are HBM streams. us per launch and TB/s over the algorithmic
   bytes (2 N K, N K + N, N K / 2 + N K / 32 weight bytes + activations + output). The bf16 and MXFP4 results are compared bit for bit.
2. The decode + latent-query launch sequence of --envs prompts (4 frames of 28 x 28 patches, 64 instruction tokens, 8 answer tokens) at the full
   depth of the 7B geometry, captured three times on ONE engine built with mx4_decode=True: with the quantised copies off (bf16 stream of the
   dequantised model), with e4m3 copies of those tensors (time only) and with the MXFP4 copies; replayed alternately. Tokens and latents of the
   bf16 and MXFP4 graphs are compared bit for bit.
3. Drift of the quantised model from the unquantised engine on QWEN_TEST_CFG: last-position logits, greedy tokens, and the largest shift of
   a score_answers(share_prefix=True) token log-probability (one prompt, the unquantised model's greedy answer and two fixed candidates).
Prints a table and one JSON line; --out also writes them to a file."""
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
KINDS = ("bf16", "w8", "mx4")


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
    w4, wscale, wd = ops.mx4_quantize(w)
    del w
    w8, wexp, _ = ops.w8_quantize(wd)
    wbytes = dict(bf16=2 * N * K, w8=N * K + N, mx4=N * K // 2 + N * K // 32)
    ncopy = {k: max(2, -(-CACHE_BYTES // v)) for k, v in wbytes.items()}
    wds = [wd] + [wd.clone() for _ in range(ncopy["bf16"] - 1)]
    w8s = [w8] + [w8.clone() for _ in range(ncopy["w8"] - 1)]
    w4s = [(w4, wscale)] + [(w4.clone(), wscale.clone()) for _ in range(ncopy["mx4"] - 1)]
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
    o = {k: torch.empty(M, n_out, dtype=odt, device=dev) for k in KINDS}
    fns = dict(bf16=[lambda t=t: ops.linear(x, t, out=o["bf16"], **kw) for t in wds],
               w8=[lambda t=t: ops.linear_w8(x, t, wexp, out=o["w8"], **kw) for t in w8s],
               mx4=[lambda t=t: ops.linear_mx4(x, t[0], t[1], out=o["mx4"], **kw) for t in w4s])
    for k in KINDS:
        fns[k][0]()
    torch.cuda.synchronize()
    equal = bool(torch.equal(o["bf16"], o["mx4"]))
    for k in KINDS:
        _events_us(fns[k], len(fns[k]))
    t = {k: [] for k in KINDS}
    for _ in range(repeats):
        for k in KINDS:
            t[k].append(_events_us(fns[k], iters))
    med = {k: statistics.median(v) for k, v in t.items()}
    act = M * K * (4 if "prenorm" in kw else 2) + M * n_out * (2 if odt == BF16 else 4) * (2 if "residual" in kw else 1)
    row = dict(shape=name, M=M, N=N, K=K, bit_equal=equal, copies=ncopy)
    for k in KINDS:
        row[k + "_us"] = round(med[k], 1)
        row[k + "_tbps"] = round((wbytes[k] + act) / med[k] / 1e6, 2)
    row["spread_pct"] = {k: round(100 * (max(t[k]) - min(t[k])) / med[k], 1) for k in KINDS}
    row["w8_over_mx4"] = round(med["w8"] / med["mx4"], 3)
    row["bf16_over_mx4"] = round(med["bf16"] / med["mx4"], 3)
    return row


def graph_rows(envs, steps, repeats, dev):
    cfg = synthetic.QWEN_N1_CFG
    n_img, n_text, n_dec = 4, 64, 8
    inp = synthetic.qwen_inputs(envs, n_img, seed=0, cfg=cfg, n_text=n_text, n_tail=8)
    ids, grid = inp["input_ids"], inp["grid_thw"]
    pv = inp["pixel_values"].to(dev, BF16)
    S = ids.shape[1]
    eng = QwenVLEngine(synthetic.LazyDeviceWeights(synthetic.qwen_spec(cfg), dev, seed=0), cfg, dev, max_seqs=envs,
                       max_seq_len=(S + n_dec + 8 + 63) // 64 * 64, max_patches=pv.shape[0], mx4_decode=True)
    # the fp8 yardstick: e4m3 copies of the SAME (MXFP4-dequantised) tensors, kept beside them without touching them - time only
    for L in eng.layers:
        for k in eng.W8_LAYER_WEIGHTS:
            w8, e, _ = ops.w8_quantize(L[k])
            L[k + "8"] = (w8, e)
    P = eng.plan(ids, grid, n_decode=n_dec, with_latents=True)
    eng.run_prefill(P, pv)
    torch.cuda.synchronize()
    out, graphs = {}, {}
    for name in KINDS:
        eng.mx4_decode, eng.w8_decode = name == "mx4", name == "w8"
        if name == "bf16":
            keep, eng.lm_head8 = eng.lm_head8, None
        toks = torch.zeros(envs, n_dec, dtype=torch.int32, device=dev)
        lat = torch.zeros(envs, cfg["n_query"], cfg["t_hidden"], dtype=BF16, device=dev)

        def seq(toks=toks, lat=lat):
            eng.run_decode(P, toks)
            eng.run_latents(P, lat)
        graphs[name] = runtime.GraphedCall(seq, {})
        out[name] = (toks, lat)
        if name == "bf16":
            eng.lm_head8 = keep
    eng.mx4_decode, eng.w8_decode = True, False

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
    t = {k: [] for k in KINDS}
    for _ in range(repeats):
        for name in KINDS:
            t[name].append(ms(graphs[name]))
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in t.items()}
    equal = bool(torch.equal(out["bf16"][0], out["mx4"][0]) and torch.equal(out["bf16"][1], out["mx4"][1]))
    extra = sum(L[k + "4"][0].numel() + L[k + "4"][1].numel() for L in eng.layers for k in eng.W8_LAYER_WEIGHTS)
    extra8 = eng.lm_head8[0].numel() + eng.lm_head8[1].numel()
    r = dict(envs=envs, prompt_tokens=S, passes=f"{n_dec - 1} decode + {n_dec} lm_head + 1 latent-query pass of {envs * (1 + cfg['n_query'])} rows",
             bit_equal=equal, mx4_extra_gb=round(extra / 1e9, 2), lm_head8_extra_gb=round(extra8 / 1e9, 2), tokens=out["mx4"][0][0].tolist())
    for k in KINDS:
        r[k + "_ms"] = round(med[k], 3)
        r[k + "_runs"] = [round(v, 3) for v in t[k]]
    r["bf16_over_mx4"], r["w8_over_mx4"] = round(med["bf16"] / med["mx4"], 3), round(med["w8"] / med["mx4"], 3)
    return r


def drift(dev):
    cfg = synthetic.QWEN_TEST_CFG
    sd = {k: v.to(dev) for k, v in synthetic.qwen_state_dict(seed=12, cfg=cfg).items()}
    inp = synthetic.qwen_inputs(3, 1, seed=12, cfg=cfg)
    pv = inp["pixel_values"].to(dev, BF16)
    res = {}
    for name, on in (("bf16", False), ("mx4", True)):
        eng = QwenVLEngine(sd, cfg, dev, max_seqs=3, max_seq_len=512, max_patches=pv.shape[0], mx4_decode=on)
        st = eng.prefill(inp["input_ids"], pv, inp["grid_thw"])
        eng._last_logits(3, st["S_run"], st["S_run"] - 1)
        logits = eng.logits[:3].float().clone()
        res[name] = (logits, eng.decode(st, 8).cpu())
        del eng
    err = (res["mx4"][0] - res["bf16"][0]).abs()
    flipped = int((res["mx4"][1] != res["bf16"][1]).sum())
    out = dict(prompt="QWEN_TEST_CFG, 3 prompts, seed 12", logits_mean_abs_err=float(err.mean()), logits_max_abs_err=float(err.max()),
               logits_max_abs=float(res["bf16"][0].abs().max()), tokens_bf16=res["bf16"][1].tolist(), tokens_mx4=res["mx4"][1].tolist(),
               tokens_flipped=flipped, tokens_total=int(res["bf16"][1].numel()))
    # score_answers(share_prefix=True): one prompt, the unquantised model's greedy answer + two fixed candidates, 3 tokens each
    from internnav_amd.policy import InternVLAN1ForCausalLM

    full = {k: v.to(dev, BF16) for k, v in synthetic.materialize(synthetic.n1_full_spec(cfg, "nextdit_async"), 5).items()}
    sin = synthetic.qwen_inputs(1, 1, seed=33, cfg=cfg, n_text=20, n_tail=12)
    ids, grid, spv = sin["input_ids"], sin["grid_thw"], sin["pixel_values"]
    kw = dict(device=dev, max_envs=2, num_history=3, resize_w=280, resize_h=280, max_seq_len=512, max_patches=2 * spv.shape[0])
    plain = InternVLAN1ForCausalLM(full, cfg, "nextdit_async", **kw)
    st = plain.qwen.prefill(ids, spv.to(dev, BF16), grid)
    greedy = plain.qwen.decode(st, 3)[0].tolist()
    answers = [[greedy, [17, 905, 3001], [17, 2222, 64]]]
    lp = {}
    for name, m in (("bf16", plain), ("mx4", InternVLAN1ForCausalLM(full, cfg, "nextdit_async", mx4_decode=True, **kw))):
        r = m.score_answers(ids, answers, pixel_values=spv, image_grid_thw=grid, share_prefix=True)
        lp[name] = [t.float().cpu() for t in r.token_logprobs[0]]
    shift = max(float((a - b).abs().max()) for a, b in zip(lp["bf16"], lp["mx4"]))
    out["score_answers"] = dict(candidates=answers[0], logprob_bf16=[t.tolist() for t in lp["bf16"]], logprob_mx4=[t.tolist() for t in lp["mx4"]],
                                max_abs_shift=shift, sum_bf16=[float(t.sum()) for t in lp["bf16"]], sum_mx4=[float(t.sum()) for t in lp["mx4"]])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graph-steps", type=int, default=10)
    ap.add_argument("--skip-graph", action="store_true")
    ap.add_argument("--skip-drift", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device:", runtime.require_gfx950(), file=sys.stderr)
    M = a.envs
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    rows = [shape_row(*s, a.iters, a.repeats, dev) for s in (("q|k|v", M, QKV, H, "qkv"), ("o", M, H, H, "res"), ("gate|up", M, 2 * TI, H, "gu"),
                                                             ("down", M, H, TI, "res"), ("lm_head", M, VOCAB, H, "plain"))]
    say(f"{'shape':8s} {'N':>7s} {'K':>6s} {'bf16 us':>9s} {'TB/s':>6s} {'w8 us':>9s} {'TB/s':>6s} {'mx4 us':>9s} {'TB/s':>6s} {'w8/mx4':>7s} {'bf16/mx4':>8s}  bits")
    for r in rows:
        say(f"{r['shape']:8s} {r['N']:7d} {r['K']:6d} {r['bf16_us']:9.1f} {r['bf16_tbps']:6.2f} {r['w8_us']:9.1f} {r['w8_tbps']:6.2f} {r['mx4_us']:9.1f} "
            f"{r['mx4_tbps']:6.2f} {r['w8_over_mx4']:7.3f} {r['bf16_over_mx4']:8.3f}  {'equal' if r['bit_equal'] else 'DIFFER'}   spread % {r['spread_pct']}")
    out = dict(workload="mx4_decode_step", envs=M, iters=a.iters, repeats=a.repeats, shapes=rows)
    if not a.skip_graph:
        out["graph"] = graph_rows(M, a.graph_steps, a.repeats, dev)
        gr = out["graph"]
        say(f"decode + latents graph, {M} envs, full depth: bf16 {gr['bf16_ms']} ms  w8 {gr['w8_ms']} ms  mx4 {gr['mx4_ms']} ms  bf16/mx4 {gr['bf16_over_mx4']}  "
            f"w8/mx4 {gr['w8_over_mx4']}  bits (bf16 vs mx4) {'equal' if gr['bit_equal'] else 'DIFFER'}  (+{gr['mx4_extra_gb']} GB MXFP4, +{gr['lm_head8_extra_gb']} GB fp8 lm_head)")
    if not a.skip_drift:
        out["drift"] = drift(dev)
        d = out["drift"]
        say(f"drift vs the unquantised engine ({d['prompt']}): logits mean|err| {d['logits_mean_abs_err']:.4e} max|err| {d['logits_max_abs_err']:.4e} "
            f"(max|logit| {d['logits_max_abs']:.3f}); greedy tokens flipped {d['tokens_flipped']} of {d['tokens_total']}; "
            f"score_answers largest |log-probability shift| {d['score_answers']['max_abs_shift']:.4e}")
    say("")
    say("# JSON line")
    say(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
