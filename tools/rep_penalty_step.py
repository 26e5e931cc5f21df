"""Time the repetition penalty of System-2 greedy decoding against the plain selection, in one process on one GPU.

    python tools/rep_penalty_step.py [--envs 7] [--prompt 920] [--iters 200] [--repeats 5] [--graph-steps 10] [--skip-graph]

1. ops.argmax_rows against ops.argmax_penalty_rows (mark on) at --envs rows of 152064 fp32 logits, a seen set of --prompt tokens per row:
   `--iters` launches between two device events, the two kernels alternating, `--repeats` times, median. Every launch of a loop reads ANOTHER
   copy of the logits (32 copies of 4.3 MB; the rows of a real decode step were just written by lm_head, so they come from the caches there
   too). The penalised selection also reads the row's 19 KB bitmap (+3 % bytes); the ratio of the two medians is printed, 1.2 x is the
   bound the selection loop is held to.
2. The seen-set launch (ops.token_seen_set) for --prompt ids per row: once per System-2 call. The loop relaunches on the SAME ids and bitmap
   (26 KB + 133 KB, cache-resident after the first launch), so this is a warm figure: in a real call the ids were just uploaded.
3. The decode + latent-query launch sequence of --envs prompts (4 frames of 28 x 28 patches, 64 instruction tokens, 8 answer tokens) at the full
   depth of the 7B geometry, captured once with penalty 1.0 (the plain launch sequence) and once with 1.05, replayed alternately. Reported,
   not gated. The tokens of the two graphs may differ: that is what a penalty is for.
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

VOCAB = 152064
BF16 = torch.bfloat16


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


def _median_pair(fa, fb, iters, repeats):
    _events_us(fa, len(fa))
    _events_us(fb, len(fb))
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(_events_us(fa, iters))
        tb.append(_events_us(fb, iters))
    return statistics.median(ta), statistics.median(tb), ta, tb


def selection_rows(M, S, iters, repeats, dev):
    g = torch.Generator(device=dev).manual_seed(M)
    copies = 32
    xs = [torch.randn(M, VOCAB, generator=g, device=dev) * 4 for _ in range(copies)]
    ids = torch.randint(0, VOCAB, (M, S), generator=g, device=dev, dtype=torch.int32)
    lens = torch.full((M,), S, dtype=torch.int32, device=dev)
    ldw = ((VOCAB + 31) // 32 + 3) // 4 * 4
    seen0 = torch.zeros(M, ldw, dtype=torch.uint32, device=dev)
    ops.token_seen_set(seen0, ids, lens, VOCAB)
    seen = seen0.clone()
    o1, o2 = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
    plain = [lambda x=x: ops.argmax_rows(x, o1) for x in xs]
    pen = [lambda x=x: ops.argmax_penalty_rows(x, seen, 1.05, o2, mark=True) for x in xs]
    sets = [lambda: ops.token_seen_set(seen, ids, lens, VOCAB)]
    a, b, ta, tb = _median_pair(plain, pen, iters, repeats)
    ts = [_events_us(sets, iters) for _ in range(repeats)]
    c = statistics.median(ts)
    moved = 0
    for x in xs[:4]:
        ops.argmax_rows(x, o1)
        ops.argmax_penalty_rows(x, seen0, 1.05, o2, mark=False)
        moved += int((o1 != o2).sum())
    return dict(rows=M, n=VOCAB, seen_per_row=S, argmax_us=round(a, 2), argmax_penalty_us=round(b, 2), ratio=round(b / a, 3),
                argmax_runs=[round(v, 2) for v in ta], argmax_penalty_runs=[round(v, 2) for v in tb], seen_set_us=round(c, 2),
                seen_set_runs=[round(v, 2) for v in ts], rows_moved_by_1p05_of_4x=moved, logits_copies=copies)


def graph_rows(envs, steps, repeats, dev):
    cfg = synthetic.QWEN_N1_CFG
    n_img, n_text, n_dec = 4, 64, 8
    inp = synthetic.qwen_inputs(envs, n_img, seed=0, cfg=cfg, n_text=n_text, n_tail=8)
    ids, grid = inp["input_ids"], inp["grid_thw"]
    pv = inp["pixel_values"].to(dev, BF16)
    S = ids.shape[1]
    eng = QwenVLEngine(synthetic.LazyDeviceWeights(synthetic.qwen_spec(cfg), dev, seed=0), cfg, dev, max_seqs=envs,
                       max_seq_len=(S + n_dec + 8 + 63) // 64 * 64, max_patches=pv.shape[0])
    out, graphs = {}, {}
    for name, p in (("plain", 1.0), ("penalty", 1.05)):
        P = eng.plan(ids, grid, n_decode=n_dec, with_latents=True, repetition_penalty=p)
        if name == "plain":
            eng.run_prefill(P, pv)          # both plans decode from the same prefilled prompt
            torch.cuda.synchronize()
        toks = torch.zeros(envs, n_dec, dtype=torch.int32, device=dev)
        lat = torch.zeros(envs, cfg["n_query"], cfg["t_hidden"], dtype=BF16, device=dev)

        def seq(P=P, toks=toks, lat=lat):
            eng.run_decode(P, toks)
            eng.run_latents(P, lat)
        graphs[name] = runtime.GraphedCall(seq, {})
        out[name] = toks

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
    t = {"plain": [], "penalty": []}
    for _ in range(repeats):
        for name in ("plain", "penalty"):
            t[name].append(ms(graphs[name]))
    torch.cuda.synchronize()
    a, b = statistics.median(t["plain"]), statistics.median(t["penalty"])
    return dict(envs=envs, prompt_tokens=S, passes=f"{n_dec - 1} decode + {n_dec} lm_head + selection, 1 latent-query pass; the penalty graph adds 1 seen-set launch",
                plain_ms=round(a, 3), penalty_ms=round(b, 3), ratio=round(b / a, 4), plain_runs=[round(v, 3) for v in t["plain"]],
                penalty_runs=[round(v, 3) for v in t["penalty"]], tokens_plain=out["plain"][0].tolist(), tokens_penalty=out["penalty"][0].tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=7)
    ap.add_argument("--prompt", type=int, default=920)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graph-steps", type=int, default=10)
    ap.add_argument("--skip-graph", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device:", runtime.require_gfx950(), file=sys.stderr)
    r = selection_rows(a.envs, a.prompt, a.iters, a.repeats, dev)
    print(f"selection, {r['rows']} rows x {r['n']} logits, {r['seen_per_row']} seen ids per row ({a.iters} launches x {a.repeats}, median)")
    print(f"  argmax_rows          {r['argmax_us']:8.2f} us   runs {r['argmax_runs']}")
    print(f"  argmax_penalty_rows  {r['argmax_penalty_us']:8.2f} us   runs {r['argmax_penalty_runs']}   penalty / plain {r['ratio']:.3f}")
    print(f"  token_seen_set       {r['seen_set_us']:8.2f} us   runs {r['seen_set_runs']}   (once per System-2 call; warm: the loop reuses one set of ids and one bitmap)")
    out = dict(workload="rep_penalty_step", envs=a.envs, iters=a.iters, repeats=a.repeats, selection=r)
    if not a.skip_graph:
        gr = out["graph"] = graph_rows(a.envs, a.graph_steps, a.repeats, dev)
        print(f"decode + latents graph, {gr['envs']} envs x {gr['prompt_tokens']} prompt tokens, full depth: penalty 1.0 {gr['plain_ms']} ms  "
              f"penalty 1.05 {gr['penalty_ms']} ms  ratio {gr['ratio']}   runs {gr['plain_runs']} / {gr['penalty_runs']}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
