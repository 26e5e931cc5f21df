"""Time the automaton mask of constrained System-2 decoding beside the selection it runs in front of, and the decode + latents graph without and
with a constraint, in one process on one GPU.

    python tools/constrain_step.py [--envs 7] [--iters 200] [--repeats 5] [--images 4] [--decode 8] [--skip-graph]

1. ops.argmax_rows (the yardstick), ops.automaton_mask_rows with a navigation-sized allow set (a few dozen tokens allowed: almost every logit
   is written) and with the universal set (nothing is written), at --envs rows of 152064 fp32 logits: `--iters` launches between two device
   events, the kernels alternating, `--repeats` times, median and all runs. Every launch of a loop takes ANOTHER of 32 copies of the logits
   (4.3 MB each), as in tools/sample_step.py. Both mask loops run without an advance (prev_tok = None, the state stays the start state), so a
   loop's launches all do the same work.
2. The captured decode + latent-queries graph of --envs envs at the full depth of the 7B geometry (plan(n_decode, with_latents) -> run_decode +
   run_latents), without and with the navigation constraint, replayed alternately: `--repeats` windows of 10 replays each.
Prints a table and one JSON line. Ratios are printed, not asserted."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from internnav_amd import ops, runtime, synthetic  # noqa: E402
from internnav_amd.constrain import TokenAutomaton  # noqa: E402
from internnav_amd.qwen_vl import QwenVLEngine  # noqa: E402

VOCAB = 152064


def navigation_automaton(vocab: int, eos: int) -> TokenAutomaton:
    """navigation_answers over a made-up byte vocabulary (no real tokenizer has been seen): digits, two-digit tokens, ' d' tokens, separators,
    arrows and STOP pieces on the first ids, every other token without bytes (never allowed)"""
    toks = [bytes([48 + d]) for d in range(10)] + [f"{d:02d}".encode() for d in range(100)] + [f" {d}".encode() for d in range(10)]
    toks += [b" ", b",", b", "] + [a.encode("utf-8") for a in "↑←→↓"] + [b"ST", b"OP", b"STOP"]
    tb = [b""] * vocab
    tb[100: 100 + len(toks)] = toks
    return TokenAutomaton.navigation_answers(tb, [eos])


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


def kernel_rows(M, iters, repeats, dev):
    g = torch.Generator(device=dev).manual_seed(M)
    copies = 32
    xs = [torch.randn(M, VOCAB, generator=g, device=dev) * 4 for _ in range(copies)]
    nav, uni = navigation_automaton(VOCAB, VOCAB - 1), TokenAutomaton.universal(VOCAB, [VOCAB - 1])
    tok = torch.empty(M, dtype=torch.int32, device=dev)
    st = torch.zeros(2, M, dtype=torch.int32, device=dev)
    loops = {"argmax_rows": [lambda x=x: ops.argmax_rows(x, tok) for x in xs]}
    for name, a in (("mask_navigation", nav), ("mask_universal", uni)):
        tb = a.to(dev)
        st.fill_(a.start)
        assert a.start == 0
        loops[name] = [lambda x=x, tb=tb: ops.automaton_mask_rows(x, tb, st[0], None, st[1]) for x in xs]
    for fns in loops.values():
        _events_us(fns, len(fns))
    runs = {name: [] for name in loops}
    for _ in range(repeats):
        for name, fns in loops.items():
            runs[name].append(_events_us(fns, iters))
    med = {name: statistics.median(v) for name, v in runs.items()}
    out = dict(rows=M, n=VOCAB, logits_copies=copies, allowed_in_start_state=int(nav.allowed_ids(nav.start).size), states=nav.n_states,
               classes=int(nav.token_class.max()) + 1)
    for name in loops:
        out[name] = dict(us=round(med[name], 2), vs_argmax_rows=round(med[name] / med["argmax_rows"], 3), runs=[round(v, 2) for v in runs[name]])
    return out


def graph_rows(envs, n_img, n_dec, repeats, dev):
    cfg = synthetic.QWEN_N1_CFG
    inp = synthetic.qwen_inputs(envs, n_img, seed=0, cfg=cfg, n_text=64, n_tail=8)
    ids, grid = inp["input_ids"], inp["grid_thw"]
    pv = inp["pixel_values"].to(dev, torch.bfloat16)
    S = ids.shape[1]
    eng = QwenVLEngine(synthetic.LazyDeviceWeights(synthetic.qwen_spec(cfg), dev, seed=0), cfg, dev, max_seqs=envs, max_seq_len=(S + n_dec + 8 + 63) // 64 * 64,
                       max_patches=pv.shape[0])
    nav = navigation_automaton(cfg["vocab"], cfg["eos_token_id"])
    toks = torch.zeros(envs, n_dec, dtype=torch.int32, device=dev)
    lat = torch.zeros(envs, cfg["n_query"], cfg["t_hidden"], dtype=torch.bfloat16, device=dev)
    graphs = {}
    for name, kw in (("off", {}), ("on", {"constraint": nav})):
        P = eng.plan(ids, grid, n_decode=n_dec, with_latents=True, **kw)
        if name == "off":
            eng.run_prefill(P, pv)              # both plans decode from the same prefilled prompt
            torch.cuda.synchronize()

        def chain(P=P):
            eng.run_decode(P, toks)
            eng.run_latents(P, lat)

        graphs[name] = runtime.GraphedCall(chain, {})
    runs = {name: [] for name in graphs}
    for g in graphs.values():
        _events_us([g], 3)
    for _ in range(repeats):
        for name, g in graphs.items():
            runs[name].append(_events_us([g], 10) / 1e3)
    med = {k: statistics.median(v) for k, v in runs.items()}
    return dict(envs=envs, prompt_tokens=S, n_decode=n_dec, layers=len(eng.layers), off_ms=round(med["off"], 3), on_ms=round(med["on"], 3),
                on_vs_off=round(med["on"] / med["off"], 4), per_step_us=round((med["on"] - med["off"]) * 1e3 / n_dec, 2),
                runs={k: [round(v, 3) for v in vs] for k, vs in runs.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--decode", type=int, default=8)
    ap.add_argument("--skip-graph", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device:", runtime.require_gfx950(), file=sys.stderr)
    r = kernel_rows(a.envs, a.iters, a.repeats, dev)
    print(f"{r['rows']} rows x {r['n']} logits ({a.iters} launches x {a.repeats}, median); navigation automaton: {r['states']} states, {r['classes']} classes, "
          f"{r['allowed_in_start_state']} tokens allowed in the start state")
    for name in ("argmax_rows", "mask_navigation", "mask_universal"):
        p = r[name]
        print(f"  {name:16s} {p['us']:9.2f} us   {p['vs_argmax_rows']:7.3f} x argmax_rows   runs {p['runs']}")
    out = dict(workload="constrain_step", envs=a.envs, iters=a.iters, repeats=a.repeats, kernel=r)
    if not a.skip_graph:
        f = out["graph"] = graph_rows(a.envs, a.images, a.decode, a.repeats, dev)
        print(f"decode + latents graph, {f['envs']} envs, {f['prompt_tokens']} prompt tokens, {f['n_decode']} answer tokens, {f['layers']} layers: "
              f"off {f['off_ms']} ms, on {f['on_ms']} ms ({f['on_vs_off']} x, {f['per_step_us']} us per step)   runs {f['runs']}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
