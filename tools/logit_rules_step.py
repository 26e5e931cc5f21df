"""Time the logits-processor rule launch of System-2 decoding beside the automaton mask it runs behind, and the decode + latents graph without
and with a rule set, in one process on one GPU.

    python tools/logit_rules_step.py [--envs 7] [--iters 200] [--repeats 5] [--images 4] [--decode 8] [--skip-graph]

1. ops.automaton_mask_rows with the universal automaton (the yardstick: the other launch that sits in front of a selection) and
   ops.logit_rules_rows at --envs rows of 152064 fp32 logits with
     navigation   a navigation-sized set: a bias on one (made-up) STOP id, 8 multi-token bad words, no_repeat_ngram_size 3, 920-token histories,
                  at answer column 1 (the append included)
     limits       1024 sequences of up to 32 tokens (512 biased over 256 targets, 512 bad words), no_repeat_ngram_size 16, 4096-token
                  histories over 16 distinct tokens (every window compares several tokens)
     forced       the navigation set with forced_eos_token_id, at the forced column (the one dense fill of the row)
   `--iters` launches between two device events, the loops alternating, `--repeats` times, median and all runs. Every launch of a loop takes
   ANOTHER of 32 copies of the logits (4.3 MB each), as in tools/constrain_step.py.
2. The captured decode + latent-queries graph of --envs envs at the full depth of the 7B geometry (plan(n_decode, with_latents) -> run_decode +
   run_latents), without and with the navigation set, replayed alternately: `--repeats` windows of 10 replays each.
No real tokenizer or checkpoint has been seen: which ids mean STOP, and which sequences are worth banning, is the user's input.
Prints a table and one JSON line. Ratios are printed, not asserted."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from internnav_amd import logit_rules, ops, runtime, synthetic  # noqa: E402
from internnav_amd.constrain import TokenAutomaton  # noqa: E402
from internnav_amd.qwen_vl import QwenVLEngine  # noqa: E402

VOCAB = 152064
STOP = 30000               # a made-up id


def navigation_spec(g, forced=False) -> dict:
    words = [[int(t) for t in g.integers(1000, 100000, int(g.integers(2, 4)))] for _ in range(8)]
    spec = dict(sequence_bias={(STOP,): -1.5}, bad_words_ids=words, no_repeat_ngram_size=3)
    return dict(spec, forced_eos_token_id=VOCAB - 1) if forced else spec


def limits_spec(g, alphabet) -> dict:
    seq = lambda: [int(t) for t in alphabet[g.integers(0, alphabet.size, int(g.integers(1, 32)))]]     # noqa: E731
    targets = [int(t) for t in g.permutation(np.arange(1000, 100000))[:768]]
    sb = {tuple(seq() + [targets[i % 256]]): float(g.normal()) for i in range(512)}
    while len(sb) < 512:
        sb[tuple(seq() + [targets[len(sb) % 256]])] = 0.5
    return dict(sequence_bias=sb, bad_words_ids=[seq() + [targets[256 + i]] for i in range(512)], no_repeat_ngram_size=16)


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
    tg = torch.Generator(device=dev).manual_seed(M)
    g = np.random.default_rng(M)
    copies = 32
    xs = [torch.randn(M, VOCAB, generator=tg, device=dev) * 4 for _ in range(copies)]
    uni = TokenAutomaton.universal(VOCAB, [VOCAB - 1]).to(dev)
    st = torch.zeros(2, M, dtype=torch.int32, device=dev)
    prev = torch.from_numpy(g.integers(0, VOCAB, M).astype(np.int32)).to(dev)
    loops = {"automaton_mask_rows": [lambda x=x: ops.automaton_mask_rows(x, uni, st[0], None, st[1]) for x in xs]}
    alphabet = g.integers(1000, 100000, 16)
    sets = {"rules_navigation": (navigation_spec(g), 920, 1, 8, None), "rules_limits": (limits_spec(g, alphabet), 4096, 1, 8, alphabet),
            "rules_forced_column": (navigation_spec(g, forced=True), 920, 7, 8, None)}
    info = {}
    for name, (spec, H, col, T, alpha) in sets.items():
        tb_host = logit_rules.compile_rules(spec, VOCAB, [VOCAB - 1], [H - col] * M, T)
        tb = tb_host.to(dev)
        h = g.integers(0, VOCAB, (M, H + 8)) if alpha is None else alpha[g.integers(0, alpha.size, (M, H + 8))]
        hist = torch.from_numpy(h.astype(np.int32)).to(dev)
        loops[name] = [lambda x=x, tb=tb, hist=hist, col=col: ops.logit_rules_rows(x, tb, col, hist, tb.len0, prev, tb.eos_first) for x in xs]
        info[name] = dict(history=H, col=col, sequences=int(tb_host.seq_bias.size), groups=int(tb_host.grp_tok.size), ngram=tb_host.ngram)
    for fns in loops.values():
        _events_us(fns, len(fns))
    runs = {name: [] for name in loops}
    for _ in range(repeats):
        for name, fns in loops.items():
            runs[name].append(_events_us(fns, iters))
    med = {name: statistics.median(v) for name, v in runs.items()}
    out = dict(rows=M, n=VOCAB, logits_copies=copies, sets=info)
    for name in loops:
        out[name] = dict(us=round(med[name], 2), vs_automaton_mask=round(med[name] / med["automaton_mask_rows"], 3), runs=[round(v, 2) for v in runs[name]])
    return out


def graph_rows(envs, n_img, n_dec, repeats, dev):
    cfg = synthetic.QWEN_N1_CFG
    inp = synthetic.qwen_inputs(envs, n_img, seed=0, cfg=cfg, n_text=64, n_tail=8)
    ids, grid = inp["input_ids"], inp["grid_thw"]
    pv = inp["pixel_values"].to(dev, torch.bfloat16)
    S = ids.shape[1]
    eng = QwenVLEngine(synthetic.LazyDeviceWeights(synthetic.qwen_spec(cfg), dev, seed=0), cfg, dev, max_seqs=envs, max_seq_len=(S + n_dec + 8 + 63) // 64 * 64,
                       max_patches=pv.shape[0])
    rules = logit_rules.compile_rules(navigation_spec(np.random.default_rng(0)), cfg["vocab"], [cfg["eos_token_id"]], [S] * envs, n_dec)
    toks = torch.zeros(envs, n_dec, dtype=torch.int32, device=dev)
    lat = torch.zeros(envs, cfg["n_query"], cfg["t_hidden"], dtype=torch.bfloat16, device=dev)
    graphs = {}
    for name, kw in (("off", {}), ("on", {"logit_rules": rules})):
        P = eng.plan(ids, grid, n_decode=n_dec, with_latents=True, **kw)
        if name == "off":
            eng.run_prefill(P, pv)              # both plans decode from the same prefilled prompt
            torch.cuda.synchronize()

        def chain(P=P):
            eng.run_decode(P, toks)
            eng.run_latents(P, lat)

        graphs[name] = runtime.GraphedCall(chain, {})
    runs = {name: [] for name in graphs}
    for gr in graphs.values():
        _events_us([gr], 3)
    for _ in range(repeats):
        for name, gr in graphs.items():
            runs[name].append(_events_us([gr], 10) / 1e3)
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
    print(f"{r['rows']} rows x {r['n']} logits ({a.iters} launches x {a.repeats}, median); sets: {r['sets']}")
    for name in ("automaton_mask_rows", "rules_navigation", "rules_limits", "rules_forced_column"):
        p = r[name]
        print(f"  {name:20s} {p['us']:9.2f} us   {p['vs_automaton_mask']:7.3f} x automaton_mask_rows   runs {p['runs']}")
    out = dict(workload="logit_rules_step", envs=a.envs, iters=a.iters, repeats=a.repeats, kernel=r)
    if not a.skip_graph:
        f = out["graph"] = graph_rows(a.envs, a.images, a.decode, a.repeats, dev)
        print(f"decode + latents graph, {f['envs']} envs, {f['prompt_tokens']} prompt tokens, {f['n_decode']} answer tokens, {f['layers']} layers: "
              f"off {f['off_ms']} ms, on {f['on_ms']} ms ({f['on_vs_off']} x, {f['per_step_us']} us per step)   runs {f['runs']}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
