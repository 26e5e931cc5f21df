"""Time score_answers(share_prefix=True) against the per-pair path at the full depth of the 7B geometry, in one process on one GPU.

    python tools/score_prefix_step.py [--prompts 7] [--cands 4] [--tokens 4] [--repeats 5] [--iters 56]

--prompts prompts of 4 frames x --cands candidates x --tokens tokens on an engine of --prompts sequences (lazily materialised weights):
1. wall time (host clock around the call, device synchronised) of score_answers(share_prefix=False) and (share_prefix=True), alternating,
   `--repeats` times after one warm-up of each, median and all runs, and the largest difference between their token log-probabilities;
2. device-event times of the parts of the shared path: the prefill of the prompts, the suffix pass (all layers), the scoring of the first
   rows and of the suffix rows (gather + norm + lm_head + logprob_rows);
3. the attention launch alone: ops.attention_prefix on the suffix pass's shape (pairs x (tokens - 1) rows, the prompts' K/V in their cache
   slots) against ops.attention (causal) on a materialised [prefix | suffix] copy per pair of the same data, `--iters` launches between two
   device events, alternating, every launch on another layer's cache / another of as many copies (more bytes than the Infinity Cache holds).
Prints a table and one JSON line."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from internnav_amd import ops, runtime, synthetic  # noqa: E402
from internnav_amd.policy import InternVLAN1ForCausalLM, score_prefix_plan  # noqa: E402
from internnav_amd.qwen_vl import QwenVLEngine  # noqa: E402

BF16 = torch.bfloat16
med = statistics.median


def _timed(fn, repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(repeats + 1):
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts[1:]                                       # the first run warms the caches and the allocator


def _wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _events_us(fns, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(iters):
        fns[i % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, default=7)
    ap.add_argument("--cands", type=int, default=4)
    ap.add_argument("--tokens", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=56)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device:", runtime.require_gfx950(), file=sys.stderr)
    cfg = synthetic.QWEN_N1_CFG
    B, C, T = a.prompts, a.cands, a.tokens
    inp = synthetic.qwen_inputs(B, 4, seed=0, cfg=cfg, n_text=64, n_tail=8)
    ids, grid = inp["input_ids"], inp["grid_thw"]
    pv = inp["pixel_values"].to(dev, BF16)
    Sp = ids.shape[1]
    eng = QwenVLEngine(synthetic.LazyDeviceWeights(synthetic.qwen_spec(cfg), dev, seed=0), cfg, dev, max_seqs=B,
                       max_seq_len=(Sp + T + 8 + 63) // 64 * 64, max_patches=pv.shape[0])
    model = InternVLAN1ForCausalLM.__new__(InternVLAN1ForCausalLM)      # the System-2 surface alone: no System-1 head is built
    model.qwen, model.device, model._score_logits, model._gen, model.last_score = eng, dev, None, None, {}
    g = torch.Generator().manual_seed(1)
    answers = [[torch.randint(0, 3000, (T,), generator=g).tolist() for _ in range(C)] for _ in range(B)]
    kw = dict(pixel_values=pv, image_grid_thw=grid)

    # ---- 1. the two paths of the public call
    runs = {False: [], True: []}
    res = {}
    for share in (False, True):
        _, res[share] = _wall_ms(lambda: model.score_answers(ids, answers, share_prefix=share, **kw))
    stats = {}
    for _ in range(a.repeats):
        for share in (False, True):
            t, _ = _wall_ms(lambda: model.score_answers(ids, answers, share_prefix=share, **kw))
            runs[share].append(t)
            stats[share] = dict(model.last_score)
    diff = max(float((x - y).abs().max()) for b in range(B) for x, y in zip(res[False].token_logprobs[b], res[True].token_logprobs[b]))
    out = dict(workload="score_prefix_step", prompts=B, candidates=C, tokens=T, prompt_tokens=int(Sp), repeats=a.repeats,
               per_pair_ms=round(med(runs[False]), 3), shared_ms=round(med(runs[True]), 3), speedup=round(med(runs[False]) / med(runs[True]), 3),
               per_pair_runs=[round(v, 3) for v in runs[False]], shared_runs=[round(v, 3) for v in runs[True]], per_pair_stats=stats[False],
               shared_stats=stats[True], max_logprob_difference=round(diff, 5))

    # ---- 2. the parts of the shared path
    plens = np.full(B, Sp, dtype=np.int64)
    plan = score_prefix_plan(plens, [[T] * C] * B, int(eng.x.shape[0]))
    state = {}
    t_pre = _timed(lambda: state.update(eng.prefill(ids, pv, grid, seq_lens=plens)), a.repeats)
    cand_of = [answers[b][c] for b, c in plan["pairs"]]
    lp1 = torch.empty(plan["first_pair"].size, dtype=torch.float32, device=dev)
    t_first = _timed(lambda: model._score_rows(eng.x[: B * Sp], plan["first_rows"], plan["first_slabs"], [c[0] for c in cand_of], lp1), a.repeats)
    parts = dict(prefill_ms=round(med(t_pre), 3), first_rows=int(plan["first_pair"].size), first_rows_ms=round(med(t_first), 3), suffix=[])
    for ps in plan["passes"]:
        P, m = ps["pair"].size, ps["m"]
        toks = np.asarray([cand_of[p][:-1] + [0] * (m - len(cand_of[p]) + 1) for p in ps["pair"]], dtype=np.int64)
        t_suf = _timed(lambda: eng.suffix_pass(state, ps["prompt"], toks, ps["suf_len"]), a.repeats)
        lp2 = torch.empty(ps["rows"].size, dtype=torch.float32, device=dev)
        t_rows = _timed(lambda: model._score_rows(eng.x[: P * m], ps["rows"], ps["slabs"], [t for p in ps["pair"] for t in cand_of[p][1:]], lp2), a.repeats)
        parts["suffix"].append(dict(pairs=int(P), m=int(m), pass_ms=round(med(t_suf), 3), rows=int(ps["rows"].size), rows_ms=round(med(t_rows), 3),
                                    pass_runs=[round(v, 3) for v in t_suf]))
    parts["prefill_runs"] = [round(v, 3) for v in t_pre]
    out["parts"] = parts

    # ---- 3. the attention launch alone (the caches hold the prompts of the last prefill)
    ps = plan["passes"][0]
    P, m = int(ps["pair"].size), int(ps["m"])
    nh, nkv, hd = eng.nh, eng.nkv, eng.hd
    nl = min(len(eng.layers), 28)
    gq = torch.Generator(device=dev).manual_seed(2)
    qkv = torch.randn(P * m, eng.qkv_w, generator=gq, device=dev).to(BF16)
    q4 = qkv[:, : nh * hd].view(P, m, nh, hd)
    k4 = qkv[:, nh * hd:(nh + nkv) * hd].view(P, m, nkv, hd)
    v4 = qkv[:, (nh + nkv) * hd:].view(P, m, nkv, hd)
    i32 = lambda v: torch.tensor(np.asarray(v), dtype=torch.int32, device=dev)
    slot, pfx, suf = i32(ps["prompt"]), i32([Sp] * P), i32(ps["suf_len"])
    o1, o2 = (torch.empty(P, m, nh, hd, dtype=BF16, device=dev) for _ in range(2))
    caches = [L["kv"].view(eng.B_max, eng.S_max, 2, nkv, hd) for L in eng.layers[:nl]]
    mats = []
    sl64 = torch.from_numpy(np.asarray(ps["prompt"], dtype=np.int64)).to(dev)
    for c5 in caches:                                  # materialised copy per layer: [P, Sp + m] keys / values
        K = torch.cat([c5[sl64, :Sp, 0], k4], 1).contiguous()
        V = torch.cat([c5[sl64, :Sp, 1], v4], 1).contiguous()
        mats.append((K, V))
    fa = [lambda c5=c5: ops.attention_prefix(q4, k4, v4, c5[:, :, 0], c5[:, :, 1], slot, pfx, suf, out=o1, max_pfx=int(Sp)) for c5 in caches]
    fb = [lambda K=K, V=V: ops.attention(q4, K, V, causal=True, out=o2) for K, V in mats]
    fa[0](), fb[0]()
    torch.cuda.synchronize()
    d_att = float((o1.float() - o2.float()).abs().max())
    _events_us(fa, len(fa)), _events_us(fb, len(fb))
    ta, tb = [], []
    for _ in range(a.repeats):
        ta.append(_events_us(fa, a.iters))
        tb.append(_events_us(fb, a.iters))
    out["attention"] = dict(pairs=P, m=m, prefix=int(Sp), layers_cycled=nl, prefix_us=round(med(ta), 2), materialised_us=round(med(tb), 2),
                            ratio=round(med(ta) / med(tb), 3), prefix_runs=[round(v, 2) for v in ta], materialised_runs=[round(v, 2) for v in tb],
                            max_abs_difference=round(d_att, 5),
                            cache_bytes_read_once=int(B * nkv * Sp * hd * 2 * 2), materialised_bytes=int(P * nkv * (Sp + m) * hd * 2 * 2))

    print(f"score_answers, {B} prompts x {C} candidates x {T} tokens, {Sp} prompt tokens, full depth ({a.repeats} alternating runs, median)")
    print(f"  share_prefix=False {out['per_pair_ms']:9.3f} ms   {out['per_pair_stats']}   runs {out['per_pair_runs']}")
    print(f"  share_prefix=True  {out['shared_ms']:9.3f} ms   {out['shared_stats']}   runs {out['shared_runs']}")
    print(f"  speed-up {out['speedup']:.3f} x   max |token logprob difference| {out['max_logprob_difference']}")
    print(f"parts of the shared path (device events): prefill of {B} prompts {parts['prefill_ms']} ms; first-token rows ({parts['first_rows']}) "
          f"{parts['first_rows_ms']} ms")
    for s in parts["suffix"]:
        print(f"  suffix pass {s['pairs']} pairs x {s['m']} rows {s['pass_ms']} ms (runs {s['pass_runs']}); scoring its {s['rows']} rows {s['rows_ms']} ms")
    at = out["attention"]
    print(f"attention launch alone, {at['pairs']} pairs x {at['m']} rows behind {at['prefix']} cached keys ({a.iters} launches x {a.repeats}, median): "
          f"attention_prefix {at['prefix_us']} us, ops.attention on the materialised copy {at['materialised_us']} us, ratio {at['ratio']}; "
          f"max |difference| {at['max_abs_difference']}; runs {at['prefix_runs']} / {at['materialised_runs']}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
