"""Time the per-token log-probability kernel of System-2 decoding against the selections it replaces, in one process on one GPU.

    python tools/logprob_step.py [--envs 7] [--prompt 920] [--iters 200] [--repeats 5] [--graph-steps 10] [--skip-graph] [--skip-score]

1. ops.argmax_rows against ops.logprob_rows(seen=None), and ops.argmax_penalty_rows against ops.logprob_rows(seen, 1.05, mark), at --envs rows
   of 152064 fp32 logits with a seen set of --prompt tokens per row: `--iters` launches between two device events, the two kernels of a pair
   alternating, `--repeats` times, median and all runs. Every launch of a loop reads ANOTHER of 32 copies of the logits (4.3 MB each), as in
   tools/rep_penalty_step.py. 1.2 x the replaced kernel is the allowance; the ratio is printed, not asserted (the switch is opt-in).
2. The decode + latent-query launch sequence of --envs prompts at the full depth of the 7B geometry, captured on an engine without and on an
   engine with token_logprobs (same lazily materialised weights), replayed alternately.
3. score_answers for --envs prompts x 4 candidates x 4 tokens on the token_logprobs-free engine: wall time of the call, and device-event times
   of one prefill group, of the lm_head GEMM of its rows and of the logprob_rows launch on them.
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


def kernel_rows(M, S, iters, repeats, dev):
    g = torch.Generator(device=dev).manual_seed(M)
    copies = 32
    xs = [torch.randn(M, VOCAB, generator=g, device=dev) * 4 for _ in range(copies)]
    ids = torch.randint(0, VOCAB, (M, S), generator=g, device=dev, dtype=torch.int32)
    lens = torch.full((M,), S, dtype=torch.int32, device=dev)
    ldw = ((VOCAB + 31) // 32 + 3) // 4 * 4
    seen0 = torch.zeros(M, ldw, dtype=torch.uint32, device=dev)
    ops.token_seen_set(seen0, ids, lens, VOCAB)
    sa, sb = seen0.clone(), seen0.clone()
    o1, o2 = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
    lp, mg = torch.empty(M, dtype=torch.float32, device=dev), torch.empty(M, dtype=torch.float32, device=dev)
    out = dict(rows=M, n=VOCAB, seen_per_row=S, logits_copies=copies)
    pairs = (("plain", [lambda x=x: ops.argmax_rows(x, o1) for x in xs], [lambda x=x: ops.logprob_rows(x, o2, lp, mg) for x in xs]),
             ("penalty", [lambda x=x: ops.argmax_penalty_rows(x, sa, 1.05, o1, mark=True) for x in xs],
              [lambda x=x: ops.logprob_rows(x, o2, lp, mg, seen=sb, penalty=1.05, mark=True) for x in xs]))
    for name, fa, fb in pairs:
        a, b, ta, tb = _median_pair(fa, fb, iters, repeats)
        out[name] = dict(argmax_us=round(a, 2), logprob_us=round(b, 2), ratio=round(b / a, 3), argmax_runs=[round(v, 2) for v in ta],
                         logprob_runs=[round(v, 2) for v in tb])
    same = 0
    for x in xs[:4]:
        ops.argmax_penalty_rows(x, seen0, 1.05, o1, mark=False)
        ops.logprob_rows(x, o2, lp, mg, seen=seen0, penalty=1.05)
        same += int((o1 == o2).sum())
    out["ids_equal_of_4x"] = f"{same} of {4 * M}"
    return out


def _engine(cfg, dev, envs, S, n_dec, patches, **kw):
    return QwenVLEngine(synthetic.LazyDeviceWeights(synthetic.qwen_spec(cfg), dev, seed=0), cfg, dev, max_seqs=envs,
                        max_seq_len=(S + n_dec + 8 + 63) // 64 * 64, max_patches=patches, **kw)


def graph_rows(envs, steps, repeats, dev):
    cfg = synthetic.QWEN_N1_CFG
    n_img, n_text, n_dec = 4, 64, 8
    inp = synthetic.qwen_inputs(envs, n_img, seed=0, cfg=cfg, n_text=n_text, n_tail=8)
    ids, grid = inp["input_ids"], inp["grid_thw"]
    pv = inp["pixel_values"].to(dev, BF16)
    S = ids.shape[1]
    out, graphs, toks_of = {}, {}, {}
    for name, kw in (("off", {}), ("on", dict(token_logprobs=True, max_decode=n_dec))):
        eng = _engine(cfg, dev, envs, S, n_dec, pv.shape[0], **kw)
        P = eng.plan(ids, grid, n_decode=n_dec, with_latents=True)
        eng.run_prefill(P, pv)
        torch.cuda.synchronize()
        toks = torch.zeros(envs, n_dec, dtype=torch.int32, device=dev)
        lat = torch.zeros(envs, cfg["n_query"], cfg["t_hidden"], dtype=BF16, device=dev)

        def seq(eng=eng, P=P, toks=toks, lat=lat):
            eng.run_decode(P, toks)
            eng.run_latents(P, lat)
        graphs[name] = runtime.GraphedCall(seq, {})
        toks_of[name] = toks
        if name == "on":
            out["logprob_row0"] = [round(v, 4) for v in eng.last_logprobs(P)[0][0].tolist()]

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
    t = {"off": [], "on": []}
    for _ in range(repeats):
        for name in ("off", "on"):
            t[name].append(ms(graphs[name]))
    torch.cuda.synchronize()
    a, b = statistics.median(t["off"]), statistics.median(t["on"])
    out.update(envs=envs, prompt_tokens=S, passes=f"{n_dec - 1} decode + {n_dec} lm_head + selection, 1 latent-query pass", off_ms=round(a, 3),
               on_ms=round(b, 3), ratio=round(b / a, 4), off_runs=[round(v, 3) for v in t["off"]], on_runs=[round(v, 3) for v in t["on"]],
               tokens_equal=bool(torch.equal(toks_of["off"], toks_of["on"])))
    return out


def score_rows(envs, repeats, dev):
    """score_answers' three parts for envs prompts x 4 candidates x 4 tokens (one prefill group = envs pairs on an engine of envs sequences)"""
    from internnav_amd.policy import score_row_plan

    cfg = synthetic.QWEN_N1_CFG
    n_cand, n_tok = 4, 4
    inp = synthetic.qwen_inputs(envs, 4, seed=0, cfg=cfg, n_text=64, n_tail=8)
    ids, grid = inp["input_ids"], inp["grid_thw"]
    pv = inp["pixel_values"].to(dev, BF16)
    Sp = ids.shape[1]
    eng = _engine(cfg, dev, envs, Sp + n_tok, 0, pv.shape[0])
    g = torch.Generator().manual_seed(1)
    cand = torch.randint(0, 3000, (envs, n_tok), generator=g)
    full = torch.cat([ids, cand], 1)
    S, rows, off, slabs = score_row_plan([Sp] * envs, [n_tok] * envs)
    rows_d = torch.from_numpy(rows).to(dev)
    R = rows.size
    x, h = torch.empty(R, eng.H, dtype=torch.float32, device=dev), torch.empty(R, eng.H, dtype=BF16, device=dev)
    logits = torch.empty(R, VOCAB, dtype=torch.float32, device=dev)
    tgt = cand.reshape(-1).to(dev, torch.int32)
    tok, lp = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.float32, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(repeats + 1):
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return ts[1:]                                   # the first run warms the caches and the allocator

    def head():
        ops.gather_rows(eng.x[: envs * S], x, src=rows_d)
        ops.norm(x, eng.norm_w, None, eps=1e-6, rms=True, out=h, rows=R)
        ops.linear(h, eng.lm_head, out=logits)
    t_pre = timed(lambda: eng.prefill(full, pv, grid))
    t_head = timed(head)
    t_k = timed(lambda: ops.logprob_rows(logits, tok, lp, target=tgt))
    med = statistics.median
    return dict(prompts=envs, candidates=n_cand, tokens=n_tok, prompt_tokens=Sp, rows_per_group=R, groups=n_cand,
                prefill_group_ms=round(med(t_pre), 3), lm_head_group_ms=round(med(t_head), 3), logprob_kernel_group_us=round(med(t_k) * 1e3, 1),
                total_ms_est=round(n_cand * (med(t_pre) + med(t_head) + med(t_k)), 3), prefill_runs=[round(v, 3) for v in t_pre],
                lm_head_runs=[round(v, 3) for v in t_head], kernel_runs_us=[round(v * 1e3, 1) for v in t_k])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=7)
    ap.add_argument("--prompt", type=int, default=920)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graph-steps", type=int, default=10)
    ap.add_argument("--skip-graph", action="store_true")
    ap.add_argument("--skip-score", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device:", runtime.require_gfx950(), file=sys.stderr)
    r = kernel_rows(a.envs, a.prompt, a.iters, a.repeats, dev)
    print(f"selection + log-probability, {r['rows']} rows x {r['n']} logits, {r['seen_per_row']} seen ids per row ({a.iters} launches x {a.repeats}, median)")
    for name, what in (("plain", "argmax_rows         / logprob_rows(seen=None)      "), ("penalty", "argmax_penalty_rows / logprob_rows(seen, 1.05, mark)")):
        p = r[name]
        print(f"  {what} {p['argmax_us']:8.2f} / {p['logprob_us']:8.2f} us   ratio {p['ratio']:.3f}   runs {p['argmax_runs']} / {p['logprob_runs']}")
    print(f"  ids equal to argmax_penalty_rows: {r['ids_equal_of_4x']}")
    out = dict(workload="logprob_step", envs=a.envs, iters=a.iters, repeats=a.repeats, kernel=r)
    if not a.skip_graph:
        gr = out["graph"] = graph_rows(a.envs, a.graph_steps, a.repeats, dev)
        print(f"decode + latents graph, {gr['envs']} envs x {gr['prompt_tokens']} prompt tokens, full depth: token_logprobs off {gr['off_ms']} ms  "
              f"on {gr['on_ms']} ms  ratio {gr['ratio']}  tokens equal {gr['tokens_equal']}   runs {gr['off_runs']} / {gr['on_runs']}")
    if not a.skip_score:
        sc = out["score"] = score_rows(a.envs, a.repeats, dev)
        print(f"score_answers, {sc['prompts']} prompts x {sc['candidates']} candidates x {sc['tokens']} tokens ({sc['groups']} prefill groups of "
              f"{sc['prompts']} pairs, {sc['rows_per_group']} answer rows each): per group prefill {sc['prefill_group_ms']} ms, gather + norm + lm_head "
              f"{sc['lm_head_group_ms']} ms, logprob_rows {sc['logprob_kernel_group_us']} us; all groups {sc['total_ms_est']} ms")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
