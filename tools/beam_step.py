"""Time the beam-search launches of System-2 decoding against the selections beside them, and generate(num_beams=K) against the sampled
shared-prompt call, in one process on one GPU.

    python tools/beam_step.py [--prompts 7] [--K 4] [--new 8] [--prompt 920] [--iters 128] [--repeats 5] [--skip-call]

1. ops.beam_topm_rows at M = 8 and M = 24 against ops.logprob_rows and ops.sample_rows (T 0.7, top-k 50, top-p 0.9), all at --prompts x --K rows of
   152064 fp32 logits with a seen set of --prompt tokens per row and penalty 1.05: `--iters` launches between two device events, the kernels
   alternating, `--repeats` times, median and all runs. Every launch of a loop reads ANOTHER of 32 copies of the logits, as in tools/sample_step.py.
   ops.beam_step and ops.beam_reorder (full depth, 4 tail rows) are timed the same way on their own buffers.
2. generate(num_beams=K) against generate(do_sample=True, num_return_sequences=K, share_prefix=True) on one engine at the full depth of the 7B
   geometry (wall clock around the call, device synchronised, alternating), and one single-token pass with its selection (and, for beams,
   reorder) launches on each path (device events around decode(state, 2)).
Ratios are printed, not asserted. Prints a table and one JSON line."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from internnav_amd import ops, runtime, synthetic  # noqa: E402
from internnav_amd.policy import InternVLAN1ForCausalLM, generation_config_from_hf  # noqa: E402
from internnav_amd.qwen_vl import QwenVLEngine  # noqa: E402

VOCAB = 152064
med = statistics.median


def _events_us(fns, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(iters):
        fns[i % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def _event_ms(fn):
    return _events_us([fn], 1) / 1e3


def _wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _r(v, n=2):
    return [round(x, n) for x in v]


def kernel_rows(R, K, S, iters, repeats, dev):
    g = torch.Generator(device=dev).manual_seed(R)
    copies = 32
    xs = [torch.randn(R, VOCAB, generator=g, device=dev) * 4 for _ in range(copies)]
    ids = torch.randint(0, VOCAB, (R, S), generator=g, device=dev, dtype=torch.int32)
    ldw = ((VOCAB + 31) // 32 + 3) // 4 * 4
    seen = torch.zeros(R, ldw, dtype=torch.uint32, device=dev)
    ops.token_seen_set(seen, ids, torch.full((R,), S, dtype=torch.int32, device=dev), VOCAB)
    u = torch.rand(R, generator=g, device=dev)
    tok = torch.empty(R, dtype=torch.int32, device=dev)
    lp, mg = torch.empty(R, device=dev), torch.empty(R, device=dev)
    run = -torch.rand(R, generator=g, device=dev) * 5
    s_lp, s_smp = seen.clone(), seen.clone()
    loops = {"logprob_rows": [lambda x=x: ops.logprob_rows(x, tok, lp, mg, seen=s_lp, penalty=1.05, mark=True) for x in xs],
             "sample_50_0.9": [lambda x=x: ops.sample_rows(x, u, tok, lp, temperature=0.7, top_k=50, top_p=0.9, seen=s_smp, penalty=1.05, mark=True) for x in xs]}
    for M in (8, 24):
        cs, ct = torch.empty(R, M, device=dev), torch.empty(R, M, dtype=torch.int32, device=dev)
        loops[f"beam_topm_M{M}"] = [lambda x=x, cs=cs, ct=ct: ops.beam_topm_rows(x, run, cs, ct, seen=seen, penalty=1.05) for x in xs]
    # the bookkeeping and the re-parenting on buffers of their own: K beams, M = 2 K candidates, 8 history columns; 28 layers of 4 tail rows
    M, T, B = 2 * K, 8, R // K
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731
    st = SimpleNamespace(K=K, eos=torch.tensor([VOCAB - 1], dtype=torch.int32, device=dev), run_score=z(R, dt=torch.float32), next_tok=z(R), parent=z(R),
                         hist=z(2, R, T), ts=z(2, R, T, dt=torch.float32), fin_tok=z(R, T), fin_ts=z(R, T, dt=torch.float32), fin_score=z(R, dt=torch.float32),
                         fin_len=z(R), fin_flag=z(R), heur=z(B), done=z(B))
    cs, ct = torch.empty(R, M, device=dev), torch.empty(R, M, dtype=torch.int32, device=dev)
    ops.beam_topm_rows(xs[0], run, cs, ct)
    loops["beam_step"] = [lambda j=j: ops.beam_step(cs, ct, st, j, T) for j in (0, 1, 2, 3)]
    kv_w, layers, Tt = 1024, 28, 8
    sets = [[torch.zeros(R * Tt, kv_w, dtype=torch.bfloat16, device=dev) for _ in range(layers)] for _ in range(2)]
    base = torch.tensor([[t.data_ptr() for t in s_] for s_ in sets], dtype=torch.int64, device=dev)
    seen2 = seen.clone()
    par = torch.arange(R, dtype=torch.int32, device=dev).view(B, K).flip(1).reshape(-1).contiguous()
    loops["beam_reorder"] = [lambda f=f: ops.beam_reorder(par, base[f], base[1 - f], T=Tt, t=4, row_bytes=kv_w * 2, seen_src=(seen, seen2)[f],
                                                          seen_dst=(seen, seen2)[1 - f], next_tok=tok, n=VOCAB) for f in (0, 1)]
    for fns in loops.values():
        _events_us(fns, len(fns))
    runs = {name: [] for name in loops}
    for _ in range(repeats):
        for name, fns in loops.items():
            runs[name].append(_events_us(fns, iters))
    m = {name: med(v) for name, v in runs.items()}
    out = dict(rows=R, n=VOCAB, seen_per_row=S, logits_copies=copies)
    for name in loops:
        out[name] = dict(us=round(m[name], 2), vs_logprob_rows=round(m[name] / m["logprob_rows"], 3), vs_sample_rows=round(m[name] / m["sample_50_0.9"], 3),
                         runs=_r(runs[name]))
    return out


def call_rows(B, K, n_new, repeats, dev):
    cfg = synthetic.QWEN_N1_CFG
    inp = synthetic.qwen_inputs(B, 4, seed=0, cfg=cfg, n_text=64, n_tail=8)
    ids, grid = inp["input_ids"], inp["grid_thw"]
    pv = inp["pixel_values"].to(dev, torch.bfloat16)
    Sp, steps = ids.shape[1], 32
    eng = QwenVLEngine(synthetic.LazyDeviceWeights(synthetic.qwen_spec(cfg), dev, seed=0), cfg, dev, max_seqs=B,
                       max_seq_len=(Sp + steps + 8 + 63) // 64 * 64, max_patches=pv.shape[0])
    model = InternVLAN1ForCausalLM.__new__(InternVLAN1ForCausalLM)      # the System-2 surface alone: no System-1 head is built
    model.qwen, model.device, model._gen = eng, dev, None
    model.generation_config = generation_config_from_hf(None, cfg["eos_token_id"])
    model._sample_gen = torch.Generator(device="cpu").manual_seed(0)
    gkw = dict(input_ids=ids, pixel_values=pv, image_grid_thw=grid, max_new_tokens=n_new, eos_token_id=-1, repetition_penalty=1.05)
    calls = {"sampled": lambda: model.generate(**gkw, do_sample=True, temperature=1.0, top_k=0, top_p=1.0, seed=1, num_return_sequences=K, share_prefix=True),
             "beams": lambda: model.generate(**gkw, num_beams=K, num_return_sequences=K)}
    for fn in calls.values():
        _wall_ms(fn)
    runs = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():
            runs[k].append(_wall_ms(fn))
    out = dict(prompts=B, K=K, new_tokens=n_new, prompt_tokens=int(Sp), sampled_ms=round(med(runs["sampled"]), 3), beams_ms=round(med(runs["beams"]), 3),
               ratio=round(med(runs["beams"]) / med(runs["sampled"]), 3), sampled_runs=_r(runs["sampled"], 3), beams_runs=_r(runs["beams"], 3))
    # one single-token pass of B * K rows with its selection launches (and the reorder in front of it) on each path
    plens = np.full(B, Sp, dtype=np.int64)
    u = torch.rand(steps, B * K, generator=torch.Generator().manual_seed(2), dtype=torch.float32).to(dev)
    st_s = eng.prefill(ids, pv, grid, seq_lens=plens, repetition_penalty=1.05, sampling=dict(temperature=1.0, top_k=0, top_p=1.0, u=u, K=K, share_prefix=True))
    eng.decode(st_s, 1)
    shared = eng._shared                                             # (both states live on one set of twins: the beam state is made second and timed
    st_b = eng.prefill(ids, pv, grid, seq_lens=plens, repetition_penalty=1.05, beam=dict(K=K, max_new_tokens=steps, eos=(-1,)))      # on tails it owns)
    eng.decode(st_b, 1)
    assert eng._shared is shared
    passes = {"sampled": [], "beams": []}
    for st in (st_s, st_b):
        _event_ms(lambda: eng.decode(st, 2))
    for _ in range(repeats):
        for name, st in (("sampled", st_s), ("beams", st_b)):
            passes[name].append(_event_ms(lambda: eng.decode(st, 2)))
    out["pass"] = dict(rows=B * K, sampled_ms=round(med(passes["sampled"]), 3), beams_ms=round(med(passes["beams"]), 3),
                       ratio=round(med(passes["beams"]) / med(passes["sampled"]), 3), sampled_runs=_r(passes["sampled"], 3), beams_runs=_r(passes["beams"], 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, default=7)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--new", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=920)
    ap.add_argument("--iters", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-call", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device:", runtime.require_gfx950(), file=sys.stderr)
    R = a.prompts * a.K
    r = kernel_rows(R, a.K, a.prompt, a.iters, a.repeats, dev)
    print(f"selection kernels, {r['rows']} rows x {r['n']} logits, {r['seen_per_row']} seen ids per row, penalty 1.05 ({a.iters} launches x {a.repeats}, median)")
    for name in ("logprob_rows", "sample_50_0.9", "beam_topm_M8", "beam_topm_M24", "beam_step", "beam_reorder"):
        p = r[name]
        print(f"  {name:16s} {p['us']:9.2f} us   {p['vs_logprob_rows']:7.3f} x logprob_rows   {p['vs_sample_rows']:7.3f} x sample_rows   runs {p['runs']}")
    out = dict(workload="beam_step", prompts=a.prompts, K=a.K, iters=a.iters, repeats=a.repeats, kernel=r)
    if not a.skip_call:
        c = out["call"] = call_rows(a.prompts, a.K, a.new, a.repeats, dev)
        print(f"generate, {c['prompts']} prompts x {c['K']} x {c['new_tokens']} new tokens, {c['prompt_tokens']} prompt tokens, full depth ({a.repeats} alternating runs, median)")
        print(f"  do_sample, num_return_sequences={c['K']}, share_prefix   {c['sampled_ms']:9.3f} ms   runs {c['sampled_runs']}")
        print(f"  num_beams={c['K']}                                      {c['beams_ms']:9.3f} ms   runs {c['beams_runs']}   beams / sampled {c['ratio']:.3f}")
        p = c["pass"]
        print(f"one single-token pass of {p['rows']} rows, layers + selection (+ reorder) launches (device events): sampled {p['sampled_ms']} ms, beams {p['beams_ms']} ms, "
              f"beams / sampled {p['ratio']:.3f}; runs {p['sampled_runs']} / {p['beams_runs']}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
