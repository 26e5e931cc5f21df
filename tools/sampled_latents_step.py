"""Time generate_latents on chosen rows of a SAMPLED generate() - continuing the state that call left (QwenVLEngine.latents_behind over
ops.attention_prefix_tail) on the shared-prefix and on the fan-out path - against the re-run path (ViT + prefill of every requested row), at the
full depth of the 7B geometry, in one process on one GPU (random weights, lazily materialised).

    python tools/sampled_latents_step.py [--prompts 7] [--K 4] [--new 8] [--repeats 5] [--iters 56]

--prompts prompts of 4 frames on ONE engine of --prompts x --K cache slots (what the fan-out path needs):
1. generate(--new tokens, num_return_sequences=--K) once per path; then wall time (host clock around the call, device synchronised) of
   generate_latents for ONE chosen row per prompt: the re-run on those rows, the shared-prefix state, the fan-out state, alternating, `--repeats`
   times after one warm-up of each: median and all runs. The re-run rewrites the first --prompts cache slots: the two sampled states keep their
   GEOMETRY (equal prompt lengths), which is all a timing needs; their values are compared with the re-run's BEFORE it first runs;
2. the attention launch alone: ops.attention_prefix_tail for --prompts pairs x (1 + N_QUERY) rows behind the prompt and --new - 1 tail keys against
   ops.attention_prefix on slots that hold [prompt | tail], `--iters` launches between two device events, alternating, every launch on another
   layer's cache and tail;
3. the device memory one call on the shared-prefix state allocates (peak above what was allocated before it).
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
from internnav_amd.policy import InternVLAN1ForCausalLM, generation_config_from_hf  # noqa: E402
from internnav_amd.qwen_vl import QwenVLEngine  # noqa: E402

BF16 = torch.bfloat16
med = statistics.median


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


def _r(v, n=3):
    return [round(x, n) for x in v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, default=7)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--new", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=56)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device:", runtime.require_gfx950(), file=sys.stderr)
    cfg = synthetic.QWEN_N1_CFG
    B, K, n_new = a.prompts, a.K, a.new
    inp = synthetic.qwen_inputs(B, 4, seed=0, cfg=cfg, n_text=64, n_tail=8)
    ids, grid = inp["input_ids"], inp["grid_thw"]
    pv = inp["pixel_values"].to(dev, BF16)
    Sp = ids.shape[1]
    eng = QwenVLEngine(synthetic.LazyDeviceWeights(synthetic.qwen_spec(cfg), dev, seed=0), cfg, dev, max_seqs=B * K,
                       max_seq_len=(Sp + n_new + 8 + 63) // 64 * 64, max_patches=pv.shape[0])
    nq = eng.latent_q.shape[0]
    model = InternVLAN1ForCausalLM.__new__(InternVLAN1ForCausalLM)      # the System-2 surface alone: no System-1 head is built
    model.qwen, model.device, model._gen = eng, dev, None
    model.generation_config = generation_config_from_hf(None, cfg["eos_token_id"])
    model._sample_gen = torch.Generator(device="cpu").manual_seed(0)
    gkw = dict(input_ids=ids, pixel_values=pv, image_grid_thw=grid, max_new_tokens=n_new, eos_token_id=-1, do_sample=True, temperature=1.0, top_k=0,
               top_p=1.0, repetition_penalty=1.05, num_return_sequences=K)
    rows = [b * K + b % K for b in range(B)]                            # one chosen row per prompt

    # ---- 1. the three ways to the latents of the chosen rows
    gens, seqs = {}, {}
    seqs[False] = model.generate(**gkw, seed=1, share_prefix=False)
    gens[False] = model._gen
    # (the shared state last: its prompt slots are intact for the comparison; a seed whose chosen rows hold no vision marker, which the re-run
    #  would read as an image)
    special = torch.tensor([cfg[k] for k in ("image_token_id", "traj_token_id", "vision_start_id", "vision_end_id")], device=dev)
    for seed in range(1, 9):
        seqs[True] = model.generate(**gkw, seed=seed, share_prefix=True)
        gens[True] = model._gen
        clean = not bool(torch.isin(seqs[True][rows, Sp:], special).any())
        if clean:
            break
    assert clean, "eight seeds in a row drew a vision marker in a chosen row"

    def behind(share):
        model._gen = gens[share]                                        # (the re-run drops it: a host dict, put back for the next timing)
        return model.generate_latents(seqs[share], None, grid, rows=rows)

    def rerun():
        return model.generate_latents(seqs[True][rows], pv, grid)        # --prompts rows, each with its own 4 frames: another row count -> the re-run

    lat_sh = behind(True)
    lat_rr = rerun()
    torch.cuda.synchronize()
    dist = float((lat_sh.float() - lat_rr.float()).abs().mean() / lat_rr.float().pow(2).mean().sqrt())
    runs = dict(rerun=[], shared=[], fan=[])
    fns = dict(rerun=rerun, shared=lambda: behind(True), fan=lambda: behind(False))
    for name in fns:
        _wall_ms(fns[name])
    for _ in range(a.repeats):
        for name in fns:
            runs[name].append(_wall_ms(fns[name])[0])
    m_ = {k: med(v) for k, v in runs.items()}
    out = dict(workload="sampled_latents_step", prompts=B, K=K, new_tokens=n_new, prompt_tokens=int(Sp), rows=len(rows), pass_rows=len(rows) * (1 + nq),
               repeats=a.repeats, rerun_ms=round(m_["rerun"], 3), shared_ms=round(m_["shared"], 3), fan_ms=round(m_["fan"], 3),
               shared_over_rerun=round(m_["shared"] / m_["rerun"], 4), fan_over_rerun=round(m_["fan"] / m_["rerun"], 4),
               rerun_runs=_r(runs["rerun"]), shared_runs=_r(runs["shared"]), fan_runs=_r(runs["fan"]),
               shared_vs_rerun_mean_abs_over_rms=round(dist, 5))

    # ---- 3. memory of one call on the shared-prefix state
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = behind(True)
    torch.cuda.synchronize()
    out["memory"] = dict(peak_added_bytes=int(torch.cuda.max_memory_allocated() - base), output_bytes=int(res.numel() * res.element_size()))
    del res

    # ---- 2. the attention launch alone (slot p holds prompt p; its rows Sp .. Sp + tl - 1 are overwritten with pair p's tail: the materialised copy)
    nh, nkv, hd = eng.nh, eng.nkv, eng.hd
    P, m, tl, Tt = B, 1 + nq, n_new - 1, n_new
    gq = torch.Generator(device=dev).manual_seed(3)
    qkv = torch.randn(P * m, eng.qkv_w, generator=gq, device=dev).to(BF16)
    q4 = qkv[:, : nh * hd].view(P, m, nh, hd)
    k4 = qkv[:, nh * hd:(nh + nkv) * hd].view(P, m, nkv, hd)
    v4 = qkv[:, (nh + nkv) * hd:].view(P, m, nkv, hd)
    tails = [torch.randn(P * Tt, eng.kv_w, generator=gq, device=dev).to(BF16).view(P, Tt, 2, nkv, hd) for _ in eng.layers]
    caches = [L["kv"].view(eng.B_max, eng.S_max, 2, nkv, hd) for L in eng.layers]
    for c5, t5 in zip(caches, tails):
        c5[:P, Sp:Sp + tl] = t5[:, :tl]
    i32 = lambda v: torch.tensor(np.asarray(v), dtype=torch.int32, device=dev)
    slot, pfx, pfx_mat, suf, trow, tlen = i32(np.arange(P)), i32(np.full(P, Sp)), i32(np.full(P, Sp + tl)), i32(np.full(P, m)), i32(np.arange(P)), i32(np.full(P, tl))
    o1, o2 = (torch.empty(P, m, nh, hd, dtype=BF16, device=dev) for _ in range(2))
    fa = [lambda c5=c5, t5=t5: ops.attention_prefix_tail(q4, k4, v4, c5[:, :, 0], c5[:, :, 1], slot, pfx, suf, t5[:, :, 0], t5[:, :, 1], trow, tlen, out=o1,
                                                         max_pfx=int(Sp), max_tail=tl) for c5, t5 in zip(caches, tails)]
    fb = [lambda c5=c5: ops.attention_prefix(q4, k4, v4, c5[:, :, 0], c5[:, :, 1], slot, pfx_mat, suf, out=o2, max_pfx=int(Sp + tl)) for c5 in caches]
    fa[0](), fb[0]()
    torch.cuda.synchronize()
    d_att = float((o1.float() - o2.float()).abs().max())
    _events_us(fa, len(fa)), _events_us(fb, len(fb))
    ta, tb = [], []
    for _ in range(a.repeats):
        ta.append(_events_us(fa, a.iters))
        tb.append(_events_us(fb, a.iters))
    out["attention"] = dict(pairs=P, rows=m, prefix=int(Sp), tail=tl, layers_cycled=len(caches), tail_us=round(med(ta), 2), materialised_us=round(med(tb), 2),
                            ratio=round(med(ta) / med(tb), 3), tail_runs=_r(ta, 2), materialised_runs=_r(tb, 2), max_abs_difference=round(d_att, 5))

    print(f"generate_latents for {len(rows)} chosen rows (one per prompt) after generate({B} prompts x {K} returned sequences x {n_new} new tokens), {Sp} prompt "
          f"tokens, full depth ({a.repeats} alternating runs, median)")
    print(f"  re-run (ViT + prefill of {len(rows)} rows)        {out['rerun_ms']:9.3f} ms   runs {out['rerun_runs']}")
    print(f"  shared-prefix state ({out['pass_rows']} rows, 1 pass)  {out['shared_ms']:9.3f} ms   runs {out['shared_runs']}   / re-run {out['shared_over_rerun']:.4f}")
    print(f"  fan-out state ({out['pass_rows']} rows, 1 pass)        {out['fan_ms']:9.3f} ms   runs {out['fan_runs']}   / re-run {out['fan_over_rerun']:.4f}")
    print(f"  shared-prefix latents against the re-run's on the same rows: mean |difference| / rms = {out['shared_vs_rerun_mean_abs_over_rms']}")
    at = out["attention"]
    print(f"attention launch alone, {at['pairs']} pairs x {at['rows']} rows behind {at['prefix']} cached + {at['tail']} tail keys ({a.iters} launches x {a.repeats}, "
          f"median): attention_prefix_tail {at['tail_us']} us, attention_prefix on the materialised copy {at['materialised_us']} us, ratio {at['ratio']}; "
          f"max |difference| {at['max_abs_difference']}; runs {at['tail_runs']} / {at['materialised_runs']}")
    mem = out["memory"]
    print(f"device memory one call on the shared-prefix state adds at its peak: {mem['peak_added_bytes']} bytes (its output: {mem['output_bytes']} bytes)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
