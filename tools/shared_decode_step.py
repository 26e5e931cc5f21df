"""Time generate(do_sample=True, num_return_sequences=K) behind shared prompts (share_prefix=True) against the KV fan-out path at the full depth of
the 7B geometry, in one process on one GPU (random weights, lazily materialised).

    python tools/shared_decode_step.py [--prompts 7] [--K 4] [--new 8] [--wide-K 9] [--repeats 5] [--iters 56]

--prompts prompts of 4 frames on ONE engine of --prompts x --K cache slots (what the fan-out path needs; the shared path uses the first --prompts):
1. wall time (host clock around the call, device synchronised) of generate(--new tokens, num_return_sequences=--K) on the fan-out path and with
   share_prefix=True, alternating, `--repeats` times after one warm-up of each: median and all runs;
2. one single-token pass of --prompts x --K rows (all layers + the selection step) on each path: device events around decode(state, 2),
   alternating, one warm-up;
3. the attention launch alone: ops.attention_shared (prompts in place, 4-token tails) against ops.attention on the fanned-out cache that holds
   the same keys, `--iters` launches between two device events, alternating, every launch on another layer's cache and tail;
4. generate with --wide-K returned sequences per prompt on the shared path (beyond the slots of this engine), and the bytes of its tails and
   twin buffers beside the bytes of the cache slots the fan-out path would need for as many rows.
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


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


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
    ap.add_argument("--wide-K", type=int, default=9)
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
    steps = 32                                                       # rows of the uniform table of part 2 (= tail rows of its shared state)
    eng = QwenVLEngine(synthetic.LazyDeviceWeights(synthetic.qwen_spec(cfg), dev, seed=0), cfg, dev, max_seqs=B * K,
                       max_seq_len=(Sp + steps + 8 + 63) // 64 * 64, max_patches=pv.shape[0])
    model = InternVLAN1ForCausalLM.__new__(InternVLAN1ForCausalLM)      # the System-2 surface alone: no System-1 head is built
    model.qwen, model.device, model._gen = eng, dev, None
    model.generation_config = generation_config_from_hf(None, cfg["eos_token_id"])
    model._sample_gen = torch.Generator(device="cpu").manual_seed(0)
    gkw = dict(input_ids=ids, pixel_values=pv, image_grid_thw=grid, max_new_tokens=n_new, eos_token_id=-1, do_sample=True, temperature=1.0, top_k=0,
               top_p=1.0, repetition_penalty=1.05, seed=1)

    # ---- 1. the two paths of the public call
    runs = {False: [], True: []}
    for share in (False, True):
        _wall_ms(lambda: model.generate(**gkw, num_return_sequences=K, share_prefix=share))
    for _ in range(a.repeats):
        for share in (False, True):
            t, _ = _wall_ms(lambda: model.generate(**gkw, num_return_sequences=K, share_prefix=share))
            runs[share].append(t)
    out = dict(workload="shared_decode_step", prompts=B, K=K, new_tokens=n_new, prompt_tokens=int(Sp), repeats=a.repeats,
               fan_out_ms=round(med(runs[False]), 3), shared_ms=round(med(runs[True]), 3), ratio=round(med(runs[True]) / med(runs[False]), 3),
               fan_out_runs=_r(runs[False]), shared_runs=_r(runs[True]))

    # ---- 4. more returned sequences than the engine has slots (measured here, while the tails are still those of --new tokens)
    Kw = a.wide_K
    _wall_ms(lambda: model.generate(**gkw, num_return_sequences=Kw, share_prefix=True))
    wide = [_wall_ms(lambda: model.generate(**gkw, num_return_sequences=Kw, share_prefix=True))[0] for _ in range(a.repeats)]
    sh = eng._shared
    nbytes = lambda t: t.numel() * t.element_size()
    twins = sum(nbytes(getattr(sh, n)) for n in ("logits", "next_tok", "seen", "xl", "hl", "_smp_lp"))
    tail_b = sum(nbytes(t) for t in sh.tails)
    slot_b = len(eng.layers) * eng.S_max * eng.kv_w * 2
    out["wide"] = dict(K=Kw, rows=B * Kw, shared_ms=round(med(wide), 3), shared_runs=_r(wide), buffer_rows=sh.rows, tail_rows=sh.T, tail_bytes=tail_b,
                       twin_bytes=twins, slot_bytes=slot_b, fan_out_slots_bytes=B * Kw * slot_b)

    # ---- 2. one single-token pass of B * K rows (layers + selection) on each path
    plens = np.full(B, Sp, dtype=np.int64)
    u = torch.rand(steps, B * K, generator=torch.Generator().manual_seed(2), dtype=torch.float32).to(dev)
    spec = dict(temperature=1.0, top_k=0, top_p=1.0, u=u, K=K)
    passes = {False: [], True: []}
    states = {}
    for share in (True, False):                                      # (the fan-out state last: part 3 reads the fanned-out cache it leaves)
        st = eng.prefill(ids, pv, grid, seq_lens=plens, repetition_penalty=1.05, sampling=dict(spec, **({"share_prefix": True} if share else {})))
        eng.decode(st, 1)                                            # the first draw; the fan-out / the tile plan
        states[share] = st
    # the shared state reads slots 0 .. B - 1, which the fan-out rewrote (slot 0 = prompt 0, slot 1 = prompt 0 ...): equal prompt LENGTHS keep
    # its geometry valid, which is all a timing needs
    for share in (False, True):
        _event_ms(lambda: eng.decode(states[share], 2))
    for _ in range(a.repeats):
        for share in (False, True):
            passes[share].append(_event_ms(lambda: eng.decode(states[share], 2)))
    out["pass"] = dict(rows=B * K, fan_out_ms=round(med(passes[False]), 3), shared_ms=round(med(passes[True]), 3),
                       ratio=round(med(passes[True]) / med(passes[False]), 3), fan_out_runs=_r(passes[False]), shared_runs=_r(passes[True]))

    # ---- 3. the attention launch alone (slot b * K + c holds prompt b: the shared launch reads slot b * K, the decode kernel all of them)
    nh, nkv, hd = eng.nh, eng.nkv, eng.hd
    R, Tt, tl = B * K, 8, 4
    gq = torch.Generator(device=dev).manual_seed(3)
    q = torch.randn(R, eng.qkv_w, generator=gq, device=dev).to(BF16)[:, : nh * hd]
    q3, q4 = q.view(R, nh, hd), q.view(R, 1, nh, hd)
    tails = [torch.randn(R * Tt, eng.kv_w, generator=gq, device=dev).to(BF16) for _ in eng.layers]
    caches = [L["kv"].view(eng.B_max, eng.S_max, 2, nkv, hd) for L in eng.layers]
    for c5, t in zip(caches, tails):                                 # the same tail keys behind every slot's prompt
        c5[:R, Sp:Sp + tl] = t.view(R, Tt, 2, nkv, hd)[:, :tl]
    i32 = lambda v: torch.tensor(np.asarray(v), dtype=torch.int32, device=dev)
    tiles, owner = ops.attention_shared_plan(np.repeat(np.arange(B), K), nh // nkv)
    tile_rows, tile_slot, tile_pfx, tail_len = i32(tiles), i32(owner * K), i32(np.full(owner.size, Sp)), i32(np.full(R, tl))
    k_len = i32(np.full(R, Sp + tl))
    o1, o2 = torch.empty(R, nh, hd, dtype=BF16, device=dev), torch.empty(R, 1, nh, hd, dtype=BF16, device=dev)
    fa = [lambda c5=c5, t=t.view(R, Tt, 2, nkv, hd): ops.attention_shared(q3, t[:, :, 0], t[:, :, 1], c5[:, :, 0], c5[:, :, 1], tile_rows, tile_slot,
                                                                           tile_pfx, tail_len, out=o1, max_pfx=int(Sp)) for c5, t in zip(caches, tails)]
    fb = [lambda c5=c5: ops.attention(q4, c5[:R, : Sp + tl, 0], c5[:R, : Sp + tl, 1], causal=True, out=o2, k_len=k_len) for c5 in caches]
    fa[0](), fb[0]()
    torch.cuda.synchronize()
    d_att = float((o1.float() - o2.view(R, nh, hd).float()).abs().max())
    _events_us(fa, len(fa)), _events_us(fb, len(fb))
    ta, tb = [], []
    for _ in range(a.repeats):
        ta.append(_events_us(fa, a.iters))
        tb.append(_events_us(fb, a.iters))
    out["attention"] = dict(rows=R, tiles=int(tiles.shape[0]), prefix=int(Sp), tail=tl, layers_cycled=len(caches), shared_us=round(med(ta), 2),
                            decode_us=round(med(tb), 2), ratio=round(med(ta) / med(tb), 3), shared_runs=_r(ta, 2), decode_runs=_r(tb, 2),
                            max_abs_difference=round(d_att, 5))

    print(f"generate, {B} prompts x {K} returned sequences x {n_new} new tokens, {Sp} prompt tokens, full depth ({a.repeats} alternating runs, median)")
    print(f"  fan-out (engine of {B * K} slots) {out['fan_out_ms']:9.3f} ms   runs {out['fan_out_runs']}")
    print(f"  share_prefix=True            {out['shared_ms']:9.3f} ms   runs {out['shared_runs']}   shared / fan-out {out['ratio']:.3f}")
    p = out["pass"]
    print(f"one single-token pass of {p['rows']} rows, layers + selection (device events): fan-out {p['fan_out_ms']} ms, shared {p['shared_ms']} ms, "
          f"shared / fan-out {p['ratio']:.3f}; runs {p['fan_out_runs']} / {p['shared_runs']}")
    at = out["attention"]
    print(f"attention launch alone, {at['rows']} rows in {at['tiles']} tiles behind {at['prefix']} cached keys + {at['tail']} tail keys ({a.iters} launches x "
          f"{a.repeats}, median): attention_shared {at['shared_us']} us, ops.attention on the fanned-out cache {at['decode_us']} us, ratio {at['ratio']}; "
          f"max |difference| {at['max_abs_difference']}; runs {at['shared_runs']} / {at['decode_runs']}")
    w = out["wide"]
    print(f"share_prefix=True at K = {w['K']} ({w['rows']} rows on {B * K} slots): {w['shared_ms']} ms, runs {w['shared_runs']}; tails {w['tail_bytes'] / 2**20:.1f} MiB "
          f"({w['buffer_rows']} rows x {w['tail_rows']} tokens x {len(eng.layers)} layers) + twin buffers {w['twin_bytes'] / 2**20:.1f} MiB, against "
          f"{w['fan_out_slots_bytes'] / 2**20:.1f} MiB of cache for {w['rows']} slots ({w['slot_bytes'] / 2**20:.1f} MiB each)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
