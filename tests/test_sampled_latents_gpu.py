"""GPU: generate_latents after a SAMPLED generate() on the 2-layer test model - the latent queries of chosen returned rows continue the state the
call left (the prompt in its cache slot, the row's own answer K/V in its slot on the fan-out path or in its tail on the shared-prefix path,
QwenVLEngine.latents_behind over ops.attention_prefix_tail) instead of re-running prompt and ViT: against the fp32 oracle on every row's own
prompt + kept answer, with no prefill and no vision pass inside the call, nothing written, repeatable, and the greedy path what it was."""
import functools

import numpy as np
import pytest
import torch

from internnav_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, SEQS, N_P, N_NEW = 3, 6, 2, 4


@pytest.fixture(scope="module")
def setup(built_lib):
    from internnav_amd.policy import InternVLAN1ForCausalLM

    cfg = S.QWEN_TEST_CFG
    sd = {k: v.to(torch.bfloat16) for k, v in S.materialize(S.n1_full_spec(cfg, "nextdit_async"), 5).items()}
    inp = S.qwen_inputs(B, 1, seed=33, cfg=cfg, n_text=20, n_tail=12)
    kw = dict(device=DEV, max_envs=SEQS, num_history=3, resize_w=280, resize_h=280, max_seq_len=512, max_patches=SEQS * (inp["pixel_values"].shape[0] // B))
    m = InternVLAN1ForCausalLM(sd, cfg, "nextdit_async", **kw)
    # the 2 ragged prompts of test_sample_shared_gpu.py: prompt 1 loses its last three tokens
    per_img, Sp = inp["pixel_values"].shape[0] // B, inp["input_ids"].shape[1]
    plens = [Sp, Sp - 3]
    ids = inp["input_ids"][:N_P].clone()
    mask = torch.ones(N_P, Sp, dtype=torch.long)
    ids[1, plens[1]:], mask[1, plens[1]:] = 0, 0
    rag = dict(input_ids=ids, attention_mask=mask, pixel_values=inp["pixel_values"][: N_P * per_img], image_grid_thw=inp["grid_thw"][:N_P], eos_token_id=-1)
    qsd = {k: v.float().cpu() for k, v in sd.items() if not k.startswith("model.traj_dit") and not k.startswith("model.rgb_")}
    return dict(m=m, cfg=cfg, sd=sd, kw=kw, rag=rag, plens=plens, Sp=Sp, per_img=per_img, qsd=qsd, oracle={})


def _oracle(s, qsd, key, row_ids, b):
    """fp32 oracle latents [N_QUERY, H] of ONE row: its own prompt + kept answer (computed once per distinct row and weight set)"""
    from oracle import qwen_vl as o_q

    k = (key, b, tuple(row_ids.tolist()))
    if k not in s["oracle"]:
        rag, per = s["rag"], s["per_img"]
        with torch.no_grad():
            s["oracle"][k] = o_q.generate_latents(qsd, s["cfg"], row_ids[None], rag["pixel_values"][b * per:(b + 1) * per], rag["image_grid_thw"][b:b + 1])[0]
    return s["oracle"][k]


def _draw(s, m, K, share, eos_row=None):
    """test data: K sampled answers per prompt free of image / vision markers (the re-run path and the oracle would read them as images: the seed
    loop of test_sample_shared_gpu.py). eos_row: the first token that row draws plays EOS in a second call with the same seed - the same draws,
    and that row keeps ONE token. -> (result, kept answer tokens per row)"""
    cfg, rag, plens = s["cfg"], s["rag"], s["plens"]
    special = torch.tensor([cfg[k] for k in ("image_token_id", "traj_token_id", "vision_start_id", "vision_end_id")], device=DEV)
    for seed in range(8):
        kw = dict(max_new_tokens=N_NEW, return_dict_in_generate=True, do_sample=True, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0,
                  num_return_sequences=K, seed=seed, share_prefix=share)
        res = m.generate(**rag, **kw)
        ans = [res.sequences[r, plens[r // K]: plens[r // K] + N_NEW] for r in range(N_P * K)]
        if any(bool(torch.isin(t, special).any()) for t in ans):
            continue
        if eos_row is None:
            return res, [N_NEW] * (N_P * K)
        eos = int(ans[eos_row][0])
        res2 = m.generate(**dict(rag, eos_token_id=eos), **kw)
        kept = [int((t == eos).nonzero()[0]) + 1 if bool((t == eos).any()) else N_NEW for t in ans]
        for r in range(N_P * K):
            L = plens[r // K]
            assert torch.equal(res2.sequences[r, L:L + kept[r]], ans[r][: kept[r]]), "the same seed drew other tokens"
        assert kept[eos_row] == 1
        return res2, kept
    pytest.fail("eight seeds in a row drew a vision marker")


class _Count:
    """wraps an engine method: counts the calls, passes them on"""

    def __init__(self, eng, name):
        self.eng, self.name, self.fn, self.n = eng, name, getattr(eng, name), 0
        setattr(eng, name, self)

    def __call__(self, *a, **k):
        self.n += 1
        return self.fn(*a, **k)

    def restore(self):
        delattr(self.eng, self.name)                                       # the instance attribute goes, the class's method is back


def _snapshot(eng):
    torch.cuda.synchronize()
    return [L["kv"].clone() for L in eng.layers] + ([t.clone() for t in eng._shared.tails] if eng._shared is not None else [])


def _assert_untouched(eng, before, what):
    torch.cuda.synchronize()
    now = [L["kv"] for L in eng.layers] + (list(eng._shared.tails) if eng._shared is not None else [])
    assert len(now) == len(before)
    for i, (a, b) in enumerate(zip(now, before)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{what}: cache / tail tensor {i} was written"


def _check_rows(s, qsd, key, lat, rows, res, kept, K, label):
    """mean |err| < 1e-2 x rms(ref) per row (the bound test_qwen_gpu.py holds the greedy latents to) -> worst ratio"""
    worst = 0.0
    for j, r in enumerate(rows):
        b = r // K
        ref = _oracle(s, qsd, key, res.sequences[r, : s["plens"][b] + kept[r]].cpu(), b)
        d = (lat[j].float().cpu() - ref).abs().mean().item()
        bound = 1e-2 * ref.pow(2).mean().sqrt().item()
        worst = max(worst, d / bound)
        assert d < bound, f"{label} row {r} (prompt {b}, {kept[r]} answer tokens): mean|err| {d:.3e} against 1e-2 x rms(ref) = {bound:.3e}"
    return worst


def _rerun_distance(s, m, lat, rows, res, kept, K):
    """largest mean |difference| / (1e-2 x rms) to the engine's own re-run path on each row's prompt + kept answer (printed only; rewrites slot 0)"""
    rag, per, worst = s["rag"], s["per_img"], 0.0
    for j, r in enumerate(rows):
        b = r // K
        ids = res.sequences[r: r + 1, : s["plens"][b] + kept[r]]
        rr = m.generate_latents(ids, rag["pixel_values"][b * per:(b + 1) * per], rag["image_grid_thw"][b:b + 1])[0].float()
        worst = max(worst, ((lat[j].float() - rr).abs().mean() / (1e-2 * rr.pow(2).mean().sqrt())).item())
    return worst


def _greedy(s, m):
    rag = s["rag"]
    seqs = m.generate(**rag, max_new_tokens=N_NEW)
    return seqs, m.generate_latents(seqs, rag["pixel_values"], rag["image_grid_thw"])


def test_shared_prefix_rows_continue_prompt_slot_and_tail(setup):
    from internnav_amd.runtime import CapacityError

    s, m = setup, setup["m"]
    eng, rag, K = m.qwen, setup["rag"], 5                                  # 10 rows on 6 slots: the fan-out path has no capacity for them
    g_seqs, g_lat = _greedy(s, m)
    res, kept = _draw(s, m, K, share=True, eos_row=7)
    assert m._gen is not None and m._gen["path"] == "shared" and kept[7] == 1 and max(kept) > 1
    st = m._gen["state"]
    assert st["shared"]["tail_len"] == res.sequences.shape[1] - setup["Sp"] - 1
    pv, grid = rag["pixel_values"], rag["image_grid_thw"]
    before = _snapshot(eng)
    counts = [_Count(eng, "run_prefill"), _Count(eng, "vision"), _Count(eng, "run_vision")]
    try:
        rows = [7, 0, 9, 3]                                                # out of order, both prompts, the row that kept one token (tail_len 0)
        lat = m.generate_latents(res.sequences, pv, grid, rows=rows)
        lat_all = m.generate_latents(res.sequences, pv, grid)
        again = m.generate_latents(res.sequences, pv, grid, rows=rows)
        with pytest.raises(CapacityError, match="buffer rows"):            # before any launch
            eng.latents_behind(st, [0] * (eng.x.shape[0] // 5 + 1), [1] * (eng.x.shape[0] // 5 + 1), [setup["plens"][0]] * (eng.x.shape[0] // 5 + 1))
    finally:
        for c in counts:
            c.restore()
    assert [c.n for c in counts] == [0, 0, 0], f"generate_latents after a sampled call ran prefill / vision {[(c.name, c.n) for c in counts]} times"
    _assert_untouched(eng, before, "latents behind the shared-prefix rows")
    nq = eng.latent_q.shape[0]
    assert lat.shape == (len(rows), nq, eng.H) and lat_all.shape == (N_P * K, nq, eng.H) and lat.dtype == torch.bfloat16
    assert torch.equal(again.view(torch.int16), lat.view(torch.int16)), "a second identical call gives other bits"
    w1 = _check_rows(s, setup["qsd"], "bf16", lat, rows, res, kept, K, "rows=[7, 0, 9, 3]")
    w2 = _check_rows(s, setup["qsd"], "bf16", lat_all, list(range(N_P * K)), res, kept, K, "rows=None")
    # the greedy path afterwards is what it was before the sampled calls
    g2_seqs, g2_lat = _greedy(s, m)
    assert torch.equal(g2_seqs, g_seqs) and torch.equal(g2_lat.view(torch.int16), g_lat.view(torch.int16))
    far = _rerun_distance(s, m, lat, rows, res, kept, K)
    print(f"shared-prefix K={K}: worst mean|err| / (1e-2 x rms(oracle)) = {w1:.3f} (4 rows), {w2:.3f} (all rows); to the engine's re-run path {far:.3f}")


def test_fan_out_rows_continue_their_own_slots_and_score_answers_drops_the_state(setup):
    s, m = setup, setup["m"]
    eng, rag, plens, per, K = m.qwen, setup["rag"], setup["plens"], setup["per_img"], 3
    g_seqs, g_lat = _greedy(s, m)
    res, kept = _draw(s, m, K, share=False)
    assert m._gen is not None and m._gen["path"] == "fan"
    pv, grid = rag["pixel_values"], rag["image_grid_thw"]
    before = _snapshot(eng)
    counts = [_Count(eng, "run_prefill"), _Count(eng, "vision"), _Count(eng, "run_vision")]
    try:
        rows = [4, 1]
        lat = m.generate_latents(res.sequences, pv, grid, rows=rows)
        lat_all = m.generate_latents(res.sequences, pv, grid)
        again = m.generate_latents(res.sequences, pv, grid, rows=rows)
    finally:
        for c in counts:
            c.restore()
    assert [c.n for c in counts] == [0, 0, 0], f"generate_latents after a sampled call ran prefill / vision {[(c.name, c.n) for c in counts]} times"
    _assert_untouched(eng, before, "latents behind the fan-out rows")
    assert torch.equal(again.view(torch.int16), lat.view(torch.int16)), "a second identical call gives other bits"
    w1 = _check_rows(s, setup["qsd"], "bf16", lat, rows, res, kept, K, "rows=[4, 1]")
    w2 = _check_rows(s, setup["qsd"], "bf16", lat_all, list(range(N_P * K)), res, kept, K, "rows=None")
    # score_answers in between rewrites the slots: generate_latents falls back to the re-run (every row with its own image), values as good
    m.score_answers(rag["input_ids"][:1], [[[5, 6]]], pixel_values=pv[:per], image_grid_thw=grid[:1])
    assert m._gen is None
    pv6 = torch.cat([pv[(r // K) * per:(r // K + 1) * per] for r in range(N_P * K)], 0)
    grid6 = torch.cat([grid[r // K: r // K + 1] for r in range(N_P * K)], 0)
    counts = [_Count(eng, "run_prefill"), _Count(eng, "latents_behind")]
    try:
        # (the re-run takes right-padded rows of one width: every row kept all N_NEW tokens here, prompt 1's rows are three tokens shorter)
        width = [plens[r // K] + kept[r] for r in range(N_P * K)]
        assert kept == [N_NEW] * (N_P * K)
        back0 = m.generate_latents(res.sequences[:K, : width[0]], pv6[: K * per], grid6[:K], rows=[1])
        back1 = m.generate_latents(res.sequences[K:, : width[K]], pv6[K * per:], grid6[K:], rows=[1])
    finally:
        for c in counts:
            c.restore()
    assert counts[0].n == 2 and counts[1].n == 0, "after score_answers the sampled state must not be continued"
    w3 = _check_rows(s, setup["qsd"], "bf16", torch.cat([back0, back1], 0), [1, K + 1], res, kept, K, "after score_answers")
    g2_seqs, g2_lat = _greedy(s, m)
    assert torch.equal(g2_seqs, g_seqs) and torch.equal(g2_lat.view(torch.int16), g_lat.view(torch.int16))
    # the distance to the re-run path, with the state restored by another draw of the same seed
    res, kept = _draw(s, m, K, share=False)
    lat = m.generate_latents(res.sequences, pv, grid, rows=rows)
    far = _rerun_distance(s, m, lat, rows, res, kept, K)
    print(f"fan-out K={K}: worst mean|err| / (1e-2 x rms(oracle)) = {w1:.3f} (2 rows), {w2:.3f} (all rows), {w3:.3f} (re-run after score_answers); "
          f"to the engine's re-run path {far:.3f}")


def test_w8_decode_engine_against_the_oracle_on_the_round_trip_weights(setup):
    """the pass of a w8_decode engine streams the fp8 weights (<= 64 rows): the model it computes is the round-trip checkpoint, so that is what
    the oracle runs"""
    from internnav_amd.policy import InternVLAN1ForCausalLM
    from internnav_amd.qwen_vl import w8_roundtrip_state_dict

    s, rag, K = setup, setup["rag"], 3
    m8 = InternVLAN1ForCausalLM(s["sd"], s["cfg"], "nextdit_async", w8_decode=True, **s["kw"])
    rt = w8_roundtrip_state_dict({k: v.to(DEV) for k, v in s["sd"].items()}, s["cfg"])
    qsd = {k: v.float().cpu() for k, v in rt.items() if not k.startswith("model.traj_dit") and not k.startswith("model.rgb_")}
    res, kept = _draw(s, m8, K, share=True)
    counts = [_Count(m8.qwen, "run_prefill")]
    try:
        rows = [5, 2]
        lat = m8.generate_latents(res.sequences, rag["pixel_values"], rag["image_grid_thw"], rows=rows)
    finally:
        counts[0].restore()
    assert counts[0].n == 0
    w = _check_rows(s, qsd, "w8", lat, rows, res, kept, K, "w8_decode rows=[5, 2]")
    print(f"w8_decode shared-prefix K={K}: worst mean|err| / (1e-2 x rms(oracle on the round-trip weights)) = {w:.3f}")
