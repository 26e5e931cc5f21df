"""GPU: System-2 KV reuse through the HF cache contract - generate(return_dict_in_generate=True).past_key_values handed back as
generate(past_key_values=...) - and through InternVLAN1Net(kv_reuse=True) and the batched agent.

Claim tested: a call that takes the longest common prefix of its prompt from an earlier call's EngineKVCache returns the same tokens,
last logits and latents, bit for bit, as the same call without a cache, and prefills fewer rows. Small QWEN_TEST_CFG geometry: frames of 196 /
100 merged tokens and a 640 x 480 look-down frame (391 tokens), so a look-down suffix runs the kernels of a full prefill."""
import copy

import numpy as np
import pytest
import torch

from internnav_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_TEXT, N_IMG = 40, 3
P_IMG0 = N_TEXT + 196 + 2                                    # text | <vs> image 0 <ve>


@pytest.fixture(scope="module")
def model(built_lib):
    from internnav_amd.policy import InternVLAN1ForCausalLM

    cfg = S.QWEN_TEST_CFG
    sd = S.materialize(S.n1_full_spec(cfg, "nextdit_async"), 5)
    return InternVLAN1ForCausalLM(sd, cfg, "nextdit_async", device=DEV, max_envs=2, num_history=3, resize_w=280, resize_h=280, cam_w=640, cam_h=480,
                                  max_seq_len=1536, max_patches=8192)


def _gen(model, ids, pv, grid, mask=None, past=None):
    kw = {} if mask is None else {"attention_mask": mask}
    out = model.generate(input_ids=ids, pixel_values=pv, image_grid_thw=grid, max_new_tokens=6, return_dict_in_generate=True,
                         past_key_values=past, **kw)
    logits = model.qwen.logits[: ids.shape[0]].clone()
    s_run = model._gen["state"]["S_run"]
    lat = model.generate_latents(out.sequences, pv, grid).clone()
    return out, logits, lat, s_run


def _pv_of(inp, B, k):
    """patches of the first k images of every sequence"""
    return inp["pixel_values"].view(B, N_IMG, 784, 1176)[:, :k].reshape(-1, 1176)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("cut", ["image", "mid_text"])
def test_second_call_with_the_cache_equals_the_call_without(model, ragged, cut):
    inp = S.qwen_inputs(2, N_IMG, seed=11, cfg=S.QWEN_TEST_CFG, n_text=N_TEXT, n_tail=24)
    ids, grid, pv = inp["input_ids"], inp["grid_thw"], inp["pixel_values"]
    B, S_ = ids.shape
    mask = None
    if ragged:
        mask = torch.ones_like(ids)
        mask[1, S_ - 9:] = 0
    # first call: a shorter prompt that shares the first image, or ("mid_text") 25 tokens of the leading text and then diverges
    P = P_IMG0 if cut == "image" else 25
    first_ids = ids[:, :P].clone()
    if cut == "mid_text":
        first_ids = torch.cat([first_ids, torch.full((B, 110), 4090, dtype=torch.long)], 1)   # no text token is 4090; 135 rows: full-prefill kernels
    grid1 = grid.view(B, N_IMG, 3)[:, :1].reshape(-1, 3) if cut == "image" else None
    pv1 = _pv_of(inp, B, 1) if cut == "image" else None
    out1 = model.generate(input_ids=first_ids, pixel_values=pv1, image_grid_thw=grid1, max_new_tokens=3, return_dict_in_generate=True)
    cache = out1.past_key_values
    assert cache is not None and len(cache) == B and cache.get_seq_length(0) == first_ids.shape[1] and cache.is_view
    tiny = model.generate(input_ids=first_ids[:, :30], max_new_tokens=2, return_dict_in_generate=True).past_key_values
    assert tiny.get_seq_length(0) == 0                       # 2 x 30 rows ran the weight-streaming GEMMs: not exact, not cached
    ref_out, ref_logits, ref_lat, ref_rows = _gen(model, ids, pv, grid, mask)              # without a cache (evicts the views above)
    assert not cache.is_view
    fresh = inp["pixel_values"].view(B, N_IMG, 784, 1176)[:, 1:].reshape(-1, 1176)
    for pv_in in ((pv, fresh) if cut == "image" else (pv,)):                                     # every image / only the fresh ones
        out, logits, lat, rows = _gen(model, ids, pv_in, grid, mask, past=cache)
        print(f"ragged={ragged} cut={cut}: rows {rows} vs {ref_rows}, reused {model.last_kv_reuse}")
        assert torch.equal(out.sequences, ref_out.sequences)
        assert torch.equal(logits, ref_logits) and torch.equal(lat, ref_lat)
        assert rows == S_ - P and rows < ref_rows and model.last_kv_reuse == dict(rows=B * P, fallbacks=0)
    # a per-row list with one row uncached
    out, logits, lat, rows = _gen(model, ids, pv, grid, mask, past=[cache.select([0]), None])
    assert torch.equal(out.sequences, ref_out.sequences) and torch.equal(logits, ref_logits) and torch.equal(lat, ref_lat)
    assert model.last_kv_reuse["rows"] == P


def test_held_view_survives_an_unrelated_call_and_deepcopy(model):
    inp = S.qwen_inputs(2, N_IMG, seed=12, cfg=S.QWEN_TEST_CFG, n_text=N_TEXT, n_tail=24)
    ids, grid, pv = inp["input_ids"], inp["grid_thw"], inp["pixel_values"]
    B = ids.shape[0]
    grid2 = grid.view(B, N_IMG, 3)[:, :2].reshape(-1, 3)
    first = ids[:, : P_IMG0 + 198]
    out1 = model.generate(input_ids=first, pixel_values=_pv_of(inp, B, 2), image_grid_thw=grid2, max_new_tokens=3, return_dict_in_generate=True)
    held = out1.past_key_values
    dup = copy.deepcopy(held)                                # materialised straight from the slots; `held` stays a view
    assert held.is_view and not dup.is_view
    other = S.qwen_inputs(2, 1, seed=99, cfg=S.QWEN_TEST_CFG, n_text=N_TEXT + 30, n_tail=40)
    model.generate(input_ids=other["input_ids"], pixel_values=other["pixel_values"], image_grid_thw=other["grid_thw"], max_new_tokens=3)
    assert not held.is_view                                  # the unrelated prefill materialised it before overwriting its rows
    for a, b in zip(held.kv, dup.kv):
        assert torch.equal(a, b)
    ref = _gen(model, ids, pv, grid)
    for past in (held, dup):
        got = _gen(model, ids, pv, grid, past=past)
        assert torch.equal(got[0].sequences, ref[0].sequences) and torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
        assert got[3] == ids.shape[1] - first.shape[1]


def test_kv_copy_equals_a_slice_copy(built_lib):
    from internnav_amd import ops

    g = torch.Generator(device=DEV).manual_seed(3)
    nl, Bm, Sm, w = 5, 3, 97, 1024
    layers = [torch.randn(Bm * Sm, w, device=DEV, generator=g).to(torch.bfloat16) for _ in range(nl)]
    base = torch.tensor([t.data_ptr() for t in layers], dtype=torch.int64, device=DEV)
    spec = [(0, 0, 13), (2, 5, 91), (1, 40, 1)]               # (slot, first position, rows): odd counts, one row, near the slot's end
    dst = [torch.zeros(nl, n + 4, w, device=DEV, dtype=torch.bfloat16)[:, 2:2 + n] for _, _, n in spec]   # strided over layers
    tab = torch.tensor([[d.data_ptr(), d.stride(0) * 2, s * Sm + p, n] for d, (s, p, n) in zip(dst, spec)], dtype=torch.int64, device=DEV)
    ops.kv_copy(base, tab, Bm * Sm, w * 2, max(n for _, _, n in spec), to_engine=False)
    for d, (s, p, n) in zip(dst, spec):
        want = torch.stack([t[s * Sm + p: s * Sm + p + n] for t in layers])
        assert torch.equal(d, want)
    src = [torch.randn(nl, n, w, device=DEV, generator=g).to(torch.bfloat16) for _, _, n in spec]
    before = [t.clone() for t in layers]
    tab = torch.tensor([[x.data_ptr(), x.stride(0) * 2, s * Sm + p, n] for x, (s, p, n) in zip(src, spec)], dtype=torch.int64, device=DEV)
    ops.kv_copy(base, tab, Bm * Sm, w * 2, 91, to_engine=True)
    for li in range(nl):                                     # the torch slice copy of the same rows
        for x, (s, p, n) in zip(src, spec):
            before[li][s * Sm + p: s * Sm + p + n].copy_(x[li])
        assert torch.equal(layers[li], before[li])


class _Tok:
    def __call__(self, texts, return_tensors="pt"):
        ids, i, t = [], 0, texts[0]
        cfg = S.QWEN_TEST_CFG
        special = {"<|image_pad|>": cfg["image_token_id"], "<|vision_start|>": cfg["vision_start_id"], "<|vision_end|>": cfg["vision_end_id"]}
        while i < len(t):
            for k, v in special.items():
                if t.startswith(k, i):
                    ids.append(v)
                    i += len(k)
                    break
            else:
                ids.append(ord(t[i]) % 3000)
                i += 1
        return {"input_ids": torch.tensor([ids])}

    def decode(self, ids, skip_special_tokens=True):
        return "12 34"                       # a pixel goal: every call also runs the latent queries


class _Proc:
    tokenizer = _Tok()
    image_token = "<|image_pad|>"

    def apply_chat_template(self, conv, tokenize=False, add_generation_prompt=True):
        return "".join("<|vision_start|><|image_pad|><|vision_end|>" if c["type"] == "image" else c["text"] for m in conv for c in m["content"])


def _episode(model, pre, **flags):
    from internnav_amd.policy import InternVLAN1Net

    net = InternVLAN1Net(model, _Proc(), num_history=3, resize_w=280, resize_h=280, frame_preprocessor=pre, **flags)
    rng = np.random.default_rng(4)
    frames = [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(12)]
    out, rows, lens = [], [], []
    net.step_no_infer(frames[0], None, None)
    net.step_no_infer(frames[1], None, None)
    script = ((2, False), (3, True), (4, False), (5, True), (6, False), (7, False))
    for k, (f, look_down) in enumerate(script):
        if not look_down and k:
            net.step_no_infer(frames[8 + k % 4], None, None)
        so = net.s2_step(frames[f], None, None, "go to the door", None, look_down)
        out.append((so.output_action, None if so.output_latent is None else so.output_latent.cpu()))
        rows.append(model._gen["state"]["S_run"])
        lens.append(int(model._gen["state"]["S"]))
    return net, out, rows, lens


@pytest.mark.parametrize("vit_cache", [False, True])
def test_policy_episode_with_kv_reuse_is_exact(model, vit_cache):
    from internnav_amd.preprocess import FramePreprocessor

    pre = FramePreprocessor(DEV, resize_w=280, resize_h=280)
    _, base, rows0, lens = _episode(model, pre, vit_cache=vit_cache)
    _, pc, rows_pc, _ = _episode(model, pre, prefix_cache=True)
    net, got, rows, lens_r = _episode(model, pre, vit_cache=vit_cache, kv_reuse=True)
    assert net.kv_reuse and not net.prefix_cache and net.vit_cache == vit_cache
    print(f"vit_cache={vit_cache}: rows without reuse {rows0}, prefix_cache {rows_pc}, kv_reuse {rows}")
    for (a0, l0), (a1, l1) in zip(base, got):
        assert a0 == a1 and ((l0 is None and l1 is None) or torch.equal(l0, l1))
    assert lens == lens_r
    for k in (1, 3):                                         # look-down turns: only the rows behind the previous prompt run
        assert rows[k] == lens[k] - lens[k - 1], (k, rows, lens)
    assert all(r <= p for r, p in zip(rows, rows_pc)) and sum(rows) < sum(rows_pc)


def test_agent_mixed_chunk_keeps_every_rows_reuse(model):
    """one env in its look-down turn beside an env on a fresh call: same answers as without reuse, both rows reuse, no fallback."""
    from internnav_amd.agent import InternVLAN1Agent
    from internnav_amd.policy import InternVLAN1Net
    from internnav_amd.preprocess import FramePreprocessor

    pre = FramePreprocessor(DEV, resize_w=280, resize_h=280)
    rng = np.random.default_rng(9)
    frames = [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(8)]
    results = []
    for kv in (False, True):
        agent = InternVLAN1Agent({"model_settings": {"infer_mode": "partial_async"}}, policy_factory=lambda kv=kv: InternVLAN1Net(
            model, _Proc(), num_history=3, resize_w=280, resize_h=280, frame_preprocessor=pre, kv_reuse=kv), frame_preprocessor=pre)
        envs = [agent._env(0), agent._env(1)]
        for e in envs:
            e.policy.step_no_infer(frames[0], None, None)
        obs = [{"rgb": frames[1 + i], "depth": None, "instruction": "go to the door"} for i in range(2)]
        agent._run_s2([(e, o) for e, o in zip(envs, obs)])
        envs[0].look_down = True                             # env 0: look-down turn (re-sends its whole previous prompt)
        envs[1].policy.step_no_infer(frames[5], None, None)  # env 1: the episode moved on, a fresh call
        prefix = []
        gen = model.generate

        def spy(*a, **k):
            r = gen(*a, **k)
            prefix.append(np.broadcast_to(model._gen["state"]["plan"]["prefix_len"], (k["input_ids"].shape[0],)).tolist())
            return r

        model.generate = spy
        try:
            obs = [{"rgb": frames[3 + i], "depth": None, "instruction": "go to the door"} for i in range(2)]
            agent._run_s2([(e, o) for e, o in zip(envs, obs)])
        finally:
            del model.generate
        out = [(e.s2_output.output_action, None if e.s2_output.output_latent is None else e.s2_output.output_latent.cpu()) for e in envs]
        results.append((out, prefix, agent))
    (base, _, _), (got, prefix, agent) = results
    for (a0, l0), (a1, l1) in zip(base, got):
        assert a0 == a1 and ((l0 is None and l1 is None) or torch.equal(l0, l1))
    print(f"prefix lengths per chunk {prefix}, reused rows {agent.kv_reuse_rows}, fallbacks {agent.kv_reuse_fallbacks}")
    assert agent.kv_reuse_fallbacks == 0
    assert sum(len(c) for c in prefix) == 2 and all(p > 0 for c in prefix for p in c)
