"""GPU: QwenVLEngine(mx4_decode=True) - the System-2 single-token passes on MXFP4 weights (ops.linear_mx4); tests/test_w8_decode_gpu.py on
the 4-bit format.

The engine with the switch on is ONE model, the checkpoint with its decoder projections rounded to MXFP4 (e2m1 elements, an e8m0 scale per 32
consecutive k) and lm_head to e4m3 * 2^e per output row: the prefill runs the dequantised bf16 values, the decode / latent-query / suffix
passes the packed bytes, and the MXFP4 and fp8 kernels give the bits of the bf16 weight-streaming kernels on the dequantised weights. So
engine A (mx4_decode=True on the synthetic checkpoint) must EQUAL engine B (the plain engine on qwen_vl.mx4_roundtrip_state_dict of it) bit
for bit - prefill logits, greedy tokens, latent queries, the log-probabilities of score_answers(share_prefix=True) - for dense and ragged
batches, eagerly, planned, and replayed from a captured graph; dropping the quantised copies changes no bit and refreshing them brings the
4-bit path back. With the default (off) nothing changes and no MXFP4 or fp8 kernel runs; both switches together are refused. The drift of the
quantised model from the unquantised one is printed only."""
import numpy as np
import pytest
import torch

from internnav_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_DEC = 8


@pytest.fixture(scope="module")
def engines(built_lib):
    from internnav_amd import qwen_vl
    from internnav_amd.qwen_vl import QwenVLEngine

    cfg = S.QWEN_TEST_CFG
    sd = {k: v.to(DEV) for k, v in S.qwen_state_dict(seed=12, cfg=cfg).items()}
    kw = dict(max_seqs=3, max_seq_len=512, max_patches=3 * 784)
    a = QwenVLEngine(sd, cfg, DEV, mx4_decode=True, **kw)
    b = QwenVLEngine(qwen_vl.mx4_roundtrip_state_dict(sd, cfg), cfg, DEV, **kw)
    plain = QwenVLEngine(sd, cfg, DEV, **kw)                       # the unquantised engine, constructed without the keyword
    return cfg, sd, kw, a, b, plain


def _inputs(cfg, B):
    inp = S.qwen_inputs(B, 1, seed=12, cfg=cfg)
    return inp["input_ids"], inp["pixel_values"].to(DEV, torch.bfloat16), inp["grid_thw"]


def _run(eng, ids, pv, grid, seq_lens=None):
    """(prefill logits, N_DEC greedy tokens, latent queries), (MXFP4, fp8) launches of everything behind the prefill
    (ragged: sequence 0's second token plays EOS, its answer ends there)"""
    from internnav_amd import runtime

    st = eng.prefill(ids, pv, grid, **({} if seq_lens is None else dict(seq_lens=seq_lens)))
    torch.cuda.synchronize()
    runtime.prof_enable(True)
    try:
        out = _after_prefill(eng, st, seq_lens)
        n = (runtime.prof_read_mx4()["launches"], runtime.prof_read_w8()["launches"])
    finally:
        runtime.prof_enable(False)
    return out, n


def _after_prefill(eng, st, seq_lens):
    B, Sr = st["B"], st["S_run"]
    if "lens" in st:
        rows = torch.from_numpy((np.arange(B) * Sr + st["lens"] - 1).astype(np.int32)).to(DEV)
        eng._last_logits(B, Sr, None, rows_idx=rows)
    else:
        eng._last_logits(B, Sr, Sr - 1)
    logits = eng.logits[:B].clone()
    toks = eng.decode(st, N_DEC).clone()
    if seq_lens is None:
        lat = eng.latents(st, toks[:, -1:].contiguous())
    else:
        n_ans = np.asarray([2] + [N_DEC] * (B - 1))                   # early EOS in sequence 0
        tail = torch.stack([toks[b, n_ans[b] - 1] for b in range(B)])[:, None].contiguous()
        lat = eng.latents(st, tail, seq_lens=st["lens"] + n_ans - 1)
    torch.cuda.synchronize()
    return logits, toks, lat.clone()


def _same(x, y, what):
    for name, p, q in zip(("prefill logits", "greedy tokens", "latent queries"), x, y):
        assert torch.equal(p, q), f"{what}: {name} differ ({int((p != q).sum())} of {p.numel()} elements)"


@pytest.mark.parametrize("B,ragged", [(1, False), (3, False), (3, True)])
def test_mx4_engine_equals_plain_engine_on_roundtrip_checkpoint(engines, B, ragged):
    cfg, _, _, a, b, plain = engines
    ids, pv, grid = _inputs(cfg, B)
    lens = [ids.shape[1], ids.shape[1] - 5, ids.shape[1] - 2][:B] if ragged else None
    ra, n_a = _run(a, ids, pv, grid, lens)
    rb, n_b = _run(b, ids, pv, grid, lens)
    # MXFP4: per single-token pass 4 GEMMs per layer, the latent pass 4 per layer; fp8: lm_head of every single-token pass and of the first
    # token (here and in decode())
    want = ((N_DEC - 1) * 4 * cfg["t_layers"] + 4 * cfg["t_layers"], N_DEC + 1)
    assert n_a == want and n_b == (0, 0), f"(MXFP4, fp8) launches: {n_a} (expected {want}) in the mx4 engine, {n_b} in the plain one"
    _same(ra, rb, f"B={B} ragged={ragged}")
    ru = _run(plain, ids, pv, grid, lens)[0]
    err = (ra[0].float() - ru[0].float()).abs()
    print(f"MX4_DRIFT B={B} ragged={ragged}: last-position logits mean|err| {err.mean().item():.4e} max|err| {err.max().item():.4e} "
          f"(max|logit| {ru[0].abs().max().item():.3f}); tokens mx4 {ra[1].tolist()} bf16 {ru[1].tolist()}; "
          f"latents max|err| {(ra[2].float() - ru[2].float()).abs().max().item():.4e}")


def test_planned_sequence_replays_from_a_graph(engines):
    from internnav_amd.runtime import GraphedCall

    cfg, _, _, a, b, _ = engines
    ids, pv, grid = _inputs(cfg, 3)
    outs = []
    for eng in (a, b):
        P = eng.plan(ids, grid, n_decode=N_DEC, with_latents=True)
        toks = torch.zeros(3, N_DEC, dtype=torch.int32, device=DEV)
        lat = torch.zeros(3, cfg["n_query"], cfg["t_hidden"], dtype=torch.bfloat16, device=DEV)
        eng.run_s2(P, pv, toks, lat)
        torch.cuda.synchronize()
        outs.append((eng, P, toks.clone(), lat.clone()))
    assert torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][3], outs[1][3])
    eng, P, toks_ref, lat_ref = outs[0]
    toks, lat = torch.zeros_like(toks_ref), torch.zeros_like(lat_ref)
    g = GraphedCall(lambda pixel_values: eng.run_s2(P, pixel_values, toks, lat), {"pixel_values": pv})
    toks.zero_()
    lat.zero_()
    g()
    torch.cuda.synchronize()
    assert torch.equal(toks, toks_ref) and torch.equal(lat, lat_ref)


def test_drop_and_refresh(engines):
    cfg, _, _, a, _, _ = engines
    ids, pv, grid = _inputs(cfg, 3)
    ref, n0 = _run(a, ids, pv, grid)
    tw = a.twin()
    assert tw.lm_head8[0] is a.lm_head8[0] and all(x["qkv_w4"][0] is y["qkv_w4"][0] and x["down_w4"][1] is y["down_w4"][1] for x, y in zip(a.layers, tw.layers))
    a.drop_mx4_weights()
    assert not a.mx4_decode and a.lm_head8 is None and all(k + "4" not in L for L in a.layers for k in a.W8_LAYER_WEIGHTS)
    dropped, n1 = _run(a, ids, pv, grid)
    a.refresh_mx4_weights()
    back, n2 = _run(a, ids, pv, grid)
    assert n0[0] > 0 and n0[1] > 0 and n1 == (0, 0) and n2 == n0
    _same(dropped, ref, "after drop_mx4_weights")
    _same(back, ref, "after refresh_mx4_weights")
    _same(_run(tw, ids, pv, grid)[0], ref, "twin")


def test_default_is_off_and_unchanged(engines):
    from internnav_amd.qwen_vl import QwenVLEngine

    cfg, sd, kw, _, _, plain = engines
    off = QwenVLEngine(sd, cfg, DEV, mx4_decode=False, **kw)
    assert not off.mx4_decode and not plain.mx4_decode and not off.w8_decode and off.lm_head8 is None
    assert torch.equal(off.lm_head, sd["lm_head.weight"].to(torch.bfloat16)) and all("qkv_w4" not in L and "qkv_w8" not in L for L in off.layers)
    assert torch.equal(off.layers[0]["o_w"], sd["model.layers.0.self_attn.o_proj.weight"].to(torch.bfloat16))
    ids, pv, grid = _inputs(cfg, 3)
    r_off, n_off = _run(off, ids, pv, grid)
    r_plain, n_plain = _run(plain, ids, pv, grid)
    assert n_off == (0, 0) and n_plain == (0, 0)
    _same(r_off, r_plain, "mx4_decode=False vs no keyword")


def test_both_switches_are_refused(engines):
    from internnav_amd.qwen_vl import QwenVLEngine

    cfg, sd, kw, a, _, _ = engines
    with pytest.raises(ValueError, match="w8_decode and mx4_decode"):
        QwenVLEngine(sd, cfg, DEV, w8_decode=True, mx4_decode=True, **kw)
    with pytest.raises(ValueError, match="drop_mx4_weights"):
        a.refresh_w8_weights()
    assert a.mx4_decode and not a.w8_decode


def test_stored_bytes_are_the_quantiser_s(engines):
    """what the engine streams is ops.mx4_quantize of the round-trip checkpoint's fused tensors (the rounding commutes with fusing q | k | v
    and interleaving gate | up: blocks lie inside one output row), and the bf16 tensors hold exactly the dequantised values"""
    from internnav_amd import ops

    _, _, _, a, b, _ = engines
    for La, Lb in zip(a.layers, b.layers):
        for k in a.W8_LAYER_WEIGHTS:
            w4, sc, wd = ops.mx4_quantize(Lb[k])
            assert torch.equal(La[k + "4"][0], w4) and torch.equal(La[k + "4"][1], sc), k
            assert torch.equal(La[k].view(torch.int16), Lb[k].view(torch.int16)) and torch.equal(wd.view(torch.int16), Lb[k].view(torch.int16)), k
    assert torch.equal(a.lm_head.view(torch.int16), b.lm_head.view(torch.int16))


def test_score_answers_shared_prefix_equals_plain_model_on_roundtrip_checkpoint(built_lib):
    """one prompt, two candidates of 3 tokens: the suffix pass (6 rows) streams the 4-bit copies in model A and the dequantised bf16
    weights in model B - the same log-probabilities, bit for bit"""
    from internnav_amd import qwen_vl, runtime
    from internnav_amd.policy import InternVLAN1ForCausalLM

    cfg = S.QWEN_TEST_CFG
    sd = {k: v.to(DEV, torch.bfloat16) for k, v in S.materialize(S.n1_full_spec(cfg, "nextdit_async"), 5).items()}
    inp = S.qwen_inputs(1, 1, seed=33, cfg=cfg, n_text=20, n_tail=12)
    ids, grid, pv = inp["input_ids"], inp["grid_thw"], inp["pixel_values"]
    kw = dict(device=DEV, max_envs=2, num_history=3, resize_w=280, resize_h=280, max_seq_len=512, max_patches=2 * pv.shape[0])
    answers = [[[17, 905, 3001], [17, 2222, 64]]]
    res, launches = [], []
    for weights, on in ((sd, True), (qwen_vl.mx4_roundtrip_state_dict(sd, cfg), False)):
        m = InternVLAN1ForCausalLM(weights, cfg, "nextdit_async", mx4_decode=on, **kw)
        runtime.prof_enable(True)
        try:
            res.append(m.score_answers(ids, answers, pixel_values=pv, image_grid_thw=grid, share_prefix=True))
            torch.cuda.synchronize()
            launches.append(runtime.prof_read_mx4()["launches"])
        finally:
            runtime.prof_enable(False)
        assert m.last_score["prompt_prefills"] == 1 and m.last_score["suffix_passes"] == 1 and m.last_score["suffix_rows"] == 2 * 2
        del m
    assert launches == [4 * cfg["t_layers"], 0], launches
    for c in range(2):
        x, y = res[0].token_logprobs[0][c], res[1].token_logprobs[0][c]
        assert x.shape == (3,) and torch.equal(x.view(torch.int32), y.view(torch.int32)), (c, x.tolist(), y.tolist())
    assert torch.equal(res[0].sequences_logprob[0], res[1].sequences_logprob[0])
    print(f"MX4_SCORE log-probabilities {[t.tolist() for t in res[0].token_logprobs[0]]}")
