"""GPU: QwenVLEngine(w8_decode=True) - the System-2 single-token passes on FP8 weights (ops.linear_w8).

The engine with the switch on is ONE model, the checkpoint with its decoder projections and lm_head rounded to e4m3 * 2^e per output row: the
prefill runs the dequantised bf16 values, the decode / latent-query passes the fp8 bytes, and the fp8 kernels give the bits of the bf16
weight-streaming kernels on the dequantised weights. So engine A (w8_decode=True on the synthetic checkpoint) must EQUAL engine B (the plain
engine on qwen_vl.w8_roundtrip_state_dict of it) bit for bit - prefill logits, greedy tokens, latent queries - for dense and ragged batches,
eagerly, planned, and replayed from a captured graph; dropping the fp8 copies changes no bit and refreshing them brings the fp8 path back.
With the default (off) nothing changes and no fp8 kernel runs. The drift of the quantised model from the unquantised one is printed only."""
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
    a = QwenVLEngine(sd, cfg, DEV, w8_decode=True, **kw)
    b = QwenVLEngine(qwen_vl.w8_roundtrip_state_dict(sd, cfg), cfg, DEV, **kw)
    plain = QwenVLEngine(sd, cfg, DEV, **kw)                       # the unquantised engine, constructed without the keyword
    return cfg, sd, kw, a, b, plain


def _inputs(cfg, B):
    inp = S.qwen_inputs(B, 1, seed=12, cfg=cfg)
    return inp["input_ids"], inp["pixel_values"].to(DEV, torch.bfloat16), inp["grid_thw"]


def _run(eng, ids, pv, grid, seq_lens=None):
    """(prefill logits, N_DEC greedy tokens, latent queries), fp8 launches of everything behind the prefill
    (ragged: sequence 0's second token plays EOS, its answer ends there)"""
    from internnav_amd import runtime

    st = eng.prefill(ids, pv, grid, **({} if seq_lens is None else dict(seq_lens=seq_lens)))
    torch.cuda.synchronize()
    runtime.prof_enable(True)
    try:
        out = _after_prefill(eng, st, seq_lens)
        n = runtime.prof_read_w8()["launches"]
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
def test_w8_engine_equals_plain_engine_on_roundtrip_checkpoint(engines, B, ragged):
    cfg, _, _, a, b, plain = engines
    ids, pv, grid = _inputs(cfg, B)
    lens = [ids.shape[1], ids.shape[1] - 5, ids.shape[1] - 2][:B] if ragged else None
    ra, n_a = _run(a, ids, pv, grid, lens)
    rb, n_b = _run(b, ids, pv, grid, lens)
    # per single-token pass 4 GEMMs per layer + lm_head; the latent pass 4 per layer; the first token's lm_head (here and in decode())
    want = (N_DEC - 1) * (4 * cfg["t_layers"] + 1) + 4 * cfg["t_layers"] + 2
    assert n_a == want and n_b == 0, f"fp8 launches: {n_a} (expected {want}) in the w8 engine, {n_b} in the plain one"
    _same(ra, rb, f"B={B} ragged={ragged}")
    ru = _run(plain, ids, pv, grid, lens)[0]
    err = (ra[0].float() - ru[0].float()).abs()
    print(f"W8_DRIFT B={B} ragged={ragged}: last-position logits mean|err| {err.mean().item():.4e} max|err| {err.max().item():.4e} "
          f"(max|logit| {ru[0].abs().max().item():.3f}); tokens w8 {ra[1].tolist()} bf16 {ru[1].tolist()}; "
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
    assert tw.lm_head8[0] is a.lm_head8[0] and all(x["qkv_w8"][0] is y["qkv_w8"][0] for x, y in zip(a.layers, tw.layers))
    a.drop_w8_weights()
    assert not a.w8_decode and a.lm_head8 is None and all("qkv_w8" not in L for L in a.layers)
    dropped, n1 = _run(a, ids, pv, grid)
    a.refresh_w8_weights()
    back, n2 = _run(a, ids, pv, grid)
    assert n0 > 0 and n1 == 0 and n2 == n0
    _same(dropped, ref, "after drop_w8_weights")
    _same(back, ref, "after refresh_w8_weights")
    _same(_run(tw, ids, pv, grid)[0], ref, "twin")


def test_default_is_off_and_unchanged(engines):
    from internnav_amd.qwen_vl import QwenVLEngine

    cfg, sd, kw, _, _, plain = engines
    off = QwenVLEngine(sd, cfg, DEV, w8_decode=False, **kw)
    assert not off.w8_decode and not plain.w8_decode and off.lm_head8 is None
    assert torch.equal(off.lm_head, sd["lm_head.weight"].to(torch.bfloat16)) and all("qkv_w8" not in L for L in off.layers)
    ids, pv, grid = _inputs(cfg, 3)
    r_off, n_off = _run(off, ids, pv, grid)
    r_plain, n_plain = _run(plain, ids, pv, grid)
    assert n_off == 0 and n_plain == 0
    _same(r_off, r_plain, "w8_decode=False vs no keyword")
