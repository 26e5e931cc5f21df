"""GPU: per-token log-probabilities of System-2 answers (QwenVLEngine(token_logprobs=True), generate(output_logprobs=True)) and teacher-forced
candidate scoring (InternVLAN1ForCausalLM.score_answers).

Engine: the switch changes no token; every per-step value equals the float64 restatement (tests/logprob_ref.py) applied to the raw logits the
engine leaves in `engine.logits` after that step, within the bound model. Policy: chunked decoding yields one value per emitted token, zeros
behind EOS, the masked sum. score_answers against the fp32 oracle (oracle/qwen_vl.py)."""
import numpy as np
import pytest
import torch

import decode_penalty_ref as R
import logprob_ref as L
from internnav_amd import synthetic as S
from test_decode_penalty_gpu import _craft

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N_DEC = 3, 8


@pytest.fixture(scope="module")
def engines(built_lib):
    """two engines on the same weights (the crafted rows of test_decode_penalty_gpu._craft included: a penalty >= 1.05 then moves tokens), one
    without and one with token_logprobs"""
    from internnav_amd.qwen_vl import QwenVLEngine

    cfg = S.QWEN_TEST_CFG
    inp = S.qwen_inputs(B, 1, seed=21, cfg=cfg)
    sd = S.qwen_state_dict(seed=21, cfg=cfg)
    pv = inp["pixel_values"].to(DEV, torch.bfloat16)
    kw = dict(max_seqs=B, max_seq_len=512, max_patches=pv.shape[0])
    off = QwenVLEngine(sd, cfg, DEV, **kw)
    _, _, patch = _craft(off, inp["input_ids"], pv, inp["grid_thw"])
    on = QwenVLEngine(sd, cfg, DEV, token_logprobs=True, max_decode=16, **kw)
    for k, v in patch["lm_head"].items():
        on.lm_head[k].copy_(v)
    for k, v in patch["embed"].items():
        on.embed[k].copy_(v)
    assert off.tok_logprob is None and on.tok_logprob.shape == (B, 16)
    return off, on, cfg, inp["input_ids"], pv, inp["grid_thw"]


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("p", [1.0, 1.05])
def test_switch_on_decodes_the_same_tokens(engines, p, ragged):
    off, on, cfg, ids, pv, grid = engines
    S_ = ids.shape[1]
    kw = dict(repetition_penalty=p, **({"seq_lens": [S_, S_ - 9, S_ - 3]} if ragged else {}))
    a = off.decode(off.prefill(ids, pv, grid, **kw), N_DEC)
    st = on.prefill(ids, pv, grid, **kw)
    b = on.decode(st, N_DEC)
    assert torch.equal(a, b), (a.tolist(), b.tolist())
    lp, mg = on.last_logprobs(st)
    assert lp.shape == (B, N_DEC) and mg.shape == (B, N_DEC) and bool((lp <= 0).all()) and bool((mg >= 0).all())
    with pytest.raises(RuntimeError, match="token_logprobs"):
        off.last_logprobs(st)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("p", [1.0, 1.05])
def test_every_step_equals_the_restatement_on_the_raw_logits(engines, p, ragged):
    """one token at a time: after each step engine.logits holds the raw logits the selection read; prompt + answer so far is the seen set"""
    off, on, cfg, ids, pv, grid = engines
    S_ = ids.shape[1]
    lens = [S_, S_ - 9, S_ - 3] if ragged else [S_] * B
    st = on.prefill(ids, pv, grid, repetition_penalty=p, **({"seq_lens": lens} if ragged else {}))
    assert on.logits.data_ptr() % 16 == 0 and (on.logits.stride(0) * 4) % 16 == 0       # every row takes the kernel's 16-byte path
    toks, worst, moved = [], 0.0, 0
    for j in range(N_DEC):
        t = on.decode(st, 1) if j == 0 else on.decode(st, 2)[:, 1:]
        raw = on.logits[:B].cpu().numpy().copy()
        lp, mg = (v.cpu().numpy() for v in on.last_logprobs(st))
        assert lp.shape == (B, j + 1)
        for b in range(B):
            hist = ids[b, : lens[b]].tolist() + [int(tt[b]) for tt in toks]
            bm = None if p == 1.0 else R.seen_bitmap([hist], [len(hist)], cfg["vocab"])[0]
            want_t, wl, wm, y = L.logprob_row(raw[b], bm, p)
            ok, msg, err, bound = L.check_row(float(lp[b, j]), float(mg[b, j]), y, want_t, wl, wm, True)
            assert int(t[b, 0]) == want_t and ok, f"step {j} row {b}: tok {int(t[b, 0])} want {want_t}; {msg}"
            worst = max(worst, err / bound)
            moved += int(want_t != int(np.argmax(raw[b])))
        toks.append(t[:, 0].cpu().numpy())
    print(f"p={p} ragged={ragged}: worst |logprob - float64| / bound = {worst:.3f}; steps the penalty moved: {moved} of {B * N_DEC}")
    assert p == 1.0 or ragged or moved > 0, "test data: the penalty moves no token"
    # earlier columns are not rewritten by later steps, and a chunked decode fills the same columns with the same bits
    lp_all, mg_all = (v.clone() for v in on.last_logprobs(st))
    st2 = on.prefill(ids, pv, grid, repetition_penalty=p, **({"seq_lens": lens} if ragged else {}))
    a = on.decode(st2, 3)
    b_ = on.decode(st2, N_DEC - 3 + 1)[:, 1:]
    assert np.array_equal(torch.cat([a, b_], 1).cpu().numpy(), np.stack(toks, 1))
    lp2, mg2 = on.last_logprobs(st2)
    assert torch.equal(lp2, lp_all) and torch.equal(mg2, mg_all)


def test_captured_decode_refills_the_buffers_on_every_replay(engines):
    from internnav_amd.runtime import GraphedCall

    off, on, cfg, ids, pv, grid = engines
    p = 1.5
    P = on.plan(ids, grid, n_decode=4, repetition_penalty=p)
    on.run_prefill(P, pv)                                                     # eager; the capture below holds run_decode alone (one stream)
    toks = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    on.run_decode(P, toks)
    want_t = toks.clone()
    want_lp, want_mg = (v.clone() for v in on.last_logprobs(P))
    assert want_lp.shape == (B, 4) and bool(torch.isfinite(want_lp).all())
    ref = off.decode(off.prefill(ids, pv, grid, repetition_penalty=p), 4)
    assert torch.equal(ref, want_t)
    g = GraphedCall(lambda: on.run_decode(P, toks), {})
    for _ in range(2):
        toks.zero_()
        on.seen.view(torch.int32).fill_(-1)
        on._lp_steps.fill_(float("nan"))                                      # junk: a replay that did not write a column would leave it
        on._mg_steps.fill_(-5.0)
        g()
        torch.cuda.synchronize()
        lp, mg = on.last_logprobs(P)
        assert torch.equal(toks, want_t) and torch.equal(lp, want_lp) and torch.equal(mg, want_mg)
        assert bool(torch.isnan(on._lp_steps[4:]).all())                      # and nothing beyond the plan's columns


def test_answers_beyond_max_decode_are_refused_before_any_launch(engines):
    from internnav_amd.runtime import CapacityError

    off, on, cfg, ids, pv, grid = engines
    with pytest.raises(CapacityError, match="max_decode"):
        on.plan(ids, grid, n_decode=17)                                        # (in plan(): run_decode may run under a capture)
    assert off.plan(ids, grid, n_decode=17)["n_decode"] == 17                   # an engine without the setting has no such limit
    st = on.prefill(ids, pv, grid)
    before = on.next_tok.clone()
    with pytest.raises(CapacityError, match="max_decode"):
        on.decode(st, 17)
    assert "cur" not in st and torch.equal(on.next_tok, before)                # nothing was launched
    assert on.decode(st, 16).shape == (B, 16)
    with pytest.raises(CapacityError, match="max_decode"):
        on.decode(st, 2)                                                       # the 17th selection


# ---------------------------------------------------------------------------------------------------- policy surface
@pytest.fixture(scope="module")
def models(built_lib):
    from internnav_amd.policy import InternVLAN1ForCausalLM

    cfg = S.QWEN_TEST_CFG
    sd = {k: v.to(torch.bfloat16) for k, v in S.materialize(S.n1_full_spec(cfg, "nextdit_async"), 5).items()}
    inp = S.qwen_inputs(B, 1, seed=33, cfg=cfg, n_text=20, n_tail=12)
    kw = dict(device=DEV, max_envs=B, num_history=3, resize_w=280, resize_h=280, max_seq_len=512, max_patches=inp["pixel_values"].shape[0])
    plain = InternVLAN1ForCausalLM(sd, cfg, "nextdit_async", **kw)
    with_lp = InternVLAN1ForCausalLM(sd, cfg, "nextdit_async", token_logprobs=True, **kw)
    qsd = {k: v.float() for k, v in sd.items() if not k.startswith("model.traj_dit") and not k.startswith("model.rgb_")}
    return plain, with_lp, cfg, inp, qsd


def test_chunked_generate_returns_one_value_per_token(models):
    plain, m, cfg, inp, _ = models
    ids, pv, grid = inp["input_ids"], inp["pixel_values"], inp["grid_thw"]
    kw = dict(input_ids=ids, pixel_values=pv, image_grid_thw=grid, max_new_tokens=7, return_dict_in_generate=True, repetition_penalty=1.05)
    free = m.generate(**kw, eos_token_id=-1, output_logprobs=True, decode_chunk=128)
    n = free.sequences.shape[1] - ids.shape[1]
    assert n == 7 and free.token_logprobs.shape == (B, 7) and free.token_margins.shape == (B, 7) and free.sequences_logprob.shape == (B,)
    assert free.token_logprobs.dtype == torch.float32 and bool((free.token_logprobs < 0).all()) and bool((free.token_margins >= 0).all())
    assert torch.equal(free.sequences, plain.generate(**kw, eos_token_id=-1).sequences)            # the same answer as without the setting
    # chunks of 3 (the pending token of a chunk is re-emitted by the next): the same columns, bit for bit
    ch = m.generate(**kw, eos_token_id=-1, output_logprobs=True, decode_chunk=3)
    assert torch.equal(ch.sequences, free.sequences) and torch.equal(ch.token_logprobs, free.token_logprobs)
    assert torch.equal(ch.token_margins, free.token_margins)
    # an EOS in row 0 at its third token (and wherever else that id occurs): zeros behind it, the sum runs up to and including it
    toks = free.sequences[:, ids.shape[1]:].cpu().numpy()
    eos = int(toks[0, 2])
    out = m.generate(**kw, eos_token_id=[-1, eos], output_logprobs=True, decode_chunk=2)
    nn = out.sequences.shape[1] - ids.shape[1]
    assert out.token_logprobs.shape == (B, nn) and out.token_margins.shape == (B, nn)
    want, lens = L.mask_after_eos(free.token_logprobs.cpu().numpy()[:, :nn], toks[:, :nn], (eos,))
    assert lens[0] <= 3 and np.array_equal(out.token_logprobs.cpu().numpy(), want)
    assert bool((out.token_logprobs[0, lens[0]:] == 0).all()) and bool((out.token_margins[0, lens[0]:] == 0).all())
    assert np.array_equal(out.answer_lengths.cpu().numpy(), lens)
    assert torch.equal(out.sequences_logprob, out.token_logprobs.sum(1))
    assert np.allclose(out.sequences_logprob.cpu().numpy(), [want[b, : lens[b]].astype(np.float64).sum() for b in range(B)], rtol=1e-6, atol=0)
    # without return_dict_in_generate the call returns the sequences, as HF does
    assert torch.equal(m.generate(**dict(kw, return_dict_in_generate=False), eos_token_id=-1, output_logprobs=True), free.sequences)
    with pytest.raises(Exception, match="max_decode"):                         # (CapacityError: the model keeps 128 columns by default)
        m.generate(**dict(kw, max_new_tokens=129), output_logprobs=True)
    # a model built without the setting names it
    with pytest.raises(ValueError, match="token_logprobs"):
        plain.generate(**kw, output_logprobs=True)
    assert not hasattr(plain.generate(**kw, eos_token_id=-1, output_scores=True, output_logits=True), "scores")


def test_score_answers_against_the_fp32_oracle(models):
    """two prompts x two candidates of different length, one of them the oracle's greedy answer, chosen with the oracle alone. 4 pairs on an engine
    of 3 sequences: two prefill groups."""
    from oracle import qwen_vl as o_q

    plain, with_lp, cfg, inp, qsd = models
    n_p, per_img = 2, inp["pixel_values"].shape[0] // B
    ids, grid = inp["input_ids"][:n_p], inp["grid_thw"][:n_p]
    pv = inp["pixel_values"][: n_p * per_img]
    Sp = ids.shape[1]
    torch.set_num_threads(16)
    answers, want, scale = [], [], []
    with torch.no_grad():
        for b in range(n_p):
            pvb, gb = pv[b * per_img:(b + 1) * per_img].float(), grid[b:b + 1]
            greedy = o_q.generate(qsd, cfg, ids[b:b + 1], pvb, gb, 3)[0, Sp:].tolist()
            # the other candidate: two tokens, each the LEAST likely at its position (decided by the oracle's logits alone)
            l0, _ = o_q.forward_logits(qsd, cfg, ids[b:b + 1], pvb, gb)
            u0 = int(l0[0, -1].argmin())
            l1, _ = o_q.forward_logits(qsd, cfg, torch.cat([ids[b:b + 1], torch.tensor([[u0]])], 1), pvb, gb)
            other = [u0, int(l1[0, -1].argmin())]
            answers.append([greedy, other])
            w = []
            for cand in (greedy, other):
                full = torch.cat([ids[b:b + 1], torch.tensor([cand])], 1)
                lg, _ = o_q.forward_logits(qsd, cfg, full, pvb, gb)
                rows = lg[0, Sp - 1: Sp - 1 + len(cand)].double()
                w.append(torch.log_softmax(rows, -1)[torch.arange(len(cand)), torch.tensor(cand)].numpy())
                scale.append(float(rows.std()))
            want.append(w)
    # tolerance: test_qwen_gpu.py asserts max |logit error| < 5e-2 * std(oracle logits) for this configuration; a logit error eps moves a
    # log-softmax entry by at most 2 eps -> 2 * 5e-2 * std (std over the scored rows' oracle logits, the largest of the four pairs)
    tol = 2 * 5e-2 * max(scale)
    res = plain.score_answers(ids, answers, pixel_values=pv, image_grid_thw=grid)          # (the model WITHOUT token_logprobs: not needed)
    worst = 0.0
    for b in range(n_p):
        assert res.lengths[b] == [3, 2] and res.sequences_logprob[b].shape == (2,)
        for c in range(2):
            got = res.token_logprobs[b][c].cpu().numpy()
            err = np.abs(got - want[b][c]).max()
            worst = max(worst, err)
            assert got.shape == want[b][c].shape and err <= tol, f"prompt {b} candidate {c}: {got.tolist()} want {want[b][c].tolist()} tol {tol:.3f}"
            assert abs(float(res.sequences_logprob[b][c]) - float(got.astype(np.float64).sum())) <= 1e-5 * max(1.0, abs(float(got.sum())))
        # ranking: the oracle's gap must exceed what the tolerance allows the two sums to move (the precondition), then the order must agree
        gap = want[b][0].sum() - want[b][1].sum()
        assert gap > (3 + 2) * tol, f"test data: oracle gap {gap:.2f} within the tolerance {(3 + 2) * tol:.2f}"
        assert float(res.sequences_logprob[b][0]) > float(res.sequences_logprob[b][1])
    print(f"score_answers: max |logprob - oracle| {worst:.3e} (tolerance {tol:.3f}, oracle logit std {max(scale):.2f})")
    # ragged prompts (attention_mask) give the values of the unpadded call for the shorter prompt
    pad = torch.zeros(n_p, Sp + 5, dtype=torch.long)
    mask = torch.zeros(n_p, Sp + 5, dtype=torch.long)
    pad[:, :Sp], mask[:, :Sp] = ids, 1
    r2 = plain.score_answers(pad, answers, pixel_values=pv, image_grid_thw=grid, attention_mask=mask)
    for b in range(n_p):
        for c in range(2):
            assert (r2.token_logprobs[b][c] - res.token_logprobs[b][c]).abs().max().item() <= tol
    # a one-token candidate = the first greedy step of generate() at penalty 1.0: the same position through the prefill's last row
    g = with_lp.generate(input_ids=ids, pixel_values=pv, image_grid_thw=grid, max_new_tokens=1, eos_token_id=-1, repetition_penalty=1.0,
                         return_dict_in_generate=True, output_logprobs=True)
    first = g.sequences[:, Sp].tolist()
    r1 = with_lp.score_answers(ids, [[[t]] for t in first], pixel_values=pv, image_grid_thw=grid)
    a = torch.stack([r1.token_logprobs[b][0][0] for b in range(n_p)])
    d = (a - g.token_logprobs[:, 0]).abs().max().item()
    print(f"one-token candidate vs generate's first step: max |difference| {d:.3e} ({'bit-equal' if d == 0.0 else 'not bit-equal'})")
    assert d <= tol
