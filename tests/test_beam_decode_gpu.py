"""GPU: beam search on the 2-layer test model (6 slots, 2 ragged prompts) - QwenVLEngine.prefill(beam=) / decode driven one step at a time against
tests/beam_ref.py fed with the engine's own logits, then generate(num_beams=K): scores against score_answers, untouched prompt slots, repeatability,
a closed answer set under a constraint, the refusals, generate_latents behind the prompt slot, and the other paths' bits before and after.
The fixture records the other paths' bits and looks at the engine before any beam call: the tests do not depend on their order."""
import numpy as np
import pytest
import torch

import beam_ref as R

from internnav_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, SEQS, N_P = 3, 6, 2
LM_SCALE = 6.0           # lm_head of the synthetic weights scaled: peaked answer distributions, decisions far apart


@pytest.fixture(scope="module")
def setup(built_lib):
    from internnav_amd.policy import InternVLAN1ForCausalLM

    cfg = S.QWEN_TEST_CFG
    sd = {k: v.to(torch.bfloat16) for k, v in S.materialize(S.n1_full_spec(cfg, "nextdit_async"), 5).items()}
    sd["lm_head.weight"] = (sd["lm_head.weight"].float() * LM_SCALE).to(torch.bfloat16)
    inp = S.qwen_inputs(B, 1, seed=33, cfg=cfg, n_text=20, n_tail=12)
    kw = dict(device=DEV, max_envs=SEQS, num_history=3, resize_w=280, resize_h=280, max_seq_len=512, max_patches=SEQS * (inp["pixel_values"].shape[0] // B))
    m = InternVLAN1ForCausalLM(sd, cfg, "nextdit_async", **kw)
    per_img, Sp = inp["pixel_values"].shape[0] // B, inp["input_ids"].shape[1]
    plens = [Sp, Sp - 3]                                           # 2 ragged prompts: prompt 1 loses its last three tokens
    ids = inp["input_ids"][:N_P].clone()
    mask = torch.ones(N_P, Sp, dtype=torch.long)
    ids[1, plens[1]:], mask[1, plens[1]:] = 0, 0
    rag = dict(input_ids=ids, attention_mask=mask, pixel_values=inp["pixel_values"][: N_P * per_img], image_grid_thw=inp["grid_thw"][:N_P], eos_token_id=-1)
    qsd = {k: v.float().cpu() for k, v in sd.items() if not k.startswith("model.traj_dit") and not k.startswith("model.rgb_")}
    special = [cfg[k] for k in ("image_token_id", "traj_token_id", "vision_start_id", "vision_end_id")]
    # what the other paths give on this engine BEFORE any beam call, and that nothing of the beam path exists by then
    g1 = m.generate(**rag, max_new_tokens=4)
    s1 = m.generate(**rag, max_new_tokens=4, do_sample=True, num_return_sequences=3, seed=3, share_prefix=True)
    assert m.qwen._beam is None, "a beam buffer exists before the first beam call"
    return dict(before=(g1.clone(), s1.clone()), m=m, cfg=cfg, rag=rag, plens=plens, Sp=Sp, per_img=per_img, qsd=qsd, special=special)


class _Count:
    def __init__(self, eng, name):
        self.eng, self.name, self.fn, self.n = eng, name, getattr(eng, name), 0
        setattr(eng, name, self)

    def __call__(self, *a, **k):
        self.n += 1
        return self.fn(*a, **k)

    def restore(self):
        delattr(self.eng, self.name)


def _answers(res, plens, n):
    L = res.answer_lengths.cpu().tolist()
    return [res.sequences[r, plens[r // n]: plens[r // n] + L[r]].cpu().tolist() for r in range(res.sequences.shape[0])]


def test_refusals_before_any_launch(setup):
    from internnav_amd.runtime import CapacityError

    m, rag = setup["m"], setup["rag"]
    g1 = setup["before"][0]
    allocated = m.qwen._beam
    assert torch.equal(m.generate(**rag, max_new_tokens=4, num_beams=1), g1), "num_beams=1 is not the greedy path"
    assert m.qwen._beam is allocated, "num_beams=1 allocated beam buffers"
    seven = dict(rag, input_ids=rag["input_ids"][[0, 1, 0, 1, 0, 1, 0]], attention_mask=rag["attention_mask"][[0, 1, 0, 1, 0, 1, 0]])      # 7 prompts, 6 slots
    nine = dict(rag, input_ids=rag["input_ids"][[0, 1] * 4 + [0]], attention_mask=rag["attention_mask"][[0, 1] * 4 + [0]])                # 9 x 8 rows > 64
    c = _Count(m.qwen, "run_prefill")
    try:
        for kw, exc in ((dict(num_beams=9), CapacityError), (dict(num_beams=4, eos_token_id=[1, 2, 3, 4]), CapacityError),
                        (dict(num_beams=3, max_new_tokens=m.qwen.max_decode + 1), CapacityError), (dict(num_beams=3, num_return_sequences=4), ValueError),
                        (dict(num_beams=3, length_penalty=float("nan")), ValueError), (dict(num_beams=3, early_stopping="x"), ValueError),
                        (dict(num_beams=3, share_prefix=False), ValueError), (dict(num_beams=3, export_prefix=[4, 0]), ValueError),
                        (dict(num_beams=3, do_sample=True), NotImplementedError), (dict(num_beams=4, num_beam_groups=2), NotImplementedError),
                        (dict(num_beams=4, diversity_penalty=0.5), NotImplementedError), (dict(num_beams=4, force_words_ids=[[5]]), NotImplementedError)):
            with pytest.raises(exc):
                m.generate(**{**rag, "max_new_tokens": 4, **kw})
        with pytest.raises(CapacityError, match="max_seqs"):         # B > max_seqs
            m.generate(**seven, max_new_tokens=4, num_beams=2)
        slots = m.qwen.B_max
        try:                                                         # B * K > 64 on its own: an engine that claims 16 slots for the length of the check
            m.qwen.B_max = 16
            with pytest.raises(CapacityError, match="64"):
                m.generate(**nine, max_new_tokens=4, num_beams=8)
            with pytest.raises(CapacityError, match="64"):           # the engine's own check, which generate() does not reach
                m.qwen._beam_state(dict(K=8, max_new_tokens=4, eos=(1,)), 9)
        finally:
            m.qwen.B_max = slots
        with pytest.raises(CapacityError, match="max_seqs"):
            m.qwen._beam_state(dict(K=2, max_new_tokens=4, eos=(1,)), 7)
        assert c.n == 0 and m.qwen._beam is allocated, "a refused call prefilled or allocated"
    finally:
        c.restore()


@pytest.mark.parametrize("K,pen", [(3, 1.0), (5, 1.05), (3, 1.05), (5, 1.0)])
def test_decode_step_by_step_against_the_restatement(setup, K, pen):
    m, rag, plens, cfg = setup["m"], setup["rag"], setup["plens"], setup["cfg"]
    eng, T, V = m.qwen, 5, setup["cfg"]["vocab"]
    g = m.generate(**rag, max_new_tokens=4)                        # EOS ids that the search will meet: greedy tokens of the two prompts
    eos = sorted({int(g[0, plens[0] + 1]), int(g[1, plens[1] + 2])})
    M = R.beams_to_keep(K, len(eos))
    pv = rag["pixel_values"].to(DEV, torch.bfloat16)
    state = eng.prefill(rag["input_ids"], pv, rag["image_grid_thw"], seq_lens=np.asarray(plens), beam=dict(K=K, max_new_tokens=T, eos=eos),
                        **({} if pen == 1.0 else {"repetition_penalty": pen}))
    torch.cuda.synchronize()
    cache0 = [L["kv"].clone() for L in eng.layers]
    ref = [R.BeamPrompt(K, eos, T) for _ in range(N_P)]
    prompt_ids = [rag["input_ids"][b, : plens[b]].tolist() for b in range(N_P)]
    tol, tols, compared, moved = 0.0, [], 0, 0
    for j in range(T):
        if all(bp.done for bp in ref):
            break
        if j:                                                      # what the reorder in front of this pass has to re-parent
            bm, Rr, f, t = eng._beam, N_P * K, state["beam"]["flip"], int(state["shared"]["tail_len"])
            old = [ts.clone().view(-1, eng._shared.T, eng.kv_w) for ts in bm.tails[f]]
            par = bm.parent[:Rr].cpu().long()
        eng.decode(state, 1 if j == 0 else 2)
        torch.cuda.synchronize()
        if j:
            # the tails of the pass, independently of the logits: rows [0, t) of row r in the current set are those of row parent[r] in the
            # set the pass before used, bit for bit, in every layer
            assert state["beam"]["flip"] == 1 - f and int(state["shared"]["tail_len"]) == t + 1
            for li, ts in enumerate(bm.tails[1 - f]):
                new = ts.view(-1, eng._shared.T, eng.kv_w)
                for r in range(Rr):
                    assert torch.equal(new[r, :t].view(torch.int16), old[li][int(par[r]), :t].view(torch.int16)), f"step {j} layer {li} row {r}: tail not its parent's"
            moved += int(t > 0 and bool((par != torch.arange(Rr)).any()))
        res = eng.beam_results(state)
        x = eng._shared.logits[: N_P if j == 0 else N_P * K].float().cpu().numpy()
        step_tol = 0.0
        for b, bp in enumerate(ref):
            if bp.done:                                            # frozen: only its finished set is looked at (below)
                continue
            rows = x[b: b + 1] if j == 0 else x[b * K:(b + 1) * K]
            nr = rows.shape[0]
            seen = np.zeros((nr, V), dtype=bool)
            for k in range(nr):
                seen[k, prompt_ids[b] + [int(t) for t in bp.run_tok[k, :j]]] = True
            cs, ct, full = R.topm_rows(rows, bp.run_score[:nr], M, seen=seen if pen != 1.0 else None, penalty=pen)
            for k in range(nr):
                bd = R.cand_bound(rows[k], ct[k], float(bp.run_score[k]), seen[k, ct[k]] if pen != 1.0 else False, pen)
                step_tol = max(step_tol, R.step_tolerance(bd, cs[k]))
            if nr < K:
                cs, ct = np.concatenate([cs, np.full((K - nr, M), -np.inf)]), np.concatenate([ct, np.zeros((K - nr, M), dtype=ct.dtype)])
            bp.step(cs.astype(np.float32), ct)
        tol += step_tol                                            # the bound accumulated over the steps: the tolerance on hypothesis scores
        tols.append(tol)
        for b, bp in enumerate(ref):
            assert bp.margin > 2 * tol, f"K={K} penalty={pen} step {j} prompt {b}: a decision of the reference rests on a gap of {bp.margin:.3e} (2 x bound {2 * tol:.3e})"
            L = bp.fin_len
            assert res.lengths[b].tolist() == L.tolist() and res.finished[b].tolist() == bp.fin_flag.tolist(), (j, b, res.lengths[b], L)
            for k in range(K):
                assert res.tokens[b, k, : L[k]].tolist() == bp.fin_tok[k, : L[k]].tolist(), (j, b, k)
                if bp.fin_flag[k]:
                    ft = R.finished_tolerance(tols[L[k] - 1], float(bp.fin_score[k]), int(L[k]), bp.lp)      # (accumulated up to the step it finished in)
                    assert abs(float(res.scores[b, k]) - float(bp.fin_score[k])) <= ft, (j, b, k, res.scores[b, k], bp.fin_score[k], ft)
                    compared += 1
            assert bool(res.done[b]) == bp.done and bool(res.heur[b]) == bp.flag, (j, b)
            if bp.step_idx == j + 1:                               # stepped in this round: the running rows
                assert res.run_tokens[b].tolist() == bp.run_tok[:, : j + 1].tolist(), (j, b, res.run_tokens[b], bp.run_tok)
                assert res.parents[b].tolist() == bp.parent.tolist(), (j, b)
                live = bp.run_score > -1e8
                assert np.all(np.abs(res.run_scores[b].numpy()[live] - bp.run_score[live]) <= tol), (j, b, res.run_scores[b], bp.run_score, tol)
    assert all(bp.done for bp in ref) and compared > 0
    assert moved > 0, "no step re-parented a row with a tail: the tail check above compared nothing that moved"
    torch.cuda.synchronize()
    for i, L in enumerate(eng.layers):                             # the prompts' cache slots hold exactly what the prefill wrote
        assert torch.equal(L["kv"].view(torch.int16), cache0[i].view(torch.int16)), f"layer {i}: the KV cache was written by the search"
    print(f"K={K} penalty={pen}: smallest decision gap {min(bp.margin for bp in ref):.3e}, accumulated bound {tol:.3e}, steps {[bp.step_idx for bp in ref]}")


def test_scores_against_score_answers_and_repeatable(setup):
    m, rag, plens, special = setup["m"], setup["rag"], setup["plens"], setup["special"]
    g = m.generate(**rag, max_new_tokens=4)
    eos = [int(g[0, plens[0] + 2]), int(g[1, plens[1] + 1])]
    K, n, lp = 4, 3, 2.0
    kw = dict(max_new_tokens=4, num_beams=K, num_return_sequences=n, length_penalty=lp, return_dict_in_generate=True, output_logprobs=True, repetition_penalty=1.0)
    res = m.generate(**{**rag, "eos_token_id": eos}, **kw)
    assert res.past_key_values is None and res.sequences.shape[0] == N_P * n and bool(res.valid.all())
    ans = _answers(res, plens, n)
    assert not any(t in special for a in ans for t in a), "an answer holds a vision marker (score_answers would read it as an image)"
    assert len({(r // n, tuple(a)) for r, a in enumerate(ans)}) == N_P * n, "the hypotheses of a prompt are not distinct"
    sc = res.sequences_scores.cpu()
    for b in range(N_P):
        assert bool((sc[b * n:(b + 1) * n][:-1] >= sc[b * n:(b + 1) * n][1:]).all()), "not best first"
    res2 = m.generate(**{**rag, "eos_token_id": eos}, **kw)
    for name in ("sequences", "sequences_scores", "token_logprobs", "answer_lengths", "valid"):
        a, b_ = getattr(res, name), getattr(res2, name)
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b_.view(torch.int32) if b_.dtype == torch.float32 else b_), f"a second call gives another {name}"
    score = m.score_answers(rag["input_ids"], [[ans[b * n + c] for c in range(n)] for b in range(N_P)], pixel_values=rag["pixel_values"],
                            image_grid_thw=rag["image_grid_thw"], attention_mask=rag["attention_mask"], share_prefix=True)
    worst = worst_s = 0.0
    for r, a in enumerate(ans):
        b, c, L = r // n, r % n, len(a)
        want = score.token_logprobs[b][c].float().cpu()
        got = res.token_logprobs[r, :L].cpu()
        d = float((want - got).abs().max())
        worst = max(worst, d)
        assert d <= 0.10, f"prompt {b} hypothesis {c}: {got.tolist()} against score_answers {want.tolist()}"
        assert bool((res.token_logprobs[r, L:] == 0).all())
        ds = abs(float(sc[r]) * L ** lp - float(want.sum()))
        worst_s = max(worst_s, ds)
        assert ds <= 0.10, (r, float(sc[r]), float(want.sum()))
        assert abs(float(got.double().sum()) / L ** lp - float(sc[r])) <= 1e-5 * max(1.0, abs(float(sc[r])))
    print(f"K={K}: max |transition score - score_answers| = {worst:.3e}, max |sequences_scores x len**lp - sum| = {worst_s:.3e} (tolerance 0.10 each)")


def test_constraint_closed_answer_set(setup):
    from internnav_amd.constrain import TokenAutomaton

    m, rag, plens, cfg = setup["m"], setup["rag"], setup["plens"], setup["cfg"]
    eos, K = 7, 6
    closed = [[11], [11, 12], [13, 14, 15], [13, 14, 16, 17], [20, 21], [22]]
    aut = TokenAutomaton.from_token_sequences(closed, [eos], cfg["vocab"])
    res = m.generate(**{**rag, "eos_token_id": eos}, max_new_tokens=5, num_beams=K, num_return_sequences=K, constraint=aut, return_dict_in_generate=True,
                     output_logprobs=True)
    ans, valid, sc = _answers(res, plens, K), res.valid.cpu().tolist(), res.sequences_scores.cpu()
    members = {tuple(a + [eos]) for a in closed}
    for b in range(N_P):
        rows = [r for r in range(b * K, (b + 1) * K) if valid[r]]
        assert len(rows) >= 1
        assert all(tuple(ans[r]) in members for r in rows), [ans[r] for r in rows]
        assert len({tuple(ans[r]) for r in rows}) == len(rows), "two valid hypotheses are the same answer"
        s = sc[b * K:(b + 1) * K]
        assert bool((s[:-1] >= s[1:]).all()), s
        for r in range(b * K, (b + 1) * K):
            if not valid[r]:
                assert float(sc[r]) == -float("inf") and bool((res.sequences[r, plens[b]:] == eos).all())
    print(f"constraint: valid hypotheses per prompt {[sum(valid[b * K:(b + 1) * K]) for b in range(N_P)]} of {K}")


def test_generate_latents_behind_the_prompt_slot(setup):
    from oracle import qwen_vl as o_q

    s, m, rag, plens, per = setup, setup["m"], setup["rag"], setup["plens"], setup["per_img"]
    eng, K, n = m.qwen, 4, 2
    res = m.generate(**rag, max_new_tokens=4, num_beams=K, num_return_sequences=n, return_dict_in_generate=True)
    ans = _answers(res, plens, n)
    assert not any(t in s["special"] for a in ans for t in a)
    rows = [3, 0, 3]
    torch.cuda.synchronize()
    before = [L["kv"].clone() for L in eng.layers] + [t.clone() for ts in eng._beam.tails for t in ts]
    cp, cv = _Count(eng, "run_prefill"), _Count(eng, "run_vision")
    try:
        lat = m.generate_latents(res.sequences, rag["pixel_values"], rag["image_grid_thw"], rows=rows)
        lat2 = m.generate_latents(res.sequences, rag["pixel_values"], rag["image_grid_thw"], rows=rows)
        assert cp.n == 0 and cv.n == 0, "generate_latents after a beam call re-ran the prompt or the vision tower"
    finally:
        cp.restore()
        cv.restore()
    torch.cuda.synchronize()
    now = [L["kv"] for L in eng.layers] + [t for ts in eng._beam.tails for t in ts]
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(now, before)), "the cache or a tail was written"
    assert torch.equal(lat.view(torch.int16), lat2.view(torch.int16)) and torch.equal(lat[0].view(torch.int16), lat[2].view(torch.int16))
    worst = 0.0
    for j, r in enumerate(rows[:2]):
        b = r // n
        ids = torch.cat([rag["input_ids"][b, : plens[b]], torch.tensor(ans[r])])
        with torch.no_grad():
            ref = o_q.generate_latents(s["qsd"], s["cfg"], ids[None], rag["pixel_values"][b * per:(b + 1) * per], rag["image_grid_thw"][b:b + 1])[0]
        d = (lat[j].float().cpu() - ref).abs().mean().item()
        bound = 1e-2 * ref.pow(2).mean().sqrt().item()
        worst = max(worst, d / bound)
        assert d < bound, f"row {r}: mean|err| {d:.3e} against 1e-2 x rms(ref) = {bound:.3e}"
    print(f"latents behind the prompt slot: worst mean|err| / (1e-2 x rms) = {worst:.3f}")


def test_other_paths_give_the_bits_they_gave_before(setup):
    m, rag = setup["m"], setup["rag"]
    g1, s1 = setup["before"]
    assert torch.equal(m.generate(**rag, max_new_tokens=4), g1), "greedy generate changed after beam calls"
    assert torch.equal(m.generate(**rag, max_new_tokens=4, do_sample=True, num_return_sequences=3, seed=3, share_prefix=True), s1), "sampled generate changed"
