"""GPU: generate(do_sample=True) on the 2-layer test model - the sampling launch in the decode chain, num_return_sequences behind one prefill (KV
fan-out, src mapping), the log-probabilities of the draws against score_answers, and the refusals of the public surface."""
import numpy as np
import pytest
import torch

import decode_penalty_ref as R

from internnav_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, SEQS = 3, 6


@pytest.fixture(scope="module")
def model(built_lib):
    from internnav_amd.policy import InternVLAN1ForCausalLM

    cfg = S.QWEN_TEST_CFG
    sd = {k: v.to(torch.bfloat16) for k, v in S.materialize(S.n1_full_spec(cfg, "nextdit_async"), 5).items()}
    inp = S.qwen_inputs(B, 1, seed=33, cfg=cfg, n_text=20, n_tail=12)
    m = InternVLAN1ForCausalLM(sd, cfg, "nextdit_async", device=DEV, max_envs=SEQS, num_history=3, resize_w=280, resize_h=280, max_seq_len=512,
                               max_patches=SEQS * (inp["pixel_values"].shape[0] // B))          # (no token_logprobs: sampling keeps its own buffer)
    return m, cfg, inp


def _kw(inp, **extra):
    return dict(input_ids=inp["input_ids"], pixel_values=inp["pixel_values"], image_grid_thw=inp["grid_thw"], max_new_tokens=6, eos_token_id=-1,
                return_dict_in_generate=True, **extra)


def test_top_k_1_is_greedy_and_seeds_repeat(model):
    m, cfg, inp = model
    assert m.qwen._smp_lp is None, "a sampling buffer exists before the first sampling call"
    greedy = m.generate(**_kw(inp, repetition_penalty=1.05))
    s = m.generate(**_kw(inp, repetition_penalty=1.05, do_sample=True, top_k=1, output_logprobs=True))
    assert torch.equal(s.sequences, greedy.sequences), "top_k = 1 draws the greedy tokens"
    assert s.token_logprobs.shape == (B, 6) and bool((s.token_logprobs == 0.0).all()) and bool((s.sequences_logprob == 0.0).all())
    assert s.token_margins.shape == (B, 6) and bool(torch.isnan(s.token_margins).all())         # not defined for a draw
    assert s.past_key_values is not None
    # the same seed twice, through seed= and through a generator; chunked decoding walks the same table of uniforms
    kw = _kw(inp, do_sample=True, temperature=1.5, top_k=0, top_p=1.0, repetition_penalty=1.05, output_logprobs=True)
    a = m.generate(**kw, seed=11)
    b = m.generate(**kw, generator=torch.Generator().manual_seed(11))
    c = m.generate(**kw, seed=11, decode_chunk=2)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.token_logprobs, b.token_logprobs)
    assert torch.equal(a.sequences, c.sequences) and torch.equal(a.token_logprobs, c.token_logprobs)
    assert bool((a.token_logprobs < 0).all())
    d = m.generate(**kw, seed=12)
    assert not torch.equal(a.sequences, d.sequences), "another seed at T = 1.5 gives another sequence"
    # the model's own generator advances per call; greedy after sampling is what it was
    e, f = m.generate(**kw), m.generate(**kw)
    assert not torch.equal(e.sequences, f.sequences)
    again = m.generate(**_kw(inp, repetition_penalty=1.05))
    assert torch.equal(again.sequences, greedy.sequences)
    assert torch.equal(m.generate(**dict(kw, return_dict_in_generate=False), seed=11), a.sequences)


def test_num_return_sequences_behind_one_prefill(model):
    m, cfg, inp = model
    n_p, K, n_new, per_img = 2, 3, 4, inp["pixel_values"].shape[0] // B
    Sp = inp["input_ids"].shape[1]
    plens = [Sp, Sp - 3]                                                    # ragged: prompt 1 loses its last three tokens
    ids = inp["input_ids"][:n_p].clone()
    mask = torch.ones(n_p, Sp, dtype=torch.long)
    ids[1, plens[1]:], mask[1, plens[1]:] = 0, 0
    pv, grid = inp["pixel_values"][: n_p * per_img], inp["grid_thw"][:n_p]
    special = torch.tensor([cfg[k] for k in ("image_token_id", "traj_token_id", "vision_start_id", "vision_end_id")], device=DEV)
    for seed in range(8):                                                   # test data: answers free of image / vision markers, which score_answers would read as images
        res = m.generate(input_ids=ids, attention_mask=mask, pixel_values=pv, image_grid_thw=grid, max_new_tokens=n_new, eos_token_id=-1,
                         return_dict_in_generate=True, do_sample=True, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0,
                         num_return_sequences=K, seed=seed, output_logprobs=True)
        rows = [res.sequences[r, plens[r // K]: plens[r // K] + n_new] for r in range(n_p * K)]
        if not any(bool(torch.isin(t, special).any()) for t in rows):
            break
    else:
        pytest.fail("eight seeds in a row drew a vision marker")
    assert res.sequences.shape == (n_p * K, Sp + n_new) and res.token_logprobs.shape == (n_p * K, n_new) and res.past_key_values is None
    for r in range(n_p * K):                                                # prompt-major: rows b * K .. b * K + K - 1 belong to prompt b
        b = r // K
        assert torch.equal(res.sequences[r, : plens[b]].cpu(), ids[b, : plens[b]]), f"row {r} does not start with prompt {b}"
    assert len({tuple(t.tolist()) for t in rows}) > n_p, "the K sequences of a prompt are all the same at T = 1"
    assert bool((res.token_logprobs < 0).all()) and torch.equal(res.answer_lengths.cpu(), torch.full((n_p * K,), n_new))
    # the draws' log-probabilities against teacher-forced scoring of the same answers on the same model (penalty 1.0: the same distribution):
    # a wrong cache row after the fan-out, or a draw taken from the wrong logits row, moves them by far more than 0.10
    answers = [[rows[b * K + c].tolist() for c in range(K)] for b in range(n_p)]
    worst = 0.0
    for share in (False, True):
        sc = m.score_answers(ids, answers, pixel_values=pv, image_grid_thw=grid, attention_mask=mask, share_prefix=share)
        for b in range(n_p):
            for c in range(K):
                d = (sc.token_logprobs[b][c] - res.token_logprobs[b * K + c]).abs().max().item()
                worst = max(worst, d)
                assert d <= 0.10, f"prompt {b} sequence {c} (share_prefix={share}): {sc.token_logprobs[b][c].tolist()} vs {res.token_logprobs[b * K + c].tolist()}"
    print(f"num_return_sequences={K}: max |draw logprob - score_answers| = {worst:.3e} (tolerance 0.10)")
    # with a repetition penalty every returned sequence has a seen set of its own (replicated before the first draw, marked per row):
    # at top_k = 1 each of the K sequences of a prompt is that prompt's greedy answer under the same penalty
    kw = dict(input_ids=ids, attention_mask=mask, pixel_values=pv, image_grid_thw=grid, max_new_tokens=6, eos_token_id=-1, repetition_penalty=1.3)
    pen = m.generate(**kw)
    pk = m.generate(**kw, do_sample=True, top_k=1, num_return_sequences=K, seed=3)
    assert pk.shape == (n_p * K, pen.shape[1])
    for r in range(n_p * K):
        assert torch.equal(pk[r], pen[r // K]), f"row {r}: the penalised top_k = 1 draw differs from prompt {r // K}'s greedy answer"
    # ... and after a call whose K sequences differ, row b * K + c of the engine's seen sets is exactly prompt b's tokens plus ITS OWN answer
    hot = m.generate(**kw, do_sample=True, temperature=1.5, top_k=0, top_p=1.0, num_return_sequences=K, seed=4)
    seqs, lens = hot.cpu().numpy(), [plens[r // K] + 6 for r in range(n_p * K)]
    assert len({tuple(seqs[r, plens[r // K]: lens[r]]) for r in range(n_p * K)}) == n_p * K, "test data: two of the sequences are the same"
    nw = (cfg["vocab"] + 31) // 32
    got = m.qwen.seen[: n_p * K].view(torch.int32).cpu().numpy().view(np.uint32)[:, :nw]
    assert np.array_equal(got, R.seen_bitmap(seqs, lens, cfg["vocab"])), "a returned sequence's seen set is not its prompt + its own answer"
    # greedy afterwards is what a fresh call gives (the fan-out left nothing behind)
    g1 = m.generate(**_kw(inp))
    g2 = m.generate(**_kw(inp))
    assert torch.equal(g1.sequences, g2.sequences)


def test_refusals_and_generation_config(model):
    from internnav_amd.policy import generation_config_from_hf
    from internnav_amd.runtime import CapacityError

    m, cfg, inp = model
    with pytest.raises(CapacityError, match="max_seqs"):
        m.generate(**_kw(inp, do_sample=True, num_return_sequences=3))     # 3 x 3 > 6 sequences
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.generate(**_kw(inp, num_return_sequences=2))
    with pytest.raises(ValueError, match="temperature"):
        m.generate(**_kw(inp, do_sample=True, temperature=0.0))
    for key, v in (("min_p", 0.05), ("typical_p", 0.9), ("epsilon_cutoff", 3e-4), ("eta_cutoff", 1e-3)):
        with pytest.raises(NotImplementedError, match=key):
            m.generate(**_kw(inp, do_sample=True, **{key: v}))
        m.generate(**_kw(inp, **{key: v}))                                  # greedy ignores it, as HF does
    with pytest.raises(ValueError, match="export_prefix"):
        m.generate(**_kw(inp, do_sample=True, num_return_sequences=2, export_prefix=[4, 0, 0]))
    greedy = m.generate(**_kw(inp))
    keep = m.generation_config
    try:
        # the file's sampling keys: ignored by greedy, taken by do_sample=True (top_k = 1 from the file makes the draw greedy whatever u is;
        # HF's default top_k = 50 at this temperature does not)
        m.generation_config = generation_config_from_hf({"do_sample": True, "temperature": 3.0, "top_k": 1, "top_p": 0.5}, cfg["eos_token_id"])
        assert torch.equal(m.generate(**_kw(inp)).sequences, greedy.sequences)
        assert torch.equal(m.generate(**_kw(inp, do_sample=True, seed=5)).sequences, greedy.sequences)
        assert not torch.equal(m.generate(**_kw(inp, do_sample=True, top_k=50, top_p=1.0, seed=5)).sequences, greedy.sequences)
        m.generation_config = generation_config_from_hf({"min_p": 0.1}, cfg["eos_token_id"])
        assert torch.equal(m.generate(**_kw(inp)).sequences, greedy.sequences)
        with pytest.raises(NotImplementedError, match="min_p"):
            m.generate(**_kw(inp, do_sample=True))
    finally:
        m.generation_config = keep
