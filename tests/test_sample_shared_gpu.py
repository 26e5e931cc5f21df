"""GPU: generate(do_sample=True, share_prefix=True) on the 2-layer test model - K sampled answers per prompt decoded behind the prompt's ONE cache
slot (ops.attention_shared over per-row answer tails, the selection on row-count-sized twins of the max_seqs-sized buffers): capacity beyond
max_seqs, the draws' log-probabilities against score_answers, the exact equalities that follow from the kernel's bit isolation, greedy tokens up
to small margins, per-row seen sets, an untouched cache, repeatability, and what the path leaves behind. The tests of this file run in order:
the first one looks at the engine before any shared call."""
import numpy as np
import pytest
import torch

import decode_penalty_ref as R

from internnav_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, SEQS, N_P = 3, 6, 2
TWINS = ("logits", "next_tok", "seen", "xl", "hl", "_smp_lp")


@pytest.fixture(scope="module")
def setup(built_lib):
    from internnav_amd.policy import InternVLAN1ForCausalLM

    cfg = S.QWEN_TEST_CFG
    sd = {k: v.to(torch.bfloat16) for k, v in S.materialize(S.n1_full_spec(cfg, "nextdit_async"), 5).items()}
    inp = S.qwen_inputs(B, 1, seed=33, cfg=cfg, n_text=20, n_tail=12)
    kw = dict(device=DEV, max_envs=SEQS, num_history=3, resize_w=280, resize_h=280, max_seq_len=512, max_patches=SEQS * (inp["pixel_values"].shape[0] // B))
    m = InternVLAN1ForCausalLM(sd, cfg, "nextdit_async", **kw)
    # 2 ragged prompts: prompt 1 loses its last three tokens
    per_img, Sp = inp["pixel_values"].shape[0] // B, inp["input_ids"].shape[1]
    plens = [Sp, Sp - 3]
    ids = inp["input_ids"][:N_P].clone()
    mask = torch.ones(N_P, Sp, dtype=torch.long)
    ids[1, plens[1]:], mask[1, plens[1]:] = 0, 0
    rag = dict(input_ids=ids, attention_mask=mask, pixel_values=inp["pixel_values"][: N_P * per_img], image_grid_thw=inp["grid_thw"][:N_P], eos_token_id=-1)
    return dict(m=m, cfg=cfg, sd=sd, kw=kw, inp=inp, rag=rag, plens=plens, Sp=Sp)


def _answers(seqs, plens, K, n_new):
    return [seqs[r, plens[r // K]: plens[r // K] + n_new] for r in range(seqs.shape[0])]


def _marker_free_draw(m, cfg, rag, plens, K, n_new, **kw):
    """test data: answers free of image / vision markers, which score_answers would read as images (the seed loop of test_sample_decode_gpu)"""
    special = torch.tensor([cfg[k] for k in ("image_token_id", "traj_token_id", "vision_start_id", "vision_end_id")], device=DEV)
    for seed in range(8):
        res = m.generate(**rag, max_new_tokens=n_new, return_dict_in_generate=True, do_sample=True, temperature=1.0, top_k=0, top_p=1.0,
                         repetition_penalty=1.0, num_return_sequences=K, seed=seed, output_logprobs=True, share_prefix=True, **kw)
        rows = _answers(res.sequences, plens, K, n_new)
        if not any(bool(torch.isin(t, special).any()) for t in rows):
            return res, rows
    pytest.fail("eight seeds in a row drew a vision marker")


def test_capacity_beyond_max_seqs_and_nothing_allocated_before(setup):
    from internnav_amd.runtime import CapacityError

    m, rag, plens, Sp = setup["m"], setup["rag"], setup["plens"], setup["Sp"]
    greedy = m.generate(**rag, max_new_tokens=4)
    m.generate(**rag, max_new_tokens=4, do_sample=True, num_return_sequences=2, seed=0)         # the fan-out path: 4 rows on 6 slots
    assert m.qwen._shared is None, "a twin buffer or a tail exists before the first shared call"
    K, n_new = 5, 4                                                                              # 10 rows on 6 slots
    with pytest.raises(CapacityError, match="max_seqs"):                                         # today's behaviour, and still the default's
        m.generate(**rag, max_new_tokens=n_new, do_sample=True, num_return_sequences=K, seed=0)
    out = m.generate(**rag, max_new_tokens=n_new, do_sample=True, num_return_sequences=K, seed=0, share_prefix=True, temperature=1.0, top_k=0, top_p=1.0)
    assert out.shape == (N_P * K, Sp + n_new)
    for r in range(N_P * K):                                                                     # prompt-major
        b = r // K
        assert torch.equal(out[r, : plens[b]].cpu(), rag["input_ids"][b, : plens[b]]), f"row {r} does not start with prompt {b}"
    assert len({tuple(t.tolist()) for t in _answers(out, plens, K, n_new)}) > N_P, "the K sequences of a prompt are all the same at T = 1"
    sh = m.qwen._shared
    assert sh is not None and sh.rows == N_P * K and sh.T == n_new and len(sh.tails) == len(m.qwen.layers)
    assert all(getattr(sh, n).shape[0] == N_P * K for n in TWINS if n != "_smp_lp") and sh._smp_lp.shape == (n_new, N_P * K)
    assert all(t.shape == (N_P * K * n_new, m.qwen.kv_w) for t in sh.tails)
    # a smaller call reuses the set, a longer answer grows it
    m.generate(**rag, max_new_tokens=3, do_sample=True, num_return_sequences=2, seed=0, share_prefix=True)
    assert m.qwen._shared is sh
    m.generate(**rag, max_new_tokens=6, do_sample=True, num_return_sequences=2, seed=0, share_prefix=True)
    assert m.qwen._shared is not sh and (m.qwen._shared.rows, m.qwen._shared.T) == (N_P * K, 6)
    with pytest.raises(CapacityError, match="64"):
        m.generate(**rag, max_new_tokens=2, do_sample=True, num_return_sequences=33, share_prefix=True)
    with pytest.raises(ValueError, match="do_sample"):
        m.generate(**rag, max_new_tokens=2, share_prefix=True)
    # a greedy generate after shared calls is what it was before
    assert torch.equal(m.generate(**rag, max_new_tokens=4), greedy)


def test_draw_logprobs_agree_with_score_answers(setup):
    m, cfg, rag, plens = setup["m"], setup["cfg"], setup["rag"], setup["plens"]
    K, n_new = 3, 4
    res, rows = _marker_free_draw(m, cfg, rag, plens, K, n_new)
    assert res.sequences.shape == (N_P * K, setup["Sp"] + n_new) and res.token_logprobs.shape == (N_P * K, n_new) and res.past_key_values is None
    assert bool((res.token_logprobs < 0).all()) and torch.equal(res.answer_lengths.cpu(), torch.full((N_P * K,), n_new))
    assert bool(torch.isnan(res.token_margins).all())
    answers = [[rows[b * K + c].tolist() for c in range(K)] for b in range(N_P)]
    sc_kw = {k: rag[k] for k in ("pixel_values", "image_grid_thw", "attention_mask")}
    worst = 0.0
    for share in (False, True):
        sc = m.score_answers(rag["input_ids"], answers, share_prefix=share, **sc_kw)
        for b in range(N_P):
            for c in range(K):
                d = (sc.token_logprobs[b][c] - res.token_logprobs[b * K + c]).abs().max().item()
                worst = max(worst, d)
                assert d <= 0.10, f"prompt {b} sequence {c} (score share_prefix={share}): {sc.token_logprobs[b][c].tolist()} vs {res.token_logprobs[b * K + c].tolist()}"
    print(f"share_prefix K={K}: max |draw logprob - score_answers| = {worst:.3e} (tolerance 0.10)")


def test_rows_of_a_prompt_are_bit_isolated_and_calls_repeat(setup):
    m, rag, plens = setup["m"], setup["rag"], setup["plens"]
    K = 3
    # top_k = 1 under a penalty: the K rows of a prompt see the same prompt, draw the same tokens and keep equal tails - they are equal to each
    # other and to the K = 1 call only if a row's bits do not depend on what shares its tile
    kw = dict(rag, max_new_tokens=6, repetition_penalty=1.3, do_sample=True, top_k=1, share_prefix=True)
    pk = m.generate(**kw, num_return_sequences=K, seed=3)
    p1 = m.generate(**kw, num_return_sequences=1, seed=5)
    assert pk.shape == (N_P * K, p1.shape[1]) and p1.shape[0] == N_P
    for r in range(N_P * K):
        assert torch.equal(pk[r], pk[r // K * K]), f"row {r} differs from the first row of prompt {r // K}"
        assert torch.equal(pk[r], p1[r // K]), f"row {r} differs from the K = 1 call of prompt {r // K}"
    # the same seed twice, through seed= and a generator; chunked decoding walks the same table of uniforms and the same tails
    kw = dict(rag, max_new_tokens=6, repetition_penalty=1.05, do_sample=True, temperature=1.5, top_k=0, top_p=1.0, num_return_sequences=K, share_prefix=True,
              return_dict_in_generate=True, output_logprobs=True)
    a = m.generate(**kw, seed=11)
    b = m.generate(**kw, generator=torch.Generator().manual_seed(11))
    c = m.generate(**kw, seed=11, decode_chunk=2)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.token_logprobs, b.token_logprobs)
    assert torch.equal(a.sequences, c.sequences) and torch.equal(a.token_logprobs, c.token_logprobs)
    assert not torch.equal(a.sequences, m.generate(**kw, seed=12).sequences), "another seed at T = 1.5 gives the same sequences"


def test_seen_sets_are_per_returned_sequence(setup):
    m, cfg, rag, plens = setup["m"], setup["cfg"], setup["rag"], setup["plens"]
    K = 3
    hot = m.generate(**rag, max_new_tokens=6, repetition_penalty=1.3, do_sample=True, temperature=1.5, top_k=0, top_p=1.0, num_return_sequences=K, seed=4,
                     share_prefix=True)
    seqs, lens = hot.cpu().numpy(), [plens[r // K] + 6 for r in range(N_P * K)]
    assert len({tuple(seqs[r, plens[r // K]: lens[r]]) for r in range(N_P * K)}) == N_P * K, "test data: two of the sequences are the same"
    nw = (cfg["vocab"] + 31) // 32
    got = m.qwen._shared.seen[: N_P * K].view(torch.int32).cpu().numpy().view(np.uint32)[:, :nw]
    assert np.array_equal(got, R.seen_bitmap(seqs, lens, cfg["vocab"])), "a returned sequence's seen set is not its prompt + its own answer"


def test_engine_decode_leaves_every_cache_tensor_bit_equal(setup):
    m, rag, plens = setup["m"], setup["rag"], setup["plens"]
    eng, K, n = m.qwen, 3, 5
    u = torch.rand(n, N_P * K, generator=torch.Generator().manual_seed(1), dtype=torch.float32).to(DEV)
    st = eng.prefill(rag["input_ids"], rag["pixel_values"].to(DEV, torch.bfloat16), rag["image_grid_thw"], seq_lens=np.asarray(plens),
                     repetition_penalty=1.1, sampling=dict(temperature=1.0, top_k=0, top_p=1.0, u=u, K=K, share_prefix=True))
    torch.cuda.synchronize()
    before = [L["kv"].clone() for L in eng.layers]
    toks = eng.decode(st, n)
    torch.cuda.synchronize()
    assert toks.shape == (N_P * K, n) and st["B"] == N_P * K and st["shared"]["tail_len"] == n - 1
    assert st["shared"]["slot"].tolist() == [0, 0, 0, 1, 1, 1] and st["shared"]["pfx_len"].tolist() == [plens[0]] * 3 + [plens[1]] * 3
    for li, (L, kv) in enumerate(zip(eng.layers, before)):
        assert torch.equal(L["kv"].view(torch.int16), kv.view(torch.int16)), f"layer {li}: the shared decode wrote the cache"
    assert eng.last_sample_logprobs(st).shape == (N_P * K, n)


def test_top_k_1_follows_greedy_up_to_small_margins(setup):
    """the new kernel is not bit-equal to the decode kernel: a token may differ from greedy only where the greedy top-2 margin is below 0.10 logits
    (twice the 0.05 logit tolerance of test_qwen_gpu.py: a flip needs both paths' logits to move by half the margin). Rows are compared up to
    their first differing token; the prompt seed is one whose greedy margins leave at least half of the compared positions decidable."""
    from internnav_amd.policy import InternVLAN1ForCausalLM

    m, cfg = setup["m"], setup["cfg"]
    with_lp = InternVLAN1ForCausalLM(setup["sd"], cfg, "nextdit_async", token_logprobs=True, **setup["kw"])
    K, n_new = 3, 6
    for seed in (33, 34, 35, 36, 37, 38):
        inp = S.qwen_inputs(N_P, 1, seed=seed, cfg=cfg, n_text=20, n_tail=12)
        kw = dict(input_ids=inp["input_ids"], pixel_values=inp["pixel_values"], image_grid_thw=inp["grid_thw"], max_new_tokens=n_new, eos_token_id=-1,
                  repetition_penalty=1.0)
        g = with_lp.generate(**kw, return_dict_in_generate=True, output_logprobs=True)
        Sp = inp["input_ids"].shape[1]
        assert torch.equal(g.sequences, m.generate(**kw))
        margins = g.token_margins.cpu().numpy()
        if (margins >= 0.10).mean() < 0.75:                                   # (of the greedy path alone: nothing of the path under test is looked at)
            continue
        out = m.generate(**kw, do_sample=True, top_k=1, num_return_sequences=K, seed=0, share_prefix=True)
        want, got = g.sequences[:, Sp:].cpu().numpy(), out[:, Sp:].cpu().numpy()
        compared = decidable = equal = 0
        for r in range(N_P * K):
            b = r // K
            diff = np.nonzero(got[r] != want[b])[0]
            stop = int(diff[0]) if diff.size else n_new
            equal += stop
            compared += min(stop + 1, n_new)
            decidable += int((margins[b, : min(stop + 1, n_new)] >= 0.10).sum())
            if diff.size:
                assert margins[b, stop] < 0.10, (f"seed {seed} row {r} token {stop}: {got[r, stop]} against greedy {want[b, stop]} at a top-2 margin of "
                                                 f"{margins[b, stop]:.3f} logits")
        print(f"seed {seed}: {equal} of {N_P * K * n_new} tokens equal to greedy before a first difference, {decidable} of {compared} compared positions "
              f"have a margin >= 0.10")
        assert 2 * decidable >= compared, f"only {decidable} of {compared} compared positions have a greedy margin >= 0.10"
        return
    pytest.fail("no prompt seed whose greedy margins are >= 0.10 at three quarters of the positions")


def test_w8_decode_engine_draws_what_it_scores(setup):
    from internnav_amd.policy import InternVLAN1ForCausalLM

    cfg, rag, plens = setup["cfg"], setup["rag"], setup["plens"]
    m8 = InternVLAN1ForCausalLM(setup["sd"], cfg, "nextdit_async", w8_decode=True, **setup["kw"])
    K, n_new = 3, 4
    res, rows = _marker_free_draw(m8, cfg, rag, plens, K, n_new)
    answers = [[rows[b * K + c].tolist() for c in range(K)] for b in range(N_P)]
    sc = m8.score_answers(rag["input_ids"], answers, share_prefix=True, **{k: rag[k] for k in ("pixel_values", "image_grid_thw", "attention_mask")})
    worst = max((sc.token_logprobs[b][c] - res.token_logprobs[b * K + c]).abs().max().item() for b in range(N_P) for c in range(K))
    print(f"w8_decode share_prefix K={K}: max |draw logprob - score_answers(share_prefix=True)| = {worst:.3e} (tolerance 0.10)")
    assert worst <= 0.10
