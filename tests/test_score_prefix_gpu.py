"""GPU: InternVLAN1ForCausalLM.score_answers(share_prefix=True) - every prompt prefilled once, the candidates' tokens as a suffix pass whose
attention (ops.attention_prefix) reads the prompt's K/V in place - against the fp32 oracle (oracle/qwen_vl.py), with the construction of
test_token_logprobs_gpu.test_score_answers_against_the_fp32_oracle: candidates chosen with the oracle alone, tolerance 2 * 5e-2 * std(oracle
logits) (test_qwen_gpu.py bounds the logit error of this configuration by 5e-2 * std; a logit error eps moves a log-softmax entry by <= 2 eps)."""
import numpy as np
import pytest
import torch

from internnav_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N_P = 3, 2            # engine of 3 sequences, two prompts


def _oracle_case(qsd, cfg, ids, pv, grid, per_img, prompts):
    """per prompt three candidates of 3 / 2 / 1 tokens - the oracle's greedy answer, two least likely tokens, the greedy first token alone (it
    shares its first token with candidate 0) - and the oracle's float64 log-probabilities of their tokens. -> answers, want, logit std"""
    from oracle import qwen_vl as o_q

    Sp = ids.shape[1]
    answers, want, scale = [], [], []
    lsm = lambda row, t: float(torch.log_softmax(row.double(), -1)[t])
    with torch.no_grad():
        for b in prompts:
            pvb, gb, idb = pv[b * per_img:(b + 1) * per_img].float(), grid[b:b + 1], ids[b:b + 1]
            greedy = o_q.generate(qsd, cfg, idb, pvb, gb, 3)[0, Sp:].tolist()
            lg, _ = o_q.forward_logits(qsd, cfg, torch.cat([idb, torch.tensor([greedy])], 1), pvb, gb)
            rows = lg[0, Sp - 1: Sp + 2]                                   # the rows that predict the three greedy tokens
            u0 = int(rows[0].argmin())
            lu, _ = o_q.forward_logits(qsd, cfg, torch.cat([idb, torch.tensor([[u0]])], 1), pvb, gb)
            u1 = int(lu[0, -1].argmin())
            answers.append([greedy, [u0, u1], greedy[:1]])
            want.append([np.asarray([lsm(rows[i], greedy[i]) for i in range(3)]), np.asarray([lsm(rows[0], u0), lsm(lu[0, -1], u1)]),
                         np.asarray([lsm(rows[0], greedy[0])])])
            scale += [float(rows.double().std()), float(lu[0, Sp - 1:].double().std())]
    return answers, want, max(scale)


@pytest.fixture(scope="module")
def setup(built_lib):
    from internnav_amd.policy import InternVLAN1ForCausalLM

    cfg = S.QWEN_TEST_CFG
    sd = {k: v.to(torch.bfloat16) for k, v in S.materialize(S.n1_full_spec(cfg, "nextdit_async"), 5).items()}
    inp = S.qwen_inputs(B, 1, seed=33, cfg=cfg, n_text=20, n_tail=12)
    kw = dict(device=DEV, max_envs=B, num_history=3, resize_w=280, resize_h=280, max_seq_len=512, max_patches=inp["pixel_values"].shape[0])
    model = InternVLAN1ForCausalLM(sd, cfg, "nextdit_async", **kw)
    qsd = {k: v.float() for k, v in sd.items() if not k.startswith("model.traj_dit") and not k.startswith("model.rgb_")}
    per_img = inp["pixel_values"].shape[0] // B
    ids, grid, pv = inp["input_ids"][:N_P], inp["grid_thw"][:N_P], inp["pixel_values"][: N_P * per_img]
    torch.set_num_threads(16)
    answers, want, std = _oracle_case(qsd, cfg, ids, pv, grid, per_img, range(N_P))
    tol = 2 * 5e-2 * std
    shared = model.score_answers(ids, answers, pixel_values=pv, image_grid_thw=grid, share_prefix=True)
    stats = dict(model.last_score)
    return dict(model=model, cfg=cfg, sd=sd, kw=kw, inp=inp, ids=ids, grid=grid, pv=pv, per_img=per_img, answers=answers, want=want, tol=tol, std=std,
                shared=shared, stats=stats)


def _worst(res, other, n_p=N_P):
    """max |difference| over all token log-probabilities; `other` is a result object or the oracle's nested arrays"""
    w = 0.0
    for b in range(n_p):
        for c in range(len(res.token_logprobs[b])):
            o = other[b][c] if isinstance(other, list) else other.token_logprobs[b][c].cpu().numpy()
            got = res.token_logprobs[b][c].cpu().numpy()
            assert got.shape == np.shape(o)
            w = max(w, float(np.abs(got - o).max())) if got.size else w
    return w


def test_share_prefix_against_the_fp32_oracle_and_the_per_pair_path(setup):
    s = setup
    m, res, want, tol = s["model"], s["shared"], s["want"], s["tol"]
    for b in range(N_P):
        assert res.lengths[b] == [3, 2, 1] and res.sequences_logprob[b].shape == (3,)
        for c in range(3):
            got = res.token_logprobs[b][c]
            assert got.dtype == torch.float32 and got.shape == (3 - c,)
            assert abs(float(res.sequences_logprob[b][c]) - float(got.double().sum())) <= 1e-5 * max(1.0, abs(float(got.sum())))
        # ranking: the oracle's gap between the greedy answer and the unlikely one must exceed what the tolerance lets the sums move
        sums = [w.sum() for w in want[b]]
        assert sums[0] - sums[1] > (3 + 2) * tol, f"test data: oracle gap {sums[0] - sums[1]:.2f} within the tolerance {(3 + 2) * tol:.2f}"
        for i in range(3):
            for j in range(3):
                if sums[i] - sums[j] > (len(want[b][i]) + len(want[b][j])) * tol:
                    assert float(res.sequences_logprob[b][i]) > float(res.sequences_logprob[b][j]), (b, i, j)
        # candidates 0 and 2 share their first token: one gathered row each, the same bits
        assert torch.equal(res.token_logprobs[b][0][:1], res.token_logprobs[b][2])
    worst = _worst(res, want)
    print(f"share_prefix=True: max |logprob - oracle| {worst:.3e} (tolerance {tol:.3f}, oracle logit std {s['std']:.2f})")
    assert worst <= tol
    # the per-pair path on the same inputs: both sit within one tolerance of the oracle
    per_pair = m.score_answers(s["ids"], s["answers"], pixel_values=s["pv"], image_grid_thw=s["grid"])
    n_img = int(s["grid"].shape[0])
    assert m.last_score == dict(prompt_prefills=6, images_encoded=3 * n_img, suffix_rows=0, suffix_passes=0)
    assert s["stats"] == dict(prompt_prefills=2, images_encoded=n_img, suffix_rows=4 * 2, suffix_passes=1)      # 4 pairs of >= 2 tokens, m = 2
    d = _worst(res, per_pair)
    print(f"share_prefix=True against share_prefix=False: max |difference| {d:.3e} (per-pair path against the oracle: {_worst(per_pair, want):.3e})")
    assert d <= 2 * tol
    assert per_pair.lengths == res.lengths


def test_ragged_prompts_and_split_suffix_groups(setup):
    s = setup
    m, res, tol = s["model"], s["shared"], s["tol"]
    Sp = s["ids"].shape[1]
    # prompt 1 is three tokens shorter than prompt 0 (inside its text tail) and both are right-padded by five columns: one prefill group of two
    # lengths - prompt 1's prefix ends in front of stale pad rows of its cache slot, its first row and its positions are its own
    cut = 3
    pad, mask = torch.zeros(N_P, Sp + 5, dtype=torch.long), torch.zeros(N_P, Sp + 5, dtype=torch.long)
    pad[:, :Sp], mask[:, :Sp] = s["ids"], 1
    mask[1, Sp - cut:] = 0
    assert int((s["ids"][1, Sp - cut:] == s["cfg"]["image_token_id"]).sum()) == 0      # (the cut removes text tokens only)
    r2 = m.score_answers(pad, s["answers"], pixel_values=s["pv"], image_grid_thw=s["grid"], attention_mask=mask, share_prefix=True)
    assert m.last_score == dict(prompt_prefills=2, images_encoded=int(s["grid"].shape[0]), suffix_rows=4 * 2, suffix_passes=1)
    alone = m.score_answers(s["ids"][1:2, : Sp - cut], s["answers"][1:2], pixel_values=s["pv"][s["per_img"]:], image_grid_thw=s["grid"][1:2],
                            share_prefix=True)                                          # the short prompt unpadded, on its own
    d0 = max(float((r2.token_logprobs[0][c] - res.token_logprobs[0][c]).abs().max()) for c in range(3))
    d1 = max(float((r2.token_logprobs[1][c] - alone.token_logprobs[0][c]).abs().max()) for c in range(3))
    moved = max(float((r2.token_logprobs[1][c] - res.token_logprobs[1][c]).abs().max()) for c in range(3))
    print(f"ragged group: long prompt against the dense call {d0:.3e}, short prompt against its unpadded call {d1:.3e} "
          f"(against the uncut prompt: {moved:.3e})")
    assert d0 <= tol and d1 <= tol and r2.lengths == res.lengths
    # a row budget of one pair per suffix pass: four passes, the values of the single pass
    r3 = m.score_answers(s["ids"], s["answers"], pixel_values=s["pv"], image_grid_thw=s["grid"], share_prefix=True, max_suffix_rows=2)
    # (a pass of one pair is as wide as that pair: 2 rows for the 3-token candidates, 1 row for the 2-token ones)
    assert m.last_score == dict(prompt_prefills=2, images_encoded=int(s["grid"].shape[0]), suffix_rows=2 * (2 + 1), suffix_passes=4)
    d = _worst(r3, res)
    print(f"four suffix passes of one pair against one pass of four: max |difference| {d:.3e}")
    assert d <= tol
    # one-token and empty candidates: no suffix pass at all
    r4 = m.score_answers(s["ids"], [[a[2], []] for a in s["answers"]], pixel_values=s["pv"], image_grid_thw=s["grid"], share_prefix=True)
    assert m.last_score["suffix_passes"] == 0 and m.last_score["suffix_rows"] == 0 and r4.lengths == [[1, 0]] * N_P
    for b in range(N_P):
        # (the lm_head GEMM runs 2 rows here and 6 there: the same position, not necessarily the same bits)
        assert (r4.token_logprobs[b][0] - res.token_logprobs[b][2]).abs().max().item() <= tol and r4.token_logprobs[b][1].numel() == 0


@pytest.mark.parametrize("n_prompts,n_cand,rows", [(1, 3, 24), (3, 3, 72)])
def test_wider_suffix_passes_agree_with_the_per_pair_path(setup, n_prompts, n_cand, rows):
    """9-token candidates: suffix passes of 24 rows (above the 16 rows of the fused-norm single-token chain, weight-streaming GEMMs) and of 72
    rows (above SKINNY_GEMM_MAX_ROWS: tiled GEMMs on the fragment-ordered weights) against the per-pair path on the same inputs. Both paths
    are held to one oracle tolerance each by the tests above, so they may differ by two."""
    from internnav_amd.qwen_vl import SKINNY_GEMM_MAX_ROWS

    s = setup
    m, tol, inp = s["model"], s["tol"], s["inp"]
    assert 16 < rows and (rows <= SKINNY_GEMM_MAX_ROWS) == (n_prompts == 1)
    g = torch.Generator().manual_seed(7)
    answers = [[torch.randint(0, s["cfg"]["vocab"], (9,), generator=g).tolist() for _ in range(n_cand)] for _ in range(n_prompts)]
    kw = dict(pixel_values=inp["pixel_values"][: n_prompts * s["per_img"]], image_grid_thw=inp["grid_thw"][:n_prompts])
    a = m.score_answers(inp["input_ids"][:n_prompts], answers, share_prefix=True, **kw)
    assert m.last_score == dict(prompt_prefills=n_prompts, images_encoded=n_prompts, suffix_rows=rows, suffix_passes=1)
    b = m.score_answers(inp["input_ids"][:n_prompts], answers, **kw)
    d = _worst(a, b, n_p=n_prompts)
    print(f"suffix pass of {rows} rows against the per-pair path: max |difference| {d:.3e} (allowed {2 * tol:.3f})")
    assert a.lengths == b.lengths == [[9] * n_cand] * n_prompts and d <= 2 * tol


def test_pairs_are_isolated_bit_for_bit(setup):
    """[A, B] and [A, B'] with len(B') = len(B): the same shapes and kernels, so only a leak across pairs could change a bit of A"""
    s = setup
    m, vocab = s["model"], s["cfg"]["vocab"]
    a, b1 = s["answers"][0][0], s["answers"][0][1]
    b2 = [(t + 17) % vocab for t in b1]
    kw = dict(pixel_values=s["pv"][: s["per_img"]], image_grid_thw=s["grid"][:1], share_prefix=True)
    r1 = m.score_answers(s["ids"][:1], [[a, b1]], **kw)
    r2 = m.score_answers(s["ids"][:1], [[a, b2]], **kw)
    assert torch.equal(r1.token_logprobs[0][0], r2.token_logprobs[0][0])
    assert not torch.equal(r1.token_logprobs[0][1], r2.token_logprobs[0][1])
    # and the other order: A behind B in the rectangle
    r3 = m.score_answers(s["ids"][:1], [[b1, a]], **kw)
    r4 = m.score_answers(s["ids"][:1], [[b2, a]], **kw)
    assert torch.equal(r3.token_logprobs[0][1], r4.token_logprobs[0][1])


def test_the_prompts_cache_rows_are_untouched(setup):
    s = setup
    m = s["model"]
    q = m.qwen
    pl = s["ids"].shape[1]
    q.prefill(s["ids"], s["pv"].to(DEV, torch.bfloat16), s["grid"], seq_lens=np.full(N_P, pl))
    torch.cuda.synchronize()
    keep = [L["kv"].view(q.B_max, q.S_max, q.kv_w)[:N_P, :pl].clone() for L in q.layers]
    m.score_answers(s["ids"], s["answers"], pixel_values=s["pv"], image_grid_thw=s["grid"], share_prefix=True)
    torch.cuda.synchronize()
    for li, L in enumerate(q.layers):
        assert torch.equal(L["kv"].view(q.B_max, q.S_max, q.kv_w)[:N_P, :pl].view(torch.int16), keep[li].view(torch.int16)), f"layer {li}"


def test_w8_decode_engine_against_the_oracle_on_the_round_trip_weights(setup):
    """the suffix pass of a w8_decode engine streams the fp8 weights (<= SKINNY_GEMM_MAX_ROWS rows): the model it computes is the round-trip
    checkpoint, so that is what the oracle runs. One prompt keeps the oracle's work small."""
    from internnav_amd.policy import InternVLAN1ForCausalLM
    from internnav_amd.qwen_vl import w8_roundtrip_state_dict

    s = setup
    cfg = s["cfg"]
    m8 = InternVLAN1ForCausalLM(s["sd"], cfg, "nextdit_async", w8_decode=True, **s["kw"])
    rt = w8_roundtrip_state_dict({k: v.to(DEV) for k, v in s["sd"].items()}, cfg)
    qsd = {k: v.float().cpu() for k, v in rt.items() if not k.startswith("model.traj_dit") and not k.startswith("model.rgb_")}
    ids, grid, pv = s["ids"][:1], s["grid"][:1], s["pv"][: s["per_img"]]
    answers, want, std = _oracle_case(qsd, cfg, ids, pv, grid, s["per_img"], range(1))
    tol = 2 * 5e-2 * std
    res = m8.score_answers(ids, answers, pixel_values=pv, image_grid_thw=grid, share_prefix=True)
    assert m8.last_score == dict(prompt_prefills=1, images_encoded=int(grid.shape[0]), suffix_rows=2 * 2, suffix_passes=1)
    worst = _worst(res, want, n_p=1)
    print(f"w8_decode, share_prefix=True: max |logprob - round-trip oracle| {worst:.3e} (tolerance {tol:.3f})")
    assert worst <= tol
