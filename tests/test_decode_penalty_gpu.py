"""GPU: the repetition penalty of System-2 greedy decoding (csrc/decode_penalty.hip, QwenVLEngine / InternVLAN1ForCausalLM.generate).

Kernels against the fp32 restatement of tests/decode_penalty_ref.py (itself pinned to transformers' RepetitionPenaltyLogitsProcessor in
tests/test_decode_penalty_cpu.py), bit for bit: the seen-set bitmap word for word, the selection token for token. No tolerance anywhere:
the penalised value is one IEEE fp32 multiplication or division, the same on the host and on the device.
Engine: every greedy token equals the restatement's choice on the engine's own raw logits of that step (prompt + answer so far seen)."""
import json

import numpy as np
import pytest
import torch

import decode_penalty_ref as R
from internnav_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATTERN = 0xA5A5A5A5
NS = [1, 31, 32, 33, 127, 4096, 4099, 12288, 12400, 12547, 16384, 16389, 28675, 152064]


@pytest.fixture(scope="module")
def ops(built_lib):
    from internnav_amd import ops as o

    return o


def _u32(t: torch.Tensor) -> np.ndarray:
    return t.detach().view(torch.int32).cpu().numpy().view(np.uint32)


def _seen_dev(words: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(DEV).view(torch.uint32)


def _logits_dev(x: np.ndarray, ldx: int, off: int):
    """x f32 [rows, n] as a device view with row stride ldx whose first element lies off floats behind a 16-byte aligned address;
    -> (view, backing buffer)"""
    rows, n = x.shape
    buf = torch.full((rows * ldx + 8,), 7.0, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off: off + rows * ldx].view(rows, ldx)[:, :n]
    v.copy_(torch.from_numpy(x))
    return v, buf


def _random_ids(g: np.random.Generator, rows: int, n: int, S_: int) -> np.ndarray:
    ids = g.integers(0, n, (rows, S_), dtype=np.int64)
    ids[:, : S_ // 4] = ids[:, S_ // 4: 2 * (S_ // 4)]              # duplicates
    ids[:, -6:] = np.array([0, 31, 32, n - 1, 0, n - 1])[None]      # the word edges (31 / 32 are ignored where n is smaller)
    ids[:, 3], ids[:, 4], ids[:, 5] = -1, n, n + 31                 # outside [0, n): ignored
    ids[:, 6] = -2 ** 31
    ids[:, 7] = 2 ** 31 - 1
    return ids


# ---------------------------------------------------------------------------------------------------- token_seen_set
@pytest.mark.parametrize("rows", [1, 7])
@pytest.mark.parametrize("n", NS)
def test_seen_set_equals_restatement_and_leaves_the_rest_untouched(ops, n, rows):
    g = np.random.default_rng(n * 8 + rows)
    nw = (n + 31) // 32
    ldw = nw + 3                                                     # larger than needed; one more row than the launch covers
    S_ = 900
    for trial in range(2):                                           # the second launch must clear what the first one set
        seen = _seen_dev(np.full((rows + 1, ldw), PATTERN, dtype=np.uint32)) if trial == 0 else seen
        ids = _random_ids(g, rows, n, S_)
        lens = g.integers(1, S_ + 1, rows)
        lens[0] = S_
        if rows > 1:
            lens[1] = 0                                              # an empty row: every token bit cleared
        ops.token_seen_set(seen, torch.from_numpy(ids.astype(np.int32)).to(DEV), torch.from_numpy(lens.astype(np.int32)).to(DEV), n)
        torch.cuda.synchronize()
        got = _u32(seen)
        want = np.full((rows + 1, ldw), PATTERN, dtype=np.uint32)
        bm = R.seen_bitmap(ids, lens, n)
        want[:rows, : n // 32] = bm[:, : n // 32]
        if n % 32:
            m = np.uint32((1 << (n % 32)) - 1)
            want[:rows, nw - 1] = (np.uint32(PATTERN) & ~m) | bm[:, nw - 1]
        assert np.array_equal(got, want), f"n={n} rows={rows} trial={trial}: {np.argwhere(got != want)[:4].tolist()}"
        assert bm[0].any() and (rows == 1 or not bm[1].any())


# ---------------------------------------------------------------------------------------------------- argmax_penalty_rows
def _check_selection(ops, x: np.ndarray, words: np.ndarray, p: float, ldx: int, off: int, mark: bool):
    rows, n = x.shape
    xv, buf = _logits_dev(x, ldx, off)
    before = buf.clone()
    seen = _seen_dev(words)
    out = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    ops.argmax_penalty_rows(xv, seen, p, out, mark=mark)
    torch.cuda.synchronize()
    want = R.argmax_first(R.penalised(x, words[:rows, : (n + 31) // 32], p))
    got = out.cpu().numpy()
    assert np.array_equal(got, want), f"n={n} rows={rows} ldx={ldx} off={off} p={p}: got {got.tolist()} want {want.tolist()}"
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "X was modified"       # (bitwise: rows hold NaN)
    after = _u32(seen)
    exp = words.copy()
    if mark:
        for r in range(rows):
            exp[r, want[r] >> 5] |= np.uint32(1 << (int(want[r]) & 31))
    assert np.array_equal(after, exp), "the seen set changed by something other than the chosen token's bit"
    return got


@pytest.mark.parametrize("layout", ["aligned", "offset4", "odd_stride"])
@pytest.mark.parametrize("rows", [1, 7])
@pytest.mark.parametrize("n", NS)
def test_selection_equals_restatement(ops, n, rows, layout):
    g = np.random.default_rng(n * 64 + rows * 4 + len(layout))
    x = (g.standard_normal((rows, n)) * 4.0).astype(np.float32)
    ids = g.integers(0, n, (rows + 1, min(n, 900)))
    words = np.zeros((rows + 1, (n + 31) // 32 + 2), dtype=np.uint32)     # ld_words larger than needed, one row more than the launch
    words[:, : (n + 31) // 32] = R.seen_bitmap(ids, [ids.shape[1]] * (rows + 1), n)
    words[:, (n + 31) // 32:] = PATTERN
    if n >= 33:
        words[0, (n // 2) >> 5] &= ~np.uint32(1 << ((n // 2) & 31))      # at least one unseen token in row 0
        # row 0: the raw maximum sits on a seen positive token, the runner-up is unseen and inside the factor -> the choice moves
        mask = R.bitmap_mask(words[0, : (n + 31) // 32], n)
        a, b = int(np.flatnonzero(mask)[-1]), int(np.flatnonzero(~mask)[0])
        x[0, b] = np.abs(x[0]).max() + 1.0
        x[0, a] = x[0, b] * np.float32(1.03)
    ldx, off = {"aligned": ((n + 7) // 4 * 4, 0), "offset4": ((n + 7) // 4 * 4, 1), "odd_stride": (n + 3 if n % 2 == 0 else n + 2, 0)}[layout]
    for p, mark in ((1.05, False), (2.0, True)):
        got = _check_selection(ops, x, words, p, ldx, off, mark)
        if n >= 33:
            assert got[0] == b and int(np.argmax(x[0])) == a
    # p = 1.0 with a non-empty set: the plain argmax
    xv, _ = _logits_dev(x, ldx, off)
    o1, o2 = torch.empty(rows, dtype=torch.int32, device=DEV), torch.empty(rows, dtype=torch.int32, device=DEV)
    ops.argmax_penalty_rows(xv, _seen_dev(words), 1.0, o1, mark=False)
    ops.argmax_rows(xv, o2)
    assert torch.equal(o1, o2) and words[:rows].any()


def test_selection_edges(ops):
    """n = 4099 (vector body + scalar tail), one row per edge: all-negative rows (multiplication), exact ties made by the penalty in both
    orders and in both paths, seen +inf / -inf / NaN / -0.0, rows without an entry above -inf"""
    n, g = 4099, np.random.default_rng(5)
    nw = (n + 31) // 32
    xs, sets, ps = [], [], 2.0

    def row(x, seen):
        xs.append(np.asarray(x, dtype=np.float32))
        sets.append(list(seen))

    neg = -(np.abs(g.standard_normal(n)) + 0.1).astype(np.float32)
    row(neg, [int(np.argmax(neg)), 17, 4098])                          # the least negative entry is seen: doubled, another one wins
    for a, b in ((5, 2000), (2000, 5), (4097, 4098), (4098, 4097), (4095, 4096), (4096, 4095)):
        t = -(np.abs(g.standard_normal(n)) + 1.0).astype(np.float32)
        t[a], t[b] = 6.0, 3.0                                          # 6 / 2 == 3: a tie, the lower index wins
        row(t, [a])
    t = (g.standard_normal(n) * 3).astype(np.float32)
    t[100], t[200], t[300], t[4098] = np.inf, -np.inf, np.nan, np.nan
    row(t, [100, 200, 300, 4098])                                      # +inf / 2 = +inf is still the maximum
    t = -(np.abs(g.standard_normal(n)) + 1.0).astype(np.float32)
    t[40], t[50], t[4097] = -0.0, 0.0, -0.0
    row(t, [40, 4097])                                                 # -0.0 / 2 = -0.0 == 0.0: the first of the three
    t = np.full(n, -np.inf, dtype=np.float32)
    t[7], t[4098] = np.nan, np.nan
    row(t, [7, 9, 4098])                                               # nothing above -inf -> 0
    t = np.full(n, np.nan, dtype=np.float32)
    t[4098] = -np.inf
    row(t, [4098])
    x = np.stack(xs)
    words = np.zeros((len(xs), nw), dtype=np.uint32)
    for r, s in enumerate(sets):
        words[r] = R.seen_bitmap([s], [len(s)], n)[0]
    for off in (0, 1):
        got = _check_selection(ops, x, words, ps, n + 1 if off == 0 else n + 5, off, mark=False)
        assert got[0] != int(np.argmax(neg))
        assert got[1:7].tolist() == [5, 5, 4097, 4097, 4095, 4095]
        assert got[7] == 100 and got[8] == 40 and got[9] == 0 and got[10] == 0


def test_mark_sets_exactly_the_chosen_bit_and_steps_chain(ops):
    n, rows, p = 4099, 4, 1.5
    g = np.random.default_rng(9)
    prompts = g.integers(0, n, (rows, 60))
    X = (g.standard_normal((4, rows, n)) * 3).astype(np.float32)        # four fixed logit rows per sequence
    lens = np.array([60, 41, 1, 60])
    ref0 = [R.greedy_with_penalty(lambda s, _t, r=r: X[s, r], prompts[r, : lens[r]], 1, p)[0] for r in range(rows)]
    for s in range(1, 4):
        for r in range(rows):
            X[s, r, ref0[r]] = X[s, r].max() * np.float32(1.2)          # raw maximum = the first answer token: only a chained set moves it
    want = [R.greedy_with_penalty(lambda s, _t, r=r: X[s, r], prompts[r, : lens[r]], 4, p) for r in range(rows)]
    assert all(len(set(w)) > 1 for w in want)
    seen = torch.zeros(rows, (n + 31) // 32, dtype=torch.uint32, device=DEV)
    ops.token_seen_set(seen, torch.from_numpy(prompts.astype(np.int32)).to(DEV), torch.from_numpy(lens.astype(np.int32)).to(DEV), n)
    xd = torch.from_numpy(X).to(DEV)
    outs = [torch.empty(rows, dtype=torch.int32, device=DEV) for _ in range(4)]
    snaps = [_u32(seen).copy()]
    for s in range(4):
        ops.argmax_penalty_rows(xd[s], seen, p, outs[s], mark=True)      # back to back: nothing between the steps
        snaps.append(_u32(seen).copy())
    got = np.stack([o.cpu().numpy() for o in outs], 1)
    assert got.tolist() == want
    new = 0
    for s in range(4):
        for r in range(rows):
            d = snaps[s][r] ^ snaps[s + 1][r]
            t = int(got[r, s])
            if (snaps[s][r, t >> 5] >> np.uint32(t & 31)) & np.uint32(1):     # an already seen token was chosen again: nothing changes
                assert not d.any()
            else:
                new += 1
                assert int(np.unpackbits(d.view(np.uint8)).sum()) == 1 and d[t >> 5] == np.uint32(1 << (t & 31))
    assert new >= 12, "test data: most chosen tokens must be new"


# ---------------------------------------------------------------------------------------------------- engine
B, N_DEC = 3, 8
Z0 = 3993          # synthetic.qwen_inputs draws text tokens below 3993: tokens 3993 .. 4000 occur in no prompt


def _craft(e, ids, pv, grid):
    """A random-weight model almost never prefers a token it has seen, so a penalty would move nothing. Give row b of these prompts two
    crafted tokens (rows of lm_head / embed_tokens rewritten; the prefill does not depend on lm_head):
      c_b, a text token of the prompt:  lm_head[c_b] = 1.06 lm_head[t0_b]  (t0_b = the model's own first token) - the raw maximum of step 0 is a
           PROMPT token; a penalty >= 1.05 takes it below
      z_b, a token no prompt holds:     embed[z_b] = embed[t0_b] and lm_head[z_b] = alpha lm_head[t0_b] + gamma lm_head[m_b] (m_b = the model's own
           second token), solved so that its logit is 1.03 x the maximum at step 0 (z_b is chosen and runs as t0_b would have) and 1.02 x the
           maximum at step 1 - the raw maximum of step 1 is the token the answer just produced; only a set that was marked takes it below.
    -> (z, c, patch): patch = {'lm_head': {row: bf16 tensor}, 'embed': {row: bf16 tensor}} as applied to the engine."""
    Bn = ids.shape[0]
    st = e.prefill(ids, pv, grid)
    t0 = e.decode(st, 1)[:, 0].cpu().numpy()
    r0 = e.logits[:Bn].double().cpu().numpy()
    e.decode(st, 2)
    r1 = e.logits[:Bn].double().cpu().numpy()
    z, c = [Z0 + b for b in range(Bn)], [int(ids[b, 2 + b]) for b in range(Bn)]
    used = set(t0.tolist()) | {int(np.argmax(r1[b])) for b in range(Bn)}
    assert len(set(c)) == Bn and not (set(c) | set(z)) & used and not set(z) & set(ids.reshape(-1).tolist()), "test data"
    patch = {"lm_head": {}, "embed": {}}
    for b in range(Bn):
        t, m = int(t0[b]), int(np.argmax(r1[b]))
        al, ga = 1.03, 0.0
        if m != t:
            al, ga = np.linalg.solve(np.array([[r0[b, t], r0[b, m]], [r1[b, t], r1[b, m]]]), np.array([1.03 * r0[b, t], 1.02 * r1[b, m]]))
        patch["lm_head"][z[b]] = (float(al) * e.lm_head[t].float() + float(ga) * e.lm_head[m].float()).to(torch.bfloat16)
        patch["lm_head"][c[b]] = (1.06 * e.lm_head[t].float()).to(torch.bfloat16)
        patch["embed"][z[b]] = e.embed[t].clone()
    for k, v in patch["lm_head"].items():
        e.lm_head[k].copy_(v)
    for k, v in patch["embed"].items():
        e.embed[k].copy_(v)
    return z, c, patch


@pytest.fixture(scope="module")
def eng(built_lib):
    from internnav_amd.qwen_vl import QwenVLEngine

    cfg = S.QWEN_TEST_CFG
    inp = S.qwen_inputs(B, 1, seed=21, cfg=cfg)
    e = QwenVLEngine(S.qwen_state_dict(seed=21, cfg=cfg), cfg, DEV, max_seqs=B, max_seq_len=512, max_patches=inp["pixel_values"].shape[0])
    pv = inp["pixel_values"].to(DEV, torch.bfloat16)
    e.crafted = _craft(e, inp["input_ids"], pv, inp["grid_thw"])[:2]
    return e, cfg, inp["input_ids"], pv, inp["grid_thw"]


def _stepwise(e, ids, pv, grid, n, lens=None, **kw):
    """decode n tokens one step at a time -> (tokens [B, n], raw logits [n, B, vocab]) as numpy"""
    st = e.prefill(ids, pv, grid, **({} if lens is None else {"seq_lens": lens}), **kw)
    toks, raws = [], []
    for j in range(n):
        t = e.decode(st, 1) if j == 0 else e.decode(st, 2)[:, 1:]
        toks.append(t[:, 0].cpu().numpy())
        raws.append(e.logits[:B].cpu().numpy().copy())
    return np.stack(toks, 1), np.stack(raws)


def _oracle(ids, lens, toks, raws, p):
    """the restatement's choice at every step from the engine's raw logits, prompt + answer so far seen"""
    n = raws.shape[-1]
    want = np.zeros_like(toks)
    for b in range(toks.shape[0]):
        for j in range(toks.shape[1]):
            hist = ids[b, : lens[b]].tolist() + toks[b, :j].tolist()
            want[b, j] = R.argmax_first(R.penalised(raws[j, b], R.seen_bitmap([hist], [len(hist)], n)[0], p))
    return want


def test_penalty_one_is_the_parent_behaviour(eng):
    e, cfg, ids, pv, grid = eng
    base = e.decode(e.prefill(ids, pv, grid), N_DEC).cpu()                    # never passes the argument
    e.seen.view(torch.int32).fill_(-1)                                        # a penalty of 1.0 must not even look at the set
    one = e.decode(e.prefill(ids, pv, grid, repetition_penalty=1.0), N_DEC).cpu()
    assert torch.equal(base, one) and bool((e.seen.view(torch.int32) == -1).all())
    seqs = e.generate(ids, pv, grid, max_new_tokens=N_DEC, eos_token_id=-1)
    assert torch.equal(seqs[:, ids.shape[1]:], base.long())
    assert torch.equal(e.generate(ids, pv, grid, max_new_tokens=N_DEC, eos_token_id=[-1, -2], repetition_penalty=1.0), seqs)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("p", [1.05, 1.5])
def test_every_step_equals_the_restatement_on_the_raw_logits(eng, p, ragged):
    e, cfg, ids, pv, grid = eng
    S_ = ids.shape[1]
    lens = [S_, S_ - 9, S_ - 3] if ragged else None
    toks, raws = _stepwise(e, ids, pv, grid, N_DEC, lens, repetition_penalty=p)
    want = _oracle(ids.numpy(), lens or [S_] * B, toks, raws, p)
    plain = np.stack([R.argmax_first(raws[j]) for j in range(N_DEC)], 1)
    print(f"p={p} ragged={ragged}: tokens {toks.tolist()}; steps the penalty moved: {int((want != plain).sum())} of {want.size}")
    assert np.array_equal(toks, want)
    if not ragged:
        # the crafted tokens (_craft): step 0's raw maximum is a prompt token and is passed over, step 1's is the token step 0 produced
        z, c = e.crafted
        hit = [b for b in range(B) if plain[b, 0] == c[b] and toks[b, 0] == z[b] and plain[b, 1] == z[b] and toks[b, 1] != z[b]]
        print(f"rows in which the penalty passes over a prompt token at step 0 and over the answer's own token at step 1: {hit}")
        assert hit, "test data: no row shows the crafted pattern"
    # the seen set on the device = prompt + answer (the last token is marked by the launch that chose it)
    got = _u32(e.seen)[:B, : (cfg["vocab"] + 31) // 32]
    full = [ids[b, : (lens or [S_] * B)[b]].tolist() + toks[b].tolist() for b in range(B)]
    for b in range(B):
        assert np.array_equal(got[b], R.seen_bitmap([full[b]], [len(full[b])], cfg["vocab"])[0])
    # a chunked decode (the policy's loop) gives the same tokens as single steps
    st = e.prefill(ids, pv, grid, repetition_penalty=p, **({} if lens is None else {"seq_lens": lens}))
    a = e.decode(st, 3)
    b_ = e.decode(st, N_DEC - 3 + 1)[:, 1:]
    assert np.array_equal(torch.cat([a, b_], 1).cpu().numpy(), toks)


def test_a_huge_penalty_never_repeats_a_seen_token(eng):
    e, cfg, ids, pv, grid = eng
    p, S_ = 1e4, ids.shape[1]
    toks, raws = _stepwise(e, ids, pv, grid, N_DEC, None, repetition_penalty=p)
    qualified = 0
    for b in range(B):
        for j in range(N_DEC):
            hist = set(ids[b].tolist() + toks[b, :j].tolist())
            unseen = np.ones(cfg["vocab"], dtype=bool)
            unseen[list(hist)] = False
            if bool((raws[j, b][unseen] > 0).any()):
                qualified += 1
                assert int(toks[b, j]) not in hist, (b, j)
    assert qualified > 0
    assert np.array_equal(toks, _oracle(ids.numpy(), [S_] * B, toks, raws, p))


def test_captured_decode_reinitialises_the_set_on_every_replay(eng):
    from internnav_amd.runtime import GraphedCall

    e, cfg, ids, pv, grid = eng
    p = 1.5
    want, _ = _stepwise(e, ids, pv, grid, 4, None, repetition_penalty=p)
    P = e.plan(ids, grid, n_decode=4, repetition_penalty=p)
    e.run_prefill(P, pv)                                                       # eager; the capture below holds run_decode alone (one stream)
    toks = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    e.run_decode(P, toks)
    assert np.array_equal(toks.cpu().numpy(), want)
    g = GraphedCall(lambda: e.run_decode(P, toks), {})
    for _ in range(2):
        toks.zero_()
        e.seen.view(torch.int32).fill_(-1)                                     # were the set launch outside the capture, every token would count as seen
        g()
        torch.cuda.synchronize()
        assert np.array_equal(toks.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------- policy surface
N_TEXT, N_IMG = 40, 3
P_IMG0 = N_TEXT + 196 + 2


@pytest.fixture(scope="module")
def model(built_lib):
    from internnav_amd.policy import InternVLAN1ForCausalLM

    cfg = S.QWEN_TEST_CFG
    # (bf16, as write_checkpoint stores them: the checkpoint test below loads the same weights from disk)
    sd = {k: v.to(torch.bfloat16) for k, v in S.materialize(S.n1_full_spec(cfg, "nextdit_async"), 5).items()}
    m = InternVLAN1ForCausalLM(sd, cfg, "nextdit_async", device=DEV, max_envs=B, num_history=3, resize_w=280, resize_h=280, cam_w=640, cam_h=480,
                               max_seq_len=1536, max_patches=3 * 4096)
    inp = _model_inputs()
    m.crafted = _craft(m.qwen, inp["input_ids"], inp["pixel_values"].to(DEV, torch.bfloat16), inp["grid_thw"])
    return m


def _model_inputs():
    return S.qwen_inputs(B, N_IMG, seed=31, cfg=S.QWEN_TEST_CFG, n_text=N_TEXT, n_tail=24)


def test_cached_prompt_tokens_count_like_any_other(model):
    """generate(past_key_values=...) and prefix_kv reuse with a penalty: the tokens of the call without reuse, and a seen set that holds the
    tokens whose K/V came from the cache"""
    cfg = S.QWEN_TEST_CFG
    inp = _model_inputs()
    ids, grid, pv = inp["input_ids"], inp["grid_thw"], inp["pixel_values"]
    p, n = 1.05, 6
    z, c, _ = model.crafted                                  # every c_b lies inside the prefix the calls below take from a cache
    assert model.generation_config.repetition_penalty == 1.0 and model.generation_config.eos_token_id == (cfg["eos_token_id"],)
    kw = dict(input_ids=ids, pixel_values=pv, image_grid_thw=grid, max_new_tokens=n, eos_token_id=-1, repetition_penalty=p)
    ref = model.generate(**kw)
    seen_ref = _u32(model.qwen.seen)[:B].copy()
    for b in range(B):
        assert np.array_equal(seen_ref[b, : 4096 // 32], R.seen_bitmap([ref[b].tolist()], [ref.shape[1]], 4096)[0])
    plain = model.generate(**dict(kw, repetition_penalty=1.0))
    hit = [b for b in range(B) if int(plain[b, ids.shape[1]]) == c[b] and int(ref[b, ids.shape[1]]) == z[b]]
    print(f"rows whose first token is the crafted prompt token without the penalty and the crafted new token with it: {hit}")
    assert hit, "test data: no row shows the crafted pattern"
    # past_key_values from a shorter first call (the first image), then the full prompt
    g1 = grid.view(B, N_IMG, 3)[:, :1].reshape(-1, 3)
    pv1 = pv.view(B, N_IMG, 784, 1176)[:, :1].reshape(-1, 1176)
    first = model.generate(input_ids=ids[:, :P_IMG0], pixel_values=pv1, image_grid_thw=g1, max_new_tokens=2, return_dict_in_generate=True,
                           export_prefix=[P_IMG0] * B)
    kvs = [model.last_prefix_kv()[b] for b in range(B)]
    out = model.generate(**kw, past_key_values=first.past_key_values, return_dict_in_generate=True)
    assert model.last_kv_reuse["rows"] == B * P_IMG0 and torch.equal(out.sequences, ref)
    assert np.array_equal(_u32(model.qwen.seen)[:B], seen_ref)
    model.qwen.seen.view(torch.int32).zero_()
    out = model.generate(**kw, prefix_kv=kvs)
    assert model._gen["state"]["S_run"] == ids.shape[1] - P_IMG0 and torch.equal(out, ref)
    assert np.array_equal(_u32(model.qwen.seen)[:B], seen_ref)


def test_checkpoint_generation_config_drives_generate(model, tmp_path):
    from internnav_amd.policy import InternVLAN1ForCausalLM

    from safetensors.torch import load_file, save_file

    cfg = S.QWEN_TEST_CFG
    inp = _model_inputs()
    ids, grid = inp["input_ids"], inp["grid_thw"]
    pv = inp["pixel_values"].to(DEV, torch.bfloat16)
    p, S_ = 1.3, ids.shape[1]
    # the same weights as the checkpoint below (seed 5 + the crafted rows), stepped on the module's engine: what the penalised run must decode
    toks, raws = _stepwise(model.qwen, ids, pv, grid, N_DEC, None, repetition_penalty=p)
    assert np.array_equal(toks, _oracle(ids.numpy(), [S_] * B, toks, raws, p))
    e0, e1 = cfg["eos_token_id"], int(toks[0, 2])
    S.write_checkpoint(tmp_path, cfg, "nextdit_async", seed=5, generation_config={"repetition_penalty": p, "eos_token_id": [e0, e1], "do_sample": True,
                                                                                  "temperature": 0.1, "top_k": 1, "top_p": 0.001})
    for f in sorted(tmp_path.glob("*.safetensors")):                          # the crafted rows of the module's engine, into the shards
        sd = load_file(str(f))
        for name, rows in (("lm_head.weight", model.crafted[2]["lm_head"]), ("model.embed_tokens.weight", model.crafted[2]["embed"])):
            if name in sd:
                for k, v in rows.items():
                    sd[name][k] = v.cpu()
        save_file(sd, str(f))
    m = InternVLAN1ForCausalLM.from_pretrained(tmp_path, device_map={"": DEV}, max_envs=B, num_history=3, resize_w=280, resize_h=280,
                                               max_seq_len=1536, max_patches=pv.shape[0])
    assert m.generation_config.repetition_penalty == p and m.generation_config.eos_token_id == (e0, e1)
    assert m.generation_config.raw["temperature"] == 0.1
    kw = dict(input_ids=ids, pixel_values=pv, image_grid_thw=grid, max_new_tokens=N_DEC)
    free = m.generate(**kw, eos_token_id=-1)                                   # no EOS: the whole penalised answer
    assert np.array_equal(free[:, S_:].cpu().numpy(), toks)
    assert torch.equal(free, m.generate(**kw, eos_token_id=-1, repetition_penalty=p))
    # against the unpenalised call: equal up to the first step at which the restatement says the penalty moves the choice, different there
    plain = m.generate(**kw, eos_token_id=-1, repetition_penalty=1.0)[:, S_:].cpu().numpy()
    moved = 0
    for b in range(B):
        raw_choice = [int(R.argmax_first(raws[j, b])) for j in range(N_DEC)]
        k = next((j for j in range(N_DEC) if raw_choice[j] != toks[b, j]), None)
        if k is None:
            assert plain[b].tolist() == toks[b].tolist()
        else:
            moved += 1
            assert plain[b, :k].tolist() == toks[b, :k].tolist() and plain[b, k] == raw_choice[k] != toks[b, k]
    print(f"rows whose answer the penalty {p} changes within {N_DEC} tokens: {moved} of {B}")
    assert moved, "test data: the penalty changes no row"
    # without arguments: the checkpoint's penalty and its EOS list - row 0 stops at e1 (the second id) and is filled with the first
    out = m.generate(**kw)[:, S_:].cpu().numpy()
    stops = set((e0, e1))
    for b in range(B):
        k = next((j for j in range(N_DEC) if int(toks[b, j]) in stops), None)
        if k is None:
            assert out[b, : out.shape[1]].tolist() == toks[b, : out.shape[1]].tolist()
        else:
            assert out[b, : k + 1].tolist() == toks[b, : k + 1].tolist() and (out[b, k + 1:] == e0).all()
    k0 = toks[0].tolist().index(e1)
    assert k0 <= 2 and out[0, k0] == e1 and (out[0, k0 + 1:] == e0).all() and out.shape[1] > k0 + 1
    # a key this engine does not implement is refused at load, by name; ignore_generation_config loads anyway
    gc = json.loads((tmp_path / "generation_config.json").read_text())
    (tmp_path / "generation_config.json").write_text(json.dumps(dict(gc, no_repeat_ngram_size=3)))
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):
        InternVLAN1ForCausalLM.from_pretrained(tmp_path, device_map={"": DEV})
