"""GPU: constrained System-2 decoding through the 2-layer test model - generate(constraint=) greedy and sampled (fan-out, shared prompts), the
captured plan() / run_decode chain, the engine's logits and state buffers, the unconstrained launch sequence, and the agent's
answer_constraint. The host methods of TokenAutomaton (pinned in tests/test_constrain_cpu.py) are the reference."""
import numpy as np
import pytest
import torch

import constrain_ref as R

from internnav_amd import synthetic as S
from internnav_amd.constrain import TokenAutomaton

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, SEQS, N_NEW = 2, 10, 8
CFG = S.QWEN_TEST_CFG
EOS = CFG["eos_token_id"]
TOKS, _ = R.byte_vocab(300)


@pytest.fixture(scope="module")
def model(built_lib):
    from internnav_amd.policy import InternVLAN1ForCausalLM

    sd = {k: v.to(torch.bfloat16) for k, v in S.materialize(S.n1_full_spec(CFG, "nextdit_async"), 5).items()}
    m = InternVLAN1ForCausalLM(sd, CFG, "nextdit_async", device=DEV, max_envs=SEQS, num_history=3, resize_w=280, resize_h=280, cam_w=640, cam_h=480,
                               max_seq_len=1536, max_patches=8192, token_logprobs=True)
    inp = S.qwen_inputs(B, 1, seed=33, cfg=CFG, n_text=20, n_tail=12)
    Sp = inp["input_ids"].shape[1]
    ids, mask = inp["input_ids"].clone(), torch.ones(B, Sp, dtype=torch.long)
    ids[1, Sp - 3:], mask[1, Sp - 3:] = 0, 0                              # ragged: prompt 1 loses its last three tokens
    plens = [Sp, Sp - 3]
    assert m.qwen._cstate is None, "an engine that never got a constraint holds state buffers"
    free = _gen(m, dict(ids=ids, mask=mask, inp=inp)).sequences
    free = [free[b, plens[b]: plens[b] + N_NEW].tolist() for b in range(B)]
    assert m.qwen._cstate is None
    return m, dict(ids=ids, mask=mask, inp=inp, plens=plens, free=free)


def _gen(m, d, n=N_NEW, **kw):
    return m.generate(input_ids=d["ids"], attention_mask=d["mask"], pixel_values=d["inp"]["pixel_values"], image_grid_thw=d["inp"]["grid_thw"],
                      max_new_tokens=n, return_dict_in_generate=True, output_logprobs=True, **kw)


def _answers(res, d, K=1):
    """the answer tokens of every returned row (all rows are as wide as the longest prompt + the tokens generated)"""
    n = res.sequences.shape[1] - d["ids"].shape[1]
    return [res.sequences[r, d["plens"][r // K]: d["plens"][r // K] + n].tolist() for r in range(res.sequences.shape[0])]


def _unused(d, count, lo=50):
    """`count` token ids the unconstrained answers do not hold (and no special id)"""
    used = {t for row in d["free"] for t in row}
    out = [t for t in range(lo, 4000) if t not in used][:count]
    return out


def _nav(d):
    """navigation_answers over the synthetic byte vocabulary, mapped onto a window of test-vocabulary ids the unconstrained answers avoid"""
    used = {t for row in d["free"] for t in row}
    off = next(o for o in range(100, 3600, 300) if not any(o <= t < o + 300 for t in used))
    tb = [b""] * CFG["vocab"]
    tb[off: off + 299] = TOKS[:299]
    return TokenAutomaton.navigation_answers(tb, [EOS]), tb


def test_universal_automaton_is_the_unconstrained_call(model):
    m, d = model
    u = TokenAutomaton.universal(CFG["vocab"], [EOS])
    for kw in ({}, {"repetition_penalty": 1.3}, dict(do_sample=True, temperature=1.2, top_k=0, top_p=0.95, seed=5)):
        a, b = _gen(m, d, **kw), _gen(m, d, constraint=u, **kw)
        assert torch.equal(a.sequences, b.sequences), kw
        assert torch.equal(a.token_logprobs.view(torch.int32), b.token_logprobs.view(torch.int32)), kw
    with pytest.raises(ValueError, match="constraint"):
        _gen(m, d, constraint=TokenAutomaton.universal(300, [7]))


def test_single_path_trie_forces_the_answer(model):
    m, d = model
    path = _unused(d, 3)
    a = TokenAutomaton.from_token_sequences([path], [EOS], CFG["vocab"])
    for kw in ({}, {"repetition_penalty": 1.3}, dict(do_sample=True, temperature=1.0, top_k=0, top_p=1.0, seed=1)):
        res = _gen(m, d, constraint=a, **kw)
        for b, row in enumerate(_answers(res, d)):
            assert row[:4] == path + [EOS] and set(row[4:]) <= {EOS}, (kw, b, row)
        assert bool((res.token_logprobs == 0.0).all()) and res.answer_lengths.tolist() == [4, 4], (kw, res.token_logprobs)


def test_answers_satisfy_the_automaton_where_the_free_answer_does_not(model):
    m, d = model
    t = _unused(d, 6)
    trie = TokenAutomaton.from_token_sequences([t[:3], [t[0], t[3]], [t[4], t[5], t[0], t[1]]], [EOS], CFG["vocab"])
    nav, tb = _nav(d)
    for name, a, n in (("trie", trie, N_NEW), ("nav", nav, N_NEW), ("nav cut", nav, 2)):
        assert not any(a.accepts(row) for row in d["free"]) and all(a.run(row[:1]) < 0 for row in d["free"]), name
        res = _gen(m, d, n=n, constraint=a)
        for row in _answers(res, d):
            assert len(row) == n
            assert a.accepts(row) if EOS in row else a.run(row) >= 0, (name, row)
        if name == "nav":
            text = [b"".join(tb[i] for i in row if i != EOS).decode("utf-8") for row in _answers(res, d)]
            print("constrained navigation answers:", text)
            assert all(s == "STOP" or set(s) <= set("↑←→↓") or (len(s.replace(",", " ").split()) == 2 and s.replace(",", " ").replace(" ", "").isdigit()) for s in text), text


def test_captured_decode_equals_eager_and_reinitialises_on_replay(model):
    from internnav_amd.runtime import GraphedCall

    m, d = model
    e, inp = m.qwen, d["inp"]
    nav, _ = _nav(d)
    ids, grid, pv = inp["input_ids"], inp["grid_thw"], inp["pixel_values"].to(DEV, torch.bfloat16)
    free = e.decode(e.prefill(ids, pv, grid), 4).cpu()
    want = e.decode(e.prefill(ids, pv, grid, constraint=nav), 4).cpu()
    assert not torch.equal(free, want) and all(nav.run(r) >= 0 for r in want.tolist())
    P = e.plan(ids, grid, n_decode=4, constraint=nav)
    e.run_prefill(P, pv)
    toks = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    e.run_decode(P, toks)
    assert torch.equal(toks.cpu(), want)
    g = GraphedCall(lambda: e.run_decode(P, toks), {})
    for _ in range(2):
        toks.zero_()
        e._cstate.fill_(-1)                                              # were the state fill outside the capture, no row would be masked
        g()
        torch.cuda.synchronize()
        assert torch.equal(toks.cpu(), want)


def test_sampling_fan_out_and_shared_prompts_keep_a_state_per_row(model):
    m, d = model
    nav, _ = _nav(d)
    greedy = _gen(m, d, constraint=nav)
    top1 = _gen(m, d, constraint=nav, do_sample=True, top_k=1, seed=2)
    assert torch.equal(greedy.sequences, top1.sequences)
    t = _unused(d, 8)
    fork = TokenAutomaton.from_token_sequences([[t[0], t[2], t[3], t[4]], [t[1], t[5], t[6], t[7]]], [EOS], CFG["vocab"])
    for K, share in ((3, False), (5, True)):
        both = False
        for a in (nav, fork):
            for seed in range(16 if a is fork else 1):
                res = _gen(m, d, constraint=a, do_sample=True, temperature=50.0, top_k=0, top_p=1.0, num_return_sequences=K, share_prefix=share, seed=seed)
                rows = _answers(res, d, K)
                assert len(rows) == B * K
                for row in rows:
                    assert a.accepts(row) if EOS in row else a.run(row) >= 0, (K, share, seed, row)
                # the engine's state of every row = the host automaton's after the row's own tokens but the last selected one
                st = m._gen["state"]
                n_sel = int(st["n_sel"])
                buf = (m.qwen._shared if share else m.qwen)._cstate
                got = buf[n_sel & 1, : B * K].cpu().tolist()
                assert got == [a.run(row[: n_sel - 1]) for row in rows], (K, share, seed)
                if a is fork:
                    assert all(row[:5] in ([t[0], t[2], t[3], t[4], EOS], [t[1], t[5], t[6], t[7], EOS]) for row in rows), rows
                    both = both or any(len({row[0] for row in rows[b * K: (b + 1) * K]}) == 2 for b in range(B))
                    if both:
                        break
        print(f"K={K} share_prefix={share}: rows of one prompt in both branches of the trie: {both} (seed {seed})")
        assert both, "no seed below 16 put the rows of one prompt into different branches"


def test_logits_after_step_0_are_finite_exactly_on_the_start_set(model):
    m, d = model
    e, inp = m.qwen, d["inp"]
    nav, _ = _nav(d)
    st = e.prefill(inp["input_ids"], inp["pixel_values"].to(DEV, torch.bfloat16), inp["grid_thw"], constraint=nav)
    tok = e.decode(st, 1)[:, 0].cpu().tolist()
    fin = torch.isfinite(e.logits[:B]).cpu().numpy()
    want = np.zeros(CFG["vocab"], dtype=bool)
    want[nav.allowed_ids(nav.start)] = True
    assert 0 < want.sum() < 100 and all(np.array_equal(fin[b], want) for b in range(B))
    assert bool((e.logits[:B][~torch.from_numpy(fin)] == float("-inf")).all()) and all(want[t] for t in tok)


def test_without_a_constraint_the_launch_sequence_is_the_parents(model, monkeypatch):
    from internnav_amd import ops

    m, d = model
    calls = []
    for name in dir(ops):
        fn = getattr(ops, name)
        if not name.startswith("_") and callable(fn) and getattr(fn, "__module__", None) == ops.__name__ and not isinstance(fn, type):
            monkeypatch.setattr(ops, name, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(fn, name))

    def record(**kw):
        del calls[:]
        res = _gen(m, d, n=4, use_cache=False, **kw)                     # (no cache handle in the result: a live one makes the next call export its rows first)
        return list(calls), res

    nav, _ = _nav(d)
    record()                                                             # (takes whatever an earlier test's cache handle leaves to do)
    plain, r0 = record()
    none, r1 = record(constraint=None)
    on, r2 = record(constraint=nav)
    assert plain == none and "automaton_mask_rows" not in plain and torch.equal(r0.sequences, r1.sequences)
    assert plain.count("logprob_rows") == 4                              # (a token_logprobs model: logprob_rows is the selection launch)
    want = []
    for c in plain:
        want += ["automaton_mask_rows", c] if c == "logprob_rows" else [c]
    assert on == want and not torch.equal(r0.sequences, r2.sequences)


class _Tok:
    def __init__(self, token_bytes):
        self.tb = token_bytes

    def __call__(self, texts, return_tensors="pt"):
        ids, i, t = [], 0, texts[0]
        special = {"<|image_pad|>": CFG["image_token_id"], "<|vision_start|>": CFG["vision_start_id"], "<|vision_end|>": CFG["vision_end_id"]}
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
        return b"".join(self.tb[int(i)] or (b"" if int(i) == EOS else b"#") for i in ids).decode("utf-8", errors="replace")


class _Proc:
    image_token = "<|image_pad|>"

    def __init__(self, tok):
        self.tokenizer = tok

    def apply_chat_template(self, conv, tokenize=False, add_generation_prompt=True):
        return "".join("<|vision_start|><|image_pad|><|vision_end|>" if c["type"] == "image" else c["text"] for m in conv for c in m["content"])


def test_agent_answer_constraint_parses_without_a_retry(model):
    from internnav_amd.agent import InternVLAN1Agent
    from internnav_amd.policy import InternVLAN1Net
    from internnav_amd.preprocess import FramePreprocessor

    m, d = model
    pre = FramePreprocessor(DEV, resize_w=280, resize_h=280)
    rng = np.random.default_rng(9)
    frames = [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(2)]
    tb = [b""] * CFG["vocab"]                                            # every id without bytes decodes to '#' (_Tok.decode)
    out = {}
    for name in ("free", "constrained"):
        # the byte vocabulary goes onto ids the unconstrained answers never hold (seen in the first round), so under this tokenizer the
        # unconstrained answer is all '#': it holds neither a pixel goal nor an action
        cst = TokenAutomaton.navigation_answers(tb, [EOS]) if name == "constrained" else None
        agent = InternVLAN1Agent({"model_settings": {"infer_mode": "partial_async"}}, policy_factory=lambda cst=cst: InternVLAN1Net(
            m, _Proc(_Tok(tb)), num_history=3, resize_w=280, resize_h=280, frame_preprocessor=pre, answer_constraint=cst), frame_preprocessor=pre)
        env = agent._env(0)
        env.policy.step_no_infer(frames[0], None, None)
        seqs, gen = [], m.generate

        def spy(*a, **k):
            r = gen(*a, **k)
            seqs.append(r.sequences.cpu())
            return r

        m.generate = spy
        try:
            agent._run_s2([(env, {"rgb": frames[1], "depth": None, "instruction": "go to the door"})])
        finally:
            del m.generate
        out[name] = (len(seqs), agent.s2_failures, env.s2_output, env.policy.llm_output)
        print(f"{name}: generate calls {len(seqs)}, STOP fallbacks {agent.s2_failures}, answer {env.policy.llm_output[:40]!r}")
        if name == "free":
            used = set(torch.cat([s.reshape(-1) for s in seqs]).tolist())
            pool = [t for t in range(50, 4000) if t not in used][:299]
            for i, t in enumerate(pool):
                tb[t] = TOKS[i]
            assert all(set(_Tok(tb).decode(s[0])) <= {"#"} for s in seqs)      # the free answers (and prompts) under the final tokenizer
    calls, fails, so, text = out["free"]
    assert calls == 2 and fails == 1 and so.output_action == [0], "test data: the unconstrained answer parses"
    calls, fails, so, text = out["constrained"]
    assert calls == 1 and fails == 0
    assert (so.output_action and all(a in (0, 1, 2, 3, 5) for a in so.output_action)) or (so.output_pixel is not None and so.output_latent is not None), text
