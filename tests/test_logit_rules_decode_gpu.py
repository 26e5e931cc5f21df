"""GPU: transformers' logits-processor keys through the 2-layer test model (3 prompts, 6 answer tokens) - prefill / decode with logit_rules=,
the captured plan() / run_decode chain, sampling behind a fan-out and behind shared prompts, constraint= with a forced EOS, token_logprobs,
generate() and the model's generation_rules, the agent, and the launch sequence with every key off.
The reference is tests/logit_rules_ref.py (pinned to transformers' classes in tests/test_logit_rules_cpu.py) applied to the engine's OWN raw
logits: the rule launch adds one fp32 bias per target or stores, so processed logits are compared exactly. Every rule set is derived from the
free greedy run so that it certainly binds."""
import numpy as np
import pytest
import torch

import logit_rules_ref as R
import logprob_ref as LP

from internnav_amd import logit_rules as LR
from internnav_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N = 3, 6
CFG = S.QWEN_TEST_CFG
V = CFG["vocab"]
EOS = CFG["eos_token_id"]


@pytest.fixture(scope="module")
def model(built_lib):
    from internnav_amd.policy import InternVLAN1ForCausalLM

    sd = {k: v.to(torch.bfloat16) for k, v in S.materialize(S.n1_full_spec(CFG, "nextdit_async"), 5).items()}
    m = InternVLAN1ForCausalLM(sd, CFG, "nextdit_async", device=DEV, max_envs=3 * B, num_history=3, resize_w=280, resize_h=280, cam_w=640, cam_h=480,
                               max_seq_len=1536, max_patches=8192, token_logprobs=True)
    inp = S.qwen_inputs(B, 1, seed=41, cfg=CFG, n_text=20, n_tail=12)
    ids, pv, grid = inp["input_ids"], inp["pixel_values"].to(DEV, torch.bfloat16), inp["grid_thw"]
    Sp = ids.shape[1]
    d = dict(ids=ids, pv=pv, grid=grid, S=Sp, lens=[Sp] * B, ragged=[Sp, Sp - 5, Sp - 2])
    d["free"] = _stepwise(m.qwen, d, None, None)
    d["free_ragged"] = _stepwise(m.qwen, d, None, d["ragged"])
    assert m.qwen._rhist is None, "an engine that never got rules holds history rows"
    return m, d


def _compile(d, spec, lens=None, eos=(EOS,), T=N):
    return LR.compile_rules(spec, V, list(eos), lens or d["lens"], T)


def _stepwise(e, d, rules, lens=None, n=N, ids=None, **kw):
    """decode n tokens one step at a time -> (tokens [B, n], the engine's logits after every step [n, B, vocab]: raw without rules, processed with)"""
    st = e.prefill(d["ids"] if ids is None else ids, d["pv"], d["grid"], **({} if lens is None else {"seq_lens": lens}),
                   **({} if rules is None else {"logit_rules": rules}), **kw)
    toks, logits = [], []
    for j in range(n):
        t = e.decode(st, 1) if j == 0 else e.decode(st, 2)[:, 1:]
        toks.append(t[:, 0].cpu().numpy())
        logits.append(e.logits[:B].cpu().numpy().copy())
    return np.stack(toks, 1), np.stack(logits)


def _hist(ids, lens, toks, b, j):
    return ids[b, : lens[b]].tolist() + toks[b, :j].tolist()


def _check_run(d, spec, toks, proc, free, lens=None, eos=(EOS,), ids=None, same_path=False):
    """step 0: processed == restatement(free raw) exactly and the token is its first argmax; every step: the -inf set is the restatement's ban
    set for prompt + answer so far; same_path: the tokens are the free run's and EVERY step's processed logits are restatement(free raw)"""
    lens, ids = lens or d["lens"], (d["ids"] if ids is None else ids).numpy()
    ftoks, fraw = free
    assert np.isfinite(fraw).all(), "test data: raw logits are finite"
    if same_path:
        assert np.array_equal(toks, ftoks), "test data: the rule set must not move the greedy path"
    for b in range(B):
        for j in range(N):
            h = _hist(ids, lens, toks, b, j)
            if j == 0 or same_path:
                want = R.apply_rules(fraw[j, b], h, j, spec, eos, lens[b], N)
                assert R.same(proc[j, b], want), (b, j, np.nonzero(~((proc[j, b] == want) | np.isnan(want)))[0][:6])
                assert toks[b, j] == int(np.argmax(want))
            bans = np.isneginf(R.apply_rules(np.zeros(V, dtype=np.float32), h, j, spec, eos, lens[b], N))
            assert np.array_equal(np.isneginf(proc[j, b]), bans), (b, j)
            assert not bans[toks[b, j]]
    moved = int((toks != ftoks).sum())
    return moved


def _rule_sets(d, free, lens):
    ftoks, fraw = free
    t0, t1 = ftoks[:, 0].tolist(), ftoks[:, 1].tolist()
    used = set(ftoks.reshape(-1).tolist()) | set(d["ids"].reshape(-1).tolist())
    unseen = [t for t in range(60, 3000) if t not in used][:B]
    lift = float(max(fraw[0, b].max() - fraw[0, b, unseen[b]] for b in range(B)) + 1.0)       # takes each row's unseen token above its step-0 maximum
    return {
        "suppress_tokens": (dict(suppress_tokens=sorted(set(t0))), (EOS,)),
        "bad_words_ids": (dict(bad_words_ids=[[t0[b], t1[b]] for b in range(B)]), (EOS,)),
        "sequence_bias": (dict(sequence_bias={(int(d["ids"][b, lens[b] - 1]), unseen[b]): lift for b in range(B)}), (EOS,)),
        "min_new_tokens": (dict(min_new_tokens=3), tuple(sorted(set(t1)))),
        "min_length": (dict(min_length=max(lens) + 2), tuple(sorted(set(t1)))),
        "forced_eos_token_id": (dict(forced_eos_token_id=[unseen[0], unseen[1]]), (EOS,)),
        "begin_suppress_tokens": (dict(begin_suppress_tokens=sorted(set(t0))), (EOS,)),
    }


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name", ["suppress_tokens", "bad_words_ids", "sequence_bias", "min_new_tokens", "min_length", "forced_eos_token_id",
                                  "begin_suppress_tokens"])
def test_rule_sets_that_bind(model, name, ragged):
    m, d = model
    lens = d["ragged"] if ragged else d["lens"]
    free = d["free_ragged"] if ragged else d["free"]
    spec, eos = _rule_sets(d, free, lens)[name]
    rules = _compile(d, spec, lens, eos)
    toks, proc = _stepwise(m.qwen, d, rules, lens if ragged else None)
    moved = _check_run(d, spec, toks, proc, free, lens, eos)
    print(f"{name} ragged={ragged}: tokens {toks.tolist()}, steps moved {moved}")
    assert moved, "test data: the rule set moved no step"
    ftoks = free[0]
    if name in ("suppress_tokens", "begin_suppress_tokens", "sequence_bias"):
        assert (toks[:, 0] != ftoks[:, 0]).all()
    if name == "bad_words_ids":
        assert all(toks[b, 0] == ftoks[b, 0] and toks[b, 1] != ftoks[b, 1] for b in range(B))
    if name == "forced_eos_token_id":
        assert np.array_equal(toks[:, :-1], ftoks[:, :-1]) and set(toks[:, -1].tolist()) <= set(spec[name])
    if name == "min_length" and ragged:                          # the row's OWN length: shorter prompts are held longer
        first = rules.eos_first.tolist()
        assert first == [max(lens) + 2 - n for n in lens] and len(set(first)) == B
    # a chunked decode (the policy's loop) equals single steps
    st = m.qwen.prefill(d["ids"], d["pv"], d["grid"], logit_rules=rules, **({"seq_lens": lens} if ragged else {}))
    a = m.qwen.decode(st, 2)
    b_ = m.qwen.decode(st, N - 2 + 1)[:, 1:]
    assert np.array_equal(torch.cat([a, b_], 1).cpu().numpy(), toks)


@pytest.mark.parametrize("k", [1, 2])
def test_no_repeat_ngram(model, k):
    """one text position of every prompt is rewritten to the prompt's last token, and an lm_head row crafted so that the token FOLLOWING it
    is the raw maximum of step 0: the token the rule must pass over"""
    m, d = model
    e = m.qwen
    ids = d["ids"].clone()
    for b in range(B):
        ids[b, 2 + b] = ids[b, -1]
    f = [int(ids[b, 3 + b]) for b in range(B)]
    t0 = _stepwise(e, d, None, n=1, ids=ids)[0][:, 0].tolist()
    assert len(set(f)) == B and not set(f) & set(t0), "test data"
    saved = {t: e.lm_head[t].clone() for t in f}
    try:
        for b in range(B):
            e.lm_head[f[b]].copy_((1.06 * e.lm_head[t0[b]].float()).to(torch.bfloat16))
        free = _stepwise(e, d, None, ids=ids)
        hit = [b for b in range(B) if free[0][b, 0] == f[b]]
        assert hit, "test data: the crafted follower is the raw step-0 maximum in no row"
        spec = dict(no_repeat_ngram_size=k)
        toks, proc = _stepwise(e, d, _compile(d, spec), ids=ids)
        _check_run(d, spec, toks, proc, free, ids=ids)
        assert all(toks[b, 0] != f[b] for b in hit)
        if k == 1:                                               # no token of prompt + answer is ever chosen again
            assert all(int(toks[b, j]) not in _hist(ids.numpy(), d["lens"], toks, b, j) for b in range(B) for j in range(N))
    finally:
        for t, v in saved.items():
            e.lm_head[t].copy_(v)


def _quiet_spec(d):
    """small finite biases on low-ranked tokens (single tokens and sequences behind the prompts' last tokens and the free answers' tokens) and
    bans of low-ranked tokens: the greedy path stays the free run's"""
    ftoks, fraw = d["free"]
    low = [int(t) for t in np.argsort(fraw.max(axis=(0, 1)))[:12]]      # the lowest of the per-token maxima over every step and row
    sb = {(low[0],): 0.25, (low[1],): -0.5}
    for b in range(B):                                                   # (duplicate targets: low[2 + b] and low[5])
        sb.update({(int(d["ids"][b, -1]), low[2 + b]): 0.125, (int(ftoks[b, 0]), int(ftoks[b, 1]), low[2 + b]): 0.375, (int(ftoks[b, 2]), low[5]): -0.25})
    return dict(sequence_bias=sb, suppress_tokens=[low[6]], begin_suppress_tokens=[low[7]], bad_words_ids=[[int(ftoks[0, 0]), low[8]], [low[9]]],
                no_repeat_ngram_size=16, min_new_tokens=2)


def test_path_preserving_rules_give_the_restatement_at_every_step(model):
    m, d = model
    spec = _quiet_spec(d)
    toks, proc = _stepwise(m.qwen, d, _compile(d, spec))
    _check_run(d, spec, toks, proc, d["free"], same_path=True)
    changed = sum(not R.same(proc[j, b], d["free"][1][j, b]) for j in range(N) for b in range(B))
    assert changed == N * B


def test_captured_decode_equals_eager_and_starts_over_on_replay(model):
    from internnav_amd.runtime import GraphedCall

    m, d = model
    e = m.qwen
    spec, eos = _rule_sets(d, d["free"], d["lens"])["bad_words_ids"]
    spec = dict(spec, no_repeat_ngram_size=1, min_new_tokens=2)
    rules = _compile(d, spec, eos=eos)
    want = _stepwise(e, d, rules)[0]
    assert not np.array_equal(want, d["free"][0])
    P = e.plan(d["ids"], d["grid"], n_decode=N, logit_rules=rules)
    assert P["rules_key"] == rules.key
    e.run_prefill(P, d["pv"])
    toks = torch.zeros(B, N, dtype=torch.int32, device=DEV)
    e.run_decode(P, toks)
    assert np.array_equal(toks.cpu().numpy(), want)
    g = GraphedCall(lambda: e.run_decode(P, toks), {})
    for _ in range(2):
        toks.zero_()
        e._rhist.fill_(int(want[0, 1]))                          # were the history fill outside the capture, the rows would start from this
        g()
        torch.cuda.synchronize()
        assert np.array_equal(toks.cpu().numpy(), want)
    hist = e._rhist[:B, : d["S"] + N - 1].cpu().numpy()
    assert all(hist[b].tolist() == d["ids"][b].tolist() + want[b, : N - 1].tolist() for b in range(B))


def _gen(m, d, **kw):
    return m.generate(input_ids=d["ids"], pixel_values=d["pv"], image_grid_thw=d["grid"], max_new_tokens=N, eos_token_id=-1, return_dict_in_generate=True, **kw)


def test_top_k_1_sampling_equals_greedy_with_rules_with_a_history_per_returned_row(model):
    m, d = model
    spec, _ = _rule_sets(d, d["free"], d["lens"])["bad_words_ids"]
    spec = dict(spec, no_repeat_ngram_size=2, suppress_tokens=[int(d["free"][0][1, 0])], forced_eos_token_id=77)
    greedy = _gen(m, d, **spec).sequences
    assert not np.array_equal(greedy[:, d["S"]:].cpu().numpy(), d["free"][0]) and bool((greedy[:, -1] == 77).all())
    K = 3
    for share in (False, True):
        res = _gen(m, d, do_sample=True, top_k=1, seed=3, num_return_sequences=K, share_prefix=share, **spec).sequences
        assert torch.equal(res, greedy.repeat_interleave(K, dim=0)), share
        hist = (m.qwen._shared if share else m.qwen)._rhist[: B * K, : d["S"] + N - 1].cpu()
        assert torch.equal(hist.long(), res[:, : d["S"] + N - 1].cpu()), share          # prompt + the row's own answer but the last token


def test_forced_eos_wins_over_the_automaton_and_scores_zero(model):
    from internnav_amd.constrain import TokenAutomaton

    m, d = model
    path = [t for t in range(100, 200) if t not in set(d["free"][0].reshape(-1).tolist())][:N + 2]
    trie = TokenAutomaton.from_token_sequences([path], [EOS], V)      # allows exactly path[j] at step j: 999 is banned at every step
    res = _gen(m, d, constraint=trie, forced_eos_token_id=999, output_logprobs=True)
    ans = res.sequences[:, d["S"]:].cpu()
    assert ans[:, :-1].tolist() == [path[: N - 1]] * B and ans[:, -1].tolist() == [999] * B
    assert bool((res.token_logprobs == 0.0).all())                    # one allowed token per step, and exactly 0.0 at the forced one


def test_token_logprobs_are_the_log_softmax_over_the_unbanned_entries(model):
    m, d = model
    spec, _ = _rule_sets(d, d["free"], d["lens"])["suppress_tokens"]
    spec = dict(spec, sequence_bias={(int(d["free"][0][0, 1]),): -3.0}, forced_eos_token_id=[5, 6])
    rules = _compile(d, spec)
    e = m.qwen
    st = e.prefill(d["ids"], d["pv"], d["grid"], logit_rules=rules)
    for j in range(N):
        tok = (e.decode(st, 1) if j == 0 else e.decode(st, 2)[:, 1:])[:, 0].cpu().numpy()
        y = e.logits[:B].cpu().numpy()
        lp, mg = (t.cpu().numpy() for t in e.last_logprobs(st))
        aligned = e.logits.data_ptr() % 16 == 0 and (V * 4) % 16 == 0
        for b in range(B):
            t, want, wmg, _ = LP.logprob_row(y[b])
            ok, msg, err, bound = LP.check_row(float(lp[b, j]), float(mg[b, j]), y[b], t, want, wmg, aligned)
            assert ok and t == tok[b], (b, j, msg)
            assert j < N - 1 or (tok[b] == 5 and abs(want + np.log(2.0)) < 1e-12)      # two forced ids at 0.0: the first, at log(1/2)
    res = _gen(m, d, forced_eos_token_id=5, output_logprobs=True)
    assert bool((res.token_logprobs[:, -1] == 0.0).all()) and bool((res.sequences[:, -1] == 5).all())


def test_generate_arguments_and_model_rules(model, tmp_path):
    from internnav_amd.policy import InternVLAN1ForCausalLM

    m, d = model
    ftoks = d["free"][0]
    kw = dict(input_ids=d["ids"], pixel_values=d["pv"], image_grid_thw=d["grid"], max_new_tokens=N)
    e1 = int(ftoks[0, 1])                                            # with this EOS id the free answer of row 0 ends after two tokens
    free = m.generate(**kw, eos_token_id=e1)
    held = m.generate(**kw, eos_token_id=e1, min_new_tokens=4)
    assert free[0, d["S"]: d["S"] + 2].tolist() == ftoks[0, :2].tolist() and set(free[0, d["S"] + 2:].tolist()) <= {e1} and not torch.equal(free[0], held[0])
    assert e1 not in held[0, d["S"]: d["S"] + 4].tolist()
    with pytest.raises(ValueError, match="suppress_tokens"):
        m.generate(**kw, suppress_tokens=[V])
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):
        m.generate(**kw, num_beams=2, no_repeat_ngram_size=2)
    # past_key_values: the cached prompt tokens count in the history like any other
    spec = dict(no_repeat_ngram_size=1, bad_words_ids=[[int(ftoks[1, 0]), int(ftoks[1, 1])]])
    ref = m.generate(**kw, eos_token_id=-1, return_dict_in_generate=True, **spec)
    again = m.generate(**kw, eos_token_id=-1, return_dict_in_generate=True, past_key_values=ref.past_key_values, **spec)
    print("prompt rows taken from the cache:", m.last_kv_reuse["rows"])
    assert torch.equal(ref.sequences, again.sequences)
    assert not np.array_equal(ref.sequences[:, d["S"]:].cpu().numpy(), ftoks)
    # the model's default rules: a dict, or the checkpoint's generation_config.json ("file"), overridden key by key by the arguments
    rules = dict(suppress_tokens=sorted(set(ftoks[:, 0].tolist())), min_new_tokens=2)
    want = m.generate(**kw, eos_token_id=e1, **rules)
    S.write_checkpoint(tmp_path, CFG, "nextdit_async", seed=5, generation_config=dict(rules, eos_token_id=e1))
    load = dict(device_map={"": DEV}, max_envs=B, num_history=3, resize_w=280, resize_h=280, max_seq_len=1536, max_patches=8192)
    with pytest.raises(NotImplementedError, match="suppress_tokens"):
        InternVLAN1ForCausalLM.from_pretrained(tmp_path, **load)
    m2 = InternVLAN1ForCausalLM.from_pretrained(tmp_path, generation_rules="file", **load)
    assert m2.generation_rules == LR.normalize(rules, V) and m2.qwen._rhist is None
    assert torch.equal(m2.generate(**kw), want)
    assert torch.equal(m2.generate(**kw, min_new_tokens=4), m.generate(**kw, eos_token_id=e1, **dict(rules, min_new_tokens=4)))
    del m2
    m3 = InternVLAN1ForCausalLM.from_pretrained(tmp_path, generation_rules=dict(rules, min_new_tokens=4), ignore_generation_config=True, **load)
    assert torch.equal(m3.generate(**kw, eos_token_id=e1), m.generate(**kw, eos_token_id=e1, **dict(rules, min_new_tokens=4)))


class _Tok:
    def __call__(self, texts, return_tensors="pt"):
        ids, i, t = [], 0, texts[0]
        special = {"<|image_pad|>": CFG["image_token_id"], "<|vision_start|>": CFG["vision_start_id"], "<|vision_end|>": CFG["vision_end_id"]}
        while i < len(t):
            k = next((k for k in special if t.startswith(k, i)), None)
            ids.append(special[k] if k else ord(t[i]) % 3000)
            i += len(k) if k else 1
        return {"input_ids": torch.tensor([ids])}

    def decode(self, ids, skip_special_tokens=True):
        return "#" * len(ids)


class _Proc:
    image_token = "<|image_pad|>"
    tokenizer = _Tok()

    def apply_chat_template(self, conv, tokenize=False, add_generation_prompt=True):
        return "".join("<|vision_start|><|image_pad|><|vision_end|>" if c["type"] == "image" else c["text"] for m in conv for c in m["content"])


def test_model_generation_rules_reach_the_agents_system2_calls(model):
    from internnav_amd.agent import InternVLAN1Agent
    from internnav_amd.policy import InternVLAN1Net
    from internnav_amd.preprocess import FramePreprocessor

    m, d = model
    pre = FramePreprocessor(DEV, resize_w=280, resize_h=280)
    rng = np.random.default_rng(9)
    frames = [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(2)]
    first = {}
    try:
        for name in ("free", "rules"):
            agent = InternVLAN1Agent({"model_settings": {"infer_mode": "partial_async"}}, policy_factory=lambda: InternVLAN1Net(
                m, _Proc(), num_history=3, resize_w=280, resize_h=280, frame_preprocessor=pre), frame_preprocessor=pre)
            env = agent._env(0)
            env.policy.step_no_infer(frames[0], None, None)
            seqs, plen, gen = [], [], m.generate

            def spy(*a, **k):
                r = gen(*a, **k)
                seqs.append(r.sequences.cpu())
                plen.append(k["input_ids"].shape[1])
                return r

            m.generate = spy
            try:
                agent._run_s2([(env, {"rgb": frames[1], "depth": None, "instruction": "go to the door"})])
            finally:
                del m.generate
            first[name] = int(seqs[0][0, plen[0]])
            m.generation_rules = LR.normalize(dict(suppress_tokens=[first["free"]]), V)      # what generation_rules= of the model / model_settings sets
    finally:
        m.generation_rules = {}
    assert first["rules"] != first["free"]
    assert float(m.qwen.logits[0, first["free"]]) == float("-inf")


def test_with_every_key_off_the_launch_sequence_is_the_parents(model, monkeypatch):
    from internnav_amd import ops
    from internnav_amd.policy import InternVLAN1ForCausalLM

    m, d = model
    sd = {k: v.to(torch.bfloat16) for k, v in S.materialize(S.n1_full_spec(CFG, "nextdit_async"), 5).items()}
    fresh = InternVLAN1ForCausalLM(sd, CFG, "nextdit_async", device=DEV, max_envs=B, num_history=3, resize_w=280, resize_h=280, cam_w=640, cam_h=480,
                                   max_seq_len=1536, max_patches=8192, generation_rules=dict(min_length=0, suppress_tokens=[]))
    calls = []
    for name in dir(ops):
        fn = getattr(ops, name)
        if not name.startswith("_") and callable(fn) and getattr(fn, "__module__", None) == ops.__name__ and not isinstance(fn, type):
            monkeypatch.setattr(ops, name, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(fn, name))

    def record(mm, **kw):
        del calls[:]
        res = _gen(mm, d, use_cache=False, **kw)
        return list(calls), res.sequences

    off = dict(sequence_bias=None, no_repeat_ngram_size=0, bad_words_ids=[], min_length=0, min_new_tokens=0, forced_eos_token_id=None, suppress_tokens=[],
               begin_suppress_tokens=[])
    record(fresh)
    plain, r0 = record(fresh)
    none, r1 = record(fresh, **off)
    assert plain == none and "logit_rules_rows" not in plain and torch.equal(r0, r1) and plain.count("argmax_rows") == N
    assert fresh.qwen._rhist is None and fresh.qwen._shared is None and fresh.generation_rules == {}
    on, r2 = record(fresh, begin_suppress_tokens=[int(r0[0, d["S"]])])
    want = []
    for c in plain:
        want += ["logit_rules_rows", c] if c == "argmax_rows" else [c]
    assert on == want and not torch.equal(r0, r2) and fresh.qwen._rhist is not None
