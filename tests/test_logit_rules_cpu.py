"""CPU: the logits-processor rules of internnav_amd/logit_rules.py.
 1. the numpy restatement (tests/logit_rules_ref.py, from the key values) against transformers' own processor classes in
    `_get_logits_processor`'s order, RepetitionPenaltyLogitsProcessor in its place: IEEE-equal, tolerance zero (the only arithmetic is one
    fp32 add per biased entry, in HF's order);
 2. the COMPILED tables, interpreted by a few lines of numpy, against the restatement on the same cases;
 3. the host behaviour: every ValueError and capacity refusal, the empty spec, the load-time parameter, beams + rules."""
import numpy as np
import pytest
import torch

import logit_rules_ref as R
from internnav_amd import logit_rules as LR

ALONE = [(k,) for k in R.KEYS] + [("min_length", "min_new_tokens")]
N_CASES = 18                                                   # per key set: 9 key sets x 18 + 40 all-key cases = 202 seeded cases
VOCABS = [64, 257, 1000, 4100]


def _hf(case, penalty):
    """transformers' processors for the case, as _get_logits_processor instantiates and orders them"""
    from transformers.generation import logits_process as P

    s, eos, L0, T = case["spec"], torch.tensor(case["eos"]), case["prompt_len"], case["T"]
    procs = []
    if s.get("sequence_bias"):
        procs.append(P.SequenceBiasLogitsProcessor(sequence_bias=[[list(ids), b] for ids, b in s["sequence_bias"]]))
    procs.append(P.RepetitionPenaltyLogitsProcessor(penalty=penalty))
    if s.get("no_repeat_ngram_size"):
        procs.append(P.NoRepeatNGramLogitsProcessor(s["no_repeat_ngram_size"]))
    if s.get("bad_words_ids"):
        procs.append(P.NoBadWordsLogitsProcessor(s["bad_words_ids"], eos))
    min_length = L0 + s["min_new_tokens"] if s.get("min_new_tokens") else s.get("min_length")      # generate() overwrites min_length so
    if min_length:
        procs.append(P.MinLengthLogitsProcessor(min_length, eos))
    if s.get("min_new_tokens"):
        procs.append(P.MinNewTokensLengthLogitsProcessor(L0, s["min_new_tokens"], eos))
    if s.get("forced_eos_token_id") is not None:
        procs.append(P.ForcedEOSTokenLogitsProcessor(L0 + T, s["forced_eos_token_id"]))
    if s.get("suppress_tokens"):
        procs.append(P.SuppressTokensLogitsProcessor(s["suppress_tokens"]))
    if s.get("begin_suppress_tokens"):
        procs.append(P.SuppressTokensAtBeginLogitsProcessor(s["begin_suppress_tokens"], L0))
    return procs


def _penalty(x, history, penalty):
    """RepetitionPenaltyLogitsProcessor on the processed scores: what the selection kernels do behind the rule launch"""
    x = np.array(x, dtype=np.float32, copy=True)
    seen = sorted(set(history))
    v = x[seen]
    x[seen] = np.where(v < 0, v * np.float32(penalty), v / np.float32(penalty))
    return x


def _cases(keys, seed0):
    for i in range(N_CASES):
        g = np.random.default_rng(seed0 + i)
        n = VOCABS[i % 4] if i < 8 else int(g.integers(64, 4101))
        yield R.random_case(g, n, keys)


def _check_hf(case):
    ids = torch.tensor([case["history"]], dtype=torch.long)
    ours = R.apply_rules(case["x"], case["history"], case["col"], case["spec"], case["eos"], case["prompt_len"], case["T"])
    for pen in (1.0, 1.3):
        y = torch.from_numpy(case["x"].copy())[None]
        for p in _hf(case, pen):
            y = p(ids, y)
        assert R.same(_penalty(ours, case["history"], pen), y[0].numpy()), (pen, case["spec"])
    return ours


@pytest.mark.parametrize("keys", ALONE, ids=["+".join(k) for k in ALONE])
def test_restatement_equals_transformers_one_key(keys):
    for case in _cases(keys, 1000 * (1 + ALONE.index(keys))):
        ours = _check_hf(case)
        assert not R.same(ours, case["x"]), ("test data: the rule changed nothing", case["spec"], case["col"])


def test_restatement_equals_transformers_all_keys():
    for i in range(40):
        g = np.random.default_rng(77000 + i)
        kw = dict(T=1, col=0) if i % 2 else dict(col=int(g.integers(0, 6)))       # T = 1: the begin list and the forced column bind together
        case = R.random_case(g, int(g.integers(64, 4101)), R.KEYS, **kw)
        ours = _check_hf(case)
        assert not R.same(ours, case["x"]), "test data: the rules changed nothing"


def test_restatement_edges_against_transformers():
    g = np.random.default_rng(5)
    x = (g.standard_normal(64) * 3).astype(np.float32)
    base = dict(x=x, T=4, eos=[3, 9])
    # history shorter than n - 1, exactly n - 1 (no window yet) and n
    for H, changes in ((1, False), (2, False), (3, True)):
        case = dict(base, history=[7] * H, col=0, prompt_len=H, spec=dict(no_repeat_ngram_size=3))
        assert R.same(_check_hf(case), x) != changes
    # a sequence longer than the history is ignored, one of the history's length matches
    for ids, changes in (([5, 5, 5, 8], False), ([5, 5, 8], True)):
        case = dict(base, history=[5, 5, 5], col=1, prompt_len=2, spec=dict(sequence_bias=[[ids, 2.0]], bad_words_ids=[ids[:-1] + [11]]))
        assert R.same(_check_hf(case), x) != changes
    # [eos] inside bad_words_ids is dropped, another single token is not
    out = _check_hf(dict(base, history=[5, 6], col=0, prompt_len=2, spec=dict(bad_words_ids=[[3], [9], [12]])))
    assert np.isfinite(out[[3, 9]]).all() and out[12] == -np.inf
    # duplicate targets: the biases of every matched sequence add up in dict order, on top of the single-token bias
    sb = [[[8], 0.1], [[6, 8], 1e7], [[5, 6, 8], -1e7], [[4, 8], 3.0]]
    out = _check_hf(dict(base, history=[4, 5, 6], col=0, prompt_len=3, spec=dict(sequence_bias=sb)))
    assert out[8] == x[8] + np.float32(np.float32(np.float32(0.1) + np.float32(1e7)) + np.float32(-1e7))
    # both length keys: min_new_tokens takes precedence over a larger and over a smaller min_length
    for ml in (1, 50):
        for col, banned in ((0, True), (1, True), (2, False)):
            out = _check_hf(dict(base, history=[5] * (4 + col), col=col, prompt_len=4, spec=dict(min_length=ml, min_new_tokens=2)))
            assert (out[3] == -np.inf) == banned and (out[9] == -np.inf) == banned
    # the forced column: everything -inf, the forced ids 0.0 - unless suppress_tokens names them (it runs behind)
    out = _check_hf(dict(base, history=[5] * 7, col=3, prompt_len=4, spec=dict(forced_eos_token_id=[3, 9], suppress_tokens=[9], sequence_bias=[[[3], 2.0]])))
    assert out[3] == 0.0 and np.isneginf(np.delete(out, 3)).all()


# ---- 2. the compiled tables
@pytest.mark.parametrize("keys", ALONE + [R.KEYS], ids=["+".join(k) for k in ALONE] + ["all"])
def test_compiled_tables_equal_restatement(keys):
    for i in range(N_CASES):
        g = np.random.default_rng(31000 + 100 * len(keys) + i)
        kw = dict(T=1, col=0) if len(keys) > 2 and i % 2 else {}
        case = R.random_case(g, VOCABS[i % 4], keys, adversarial=bool(i % 3 == 0), finite=bool(i % 2), **kw)
        lens = [case["prompt_len"] + 3, case["prompt_len"]]              # the case is row 1 of a ragged pair: its own length counts
        tb = LR.compile_rules(case["spec"], case["x"].size, case["eos"], lens, case["T"])
        want = R.apply_rules(case["x"], case["history"], case["col"], case["spec"], case["eos"], case["prompt_len"], case["T"])
        if tb is None:                                                   # nothing can bind in this call (e.g. min_length below the prompt)
            assert R.same(want, case["x"])
            continue
        assert R.same(R.interpret(tb, 1, case["x"], case["history"], case["col"]), want), case["spec"]
        assert all(getattr(tb, k).dtype == np.int32 for k in ("grp_tok", "grp_ptr", "seq_ptr", "seq_ids", "ban_tok", "begin_tok", "eos_tok", "eos_first",
                                                               "forced_tok", "len0")) and tb.grp_base.dtype == tb.seq_bias.dtype == np.float32
        assert len(set(tb.grp_tok[:tb.n_bias].tolist())) == tb.n_bias and len(set(tb.grp_tok[tb.n_bias:].tolist())) == tb.grp_tok.size - tb.n_bias
        hash(tb.key)


def test_compiled_key_is_the_rule_sets_identity():
    a = LR.compile_rules(dict(suppress_tokens=[3]), 64, [2], [5, 6], 4)
    assert a.key == LR.compile_rules(dict(suppress_tokens=(3,), min_length=0), 64, 2, [5, 6], 4).key
    for other in (LR.compile_rules(dict(suppress_tokens=[4]), 64, [2], [5, 6], 4), LR.compile_rules(dict(suppress_tokens=[3]), 64, [1], [5, 6], 4),
                  LR.compile_rules(dict(suppress_tokens=[3]), 64, [2], [5, 7], 4), LR.compile_rules(dict(suppress_tokens=[3]), 64, [2], [5, 6], 5)):
        assert other.key != a.key


# ---- 3. host behaviour
BAD = [
    ("sequence_bias", 3.0), ("sequence_bias", [[[1, 2]]]), ("sequence_bias", [[[], 1.0]]), ("sequence_bias", [[[0, 2], 1.0]]), ("sequence_bias", [[[1, 2], 1]]),
    ("sequence_bias", [[[1, 2], float("-inf")]]), ("sequence_bias", [[[1, 2.5], 1.0]]), ("sequence_bias", {(1, -2): 1.0}), ("sequence_bias", {"a": 1.0}),
    ("sequence_bias", [[[1, 64], 1.0]]), ("sequence_bias", [[list(range(1, 34)), 1.0]]),
    ("bad_words_ids", [3]), ("bad_words_ids", [[]]), ("bad_words_ids", [[-1]]), ("bad_words_ids", [[1, 64]]), ("bad_words_ids", [[1.5]]),
    ("bad_words_ids", [list(range(33))]), ("bad_words_ids", [[i // 60 + 1, i % 60 + 1, 5] for i in range(1025)]),
    ("no_repeat_ngram_size", -1), ("no_repeat_ngram_size", 2.0), ("no_repeat_ngram_size", 17), ("min_length", -1), ("min_length", "3"),
    ("min_new_tokens", -2), ("min_new_tokens", 1.5), ("forced_eos_token_id", -1), ("forced_eos_token_id", [64]), ("forced_eos_token_id", 2.0),
    ("suppress_tokens", [64]), ("suppress_tokens", [-1]), ("suppress_tokens", 3), ("begin_suppress_tokens", [1.0]), ("begin_suppress_tokens", [70]),
    ("top_k", 5),
]


@pytest.mark.parametrize("key,value", BAD, ids=[f"{k}-{i}" for i, (k, _) in enumerate(BAD)])
def test_malformed_values_raise_value_error_naming_the_key(key, value):
    with pytest.raises(ValueError, match=key):
        LR.normalize({key: value}, 64)
    with pytest.raises(ValueError, match=key):
        LR.compile_rules({key: value}, 64, [2], [4], 4)


def test_limits_are_accepted_at_the_limit():
    spec = dict(bad_words_ids=[[i // 60 + 1, i % 60 + 1, 5] for i in range(1024)], no_repeat_ngram_size=16)
    tb = LR.compile_rules(spec, 64, [2], [4], 4)
    assert tb.seq_bias.size == 1024 and tb.ngram == 16
    assert LR.compile_rules(dict(sequence_bias=[[list(range(1, 33)), 1.0]]), 64, [2], [4], 4).seq_ptr.tolist() == [0, 31]


def test_all_off_spec_compiles_to_none():
    off = dict(sequence_bias=None, no_repeat_ngram_size=0, bad_words_ids=[], min_length=0, min_new_tokens=None, forced_eos_token_id=None,
               suppress_tokens=[], begin_suppress_tokens=None)
    assert LR.normalize(off, 64) == {} and LR.compile_rules(off, 64, [2], [4, 9], 6) is None
    assert LR.compile_rules(None, 64, [2], [4], 6) is None and LR.compile_rules({}, 64, [2], [4], 6) is None
    assert LR.compile_rules(dict(bad_words_ids=[[2]]), 64, [2], [4], 6) is None          # only [eos]: dropped
    assert LR.compile_rules(dict(min_length=4), 64, [2], [4, 9], 6) is None              # no row is below it
    assert LR.compile_rules(dict(min_length=5), 64, [], [4, 9], 6) is None               # no EOS id to ban
    assert LR.compile_rules(dict(min_length=5), 64, [2], [4, 9], 6).eos_first.tolist() == [1, 0]
    assert LR.merge(dict(min_length=3, suppress_tokens=[1]), dict(min_length=None, suppress_tokens=[2])) == dict(min_length=3, suppress_tokens=[2])


ON = dict(sequence_bias=[[[5], 2.0]], no_repeat_ngram_size=3, bad_words_ids=[[7, 8]], min_length=4, min_new_tokens=2, forced_eos_token_id=2,
          suppress_tokens=[9], begin_suppress_tokens=[10])


@pytest.mark.parametrize("key", R.KEYS)
def test_generation_config_refuses_each_key_unless_asked(key):
    from internnav_amd.policy import generation_config_from_hf

    with pytest.raises(NotImplementedError, match=key):
        generation_config_from_hf({key: ON[key]}, 2)
    cfg = generation_config_from_hf({key: ON[key], "repetition_penalty": 1.1}, 2, rules_from_file=True)
    assert cfg.rules == {key: ON[key]} and cfg.repetition_penalty == 1.1
    assert generation_config_from_hf({"repetition_penalty": 1.1}, 2).rules == {}
    for other in ("encoder_repetition_penalty", "forced_bos_token_id", "renormalize_logits", "penalty_alpha"):      # stay refused
        with pytest.raises(NotImplementedError, match=other):
            generation_config_from_hf({key: ON[key], other: 2.0}, 2, rules_from_file=True)


def test_beams_plus_rules_raise_not_implemented():
    from internnav_amd.policy import InternVLAN1ForCausalLM
    from internnav_amd.qwen_vl import QwenVLEngine

    tb = LR.compile_rules(dict(suppress_tokens=[3]), 64, [2], [5], 4)
    with pytest.raises(NotImplementedError, match="beam"):      # raised before the engine is touched: no engine needed
        QwenVLEngine.prefill(None, None, None, None, beam=dict(K=2), logit_rules=tb)
    model = object.__new__(InternVLAN1ForCausalLM)
    model.generation_rules, model.qwen = {}, type("Q", (), {"cfg": {"vocab": 64}})()
    with pytest.raises(NotImplementedError, match="suppress_tokens"):
        model.generate(input_ids=torch.zeros(1, 4, dtype=torch.long), num_beams=2, suppress_tokens=[3])
    model.generation_rules = LR.normalize(dict(min_new_tokens=1), 64)
    with pytest.raises(NotImplementedError, match="min_new_tokens"):
        model.generate(input_ids=torch.zeros(1, 4, dtype=torch.long), num_beams=2)
