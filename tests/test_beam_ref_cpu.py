"""CPU: the restatement of the beam-search rules (tests/beam_ref.py) against transformers' generate(num_beams=K) on a tiny random Qwen2, the
ordering conventions of its top-M selection, and the host side of generate(num_beams=K): `beam_spec`'s resolutions and refusals. No GPU is needed."""
import math

import numpy as np
import pytest
import torch

import beam_ref as R

VOCAB = 97
# (num_beams, length_penalty, early_stopping, repetition_penalty, number of EOS ids)
SETTINGS = [(2, 1.0, False, 1.0, 1), (3, 0.0, True, 1.05, 2), (4, 2.0, "never", 1.3, 3), (5, 1.0, "never", 1.0, 57), (4, 1.0, True, 1.3, 10)]
SEEDS = list(range(12))
MAX_NEW = 6
_models = {}


def _model(seed: int):
    tr = pytest.importorskip("transformers")
    if seed not in _models:
        torch.manual_seed(seed)
        cfg = tr.Qwen2Config(vocab_size=VOCAB, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                             num_key_value_heads=2, max_position_embeddings=64, tie_word_embeddings=False)
        m = tr.Qwen2ForCausalLM(cfg).eval().float()
        with torch.no_grad():
            m.lm_head.weight.mul_(40.0)                      # peaked distributions, as a System-2 answer's are
        _models[seed] = m
    return _models[seed]


@pytest.mark.parametrize("setting", range(len(SETTINGS)))
@pytest.mark.parametrize("seed", SEEDS)
def test_restatement_equals_transformers_beam_search(seed, setting):
    """Sequences equal, scores within 1e-3 relative, and every decision margin of the reference above 1e-4. A decision margin is a gap whose
    sign can change the result: the order of the first K candidates and the gap behind the K-th, the running selection and the finished
    merge (their picks and the best entry left out), the gap behind the last candidate when that candidate runs on, and the heuristic's
    comparisons. Excluded, because no margin decides them: comparisons with an empty, blocked or -inf entry (-1e9 sentinels: HF's order by
    construction) and the order among candidates K .. M - 1 where it reaches no selection - with 57 EOS ids M is 290 of 485 entries, whose
    deep neighbours lie closer than 1e-4 without any effect on either set (`BeamPrompt._gap`)."""
    K, lp, early, pen, n_eos = SETTINGS[setting]
    m = _model(seed)
    g = np.random.default_rng(1000 * seed + setting)
    prompt = g.integers(0, VOCAB, size=int(g.integers(4, 8))).tolist()
    eos = sorted(g.choice(VOCAB, size=n_eos, replace=False).tolist())
    ids = torch.tensor([prompt])
    with torch.no_grad():
        hf = m.generate(ids, num_beams=K, num_return_sequences=K, length_penalty=lp, early_stopping=early, repetition_penalty=pen,
                        eos_token_id=eos, pad_token_id=eos[0], max_new_tokens=MAX_NEW, do_sample=False, return_dict_in_generate=True,
                        output_scores=True)

    def logits_fn(answers):
        with torch.no_grad():
            x = torch.tensor([prompt + [int(t) for t in a] for a in answers])
            return m(x).logits[:, -1].double().numpy()

    bp = R.beam_search(logits_fn, prompt, K, eos, MAX_NEW, lp, early, pen)
    assert bp.margin > 1e-4, f"a decision of the reference rests on a gap of {bp.margin:.3e}"
    res = bp.results(K)
    seqs = hf.sequences[:, len(prompt):].numpy()
    for k, (toks, score, L, valid, ts) in enumerate(res):
        assert valid
        row = np.full(max(seqs.shape[1], L), eos[0])
        row[:L] = toks
        assert np.array_equal(row[: seqs.shape[1]], seqs[k]) and bool((row[seqs.shape[1]:] == eos[0]).all()), (k, row, seqs[k])
        want = float(hf.sequences_scores[k])
        assert abs(score - want) <= 1e-3 * max(abs(want), 1e-30), (k, score, want)
        # the transition scores of a hypothesis add up to its score
        assert abs(float(ts.astype(np.float64).sum()) / float(L) ** lp - score) <= 1e-4 * max(1.0, abs(score))


def test_topm_order_is_value_descending_then_id_ascending():
    x = np.zeros((2, 9), dtype=np.float32)
    x[0, [7, 2, 5]] = 3.0
    x[0, 4] = np.nan                                           # counts as -inf: behind every number
    x[1] = -np.inf                                             # a row without a number: every y = -inf, ids in order
    cs, ct, _ = R.topm_rows(x, np.array([0.0, -1e9]), 5)
    assert ct[0].tolist() == [2, 5, 7, 0, 1] and cs[0, 0] == cs[0, 2] > cs[0, 3] == cs[0, 4]
    assert ct[1].tolist() == [0, 1, 2, 3, 4] and bool(np.isneginf(cs[1]).all())
    cs, ct, _ = R.topm_rows(x, np.array([0.0]), 3, src=[5])    # a src outside the logits rows: never read
    assert ct[0].tolist() == [0, 1, 2] and bool(np.isneginf(cs[0]).all())
    assert R.cand_bound(np.random.default_rng(0).standard_normal(152064).astype(np.float32) * 4, 3, 0.0) < 2e-4


def test_done_prompt_is_frozen_and_step0_reads_row0_only():
    bp = R.BeamPrompt(2, [1], 3)
    cs = np.array([[-0.1, -2.5, -3.0, -4.0], [5.0, 4.0, 3.0, 2.0]], dtype=np.float32)      # row 1 would win: it does not take part in step 0
    ct = np.array([[1, 7, 8, 9], [3, 4, 5, 6]])
    bp.step(cs, ct)
    assert bp.next_tok.tolist() == [7, 8] and bp.parent.tolist() == [0, 0] and bool(bp.fin_flag[0]) and not bool(bp.fin_flag[1])
    assert bp.fin_score[0] == np.float32(-0.1) and bp.fin_len[0] == 1 and not bp.done
    # both of the first K hit EOS far below the finished one: the set fills, the best running beam can no longer improve on its worst -> done
    cs = np.array([[-2.6, -2.7, -9.0, -9.5], [-3.1, -3.2, -9.6, -9.7]], dtype=np.float32)
    bp.step(cs, np.array([[1, 1, 4, 5], [6, 7, 8, 9]]))
    snap = (bp.fin_score.copy(), bp.fin_tok.copy(), bp.run_score.copy(), bp.done)
    assert bp.done and not bp.flag and bool(bp.fin_flag.all()) and bp.fin_tok[1, :2].tolist() == [7, 1]
    bp.step(cs, ct)
    assert np.array_equal(snap[0], bp.fin_score) and np.array_equal(snap[1], bp.fin_tok) and np.array_equal(snap[2], bp.run_score)


def test_generate_resolves_num_beams_on_the_host():
    """the seam generate(num_beams=K) goes through: absent before the beam path existed, when num_beams vanished in **kw and decoding was greedy"""
    from internnav_amd import policy

    assert policy.beam_spec(None) is None and policy.beam_spec(1, num_return_sequences=1) is None
    s = policy.beam_spec(4)
    assert (s.K, s.n, s.length_penalty, s.early_stopping) == (4, 1, 1.0, False)
    s = policy.beam_spec(4, num_return_sequences=3, length_penalty=0, early_stopping="never", share_prefix=True)
    assert (s.K, s.n, s.length_penalty, s.early_stopping) == (4, 3, 0.0, "never")
    import inspect
    assert "num_beams" in inspect.signature(policy.InternVLAN1ForCausalLM.generate).parameters


@pytest.mark.parametrize("kw,exc", [
    (dict(num_beams=0), ValueError), (dict(num_beams=3, num_return_sequences=4), ValueError), (dict(num_beams=3, num_return_sequences=0), ValueError),
    (dict(num_beams=3, length_penalty=float("nan")), ValueError), (dict(num_beams=3, length_penalty=float("inf")), ValueError),
    (dict(num_beams=3, early_stopping="always"), ValueError), (dict(num_beams=3, early_stopping=1), ValueError),
    (dict(num_beams=3, share_prefix=False), ValueError),
    (dict(num_beams=3, do_sample=True), NotImplementedError), (dict(num_beams=4, extra={"num_beam_groups": 2}), NotImplementedError),
    (dict(num_beams=4, extra={"diversity_penalty": 0.5}), NotImplementedError), (dict(num_beams=4, extra={"constraints": [object()]}), NotImplementedError),
    (dict(num_beams=4, extra={"force_words_ids": [[1]]}), NotImplementedError)])
def test_beam_spec_refusals(kw, exc):
    from internnav_amd import policy

    with pytest.raises(exc) as e:
        policy.beam_spec(**kw)
    if exc is NotImplementedError and "extra" in kw:
        assert next(iter(kw["extra"])) in str(e.value)
    assert policy.beam_spec(4, extra={"num_beam_groups": 1, "diversity_penalty": 0.0, "constraints": None}) is not None
    assert math.isfinite(policy.beam_spec(2, length_penalty=-1.5).length_penalty)


def test_file_num_beams_stays_refused_at_load():
    from internnav_amd.policy import generation_config_from_hf as G

    with pytest.raises(NotImplementedError):
        G({"num_beams": 4}, 2)
