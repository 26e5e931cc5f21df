"""CPU: the repetition penalty of System-2 greedy decoding without a GPU - the fp32 restatement (tests/decode_penalty_ref.py) against
transformers' RepetitionPenaltyLogitsProcessor bit for bit, the reading of a checkpoint's generation_config.json, and the two C-ABI
entries (exported, declared, every refusal returned before any HIP call)."""
import ctypes as C
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import decode_penalty_ref as R

ROOT = Path(__file__).resolve().parent.parent
N = 152064


# ---------------------------------------------------------------------------------------------------- restatement == transformers
def test_restatement_equals_transformers_processor_bit_for_bit():
    tr = pytest.importorskip("transformers")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, N, generator=g) * 6.0
    ids = torch.randint(0, N, (3, 900), generator=g)
    ids[:, 100:140] = ids[:, :40]                                   # duplicates
    for p in (1.05, 1.3, 2.0):
        want = tr.RepetitionPenaltyLogitsProcessor(penalty=p)(ids, x.clone()).numpy()
        got = R.penalised(x.numpy(), R.seen_bitmap(ids.numpy(), [900] * 3, N), p)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), p
        assert np.array_equal(R.argmax_first(got), torch.argmax(torch.from_numpy(want), dim=-1).numpy())


def test_greedy_loop_sees_prompt_and_answer_like_transformers():
    tr = pytest.importorskip("transformers")
    n, p = 4096, 1.5
    g = torch.Generator().manual_seed(1)
    rows = torch.randn(4, n, generator=g)
    prompt = torch.randint(0, n, (40,), generator=g).tolist()
    # the raw maximum of steps 1 .. 3 is the token step 0 chose (inside the factor of the runner-up): the answer so far must be penalised too
    proc = tr.RepetitionPenaltyLogitsProcessor(penalty=p)
    first = int(torch.argmax(proc(torch.tensor([prompt]), rows[:1].clone())[0]))
    for s in range(1, 4):
        rows[s, first] = rows[s].max() * 1.2
    toks, want = list(prompt), []
    for s in range(4):
        y = proc(torch.tensor([toks]), rows[s:s + 1].clone())[0]
        want.append(int(torch.argmax(y)))
        toks.append(want[-1])
    got = R.greedy_with_penalty(lambda s, _t: rows[s].numpy(), prompt, 4, p)
    assert got == want
    assert got != R.greedy_with_penalty(lambda s, _t: rows[s].numpy(), prompt, 4, 1.0)     # the penalty moved a choice
    assert len(set(got)) > 1


def test_restatement_selection_rule_edges():
    x = np.array([[np.nan, -np.inf, 3.0, 3.0], [np.nan, np.nan, -np.inf, -np.inf]], dtype=np.float32)
    assert R.argmax_first(x).tolist() == [2, 0]
    bm = R.seen_bitmap([[0, 31, 32, 40, -1, 99]], [6], 40)          # 40 and 99 are outside [0, 40): ignored
    assert bm.shape == (1, 2) and bm[0].tolist() == [0x80000001, 1]
    y = R.penalised(np.array([4.0, -4.0, -0.0], dtype=np.float32), np.array([0b111], dtype=np.uint32), 2.0)
    assert y.tolist() == [2.0, -8.0, 0.0] and math.copysign(1.0, float(y[2])) == -1.0


# ---------------------------------------------------------------------------------------------------- generation_config.json
REFUSED = dict(no_repeat_ngram_size=3, encoder_repetition_penalty=1.2, bad_words_ids=[[5]], suppress_tokens=[7], begin_suppress_tokens=[7],
               forced_bos_token_id=1, forced_eos_token_id=2, min_length=4, min_new_tokens=2, sequence_bias=[[[5], 1.0]], num_beams=4,
               penalty_alpha=0.6, exponential_decay_length_penalty=[4, 1.1], renormalize_logits=True)


def test_generation_config_parsing():
    from internnav_amd.policy import generation_config_from_hf as G

    none = G(None, 4005)
    assert none.repetition_penalty == 1.0 and none.eos_token_id == (4005,) and none.raw == {}
    both = G({"repetition_penalty": 1.05, "eos_token_id": [151645, 151643]}, 4005)
    assert both.repetition_penalty == 1.05 and both.eos_token_id == (151645, 151643) and both.raw["repetition_penalty"] == 1.05
    assert G({"eos_token_id": 7}, 4005).eos_token_id == (7,) and G({"repetition_penalty": 1.2}, [3, 4]).eos_token_id == (3, 4)
    # sampling-only keys are ignored (every caller passes do_sample=False), and so are the refused keys at their neutral values
    samp = G({"do_sample": True, "temperature": 0.1, "top_k": 1, "top_p": 0.001, "min_p": 0.2, "typical_p": 0.5, "repetition_penalty": 1.05,
              "no_repeat_ngram_size": 0, "num_beams": 1, "min_length": 0, "encoder_repetition_penalty": 1.0, "bad_words_ids": None}, 1)
    assert samp.repetition_penalty == 1.05
    for bad in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError):
            G({"repetition_penalty": bad}, 1)


@pytest.mark.parametrize("key", sorted(REFUSED))
def test_unimplemented_generation_keys_are_refused_by_name(key):
    from internnav_amd.policy import generation_config_from_hf as G

    with pytest.raises(NotImplementedError, match=key):
        G({"repetition_penalty": 1.05, key: REFUSED[key]}, 1)
    ok = G({"repetition_penalty": 1.05, key: REFUSED[key]}, 1, ignore=True)      # model_settings['ignore_generation_config']
    assert ok.repetition_penalty == 1.05


def test_from_pretrained_reads_the_file_before_any_weight(tmp_path, monkeypatch):
    """from_pretrained refuses a generation_config.json it cannot honour at load; write_checkpoint writes the file only when asked"""
    from internnav_amd import policy, synthetic

    seen = {}

    class Stop(Exception):
        pass

    def fake_init(self, weights, cfg, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(policy.InternVLAN1ForCausalLM, "__init__", fake_init)
    synthetic.write_checkpoint(tmp_path / "a", synthetic.QWEN_TEST_CFG, "nextdit_async", seed=1)
    assert not (tmp_path / "a" / "generation_config.json").exists()
    with pytest.raises(Stop):
        policy.InternVLAN1ForCausalLM.from_pretrained(tmp_path / "a")
    assert seen["generation_config"] is None
    (tmp_path / "a" / "generation_config.json").write_text(json.dumps({"repetition_penalty": 1.3, "eos_token_id": [4005, 4006]}))
    with pytest.raises(Stop):
        policy.InternVLAN1ForCausalLM.from_pretrained(tmp_path / "a")
    assert seen["generation_config"] == {"repetition_penalty": 1.3, "eos_token_id": [4005, 4006]}
    (tmp_path / "a" / "generation_config.json").write_text(json.dumps({"repetition_penalty": 1.3, "no_repeat_ngram_size": 2}))
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):
        policy.InternVLAN1ForCausalLM.from_pretrained(tmp_path / "a")
    with pytest.raises(Stop):
        policy.InternVLAN1ForCausalLM.from_pretrained(tmp_path / "a", ignore_generation_config=True)


def test_write_checkpoint_writes_generation_config_on_request(tmp_path):
    from internnav_amd import synthetic

    gc = {"repetition_penalty": 1.3, "eos_token_id": [4005, 4006]}
    synthetic.write_checkpoint(tmp_path / "b", synthetic.QWEN_TEST_CFG, "nextdit_async", seed=1, generation_config=gc)
    assert json.loads((tmp_path / "b" / "generation_config.json").read_text()) == gc


def test_engine_plan_uploads_ids_only_with_a_penalty():
    """penalty 1.0 (and no argument) leaves the plan exactly as it was: no ids, no lengths, no penalty entry"""
    from internnav_amd import synthetic as S
    from internnav_amd.qwen_vl import QwenVLEngine, eos_ids

    cfg = S.QWEN_TEST_CFG
    eng = QwenVLEngine(S.qwen_state_dict(seed=1, cfg=cfg), cfg, "cpu", max_seqs=2, max_seq_len=512, max_patches=2 * 784, frag_weights=False)
    assert eng.seen.dtype == torch.uint32 and tuple(eng.seen.shape) == (2, 128) and eng.seen.shape[1] % 4 == 0
    inp = S.qwen_inputs(2, 1, seed=3, cfg=cfg)
    a = eng.plan(inp["input_ids"], inp["grid_thw"], n_decode=2)
    b = eng.plan(inp["input_ids"], inp["grid_thw"], n_decode=2, repetition_penalty=1.0)
    assert set(a) == set(b) and not any(k.startswith("rep_") for k in a)
    c = eng.plan(inp["input_ids"], inp["grid_thw"], repetition_penalty=1.05, seq_lens=[inp["input_ids"].shape[1], 200], prefix_len=[0, 0])
    assert c["rep_penalty"] == 1.05 and c["rep_ids"].dtype == torch.int32 and torch.equal(c["rep_ids"].long(), inp["input_ids"])
    assert c["rep_lens"].tolist() == [inp["input_ids"].shape[1], 200]
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError):
            eng.plan(inp["input_ids"], inp["grid_thw"], repetition_penalty=bad)
    assert eos_ids(5) == (5,) and eos_ids([5, 6]) == (5, 6)


# ---------------------------------------------------------------------------------------------------- C-ABI
def test_abi_entries_are_declared_and_exported(built_lib):
    from internnav_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "internnav_amd.h").read_text(), flags=re.S)
    h = C.CDLL(str(built_lib))
    for name in ("ina_token_seen_set", "ina_argmax_penalty_rows"):
        assert re.search(rf"^int {name}\(", text, flags=re.M) and name in _lib.SYMBOLS and hasattr(h, name)
    assert _lib.lib().ina_abi_version() == 8


def test_abi_refusals_return_before_any_hip_call(built_lib):
    from internnav_amd import _lib

    lib = _lib.lib()
    buf = (C.c_uint32 * 64)()
    p = C.addressof(buf)                                             # never dereferenced: every call below is refused on its arguments
    nan, inf = float("nan"), float("inf")

    def amax(X=p, ldx=64, rows=1, n=64, seen=p, ld_words=2, penalty=1.05, mark=1, out=p):
        return lib.ina_argmax_penalty_rows(X, ldx, rows, n, seen, ld_words, penalty, mark, out, None)

    for kw in (dict(X=None), dict(seen=None), dict(out=None), dict(rows=0), dict(rows=-1), dict(n=0), dict(n=-5), dict(ld_words=1), dict(n=65),
               dict(penalty=0.0), dict(penalty=-1.0), dict(penalty=nan), dict(penalty=inf), dict(penalty=-inf)):
        assert amax(**kw) != 0, kw
        assert b"argmax_penalty_rows" in lib.ina_last_error()

    def sset(seen=p, ld_words=2, ids=p, ld_ids=8, lens=p, rows=1, n=64):
        return lib.ina_token_seen_set(seen, ld_words, ids, ld_ids, lens, rows, n, None)

    for kw in (dict(seen=None), dict(ids=None), dict(lens=None), dict(rows=0), dict(n=0), dict(ld_words=1), dict(n=262145, ld_words=8193)):
        assert sset(**kw) != 0, kw
        assert b"token_seen_set" in lib.ina_last_error()
    assert b"LDS" in lib.ina_last_error()                           # the last refusal: a vocabulary beyond the LDS bitmap


# ---------------------------------------------------------------------------------------------------- agent paths
def test_model_settings_penalty_reaches_generate_on_both_agent_paths():
    """model_settings['repetition_penalty'] is carried by every env's policy: the batched agent call and a policy's own s2_step pass it to
    generate(); without the setting neither passes the argument (generate() then uses the checkpoint's value)"""
    from test_host_logic import _FakeModel, _FakeProcessor

    from internnav_amd.agent import InternVLAN1Agent

    class Model(_FakeModel):
        def generate(self, **kw):
            self.kw = dict(kw)
            return super().generate(**kw)

    rgb, dep = np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 1), np.float32)
    obs = [{"rgb": rgb, "depth": dep, "instruction": "go to the door"}, {"rgb": rgb, "depth": dep, "instruction": "go to the wall"}]
    for setting, want in (({"repetition_penalty": 1.07}, 1.07), ({}, None)):
        model = Model(["↑", "←", "→"])
        ag = InternVLAN1Agent({"model_settings": dict(infer_mode="partial_async", **setting)}, model=model, processor=_FakeProcessor())
        ag.reset()
        out = ag.step(obs)
        assert [o["action"] for o in out] == [[1], [2]] and model.batches == [(2, model.batches[0][1])]
        assert model.kw.get("repetition_penalty") == want and ("repetition_penalty" in model.kw) == (want is not None)
        assert [e.policy.repetition_penalty for e in ag.envs] == [want, want]              # spawn() hands it on
        pol = ag.envs[1].policy
        pol.s2_step(rgb, dep, None, "go to the wall", None)                                # the per-env path
        assert model.batches[-1][0] == 1 and model.kw.get("repetition_penalty") == want
        assert ("repetition_penalty" in model.kw) == (want is not None)
