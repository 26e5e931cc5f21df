"""The launch sequence of the System-2 engine, pinned: every path through QwenVLEngine's plan / prefill / decode / latent entry points is run
on a CPU engine of a reduced geometry with every launching function of `internnav_amd.ops` replaced by a recorder that computes nothing,
and the recorded calls are compared with tests/golden/s2_launch_trace.json.

A recorded call holds the op's name and its arguments: every tensor (nested in tuples, dicts or namespaces) as dtype, shape, strides and
the engine buffer it aliases with the element offset into it; every scalar by value. A tensor that aliases no engine buffer is "other"; if
it is int32 with at most 256 elements its values are recorded as well - these are the host-built tables (pos, rows, kv_dst, tile_*, slot,
pfx_len ...). The engine's own buffers hold nothing defined here (no op computes), so their values are never recorded; neither are the
addresses inside int64 tables. Steps the engine takes in torch itself (fills and copies of automaton states, histories, beam start scores,
the tokens_out copies) are not recorded: the GPU graph-replay tests cover them.

The fixture describes what the engine launched when the fixture was made. It changes only together with a change of the launch sequence
that is meant; a refactor leaves it alone. `python tests/test_s2_launch_trace_cpu.py --write` regenerates it."""
import inspect
import json
import pathlib
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "s2_launch_trace.json"
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from internnav_amd import ops, synthetic  # noqa: E402
from internnav_amd.constrain import TokenAutomaton  # noqa: E402
from internnav_amd.logit_rules import compile_rules  # noqa: E402
from internnav_amd.qwen_vl import QwenVLEngine  # noqa: E402

# head dim 128 (the m-rope section table), everything else as small as the code paths allow
CFG = dict(synthetic.QWEN_TEST_CFG, t_hidden=256, t_heads=2, t_kv_heads=1, t_inter=64, t_layers=2, v_hidden=128, v_heads=2, v_inter=64, v_depth=1,
           v_fullatt=(0,), v_out=256, vocab=96, image_token_id=88, traj_token_id=89, vision_start_id=90, vision_end_id=91, eos_token_id=92)
EOS = (92,)
B, S = 2, 10             # 20 prefill rows: the prefill runs unfused, the single-token passes fused
PASS_THROUGH = ("attention_shared_plan", "attention_rope_ok", "shared_tail")     # host helpers: they launch nothing


# ---------------------------------------------------------------------------------------------------- recorder
def _engine_buffers(eng):
    """(name, tensor) of everything the engine allocates for activations and selection state, in a fixed order (the first match names an alias)"""
    out = [(n, getattr(eng, n)) for n in eng._BUFFERS]
    out += [(f"layers[{i}].kv", L["kv"]) for i, L in enumerate(eng.layers)]
    out += [(n, getattr(eng, n)) for n in ("_cstate", "_rhist", "_smp_lp", "_lp_steps", "_mg_steps")]

    def members(prefix, v):
        if isinstance(v, torch.Tensor):
            out.append((prefix, v))
        elif isinstance(v, (list, tuple)):
            for i, e in enumerate(v):
                members(f"{prefix}[{i}]", e)

    for owner in ("_shared", "_beam"):
        ns = getattr(eng, owner)
        for k, v in sorted(vars(ns).items()) if ns is not None else ():
            members(f"{owner}.{k}", v)
    return [(n, t) for n, t in out if t is not None and t.numel()]


def _alias(t, eng):
    if t.numel():
        p = t.data_ptr()
        for name, b in _engine_buffers(eng):
            lo = b.data_ptr()
            if lo <= p < lo + b.numel() * b.element_size():
                return name, (p - lo) // t.element_size()
    return "other", int(t.storage_offset())


def _describe(v, eng):
    if isinstance(v, torch.Tensor):
        name, off = _alias(v, eng)
        d = [str(v.dtype).replace("torch.", ""), list(v.shape), list(v.stride()), name, int(off)]
        if name == "other" and v.dtype == torch.int32 and v.numel() <= 256:
            d.append(v.reshape(-1).tolist())
        return {"t": d}
    if isinstance(v, SimpleNamespace):
        return {"ns": {k: _describe(e, eng) for k, e in sorted(vars(v).items()) if not callable(e) and not k.startswith("_")}}
    if isinstance(v, dict):
        return {"d": {str(k): _describe(e, eng) for k, e in v.items()}}
    if isinstance(v, (list, tuple)):
        return [_describe(e, eng) for e in v]
    if isinstance(v, np.ndarray):
        return {"np": v.tolist()}
    if isinstance(v, np.generic):
        return v.item()
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


class Recorder:
    """replaces every public function of `ops` but the host helpers; `engine` is the engine whose buffers name the aliases"""

    def __init__(self, monkeypatch):
        self.calls, self.engine = [], None
        for name, fn in list(vars(ops).items()):
            if inspect.isfunction(fn) and fn.__module__ == ops.__name__ and not name.startswith("_") and name not in PASS_THROUGH:
                monkeypatch.setattr(ops, name, self._stub(name))

    def _stub(self, name):
        def record(*args, **kw):
            self.calls.append([name, [_describe(a, self.engine) for a in args], {k: _describe(v, self.engine) for k, v in kw.items()}])

        return record

    def take(self):
        out, self.calls = self.calls, []
        return out


# ---------------------------------------------------------------------------------------------------- scenarios
def _engine(weights, **kw):
    return QwenVLEngine(weights, CFG, device="cpu", max_seqs=4, max_seq_len=32, max_patches=64, max_decode=8, frag_weights=False, **kw)


def _ids():
    g = torch.Generator().manual_seed(7)
    return torch.randint(0, 80, (B, S), generator=g)


def _automaton():
    return TokenAutomaton.from_token_sequences([[5, 6, 7], [5, 8]], EOS, CFG["vocab"])


def _rules(max_new_tokens, lens=(S, S)):
    return compile_rules(dict(no_repeat_ngram_size=2, bad_words_ids=[[3], [4, 9]], min_new_tokens=2, sequence_bias={(11,): 1.5, (12, 13): -2.0}),
                         CFG["vocab"], EOS, list(lens), max_new_tokens)


def planned_greedy(weights, rec):
    rec.engine = eng = _engine(weights)
    P = eng.plan(_ids(), None, n_decode=3, with_latents=True)
    eng.run_s2(P, None, torch.empty(B, 3, dtype=torch.int32), torch.empty(B, 4, eng.H, dtype=torch.bfloat16))
    plain = rec.take()
    rec.engine = eng = _engine(weights, token_logprobs=True)
    P = eng.plan(_ids(), None, n_decode=3, with_latents=True, repetition_penalty=1.1, constraint=_automaton(), logit_rules=_rules(3))
    toks = torch.empty(B, 3, dtype=torch.int32)
    eng.run_prefill(P, None)
    eng.run_decode(P, toks, 0, 2)
    eng.run_decode(P, toks, 2, None)
    eng.run_latents(P, torch.empty(B, 4, eng.H, dtype=torch.bfloat16))
    return {"plain": plain, "logprobs_penalty_constraint_rules": rec.take()}


def eager_ragged_greedy(weights, rec):
    rec.engine = eng = _engine(weights)
    st = eng.prefill(_ids(), None, None, seq_lens=[10, 7])
    eng.decode(st, 3)
    eng.decode(st, 2)
    eng.latents(st, torch.tensor([[5], [6]], dtype=torch.int32))      # (the decoded tokens are undefined here: no op computes)
    return {"calls": rec.take()}


def _sampled(weights, rec, share):
    rec.engine = eng = _engine(weights)
    spec = dict(temperature=0.8, top_k=5, top_p=0.9, K=2, u=torch.full((5, B * 2), 0.5))
    if share:
        spec["share_prefix"] = True
    st = eng.prefill(_ids(), None, None, repetition_penalty=1.1, sampling=spec, constraint=_automaton(), logit_rules=_rules(5))
    eng.decode(st, 3)
    eng.decode(st, 2)
    eng.latents_behind(st, [1, 2], [5, 6], [11, 12])
    eng.last_sample_logprobs(st)
    return {"calls": rec.take()}


def sampling_fan_out(weights, rec):
    return _sampled(weights, rec, False)


def sampling_shared_prefix(weights, rec):
    return _sampled(weights, rec, True)


def beam_search(weights, rec):
    rec.engine = eng = _engine(weights)
    st = eng.prefill(_ids(), None, None, repetition_penalty=1.1, constraint=_automaton(), beam=dict(K=2, max_new_tokens=5, eos=EOS))
    eng.decode(st, 3)
    eng.decode(st, 2)
    eng.beam_results(st)
    eng.latents_after(st, [0, 1], [[5, 6, 7, 92], [5, 8]])
    return {"calls": rec.take()}


def suffix_pass(weights, rec):
    rec.engine = eng = _engine(weights)
    st = eng.prefill(_ids(), None, None)
    eng.suffix_pass(st, [0, 1, 1], [[5, 6, 7], [5, 8, 0], [9, 0, 0]], [3, 2, 1])
    return {"calls": rec.take()}


def images_and_prefixes(weights, rec):
    inp = synthetic.qwen_inputs(2, 2, cfg=CFG, grid=(1, 4, 4), n_text=3, n_tail=2)
    ids, grid, pv = inp["input_ids"], inp["grid_thw"], inp["pixel_values"].to(torch.bfloat16).view(4, 16, -1)
    p = 3 + 1 + 4 + 1                                             # text, <vision_start>, 4 merged tokens, <vision_end>: the first image's boundary
    rec.engine = eng = _engine(weights)
    eng.split_prefill = False                                     # (the side stream needs a device)
    P = eng.plan(ids, grid, prefix_len=p)
    assert eng.images_in_prefix(ids, grid, p) == [True, False, True, False]
    eng.run_prefill(P, pv[[1, 3]].reshape(32, -1))
    planned = rec.take()
    st = eng.prefill(ids, pv[[1, 2, 3]].reshape(48, -1), grid, prefix_len=[p, 0], repetition_penalty=1.1)      # (greedy + penalty: argmax_penalty_rows)
    eng.decode(st, 2)
    return {"planned_uniform_prefix": planned, "eager_ragged_prefix": rec.take()}


SCENARIOS = (planned_greedy, eager_ragged_greedy, sampling_fan_out, sampling_shared_prefix, beam_search, suffix_pass, images_and_prefixes)


def _trace(scenario, weights, monkeypatch):
    return json.loads(json.dumps(scenario(weights, Recorder(monkeypatch))))


@pytest.fixture(scope="module")
def weights():
    return synthetic.qwen_state_dict(seed=1, cfg=CFG)


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__)
def test_launch_sequence_is_the_recorded_one(scenario, weights, golden, monkeypatch):
    got, want = _trace(scenario, weights, monkeypatch), golden[scenario.__name__]
    assert set(got) == set(want)
    for part in want:
        assert [c[0] for c in got[part]] == [c[0] for c in want[part]], f"{scenario.__name__}/{part}: another sequence of ops"
        for i, (g, w) in enumerate(zip(got[part], want[part])):
            assert g == w, f"{scenario.__name__}/{part}: call {i} ({w[0]}) differs"


def test_the_fixture_covers_every_selection_kernel_and_pass(golden):
    """the scenarios reach what they are there for: every pick, both masks' users, every attention variant"""
    names = {c[0] for sc in golden.values() for part in sc.values() for c in part}
    assert {"argmax_rows", "argmax_penalty_rows", "logprob_rows", "sample_rows", "beam_topm_rows", "beam_step", "beam_reorder", "automaton_mask_rows",
            "logit_rules_rows", "token_seen_set", "kv_copy", "attention", "attention_prefix", "attention_prefix_tail", "attention_shared",
            "gather_rows", "norm", "linear", "rope", "mrope_table"} <= names
    assert sum(len(part) for sc in golden.values() for part in sc.values()) > 400


if __name__ == "__main__":
    assert sys.argv[1:] == ["--write"], "usage: test_s2_launch_trace_cpu.py --write"
    w, out = synthetic.qwen_state_dict(seed=1, cfg=CFG), {}
    for sc in SCENARIOS:
        with pytest.MonkeyPatch.context() as mp:
            out[sc.__name__] = _trace(sc, w, mp)
    lines = []
    for name, parts in out.items():
        body = ",\n".join(f"{json.dumps(k)}: [\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in calls) + "\n]" for k, calls in parts.items())
        lines.append(f"{json.dumps(name)}: {{\n{body}\n}}")
    GOLDEN.write_text("{\n" + ",\n".join(lines) + "\n}\n")
    print({k: {p: len(c) for p, c in v.items()} for k, v in out.items()})
