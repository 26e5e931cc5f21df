"""CPU: the float64 restatement of ops.attention_prefix (tests/attn_prefix_ref.py) against torch SDPA on the per-pair concatenation, the host
plan of score_answers(share_prefix=True) against a brute-force model, the refusals of the C-ABI entry (dummy pointers: every call is refused or
has nothing to do) and the candidate-length limit of the public call. No GPU is needed."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_prefix_ref as R

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_reference_equals_sdpa_on_the_concatenation_and_ignores_the_poison(case):
    c = R.make_case(case)
    q, k, v, kc, vc = (t.double().numpy() for t in R.views(c["fused"], c["cache"], c["H"], c["Hkv"], c["m"]))
    slot, pfx, suf = c["slot"].numpy(), c["pfx_len"].numpy(), c["suf_len"].numpy()
    assert np.isnan(c["cache"].float().numpy()).any() and (np.isnan(c["fused"].float().numpy()).any() or bool((suf == c["m"]).all()))
    ref = R.attention_prefix_ref(q, k, v, kc, vc, slot, pfx, suf)
    assert np.isfinite(ref).all(), "the reference read a poisoned row"
    want = R.sdpa_ref(q, k, v, kc, vc, slot, pfx, suf)
    assert np.isfinite(want).all()
    assert np.abs(ref - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    for p in range(c["P"]):
        assert not ref[p, suf[p]:].any()                                    # rows behind suf_len: zeros
    # max_pfx clips pfx_len; a slot outside the cache gives NaN in the pair's live rows only
    clip = R.attention_prefix_ref(q, k, v, kc, vc, slot, pfx, suf, max_pfx=1)
    assert np.array_equal(clip, R.attention_prefix_ref(q, k, v, kc, vc, slot, np.minimum(pfx, 1), suf))
    bad = slot.copy()
    bad[0] = R.N_SLOTS
    out = R.attention_prefix_ref(q, k, v, kc, vc, bad, pfx, suf)
    assert np.isnan(out[0, : suf[0]]).all() and not out[0, suf[0]:].any() and np.array_equal(out[1:], ref[1:])


def _brute_force_plan(pl, lens, max_rows, slab_rows):
    """every scored token -> where its predicting row comes from, written down token by token"""
    S = max(pl)
    first, suffix, flat = [], {}, 0
    passes, cur = [], []
    for b, cs in enumerate(lens):
        for n in cs:
            if n >= 1:
                first.append((b * S + pl[b] - 1, flat))
            if n >= 2:
                m = max([n - 1] + [x[1] - 1 for x in cur])
                if cur and (len(cur) + 1) * m > max_rows:
                    passes.append(cur)
                    cur = []
                cur.append((b, n, flat))
            flat += n
    if cur:
        passes.append(cur)
    return S, first, passes, flat


@pytest.mark.parametrize("pl,lens,max_rows,slab_rows", [
    ([10, 7, 10], [[3, 2, 1], [0, 1], [2, 65]], 4096, 256),          # ragged prompts, candidates of 0 / 1 / 2 / 65 tokens
    ([5], [[0], ], 64, 256),                                         # nothing to score
    ([5, 9], [[1, 1], [1]], 64, 256),                                # one-token candidates only: no suffix pass at all
    ([6, 6], [[3, 3, 3, 3], [3, 3, 3]], 5, 256),                     # row budget: passes of 2 pairs x 2 rows
    ([6, 6], [[3, 5, 2, 9], [9, 2]], 16, 3),                         # the budget follows the longest pair of a pass; slabs of 3 rows
    ([4] * 3, [[4] * 30] * 3, 4096, 256),                            # 90 first rows, 270 suffix rows: slabs of 256 + 14
])
def test_score_prefix_plan_against_a_brute_force_model(pl, lens, max_rows, slab_rows):
    from internnav_amd.policy import SCORE_SUFFIX_MAX_ROWS, score_prefix_plan

    assert SCORE_SUFFIX_MAX_ROWS == 64
    plan = score_prefix_plan(pl, lens, max_rows, slab_rows)
    S, first, passes, total = _brute_force_plan(pl, lens, max_rows, slab_rows)
    assert plan["S"] == S and plan["total"] == total and plan["off"][-1] == total
    assert plan["pairs"] == [(b, c) for b in range(len(pl)) for c in range(len(lens[b]))]
    assert np.array_equal(np.diff(plan["off"]), [n for cs in lens for n in cs])
    assert plan["first_rows"].dtype == np.int32 and list(zip(plan["first_rows"].tolist(), plan["first_dst"].tolist())) == first
    assert len(plan["passes"]) == len(passes)
    written = set(plan["first_dst"].tolist())
    for got, want in zip(plan["passes"], passes):
        m = max(n - 1 for _, n, _ in want)
        P = len(want)
        assert got["m"] == m and 1 <= m <= 64 and (P * m <= max_rows or P == 1)
        assert got["prompt"].tolist() == [b for b, _, _ in want] and got["suf_len"].tolist() == [n - 1 for _, n, _ in want]
        assert [plan["pairs"][q][0] for q in got["pair"]] == got["prompt"].tolist()
        rows = [j * m + i for j, (_, n, _) in enumerate(want) for i in range(n - 1)]
        dst = [f + 1 + i for _, n, f in want for i in range(n - 1)]              # row at suffix position i predicts token i + 1
        assert got["rows"].dtype == np.int32 and got["rows"].tolist() == rows and got["dst"].tolist() == dst
        assert not written & set(dst)
        written |= set(dst)
        for sl, R_ in ((got["slabs"], len(rows)),):
            assert sl == [(r, min(r + slab_rows, R_)) for r in range(0, R_, slab_rows)]
    assert written == set(range(total))                                        # every token of every candidate is scored exactly once
    F = len(first)
    assert plan["first_slabs"] == [(r, min(r + slab_rows, F)) for r in range(0, F, slab_rows)]


def test_score_prefix_plan_refuses_a_66_token_candidate():
    from internnav_amd.policy import score_prefix_plan

    assert score_prefix_plan([5], [[65]], 64)["passes"][0]["m"] == 64
    with pytest.raises(ValueError, match="share_prefix=False"):
        score_prefix_plan([5], [[66]], 4096)


CTYPE = {"const void*": C.c_void_p, "void*": C.c_void_p, "const int32_t*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
NAMES = ["Q", "q_ps", "q_rs", "q_hs", "O", "o_ps", "o_rs", "o_hs", "k_cache", "v_cache", "c_ss", "c_rs", "c_hs", "n_slots", "k_suf", "v_suf", "s_ps",
         "s_rs", "s_hs", "slot", "pfx_len", "suf_len", "P", "m", "H", "Hkv", "D", "max_pfx", "scale", "stream"]


def test_lib_declares_attention_prefix_with_the_headers_signature(built_lib):
    from internnav_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "internnav_amd.h").read_text(), flags=re.S)
    mt = re.search(r"^int ina_attention_prefix\((.*?)\);", text, flags=re.M | re.S)
    assert mt, "ina_attention_prefix is not declared in include/internnav_amd.h"
    params = [" ".join(p.split()) for p in mt.group(1).split(",")]
    types = [re.sub(r"\s*\b\w+$", "", p).replace(" *", "*") for p in params]
    assert [re.search(r"(\w+)$", p).group(1) for p in params] == NAMES
    restype, argtypes = _lib.SYMBOLS["ina_attention_prefix"]
    assert restype is C.c_int and argtypes == [CTYPE[t] for t in types], (types, argtypes)
    assert hasattr(C.CDLL(str(built_lib)), "ina_attention_prefix") and _lib.lib().ina_abi_version() == 8


def test_abi_refusals_return_before_any_hip_call(built_lib):
    from internnav_amd import _lib

    lib = _lib.lib()
    buf = (C.c_uint32 * 64)()
    p = (C.addressof(buf) + 15) // 16 * 16                             # never dereferenced: every call below is refused or has nothing to do
    H, Hkv, m = 28, 4, 3
    qkv_w, kv_w = (H + 2 * Hkv) * 128, 2 * Hkv * 128
    base = dict(Q=p, q_ps=m * qkv_w, q_rs=qkv_w, q_hs=128, O=p, o_ps=m * H * 128, o_rs=H * 128, o_hs=128, k_cache=p, v_cache=p, c_ss=320 * kv_w, c_rs=kv_w,
                c_hs=128, n_slots=4, k_suf=p, v_suf=p, s_ps=m * qkv_w, s_rs=qkv_w, s_hs=128, slot=p, pfx_len=p, suf_len=p, P=2, m=m, H=H, Hkv=Hkv, D=128,
                max_pfx=300, scale=128 ** -0.5, stream=None)

    def call(**kw):
        a = dict(base, **{k: v for k, v in kw.items() if not k.endswith("_off")})
        for k, v in kw.items():
            if k.endswith("_off"):
                a[k[:-4]] = p + v                                          # a misaligned pointer
        return lib.ina_attention_prefix(*[a[n] for n in NAMES])

    for kw in R.abi_refusal_cases():
        assert call(**kw) != 0, kw
        assert b"attention_prefix" in lib.ina_last_error(), kw
    assert call(P=0) == 0                                                  # nothing to do: no launch, no error


def test_share_prefix_refuses_a_66_token_candidate_before_any_launch():
    """the limit is checked on the host before the engine is touched: a stand-in without an engine is enough (and proves nothing was launched)"""
    from internnav_amd.policy import InternVLAN1ForCausalLM

    touched = []

    class NoEngine:
        cfg = dict(image_token_id=9, vocab=100)
        B_max = 2

        def __getattr__(self, name):
            touched.append(name)
            raise AssertionError(f"engine.{name} used before the refusal")

    stub = SimpleNamespace(qwen=NoEngine(), device=torch.device("cpu"), _gen=None)
    ids = torch.tensor([[1, 2, 3]])
    with pytest.raises(ValueError, match=r"65 tokens.*share_prefix=False"):
        InternVLAN1ForCausalLM.score_answers(stub, ids, [[list(range(66))]], share_prefix=True)
    assert not touched
