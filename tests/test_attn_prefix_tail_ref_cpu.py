"""CPU: the float64 restatement of ops.attention_prefix_tail (tests/attn_prefix_tail_ref.py) against torch SDPA on the per-pair concatenation
[prefix | tail | suffix], the declaration and the refusals of the C-ABI entry (dummy pointers: every call is refused or has nothing to do), and
generate_latents' choice between continuing a sampled generate() and the re-run path, on a stand-in engine. No GPU is needed."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_prefix_ref as R0
import attn_prefix_tail_ref as R

ROOT = Path(__file__).resolve().parent.parent


def _tables(c):
    return tuple(c[n].numpy() for n in ("slot", "pfx_len", "suf_len", "tail_row", "tail_len"))


def test_the_cases_cover_what_they_claim():
    pairs = [(c[0], c[1], c[2], s, t, n, c[4][s], c[5][t] if t >= 0 else 0) for c in R.CASES for s, t, n in c[3]]
    assert {(p[0], p[1]) for p in pairs} == {(28, 4), (4, 4)} and {p[2] for p in pairs} == {1, 5, 16, 17, 64}
    assert {p[6] for p in pairs} == {0, 1, 63, 64, 65, 256, 300} and {p[7] for p in pairs} == {0, 1, 63, 64, 65, 130}
    assert any(p[5] == 0 for p in pairs) and any(p[4] == -1 and p[5] > 0 for p in pairs) and any(p[6] == 0 and p[7] == 0 and p[5] > 0 for p in pairs)
    # pairs whose chunks are those of ops.attention_prefix on [prefix | tail]: a tail behind 0, 64 and 256 prompt rows
    assert {p[6] for p in pairs if p[6] % 64 == 0 and p[7] > 0 and p[5] > 0} == {0, 64, 256}
    for c in R.CASES:
        slots, tails = [s for s, _, _ in c[3]], [t for _, t, _ in c[3] if t >= 0]
        assert slots != sorted(slots) and len(set(tails)) < len(tails), "slots out of order, one tail shared by two pairs"
    assert any(tails != sorted(tails) for tails in ([t for _, t, _ in c[3] if t >= 0] for c in R.CASES))


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_reference_equals_sdpa_on_the_concatenation_and_ignores_the_poison(case):
    c = R.make_case(case)
    q, k, v, kc, vc, kt, vt = (t.double().numpy() for t in R.views(c["fused"], c["cache"], c["tails"], c["H"], c["Hkv"], c["m"]))
    slot, pfx, suf, trow, tlen = _tables(c)
    for name in ("cache", "tails"):
        assert np.isnan(c[name].float().numpy()).any()
    assert np.isnan(c["fused"].float().numpy()).any() or bool((suf == c["m"]).all())
    ref = R.attention_prefix_tail_ref(q, k, v, kc, vc, slot, pfx, suf, kt, vt, trow, tlen)
    assert np.isfinite(ref).all(), "the reference read a poisoned row"
    want = R.sdpa_ref(q, k, v, kc, vc, slot, pfx, suf, kt, vt, trow, tlen)
    assert np.isfinite(want).all()
    assert np.abs(ref - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    for p in range(c["P"]):
        assert not ref[p, suf[p]:].any()                                    # rows behind suf_len: zeros
    # without a tail (no tail arguments, or every tail_len 0) it is attention_prefix's restatement
    plain = R0.attention_prefix_ref(q, k, v, kc, vc, slot, pfx, suf)
    assert np.array_equal(R.attention_prefix_tail_ref(q, k, v, kc, vc, slot, pfx, suf), plain)
    assert np.array_equal(R.attention_prefix_tail_ref(q, k, v, kc, vc, slot, pfx, suf, kt, vt, trow, np.zeros_like(tlen)), plain)
    # max_pfx / max_tail clip the tables
    clip = R.attention_prefix_tail_ref(q, k, v, kc, vc, slot, pfx, suf, kt, vt, trow, tlen, max_pfx=1, max_tail=2)
    assert np.array_equal(clip, R.attention_prefix_tail_ref(q, k, v, kc, vc, slot, np.minimum(pfx, 1), suf, kt, vt, trow, np.minimum(tlen, 2)))
    # a slot outside the cache, a tail outside the buffer under a positive tail_len: NaN in the pair's live rows only
    live = [p for p in range(c["P"]) if tlen[p] > 0 and suf[p] > 0]
    bad_s, bad_t = slot.copy(), trow.copy()
    bad_s[0], bad_t[live[0]] = R.N_SLOTS, R.N_TAILS
    for out, p in ((R.attention_prefix_tail_ref(q, k, v, kc, vc, bad_s, pfx, suf, kt, vt, trow, tlen), 0),
                   (R.attention_prefix_tail_ref(q, k, v, kc, vc, slot, pfx, suf, kt, vt, bad_t, tlen), live[0])):
        keep = [i for i in range(c["P"]) if i != p]
        assert np.isnan(out[p, : suf[p]]).all() and not out[p, suf[p]:].any() and np.array_equal(out[keep], ref[keep])
    # tail_len 0 does not look at tail_row
    none = [p for p in range(c["P"]) if tlen[p] == 0]
    any_t = trow.copy()
    any_t[none] = 99
    assert np.array_equal(R.attention_prefix_tail_ref(q, k, v, kc, vc, slot, pfx, suf, kt, vt, any_t, tlen), ref)


def test_materialised_slots_hold_the_same_keys():
    """the yardstick of the GPU test: ops.attention_prefix's restatement on [prefix | tail] slots is the reference"""
    c = R.make_case(R.CASES[0])
    q, k, v, kc, vc, kt, vt = (t.double().numpy() for t in R.views(c["fused"], c["cache"], c["tails"], c["H"], c["Hkv"], c["m"]))
    mat, slot, plen = R.materialised(c)
    m5 = mat.view(c["P"], R.S_CACHE, 2, c["Hkv"], R.D).double().numpy()
    got = R0.attention_prefix_ref(q, k, v, m5[:, :, 0], m5[:, :, 1], slot.numpy(), plen.numpy(), c["suf_len"].numpy())
    assert np.array_equal(got, R.reference_of(c))


CTYPE = {"const void*": C.c_void_p, "void*": C.c_void_p, "const int32_t*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
NAMES = ["Q", "q_ps", "q_rs", "q_hs", "O", "o_ps", "o_rs", "o_hs", "k_cache", "v_cache", "c_ss", "c_rs", "c_hs", "n_slots", "k_tail", "v_tail", "t_ps",
         "t_rs", "t_hs", "n_tail_rows", "k_suf", "v_suf", "s_ps", "s_rs", "s_hs", "slot", "pfx_len", "tail_row", "tail_len", "suf_len", "P", "m", "H", "Hkv",
         "D", "max_pfx", "max_tail", "scale", "stream"]


def test_lib_declares_attention_prefix_tail_with_the_headers_signature(built_lib):
    from internnav_amd import _lib, ops

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "internnav_amd.h").read_text(), flags=re.S)
    mt = re.search(r"^int ina_attention_prefix_tail\((.*?)\);", text, flags=re.M | re.S)
    assert mt, "ina_attention_prefix_tail is not declared in include/internnav_amd.h"
    params = [" ".join(p.split()) for p in mt.group(1).split(",")]
    types = [re.sub(r"\s*\b\w+$", "", p).replace(" *", "*") for p in params]
    assert [re.search(r"(\w+)$", p).group(1) for p in params] == NAMES
    restype, argtypes = _lib.SYMBOLS["ina_attention_prefix_tail"]
    assert restype is C.c_int and argtypes == [CTYPE[t] for t in types], (types, argtypes)
    assert hasattr(C.CDLL(str(built_lib)), "ina_attention_prefix_tail") and _lib.lib().ina_abi_version() == 8      # plain arguments: no ABI bump
    assert callable(ops.attention_prefix_tail)


def test_abi_refusals_return_before_any_hip_call(built_lib):
    from internnav_amd import _lib

    lib = _lib.lib()
    buf = (C.c_uint32 * 64)()
    p = (C.addressof(buf) + 15) // 16 * 16                             # never dereferenced: every call below is refused or has nothing to do
    H, Hkv, m, T = 28, 4, 5, 136
    qkv_w, kv_w = (H + 2 * Hkv) * 128, 2 * Hkv * 128
    base = dict(Q=p, q_ps=m * qkv_w, q_rs=qkv_w, q_hs=128, O=p, o_ps=m * H * 128, o_rs=H * 128, o_hs=128, k_cache=p, v_cache=p, c_ss=448 * kv_w, c_rs=kv_w,
                c_hs=128, n_slots=5, k_tail=p, v_tail=p, t_ps=T * kv_w, t_rs=kv_w, t_hs=128, n_tail_rows=5, k_suf=p, v_suf=p, s_ps=m * qkv_w, s_rs=qkv_w,
                s_hs=128, slot=p, pfx_len=p, tail_row=p, tail_len=p, suf_len=p, P=2, m=m, H=H, Hkv=Hkv, D=128, max_pfx=300, max_tail=130,
                scale=128 ** -0.5, stream=None)

    def call(**kw):
        a = dict(base, **{k: v for k, v in kw.items() if not k.endswith("_off")})
        for k, v in kw.items():
            if k.endswith("_off"):
                a[k[:-4]] = p + v                                          # a misaligned pointer
        return lib.ina_attention_prefix_tail(*[a[n] for n in NAMES])

    for kw in R.abi_refusal_cases():
        assert call(**kw) != 0, kw
        assert b"attention_prefix_tail" in lib.ina_last_error(), kw
    no_tail = dict(k_tail=None, v_tail=None, tail_row=None, tail_len=None)
    for kw in (dict(D=64), dict(m=65), dict(slot=None)):                   # the refusals of the plain entry, without a tail as well
        assert call(**no_tail, **kw) != 0 and b"attention_prefix_tail" in lib.ina_last_error(), kw
    assert call(P=0) == 0 and call(P=0, **no_tail) == 0                    # nothing to do: no launch, no error
    assert call(P=0, **no_tail, n_tail_rows=0, max_tail=-1, t_rs=3) == 0   # without a tail its sizes and strides are not looked at


class _Engine:
    """stand-in for QwenVLEngine: records which of the two ways generate_latents took"""

    def __init__(self):
        self.calls = []

    def latents_behind(self, state, rows, last_tokens, keep_len):
        self.calls.append(("behind", list(rows), list(last_tokens), list(keep_len)))
        return "behind"

    def latents(self, state, last, seq_lens=None):
        self.calls.append(("latents",))
        return "latents"

    def generate_latents(self, output_ids, pv, grid, cached_embeds=None):
        self.calls.append(("rerun", tuple(output_ids.shape)))
        return torch.arange(output_ids.shape[0] * 2.0).view(-1, 2)


def _stub(path="shared"):
    """what generate(do_sample=True, num_return_sequences=2) leaves for 2 prompts of 4 and 3 tokens: answers of 3 tokens, row 1 ended after 2"""
    toks = torch.tensor([[11, 12, 13], [21, 7, 7], [31, 32, 33], [41, 42, 43]])
    gen = dict(state="STATE", tokens=toks, lens=np.asarray([3, 2, 3, 3]), prompt_lens=np.asarray([4, 4, 3, 3]), fanned=True, path=path)
    seqs = torch.full((4, 7), 7, dtype=torch.long)
    for r in range(4):
        n = int(gen["prompt_lens"][r])
        seqs[r, :n] = 1
        seqs[r, n:n + 3] = toks[r]
    return SimpleNamespace(qwen=_Engine(), device=torch.device("cpu"), _gen=gen), seqs


@pytest.mark.parametrize("path", ["shared", "fan"])
def test_generate_latents_continues_a_sampled_generate_for_the_requested_rows_only(path):
    from internnav_amd.policy import InternVLAN1ForCausalLM

    stub, seqs = _stub(path)
    stub.generate_latents = lambda *a, **k: InternVLAN1ForCausalLM.generate_latents(stub, *a, **k)
    assert InternVLAN1ForCausalLM.generate_latents(stub, seqs, None, None, rows=[3, 1]) == "behind"
    # row 3: prompt of 3 + 3 answer tokens, the last one (43) runs in front of the queries; row 1 ended at its second token (7)
    assert stub.qwen.calls == [("behind", [3, 1], [43, 7], [3 + 3 - 1, 4 + 2 - 1])]
    assert InternVLAN1ForCausalLM.generate_latents(stub, seqs, None, None) == "behind"
    assert stub.qwen.calls[1] == ("behind", [0, 1, 2, 3], [13, 7, 33, 43], [6, 5, 5, 5]) and stub._gen is not None


def test_generate_latents_on_other_tokens_falls_back_to_the_rerun():
    from internnav_amd.policy import InternVLAN1ForCausalLM

    stub, seqs = _stub()
    stub.generate_latents = lambda *a, **k: InternVLAN1ForCausalLM.generate_latents(stub, *a, **k)
    other = seqs.clone()
    other[2, 4] = 99                                                       # row 2's second answer token is not what generate() returned
    out = InternVLAN1ForCausalLM.generate_latents(stub, other, None, None, rows=[2])
    assert stub.qwen.calls == [("rerun", (4, 7))], "the re-run path runs every row and indexes afterwards, as before"
    assert torch.equal(out, torch.tensor([[4.0, 5.0]])) and stub._gen is None, "the re-run rewrote the slots: nothing is left to continue"
    # rows that do match still continue (another stub: the state is gone after a re-run); another row count never does
    stub, seqs = _stub()
    stub.generate_latents = lambda *a, **k: InternVLAN1ForCausalLM.generate_latents(stub, *a, **k)
    other = seqs.clone()
    other[2, 4] = 99
    assert InternVLAN1ForCausalLM.generate_latents(stub, other, None, None, rows=[0, 3]) == "behind"
    InternVLAN1ForCausalLM.generate_latents(stub, seqs[:2], None, None)
    assert [c[0] for c in stub.qwen.calls] == ["behind", "rerun"]
