"""CPU: the float64 restatement of ops.attention_shared (tests/attn_shared_ref.py) against a brute-force softmax(q K^T) V on the per-row
concatenation, the host tile plan against a brute-force model, the declaration and the refusals of the C-ABI entry (dummy pointers: every call
is refused before a launch) and the refusals of generate(share_prefix=True) on a stand-in without an engine. No GPU is needed."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_shared_ref as R

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_reference_equals_brute_force_on_the_concatenation_and_ignores_the_poison(case):
    c = R.make_case(case)
    q, kt, vt, kc, vc = (t.double().numpy() for t in R.views(c["fused"], c["tail"], c["cache"], c["H"], c["Hkv"]))
    assert np.isnan(c["cache"].float().numpy()).any() and np.isnan(c["tail"].float().numpy()).any() and np.isnan(q[c["R"]]).all()
    ref = R.reference_of(c)
    n = c["R"]
    assert np.isfinite(ref).all(), "the reference read a poisoned row"
    assert (ref[n] == R.FILL).all(), "the row no tile names was written"
    want = R.brute_force(q[:n], kt[:n], vt[:n], kc, vc, c["row_slot"], c["row_pfx"], c["tail_len"].numpy()[:n])
    assert sorted(want) == list(range(n))
    for r in range(n):
        assert np.abs(ref[r] - want[r]).max() <= 1e-12 * max(1.0, np.abs(want[r]).max()), r
    # tail_len <= 0: a zero row; a slot outside the cache: NaN in the tile's rows that have a tail; the other rows unchanged
    tl = c["tail_len"].clone()
    tl[0] = 0
    z = R.reference_of(c, tail_len=tl)
    assert not z[0].any() and np.array_equal(z[1:], ref[1:])
    bad = c["tile_slot"].clone()
    bad[0] = R.N_SLOTS
    o = R.reference_of(c, tile_slot=bad, tail_len=tl)
    rows0 = [int(r) for r in c["tile_rows"][0] if r >= 0]
    assert not o[0].any() and all(np.isnan(o[r]).all() for r in rows0 if r != 0)
    keep = [r for r in range(n + 1) if r not in rows0]
    assert np.array_equal(o[keep], ref[keep])


@pytest.mark.parametrize("G,counts", [(7, [3, 5, 1]), (7, [2, 2]), (4, [5, 2, 1]), (16, [2, 3]), (1, [5, 3, 2]), (1, [17]), (2, [9]), (3, [4])])
def test_tile_plan_against_a_brute_force_model(G, counts):
    from internnav_amd import ops

    prompt_of = [b for b, k in enumerate(counts) for _ in range(k)]
    tiles, owner = ops.attention_shared_plan(prompt_of, G)
    cpt = 16 // G
    assert tiles.dtype == np.int32 and tiles.shape[1] == cpt and owner.shape == (tiles.shape[0],)
    named = tiles[tiles >= 0].tolist()
    assert sorted(named) == list(range(len(prompt_of))), "every row appears exactly once"
    assert bool(((tiles >= 0) | (tiles == -1)).all())
    for t, b in zip(tiles, owner):
        assert {prompt_of[r] for r in t[t >= 0]} == {int(b)}, "the rows of a tile share a prompt"
    want = R.brute_force_plan(prompt_of, G)
    assert [(int(b), t[t >= 0].tolist()) for t, b in zip(tiles, owner)] == want
    for b, k in enumerate(counts):                                          # a count that is no multiple of cpt leaves a partly filled last tile
        mine = [t for t, o in zip(tiles, owner) if o == b]
        assert len(mine) == -(-k // cpt) and int((mine[-1] >= 0).sum()) == (k % cpt or cpt)
        if G == 7 and k % 2:                                                # the 7B geometry: two candidates per tile, an odd count leaves half a tile
            assert cpt == 2 and mine[-1].tolist() == [sum(counts[:b]) + k - 1, -1]
    # rows of a prompt that do not follow each other still share its tiles
    tiles2, owner2 = ops.attention_shared_plan([0, 1, 0, 1, 0], 7)
    assert [(int(b), t[t >= 0].tolist()) for t, b in zip(tiles2, owner2)] == [(0, [0, 2]), (0, [4]), (1, [1, 3])]
    with pytest.raises(ValueError, match="17"):
        ops.attention_shared_plan([0], 17)


CTYPE = {"const void*": C.c_void_p, "void*": C.c_void_p, "const int32_t*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
NAMES = ["Q", "q_rs", "q_hs", "O", "o_rs", "o_hs", "k_cache", "v_cache", "c_ss", "c_rs", "c_hs", "n_slots", "k_tail", "v_tail", "t_ps", "t_rs", "t_hs", "T",
         "tile_rows", "tile_slot", "tile_pfx", "tail_len", "n_tiles", "n_rows", "H", "Hkv", "D", "max_pfx", "scale", "stream"]


def test_lib_declares_attention_shared_with_the_headers_signature(built_lib):
    from internnav_amd import _lib, ops

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "internnav_amd.h").read_text(), flags=re.S)
    mt = re.search(r"^int ina_attention_shared\((.*?)\);", text, flags=re.M | re.S)
    assert mt, "ina_attention_shared is not declared in include/internnav_amd.h"
    params = [" ".join(p.split()) for p in mt.group(1).split(",")]
    types = [re.sub(r"\s*\b\w+$", "", p).replace(" *", "*") for p in params]
    assert [re.search(r"(\w+)$", p).group(1) for p in params] == NAMES
    restype, argtypes = _lib.SYMBOLS["ina_attention_shared"]
    assert restype is C.c_int and argtypes == [CTYPE[t] for t in types], (types, argtypes)
    assert hasattr(C.CDLL(str(built_lib)), "ina_attention_shared") and _lib.lib().ina_abi_version() == 8      # plain arguments: no ABI bump
    assert callable(ops.attention_shared)


def test_abi_refusals_return_before_any_hip_call(built_lib):
    from internnav_amd import _lib

    lib = _lib.lib()
    buf = (C.c_uint32 * 64)()
    p = (C.addressof(buf) + 15) // 16 * 16                             # never dereferenced: every call below is refused
    H, Hkv, T = 28, 4, 8
    qkv_w, kv_w = (H + 2 * Hkv) * 128, 2 * Hkv * 128
    base = dict(Q=p, q_rs=qkv_w, q_hs=128, O=p, o_rs=H * 128, o_hs=128, k_cache=p, v_cache=p, c_ss=320 * kv_w, c_rs=kv_w, c_hs=128, n_slots=4, k_tail=p,
                v_tail=p, t_ps=T * kv_w, t_rs=kv_w, t_hs=128, T=T, tile_rows=p, tile_slot=p, tile_pfx=p, tail_len=p, n_tiles=3, n_rows=5, H=H, Hkv=Hkv, D=128,
                max_pfx=300, scale=128 ** -0.5, stream=None)

    def call(**kw):
        a = dict(base, **{k: v for k, v in kw.items() if not k.endswith("_off")})
        for k, v in kw.items():
            if k.endswith("_off"):
                a[k[:-4]] = p + v                                          # a misaligned pointer
        return lib.ina_attention_shared(*[a[n] for n in NAMES])

    cases = R.abi_refusal_cases()
    for need in (dict(D=64), dict(H=34, Hkv=2), dict(H=30), dict(n_tiles=0), dict(n_rows=0), dict(T=0)):     # what the contract names
        assert need in cases
    for kw in cases:
        assert call(**kw) != 0, kw
        assert b"attention_shared" in lib.ina_last_error(), kw


def test_generate_share_prefix_refusals_come_before_any_launch():
    """both limits are checked on the host before the engine is touched: a stand-in without an engine is enough (and proves nothing was launched)"""
    from internnav_amd.policy import InternVLAN1ForCausalLM, generation_config_from_hf
    from internnav_amd.runtime import CapacityError

    touched = []

    class NoEngine:
        cfg = dict(image_token_id=9, vocab=100)
        B_max = 16
        max_decode = 128

        def __getattr__(self, name):
            touched.append(name)
            raise AssertionError(f"engine.{name} used before the refusal")

    stub = SimpleNamespace(qwen=NoEngine(), device=torch.device("cpu"), _gen=None, generation_config=generation_config_from_hf(None, 2))
    ids = torch.ones(13, 5, dtype=torch.long)
    with pytest.raises(ValueError, match="do_sample"):
        InternVLAN1ForCausalLM.generate(stub, ids, share_prefix=True)
    with pytest.raises(ValueError, match="do_sample"):
        InternVLAN1ForCausalLM.generate(stub, ids, share_prefix=True, do_sample=False, max_new_tokens=4)
    with pytest.raises(CapacityError, match="64"):
        InternVLAN1ForCausalLM.generate(stub, ids, share_prefix=True, do_sample=True, num_return_sequences=5)       # 13 x 5 = 65 rows
    with pytest.raises(CapacityError, match="max_seqs"):
        InternVLAN1ForCausalLM.generate(stub, torch.ones(17, 5, dtype=torch.long), share_prefix=True, do_sample=True)   # 17 prompts on 16 slots
    with pytest.raises(ValueError, match="export_prefix"):
        InternVLAN1ForCausalLM.generate(stub, ids, share_prefix=True, do_sample=True, export_prefix=[3] + [0] * 12)
    assert not touched
