"""CPU: the float64 restatement of ops.sample_rows (tests/sample_ref.py) against transformers' warpers, its behaviour on ties, its acceptance check,
the host side of generate(do_sample=True) (generation_config fields, defaults, refusals) and the C-ABI entry's refusals. No GPU is needed."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

import sample_ref as S

ROOT = Path(__file__).resolve().parent.parent
CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "uint32_t*": C.c_void_p, "const int32_t*": C.c_void_p, "int32_t*": C.c_void_p,
         "void*": C.c_void_p, "int32_t": C.c_int32, "float": C.c_float}
# (n, sigma, T, top_k, top_p): configurations on which HF's fp32 cumulative sum seldom comes near the cut (top-p alone on thousands of entries does)
HF_CASES = [(4097, 3.0, 1.0, 50, 0.9), (33, 1.0, 1.0, 5, 0.8), (33, 2.0, 0.5, 0, 0.5)]


@pytest.mark.parametrize("n,sigma,T,top_k,top_p", HF_CASES)
def test_kept_sets_equal_hf_warpers_on_tie_free_rows(n, sigma, T, top_k, top_p):
    pytest.importorskip("transformers")
    rows = 50
    g = np.random.default_rng(n + top_k)
    x = (g.standard_normal((rows, n)) * sigma).astype(np.float32)
    for r in range(rows):
        while np.unique(S.processed(x[r], None, 1.0, T)).size < n:             # (4097 fp32 normals collide now and then)
            x[r] = (g.standard_normal(n) * sigma).astype(np.float32)
    hf = S.hf_kept(x, T, top_k, top_p)
    skipped = mismatches = 0
    for r in range(rows):
        z = S.processed(x[r], None, 1.0, T)
        assert np.unique(z).size == n, "the row has ties"
        keep, thr, vk = S.kept_row(z, top_k, top_p)
        _, m = S.value_masses(z, vk)
        if np.abs(m - (1.0 - float(np.float32(top_p)))).min() < 1e-4:       # HF sums in fp32: a mass this close to the cut may fall either way
            skipped += 1
            continue
        mismatches += int(not np.array_equal(keep, hf[r]))
        assert int(keep.sum()) == int((z >= np.float32(thr)).sum()) and keep[int(np.argmax(z))]
    print(f"n={n} T={T} top_k={top_k} top_p={top_p}: {skipped} of {rows} rows skipped, {mismatches} mismatches")
    assert skipped <= rows // 10 and mismatches == 0


def test_ties_stay_or_go_as_a_whole_and_contain_hfs_set():
    pytest.importorskip("transformers")
    g = np.random.default_rng(5)
    for top_k, top_p in ((4, 1.0), (0, 0.7), (6, 0.6)):
        for _ in range(20):
            x = g.integers(-3, 4, 24).astype(np.float32)                     # seven values over 24 entries: ties everywhere
            z = S.processed(x)
            keep, thr, vk = S.kept_row(z, top_k, top_p)
            for v in np.unique(z):
                assert keep[z == v].all() or not keep[z == v].any(), "a value was split"
            assert np.array_equal(keep, z >= np.float32(thr)) and keep[z == z.max()].all()
            hf = S.hf_kept(x[None], 1.0, top_k, top_p)[0]
            assert not (hf & ~keep).any(), "HF keeps an entry the value-level rule drops"
            if top_k:
                assert int(keep.sum()) >= min(top_k, 24) or top_p < 1.0
    z = S.processed(np.array([2.0, 1.0, 2.0, 1.0, 0.0, -np.inf, np.nan], dtype=np.float32))
    keep, thr, vk = S.kept_row(z, 3, 1.0)
    assert vk == 1.0 and thr == 1.0 and keep.tolist() == [True, True, True, True, False, False, False]      # ties at v_k all stay; NaN never
    keep, thr, _ = S.kept_row(z, 0, 1.0)
    assert thr == -math.inf and keep.tolist() == [True] * 6 + [False]                                        # top-p off: mass-0 entries stay
    keep, thr, _ = S.kept_row(z, 0, 0.999999)
    assert thr == 0.0 and int(keep.sum()) == 5                                                               # top-p on: they go
    keep, thr, _ = S.kept_row(z, 0, 1e-3)
    assert thr == 2.0 and keep.tolist() == [True, False, True, False, False, False, False]                   # the maximum (both of it) stays


def test_draw_and_conventions():
    z = S.processed(np.log(np.array([0.1, 0.2, 0.3, 0.25, 0.15])).astype(np.float32))
    c, keep, W = S.cdf_of(z, -math.inf)
    assert keep.all() and abs(c[-1] - 1.0) < 1e-15 and np.allclose(c, [0.1, 0.3, 0.6, 0.85, 1.0], atol=1e-7)
    toks = [S.draw_row(z, 0, 1.0, (i + 0.5) / 4096)[0] for i in range(4096)]
    assert np.abs(np.bincount(toks, minlength=5) - np.diff(np.concatenate([[0], c])) * 4096).max() <= 1.0
    tok, lp, nk, thr = S.draw_row(z, 1, 1.0, 0.999)
    assert (tok, lp, nk) == (2, 0.0, 1) and thr == float(z[2])
    for fill in (-np.inf, np.nan):
        tok, lp, nk, thr = S.draw_row(np.full(4, fill, dtype=np.float32), 0, 1.0, 0.5)
        assert (tok, nk) == (0, 0) and math.isnan(lp) and math.isnan(thr)
    tok, lp, nk, _ = S.draw_row(np.array([1.0, np.inf, -1.0, np.inf], dtype=np.float32), 0, 1.0, 0.75)
    assert (tok, nk) == (3, 4) and abs(lp + math.log(2.0)) < 1e-15
    # the acceptance check: exactly the drawn token at eps, its neighbours once u sits on an edge
    eps = S.eps_cdf(5)
    assert S.accepted_tokens(z, -math.inf, 0.45, eps).tolist() == [2] and S.check_token(z, -math.inf, 0.45, 2, eps)[0]
    assert not S.check_token(z, -math.inf, 0.45, 1, eps)[0] and not S.check_token(z, 0.0, 0.45, 2, eps)[0]
    assert S.accepted_tokens(z, -math.inf, float(c[1]), 1e-6).tolist() == [1, 2]
    assert S.check_thr(z, 0, 0.5, float(z[3]), eps)[0] and not S.check_thr(z, 0, 0.5, float(z[2]), eps)[0] and not S.check_thr(z, 0, 0.5, float(z[1]), eps)[0]
    assert S.check_thr(z, 2, 1.0, float(z[3]), eps)[0] and not S.check_thr(z, 2, 1.0, float(z[2]), eps)[0]
    assert S.eps_cdf(S.MAX_VOCAB) <= S.EPS_LIMIT == 1e-5


def test_generation_config_sampling_fields_defaults_and_refusals():
    from internnav_amd.policy import generation_config_from_hf, sampling_spec

    raw = {"do_sample": True, "temperature": 0.1, "top_k": 1, "top_p": 0.001, "repetition_penalty": 1.05, "eos_token_id": [7, 9]}
    g = generation_config_from_hf(raw, [3])
    assert (g.do_sample, g.temperature, g.top_k, g.top_p, g.repetition_penalty, g.eos_token_id) == (True, 0.1, 1, 0.001, 1.05, (7, 9))
    none = generation_config_from_hf(None, [3])
    assert (none.do_sample, none.temperature, none.top_k, none.top_p, none.repetition_penalty, none.eos_token_id) == (None, None, None, None, 1.0, (3,))
    # greedy ignores the file's sampling keys and the sampling arguments; sampling takes the file's values where the argument is None
    assert sampling_spec(g, False) is None and sampling_spec(g, False, temperature=0.0, top_p=7.0, extra={"min_p": 0.2}) is None
    assert vars(sampling_spec(g, True)) == dict(temperature=0.1, top_k=1, top_p=0.001, K=1)
    assert vars(sampling_spec(g, True, temperature=2.0, top_k=0, num_return_sequences=4)) == dict(temperature=2.0, top_k=0, top_p=0.001, K=4)
    assert vars(sampling_spec(none, True)) == dict(temperature=1.0, top_k=50, top_p=1.0, K=1)                   # HF's defaults
    for key, v in (("min_p", 0.05), ("typical_p", 0.9), ("epsilon_cutoff", 3e-4), ("eta_cutoff", 1e-3)):
        with pytest.raises(NotImplementedError, match=key):
            sampling_spec(none, True, extra={key: v})
        with_file = generation_config_from_hf({key: v}, [3])                                                      # loading does not refuse it ...
        with pytest.raises(NotImplementedError, match=key):
            sampling_spec(with_file, True)                                                                        # ... generate(do_sample=True) does
        assert sampling_spec(with_file, False) is None
    assert sampling_spec(none, True, extra={"min_p": None, "typical_p": 1.0, "epsilon_cutoff": 0.0, "eta_cutoff": 0.0}) is not None
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=math.nan), dict(temperature=math.inf), dict(top_k=-1),
               dict(top_p=0.0), dict(top_p=1.5), dict(num_return_sequences=0)):
        with pytest.raises(ValueError):
            sampling_spec(none, True, **kw)
    with pytest.raises(ValueError, match="num_return_sequences"):
        sampling_spec(none, False, num_return_sequences=2)


def test_lib_declares_sample_rows_with_the_headers_signature(built_lib):
    from internnav_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "internnav_amd.h").read_text(), flags=re.S)
    m = re.search(r"^int ina_sample_rows\((.*?)\);", text, flags=re.M | re.S)
    assert m, "ina_sample_rows is not declared in include/internnav_amd.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    types = [re.sub(r"\s*\b\w+$", "", p).replace(" *", "*") for p in params]
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    assert names == ["X", "ldx", "x_rows", "rows", "n", "seen", "ld_words", "penalty", "mark", "temperature", "top_k", "top_p", "u", "src", "tok",
                     "logprob", "n_kept", "thr", "stream"]
    restype, argtypes = _lib.SYMBOLS["ina_sample_rows"]
    assert restype is C.c_int and argtypes == [CTYPE[t] for t in types], (types, argtypes)
    assert hasattr(C.CDLL(str(built_lib)), "ina_sample_rows") and _lib.lib().ina_abi_version() == 8      # plain arguments: no ABI bump


def test_abi_refusals_return_before_any_hip_call(built_lib):
    from internnav_amd import _lib

    lib = _lib.lib()
    buf = (C.c_uint32 * 64)()
    p = C.addressof(buf)                                             # never dereferenced: every call below is refused on its arguments

    def call(X=p, ldx=64, x_rows=2, rows=2, n=64, seen=p, ld_words=2, penalty=1.05, mark=0, T=1.0, top_k=0, top_p=1.0, u=p, src=None, tok=p, lp=p,
             nk=p, thr=p):
        return lib.ina_sample_rows(X, ldx, x_rows, rows, n, seen, ld_words, penalty, mark, T, top_k, top_p, u, src, tok, lp, nk, thr, None)

    for kw in S.abi_refusal_cases(64, 2):
        assert call(**kw) != 0, kw
        assert b"sample_rows" in lib.ina_last_error(), kw
    assert call(n=262145, ldx=262145, ld_words=8193) != 0 and b"262144" in lib.ina_last_error()
    assert call(rows=0) == 0 and call(rows=0, seen=None, nk=None, thr=None) == 0      # nothing to do: no launch, no error
