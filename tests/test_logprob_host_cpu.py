"""CPU: the host side of the per-token log-probabilities - the C-ABI entry as the header declares it and its refusals (the list of
logprob_ref.abi_refusal_cases, which tests/test_logprob_gpu.py runs again with device pointers), the masking / summing of generate()'s outputs,
the row plan of score_answers and the kernel selection of its lm_head GEMM. No GPU is needed: every call is refused or has nothing to do."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import logprob_ref as L

ROOT = Path(__file__).resolve().parent.parent
CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "uint32_t*": C.c_void_p, "const int32_t*": C.c_void_p, "int32_t*": C.c_void_p,
         "void*": C.c_void_p, "int32_t": C.c_int32, "float": C.c_float}


def test_lib_declares_logprob_rows_with_the_headers_signature(built_lib):
    from internnav_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "internnav_amd.h").read_text(), flags=re.S)
    m = re.search(r"^int ina_logprob_rows\((.*?)\);", text, flags=re.M | re.S)
    assert m, "ina_logprob_rows is not declared in include/internnav_amd.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    types = [re.sub(r"\s*\b\w+$", "", p).replace(" *", "*") for p in params]
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    assert names == ["X", "ldx", "rows", "n", "seen", "ld_words", "penalty", "mark", "target", "tok", "logprob", "margin", "stream"]
    restype, argtypes = _lib.SYMBOLS["ina_logprob_rows"]
    assert restype is C.c_int and argtypes == [CTYPE[t] for t in types], (types, argtypes)
    assert hasattr(C.CDLL(str(built_lib)), "ina_logprob_rows") and _lib.lib().ina_abi_version() == 8


def test_abi_refusals_return_before_any_hip_call(built_lib):
    from internnav_amd import _lib

    lib = _lib.lib()
    buf = (C.c_uint32 * 64)()
    p = C.addressof(buf)                                             # never dereferenced: every call below is refused on its arguments

    def call(X=p, ldx=64, rows=1, n=64, seen=p, ld_words=2, penalty=1.05, mark=0, target=None, tok=p, lp=p, mg=p):
        return lib.ina_logprob_rows(X, ldx, rows, n, seen, ld_words, penalty, mark, target, tok, lp, mg, None)

    for kw in L.abi_refusal_cases(64, p):
        assert call(**kw) != 0, kw
        assert b"logprob_rows" in lib.ina_last_error(), kw
    assert call(rows=0) == 0 and call(rows=0, seen=None, mg=None) == 0          # nothing to do: no launch, no error


def test_generate_side_masking_and_sum():
    from internnav_amd.policy import answer_confidences, answer_logprob_summary

    nan = math.nan
    lp = torch.tensor([[-0.5, -0.25, -1.0, -2.0], [-0.125, nan, -3.0, -4.0], [-1.0, -1.0, nan, nan]])
    mg = torch.tensor([[2.0, 0.5, 1.0, 9.0], [3.0, 0.0, 7.0, 7.0], [0.25, 4.0, nan, 0.0]])
    toks = np.array([[5, 6, 7, 8], [5, 99, 7, 8], [5, 98, 6, 99]])                 # EOS ids 99 / 98: none, at 1, at 1
    want_lp, lens = L.mask_after_eos(lp.numpy(), toks, (99, 98))
    assert lens.tolist() == [4, 2, 2]
    r = answer_logprob_summary(lp, mg, lens)
    assert np.array_equal(r.token_logprobs.numpy(), want_lp, equal_nan=True)
    assert r.token_logprobs[2].tolist() == [-1.0, -1.0, 0.0, 0.0] and r.token_margins[2].tolist() == [0.25, 4.0, 0.0, 0.0]   # NaN behind EOS dropped
    assert r.token_margins[1].tolist() == [3.0, 0.0, 0.0, 0.0]
    assert r.sequences_logprob[0].item() == -3.75 and math.isnan(r.sequences_logprob[1].item()) and r.sequences_logprob[2].item() == -2.0
    assert r.answer_lengths.tolist() == [4, 2, 2]
    conf = answer_confidences(r)                                                   # (answer_logprob, answer_min_margin) per row, Python floats
    assert len(conf) == 3 and conf[0] == (-3.75, 0.5) and conf[2] == (-2.0, 0.25) and all(isinstance(v, float) for c in conf for v in c)
    assert math.isnan(conf[1][0]) and conf[1][1] == 0.0                            # a NaN INSIDE the answer is kept
    empty = answer_logprob_summary(torch.zeros(2, 0), torch.zeros(2, 0), [0, 0])
    assert answer_confidences(empty) == [(0.0, math.inf), (0.0, math.inf)]


def test_score_row_plan():
    from internnav_amd.policy import SCORE_SLAB_ROWS, score_row_plan

    assert SCORE_SLAB_ROWS == 256
    S, rows, off, slabs = score_row_plan([10, 7, 10], [3, 1, 0])
    assert S == 13 and off.tolist() == [0, 3, 4, 4] and slabs == [(0, 4)]
    # answer token i of sequence q is predicted at position plen - 1 + i: plen-1 .. plen+len-2
    assert rows.tolist() == [9, 10, 11, 13 + 6] and rows.dtype == np.int32
    S, rows, off, slabs = score_row_plan([5] * 130, [4] * 130)                      # 520 rows: slabs of 256, 256, 8
    assert S == 9 and rows.size == 520 and slabs == [(0, 256), (256, 512), (512, 520)]
    assert rows[:5].tolist() == [4, 5, 6, 7, 9 + 4] and rows[-1] == 129 * 9 + 7
    assert score_row_plan([5, 5], [2, 2], slab_rows=3)[3] == [(0, 3), (3, 4)]
    assert score_row_plan([4], [0])[3] == [] and score_row_plan([4], [256])[3] == [(0, 256)] and score_row_plan([4], [257])[3] == [(0, 256), (256, 257)]
    with pytest.raises(AssertionError):
        score_row_plan([0], [1])


@pytest.mark.parametrize("M", [1, 17, 256])
def test_lm_head_gemm_of_score_answers_selects_a_kernel(built_lib, M):
    """score_answers' lm_head GEMM (M = answer rows of a slab, N = 152064, K = 3584, fp32 output) goes through ina_gemm_select like any other:
    at most 64 rows stream the weight (32), more run a tiled kernel the library accepts when it is asked for by number - never a refusal"""
    from internnav_amd import _lib

    a = _lib.GemmArgs()
    a.A = a.W = a.C = 0x1000
    a.M, a.N, a.K = M, 152064, 3584
    a.lda = a.ldw = 3584
    a.ldc = a.ldr = 152064
    a.out_dtype = 1
    out = C.c_int(0)
    rc = _lib.lib().ina_gemm_select(C.byref(a), C.byref(out))
    assert rc == 0, _lib.lib().ina_last_error()
    assert out.value == 32 if M <= 64 else out.value > 0, out.value
    a.force_cfg, again = out.value, C.c_int(0)
    assert _lib.lib().ina_gemm_select(C.byref(a), C.byref(again)) == 0 and again.value == out.value
