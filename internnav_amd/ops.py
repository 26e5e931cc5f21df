"""Torch-tensor front end of the op-level C-ABI (gemm / attention / norm).

PyTorch is plumbing here: it owns device memory and the stream; all arithmetic runs in the hand-written gfx950
kernels of libinternnav_amd.so. Tensors must live on the current HIP device.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import AttnArgs, GemmArgs, NormArgs

ACT = {None: 0, "none": 0, "gelu": 1, "gelu_erf": 1, "gelu_tanh": 2, "relu": 3, "silu": 4, "mish": 5, "tanh": 6}
_DT = {torch.bfloat16: 0, torch.float32: 1}


# Tile selection of the GEMMs that leave it to the library (force_cfg = 0): inside `shared_tail()` they are issued with force_cfg = -1 -
# "this launch runs beside another stream's GEMMs" (include/internnav_amd.h) - so the tile cost model does not charge the under-filled last
# round that the other stream's workgroups fill. Every tile shape accumulates K in the same order, so the choice changes no bit of the
# result; that also makes the process-wide switch harmless if a launch of another host thread picks it up.
_AUTO_CFG = 0


@contextlib.contextmanager
def shared_tail():
    global _AUTO_CFG
    keep, _AUTO_CFG = _AUTO_CFG, -1
    try:
        yield
    finally:
        _AUTO_CFG = keep


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _f32(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    assert t.dtype == torch.float32 and t.is_contiguous(), "f32 parameter vectors must be contiguous float32"
    return t


def _as2d(x: torch.Tensor) -> torch.Tensor:
    assert x.stride(-1) == 1, "last dimension must be contiguous"
    if x.dim() == 2:          # the common case: no new view object (every ops call runs on the host's launch-issue path)
        return x
    return x.reshape(-1, x.shape[-1]) if x.is_contiguous() else x


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act=None,
           colscale: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None, out_dtype=torch.bfloat16, glu: bool = False,
           rowscale: Optional[torch.Tensor] = None, rowscale_div: int = 1, force_cfg: int = 0,
           batched: bool = False, group_m: int = 0, prenorm=None, w_frag: Optional[torch.Tensor] = None, seg_stats=None) -> torch.Tensor:
    """out = epilogue(x @ w.T). x: bf16 [..., K] (or a 2-D row-strided view), w: bf16 [N, K].

    seg_stats=(stats f32 [M, N // 384, 2], eps): the row-panel GEMM (K = 384, >= 16384 rows, plain epilogue) also writes (mean, rstd) of every 384-wide
    segment of its fp32 output rows - the LayerNorm statistics dit_attention(stats=) consumes. Refused where another kernel would run.
    w_frag: the same weight in MFMA fragment order (gemm_preshuffle(w)): the wide no-residual GEMMs that would run tile config 39 then take
    their B fragments from it straight into registers (config 40, bit-equal); ignored by every other tile.

    batched=True: x is [Bt, M, K] and out [Bt, M, N] views with arbitrary batch strides (rows contiguous-strided inside a
    batch); residual is [Bt, M, N] or a [M, N] table broadcast over the batch (e.g. positional embeddings).
    prenorm=(gamma f32 [K], eps): RMSNorm of x fused in front (x f32 or bf16, at most 16 rows): out = epilogue(bf16(rmsnorm(x) * gamma) @ w.T).
    """
    assert (x.dtype == torch.bfloat16 or prenorm is not None) and w.dtype == torch.bfloat16
    assert w.dim() == 2 and w.stride(1) == 1
    N, K = w.shape
    n_out = N // 2 if glu else N
    a = GemmArgs()
    if batched:
        assert x.dim() == 3 and x.stride(2) == 1 and out is not None and out.dim() == 3 and out.stride(2) == 1
        Bt, M, _ = x.shape
        assert out.shape == (Bt, M, n_out)
        a.A, a.C = x.data_ptr(), out.data_ptr()
        a.lda, a.ldc = x.stride(1), out.stride(1)
        a.batch, a.strideA, a.strideC = Bt, x.stride(0), out.stride(0)
        if residual is not None:
            assert residual.stride(-1) == 1 and residual.shape[-2:] == (M, n_out)
            a.R, a.ldr, a.res_dtype = residual.data_ptr(), residual.stride(-2), _DT[residual.dtype]
            a.strideR = residual.stride(0) if residual.dim() == 3 else 0
    else:
        lead = x.shape[:-1]
        x2 = _as2d(x)
        assert x2.dim() == 2
        M = x2.shape[0]
        if out is None:
            out = torch.empty(*lead, n_out, dtype=out_dtype, device=x.device)
        o2 = _as2d(out)
        assert o2.shape == (M, n_out), f"out {tuple(o2.shape)} vs {(M, n_out)}"
        a.A, a.C = x2.data_ptr(), o2.data_ptr()
        a.lda, a.ldc = x2.stride(0), o2.stride(0)
        a.batch = 1
        if residual is not None:
            r2 = _as2d(residual)
            assert r2.shape == (M, n_out)
            a.R, a.ldr, a.res_dtype = r2.data_ptr(), r2.stride(0), _DT[r2.dtype]
    assert x.shape[-1] == K, f"K mismatch {tuple(w.shape)} vs {tuple(x.shape)}"
    a.W, a.ldw = w.data_ptr(), w.stride(0)
    a.bias, a.colscale, a.rowscale = _ptr(_f32(bias)), _ptr(_f32(colscale)), _ptr(_f32(rowscale))
    a.M, a.N, a.K = M, N, K
    a.act = ACT[act] if not isinstance(act, int) else act
    a.out_dtype = _DT[out.dtype]
    a.glu = 1 if glu else 0
    a.rowscale_div = rowscale_div
    a.force_cfg = force_cfg if force_cfg else _AUTO_CFG
    a.group_m = group_m
    if seg_stats is not None:
        st, se = seg_stats
        assert not batched and st.dtype == torch.float32 and st.is_contiguous() and st.numel() >= M * (N // 384) * 2 and N % 384 == 0
        a.seg_stats, a.seg_eps = st.data_ptr(), float(se)
    if w_frag is not None:
        assert w_frag.dtype == torch.bfloat16 and w_frag.is_contiguous() and w_frag.numel() == N * K and N % 16 == 0 and K % 32 == 0
        a.Wp = w_frag.data_ptr()
    if prenorm is not None:
        gamma, eps = prenorm
        assert not batched and x.dtype in (torch.bfloat16, torch.float32) and gamma.dtype == torch.float32 and gamma.is_contiguous() and gamma.numel() == K
        a.norm_gamma, a.norm_eps, a.a_dtype = gamma.data_ptr(), float(eps), _DT[x.dtype]
    _lib.check(_lib.lib().ina_gemm_bf16(C.byref(a), _stream()), "gemm_bf16")
    return out


def gemm_preshuffle(w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """w bf16 [N, K] -> the same elements in MFMA fragment order (flat [N * K]): fragment (n // 16, k // 32) is one contiguous KiB whose lane
    (k % 32 // 8) * 16 + n % 16 holds 8 consecutive k. Done once per weight at load time; consumed by linear(w_frag=)."""
    assert w.dtype == torch.bfloat16 and w.dim() == 2 and w.stride(1) == 1
    N, K = w.shape
    if out is None:
        out = torch.empty(N * K, dtype=torch.bfloat16, device=w.device)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.numel() == N * K
    _lib.check(_lib.lib().ina_gemm_preshuffle(w.data_ptr(), out.data_ptr(), N, K, w.stride(0), _stream()), "gemm_preshuffle")
    return out


# ---- FP8 weights of the weight-streaming GEMMs (csrc/gemm_skinny_w8.hip): OCP e4m3 bytes + a power-of-two scale per output row
W8_MAX = 448.0          # largest finite e4m3fn value
W8_EXP_RANGE = 64       # |exponent| bound: 2^e stays a normal fp32 / bf16 with room to spare


def w8_pack(q: torch.Tensor) -> torch.Tensor:
    """uint8 [N, K] in natural k order -> the kernels' row layout (K % 128 == 0): element k = step * 128 + s * 32 + g * 8 + j (MFMA step s, lane
    group g, lane element j) moves to byte step * 128 + g * 32 + s * 8 + j of its row, so a lane's 32 bytes of a K step are contiguous."""
    assert q.dtype == torch.uint8 and q.dim() == 2 and q.shape[1] % 128 == 0, "w8 layout: uint8 [N, K] with K % 128 == 0"
    N, K = q.shape
    return q.reshape(N, K // 128, 4, 4, 8).transpose(2, 3).reshape(N, K).contiguous()


def w8_unpack(p: torch.Tensor) -> torch.Tensor:
    """inverse of w8_pack (the permutation swaps two axes of equal length: it is its own inverse)"""
    return w8_pack(p)


def w8_quantize(w: torch.Tensor):
    """w bf16 [N, K] (K % 128 == 0) -> (w8 uint8 [N, K] packed e4m3fn bytes, wexp int8 [N], w_deq bf16 [N, K]).

    Row n is stored as q = e4m3fn_rne(w / 2^e_n) with e_n the smallest exponent for which the row's amax fits 448 (an all-zero row: 0),
    clamped to [-64, 64]; w_deq = q * 2^e_n is exact in bf16 - it is the model the fp8 kernels compute, and w8_quantize(w_deq)[2] == w_deq."""
    assert w.dtype == torch.bfloat16 and w.dim() == 2 and w.shape[1] % 128 == 0, "w8_quantize: bf16 [N, K] with K % 128 == 0"
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    # amax = m * 2^x with m in [0.5, 1), 448 = 0.875 * 2^9: amax <= 448 * 2^e  <=>  e >= x - 9 (m <= 0.875) or x - 8 (exact: no log2 rounding)
    m, x = torch.frexp(amax)
    e = torch.where(m <= 0.875, x - 9, x - 8)
    e = torch.where(amax == 0, torch.zeros_like(e), e).clamp(-W8_EXP_RANGE, W8_EXP_RANGE).to(torch.int32)
    scaled = torch.ldexp(wf, (-e)[:, None]).clamp(-W8_MAX, W8_MAX)      # (torch's fp8 cast does not saturate: clamp first)
    q = scaled.to(torch.float8_e4m3fn)
    w_deq = torch.ldexp(q.float(), e[:, None]).to(torch.bfloat16)
    return w8_pack(q.view(torch.uint8)), e.to(torch.int8).contiguous(), w_deq.contiguous()


def linear_w8(x: torch.Tensor, w8: torch.Tensor, wexp: torch.Tensor, bias: Optional[torch.Tensor] = None, act=None,
              colscale: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None, out_dtype=torch.bfloat16, glu: bool = False,
              rowscale: Optional[torch.Tensor] = None, rowscale_div: int = 1, prenorm=None) -> torch.Tensor:
    """`linear` on FP8 weights for at most 64 rows (prenorm: 16): w8 uint8 [N, K] packed (w8_quantize / w8_pack), wexp int8 [N].
    Bit for bit the weight-streaming result of linear(x, w_deq, ...) on the dequantised weights, at half the weight bytes."""
    assert (x.dtype == torch.bfloat16 or prenorm is not None) and w8.dtype == torch.uint8 and wexp.dtype == torch.int8
    assert w8.dim() == 2 and w8.stride(1) == 1 and wexp.is_contiguous() and wexp.numel() == w8.shape[0]
    N, K = w8.shape
    return _linear_packed("ina_gemm_w8", "gemm_w8", x, w8, wexp, N, K, bias, act, colscale, residual, out, out_dtype, glu, rowscale, rowscale_div, prenorm)


def _linear_packed(entry: str, what: str, x, wq, wside, N: int, K: int, bias, act, colscale, residual, out, out_dtype, glu, rowscale, rowscale_div,
                   prenorm) -> torch.Tensor:
    """the call of a quantised-weight form of the weight-streaming GEMMs (ina_gemm_w8 / ina_gemm_mx4): wq = the packed weight rows (row
    pitch in bytes = stride(0)), wside = its exponents / block scales; every other operand as in `linear`"""
    n_out = N // 2 if glu else N
    lead = x.shape[:-1]
    x2 = _as2d(x)
    assert x2.dim() == 2 and x.shape[-1] == K, f"K mismatch {(N, K)} vs {tuple(x.shape)}"
    M = x2.shape[0]
    if out is None:
        out = torch.empty(*lead, n_out, dtype=out_dtype, device=x.device)
    o2 = _as2d(out)
    assert o2.shape == (M, n_out), f"out {tuple(o2.shape)} vs {(M, n_out)}"
    a = GemmArgs()
    a.A, a.C = x2.data_ptr(), o2.data_ptr()
    a.lda, a.ldc = x2.stride(0), o2.stride(0)
    a.batch = 1
    if residual is not None:
        r2 = _as2d(residual)
        assert r2.shape == (M, n_out)
        a.R, a.ldr, a.res_dtype = r2.data_ptr(), r2.stride(0), _DT[r2.dtype]
    a.ldw = wq.stride(0)
    a.bias, a.colscale, a.rowscale = _ptr(_f32(bias)), _ptr(_f32(colscale)), _ptr(_f32(rowscale))
    a.M, a.N, a.K = M, N, K
    a.act = ACT[act] if not isinstance(act, int) else act
    a.out_dtype = _DT[out.dtype]
    a.glu = 1 if glu else 0
    a.rowscale_div = rowscale_div
    if prenorm is not None:
        gamma, eps = prenorm
        assert x.dtype in (torch.bfloat16, torch.float32) and gamma.dtype == torch.float32 and gamma.is_contiguous() and gamma.numel() == K
        a.norm_gamma, a.norm_eps, a.a_dtype = gamma.data_ptr(), float(eps), _DT[x.dtype]
    _lib.check(getattr(_lib.lib(), entry)(C.byref(a), wq.data_ptr(), wside.data_ptr(), _stream()), what)
    return out


# ---- MXFP4 weights of the weight-streaming GEMMs (csrc/gemm_skinny_mx4.hip): OCP e2m1 elements, two per byte, + an e8m0 scale per 32 k
MX4_BLOCK = 32
# e2m1 codes 0 .. 7 stand for |value| 0, 0.5, 1, 1.5, 2, 3, 4, 6; bit 3 of a code is the sign


def mx4_pack(q: torch.Tensor) -> torch.Tensor:
    """e2m1 codes uint8 [N, K] (one code 0 .. 15 per element, natural k order, K % 128 == 0) -> the kernels' row layout uint8 [N, K / 2]:
    element k = step * 128 + s * 32 + g * 8 + j (MFMA step s, lane group g, lane element j) is nibble j (bits 4j .. 4j + 3) of the
    little-endian dword g * 4 + s of the row's 64-byte K step, i.e. byte step * 64 + (g * 4 + s) * 4 + j // 2, low nibble for even j. A
    lane's four fragments of a K step are 16 contiguous bytes, the four lane groups of a row 64."""
    assert q.dtype == torch.uint8 and q.dim() == 2 and q.shape[1] % 128 == 0, "mx4 layout: uint8 codes [N, K] with K % 128 == 0"
    N, K = q.shape
    c = q.reshape(N, K // 128, 4, 4, 4, 2).transpose(2, 3)          # [N, step, g, s, j // 2, j % 2]
    return (c[..., 0] | (c[..., 1] << 4)).reshape(N, K // 2).contiguous()


def mx4_unpack(p: torch.Tensor) -> torch.Tensor:
    """inverse of mx4_pack: packed uint8 [N, K / 2] -> codes uint8 [N, K] in natural k order"""
    assert p.dtype == torch.uint8 and p.dim() == 2 and p.shape[1] % 64 == 0, "mx4 layout: packed uint8 [N, K / 2] with K % 128 == 0"
    N, K = p.shape[0], p.shape[1] * 2
    b = p.reshape(N, K // 128, 4, 4, 4)                              # [N, step, g, s, j // 2]
    return torch.stack([b & 15, b >> 4], dim=-1).transpose(2, 3).reshape(N, K).contiguous()


def mx4_quantize(w: torch.Tensor):
    """w bf16 [N, K] (K % 128 == 0) -> (w4 uint8 [N, K / 2] packed e2m1, wscale uint8 [N, K / 32] e8m0 bytes 127 + e, w_deq bf16 [N, K]).

    OCP microscaling, round to nearest: a block of 32 consecutive k shares e = floor(log2(amax)) - 2 (the block's amax lands in [4, 8),
    e2m1's top binade), clamped to [-64, 64]; an element is w / 2^e rounded to nearest-even onto {0, .5, 1, 1.5, 2, 3, 4, 6} and
    saturated at 6 (an amax in (6, 8) * 2^e does). A block whose elements all round to zero - an all-zero block, or one far below the
    clamp - stores e = 0. w_deq = q * 2^e is exact in bf16 - it is the model the MXFP4 kernels compute - and mx4_quantize(w_deq)
    returns the same three tensors."""
    assert w.dtype == torch.bfloat16 and w.dim() == 2 and w.shape[1] % 128 == 0, "mx4_quantize: bf16 [N, K] with K % 128 == 0"
    N, K = w.shape
    wf = w.float().reshape(N, K // MX4_BLOCK, MX4_BLOCK)
    amax = wf.abs().amax(dim=2)
    _, x = torch.frexp(amax)                      # amax = m * 2^x, m in [0.5, 1): floor(log2(amax)) = x - 1, exactly
    e = torch.where(amax == 0, torch.zeros_like(x), x - 3).clamp(-W8_EXP_RANGE, W8_EXP_RANGE).to(torch.int32)
    a = torch.ldexp(wf.abs(), (-e)[..., None])
    # the e2m1 grid has steps of 0.5 below 2, 1 below 4 and 2 above; torch.round rounds halves to even, which is the even code here
    r = torch.where(a < 2, torch.round(a * 2) * 0.5, torch.where(a < 4, torch.round(a), (torch.round(a * 0.5) * 2).clamp(max=6.0)))
    e = torch.where((r == 0).all(dim=2), torch.zeros_like(e), e)
    code = torch.where(r < 2, r * 2, torch.where(r < 4, r + 2, r * 0.5 + 4)).to(torch.uint8) | (torch.signbit(wf).to(torch.uint8) << 3)
    w_deq = torch.ldexp(torch.where(torch.signbit(wf), -r, r), e[..., None]).to(torch.bfloat16).reshape(N, K)
    return mx4_pack(code.reshape(N, K)), (e + 127).to(torch.uint8).contiguous(), w_deq.contiguous()


def linear_mx4(x: torch.Tensor, w4: torch.Tensor, wscale: torch.Tensor, bias: Optional[torch.Tensor] = None, act=None,
               colscale: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, out_dtype=torch.bfloat16, glu: bool = False,
               rowscale: Optional[torch.Tensor] = None, rowscale_div: int = 1, prenorm=None) -> torch.Tensor:
    """`linear` on MXFP4 weights for at most 64 rows (prenorm: 16): w4 uint8 [N, K / 2] packed (mx4_quantize / mx4_pack; rows may be strided),
    wscale uint8 [N, K / 32] contiguous. Bit for bit the weight-streaming result of linear(x, w_deq, ...) on the dequantised weights, at
    0.27 of the weight bytes."""
    assert (x.dtype == torch.bfloat16 or prenorm is not None) and w4.dtype == torch.uint8 and wscale.dtype == torch.uint8
    assert w4.dim() == 2 and w4.stride(1) == 1 and wscale.is_contiguous() and wscale.shape == (w4.shape[0], w4.shape[1] // 16)
    N, K = w4.shape[0], w4.shape[1] * 2
    return _linear_packed("ina_gemm_mx4", "gemm_mx4", x, w4, wscale, N, K, bias, act, colscale, residual, out, out_dtype, glu, rowscale, rowscale_div, prenorm)


def attention_rope_ok(Lq: int, Lk: int, H: int, Hkv: int, D: int) -> bool:
    """shapes whose attention launch can carry the rotary embedding + KV append of its new tokens (the one-launch decode kernel of the d = 128
    heads; csrc/attention.hip ina_launch_attention)"""
    return D == 128 and 256 <= Lk <= 1024 and Lq <= 8 and (H // Hkv) * Lq <= 48


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: Optional[float] = None, causal: bool = False,
              kv_start: int = 0, kv_bdiv: int = 1, cu_q: Optional[torch.Tensor] = None,
              cu_k: Optional[torch.Tensor] = None, max_q: int = 0, max_k: int = 0,
              head_gate: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              accumulate: bool = False, k_len: Optional[torch.Tensor] = None, drop_p: float = 0.0, drop_seed: int = 0,
              kernel: int = 0, drop_salt: Optional[torch.Tensor] = None, rope=None) -> torch.Tensor:
    """softmax(q k^T * scale [+ masks]) v.   kernel: 0 = automatic, 1 = the 16-rows-per-wave kernel, 2 = the 32-rows-per-wave kernel
    (ina_attn_args.kernel; the parity tests compare the two).
    rope=(cos f32 [B * Lq, 128], sin, k_new bf16 [B, Lq, Hkv, 128], v_new) - single-token decoder passes (see `attention_rope_ok`): q, k_new are
    UN-rotated; the launch rotates them, appends rotate(k_new) | v_new to the last Lq rows of k / v (the cache views) and attends.

    Dense: q [B, Lq, H, D], k/v [Bk, Lk, Hkv, D] (arbitrary strides, last dim contiguous; Bk = B / kv_bdiv).
    Varlen: q [T, H, D], k/v [Tk, Hkv, D] packed with int32 cu_q / cu_k offsets and max_q / max_k.
    """
    assert q.dtype == k.dtype == v.dtype == torch.bfloat16
    a = AttnArgs()
    if cu_q is not None:
        assert q.dim() == 3 and cu_k is not None
        T, H, D = q.shape
        Hkv = k.shape[1]
        B = cu_q.numel() - 1
        if out is None:
            out = torch.empty(T, H, D, dtype=torch.bfloat16, device=q.device)
        a.q_bs, a.q_rs, a.q_hs = 0, q.stride(0), q.stride(1)
        a.k_bs, a.k_rs, a.k_hs = 0, k.stride(0), k.stride(1)
        a.v_bs, a.v_rs, a.v_hs = 0, v.stride(0), v.stride(1)
        a.o_bs, a.o_rs, a.o_hs = 0, out.stride(0), out.stride(1)
        a.Lq, a.Lk = max_q, max_k
        a.cu_q, a.cu_k = cu_q.data_ptr(), cu_k.data_ptr()
        assert cu_q.dtype == torch.int32 and cu_k.dtype == torch.int32
    else:
        B, Lq, H, D = q.shape
        Bk, Lk, Hkv, _ = k.shape
        assert Bk * kv_bdiv == B, f"kv batch {Bk} x {kv_bdiv} != {B}"
        if out is None:
            out = torch.empty(B, Lq, H, D, dtype=torch.bfloat16, device=q.device)
        a.q_bs, a.q_rs, a.q_hs = q.stride(0), q.stride(1), q.stride(2)
        a.k_bs, a.k_rs, a.k_hs = k.stride(0), k.stride(1), k.stride(2)
        a.v_bs, a.v_rs, a.v_hs = v.stride(0), v.stride(1), v.stride(2)
        a.o_bs, a.o_rs, a.o_hs = out.stride(0), out.stride(1), out.stride(2)
        a.Lq, a.Lk = Lq, Lk
    assert q.stride(-1) == 1 and k.stride(-1) == 1 and v.stride(-1) == 1 and out.stride(-1) == 1
    a.Q, a.K, a.V, a.O = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.B, a.H, a.Hkv, a.D = B, H, Hkv, D
    a.causal = 1 if causal else 0
    a.kv_start, a.kv_bdiv = kv_start, kv_bdiv
    a.scale = float(scale) if scale is not None else float(D) ** -0.5
    a.head_gate = _ptr(_f32(head_gate))
    if k_len is not None:
        assert k_len.dtype == torch.int32 and k_len.is_contiguous() and cu_q is None
        a.k_len = k_len.data_ptr()
    a.accumulate = 1 if accumulate else 0
    if rope is not None:
        cos, sin, k_new, v_new = rope
        assert cu_q is None and cos.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous() and cos.shape[-1] == 128 and cos.numel() >= B * Lq * 128
        assert k_new.dtype == torch.bfloat16 and k_new.shape == (B, Lq, Hkv, D) and v_new.shape == k_new.shape and k_new.stride() == v_new.stride() and k_new.stride(-1) == 1
        a.rope_cos, a.rope_sin, a.k_new, a.v_new = cos.data_ptr(), sin.data_ptr(), k_new.data_ptr(), v_new.data_ptr()
        a.kn_bs, a.kn_rs, a.kn_hs = k_new.stride(0), k_new.stride(1), k_new.stride(2)
    a.kernel = kernel
    if drop_p > 0.0:       # training only: attention-probability dropout, mask = counter hash of (seed, element index)
        assert cu_q is None, "dropout: dense layouts only"
        a.drop_seed, a.drop_thresh, a.drop_scale = drop_params(drop_p, drop_seed)
        if drop_salt is not None:          # one int32 device word added to the seed at kernel start (fresh masks per replay of a captured launch sequence)
            assert drop_salt.dtype == torch.int32 and drop_salt.numel() == 1 and drop_salt.is_cuda
            a.drop_salt = drop_salt.data_ptr()
    _lib.check(_lib.lib().ina_attention_bf16(C.byref(a), _stream()), "attention_bf16")
    return out


ATTN_PREFIX_MAX_ROWS = 64     # suffix rows per pair of ops.attention_prefix (one 64-key chunk, csrc/attention_prefix.hip)


def attention_prefix(q: torch.Tensor, k_suf: torch.Tensor, v_suf: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, slot: torch.Tensor,
                     pfx_len: torch.Tensor, suf_len: torch.Tensor, out: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                     max_pfx: Optional[int] = None) -> torch.Tensor:
    """causal self-attention of P short suffixes that also see a prefix kept once in a KV cache (ina_attention_prefix): query row i of pair p
    (i < suf_len[p]) sees rows [0, pfx_len[p]) of cache slot slot[p] and suffix keys j <= i of pair p. Nothing is written to the cache.
    q [P, m, H, 128], k_suf / v_suf [P, m, Hkv, 128] (equal strides), k_cache / v_cache [slots, S, Hkv, 128] (equal strides), all bf16 with a
    contiguous last dim; slot / pfx_len / suf_len int32 [P] on the device. max_pfx (default S): the largest pfx_len (longer ones are clipped).
    Rows i >= suf_len[p] come out as zeros, a slot outside the cache as NaN rows."""
    assert q.dtype == k_suf.dtype == v_suf.dtype == k_cache.dtype == v_cache.dtype == torch.bfloat16
    assert q.dim() == 4 and k_suf.dim() == 4 and k_cache.dim() == 4
    P, m, H, D = q.shape
    Hkv = k_suf.shape[2]
    n_slots, S = k_cache.shape[0], k_cache.shape[1]
    assert D == 128, f"attention_prefix: head dim {D} (128 only)"
    assert 1 <= m <= ATTN_PREFIX_MAX_ROWS, f"attention_prefix: {m} suffix rows per pair (1 .. {ATTN_PREFIX_MAX_ROWS})"
    assert Hkv > 0 and H % Hkv == 0, f"attention_prefix: {H} heads over {Hkv} KV heads"
    assert k_suf.shape == (P, m, Hkv, D) and v_suf.shape == k_suf.shape and k_suf.stride() == v_suf.stride()
    assert k_cache.shape == (n_slots, S, Hkv, D) and v_cache.shape == k_cache.shape and k_cache.stride() == v_cache.stride() and n_slots >= 1
    if out is None:
        out = torch.empty(P, m, H, D, dtype=torch.bfloat16, device=q.device)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    assert all(t.stride(-1) == 1 for t in (q, k_suf, v_suf, k_cache, v_cache, out))
    for t in (slot, pfx_len, suf_len):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == P and t.device == q.device
    max_pfx = S if max_pfx is None else int(max_pfx)
    assert 0 <= max_pfx <= S, f"attention_prefix: max_pfx={max_pfx} outside the cache's {S} rows per slot"
    rc = _lib.lib().ina_attention_prefix(q.data_ptr(), q.stride(0), q.stride(1), q.stride(2), out.data_ptr(), out.stride(0), out.stride(1), out.stride(2),
                                         k_cache.data_ptr(), v_cache.data_ptr(), k_cache.stride(0), k_cache.stride(1), k_cache.stride(2), n_slots,
                                         k_suf.data_ptr(), v_suf.data_ptr(), k_suf.stride(0), k_suf.stride(1), k_suf.stride(2), slot.data_ptr(),
                                         pfx_len.data_ptr(), suf_len.data_ptr(), P, m, H, Hkv, D, max_pfx,
                                         float(scale) if scale is not None else float(D) ** -0.5, _stream())
    _lib.check(rc, "attention_prefix")
    return out


def attention_prefix_tail(q: torch.Tensor, k_suf: torch.Tensor, v_suf: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, slot: torch.Tensor,
                          pfx_len: torch.Tensor, suf_len: torch.Tensor, k_tail: Optional[torch.Tensor] = None, v_tail: Optional[torch.Tensor] = None,
                          tail_row: Optional[torch.Tensor] = None, tail_len: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                          scale: Optional[float] = None, max_pfx: Optional[int] = None, max_tail: Optional[int] = None) -> torch.Tensor:
    """`attention_prefix` with one more read-only key segment between prefix and suffix (ina_attention_prefix_tail): query row i of pair p
    (i < suf_len[p]) sees rows [0, pfx_len[p]) of cache slot slot[p], then rows [0, tail_len[p]) of tail tail_row[p], then suffix keys j <= i of
    pair p. Nothing is written to the cache or the tails. Arguments of `attention_prefix`, and k_tail / v_tail [n_tail_rows, T, Hkv, 128] bf16
    (equal strides, contiguous last dim; a layer of the engine's shared-prefix tails), tail_row / tail_len int32 [P] on the device, max_tail
    (default T): the largest tail_len (longer ones are clipped). The four tail arguments come together; without them the call is
    `attention_prefix`. tail_len <= 0 ignores tail_row; a tail row outside the buffer with tail_len > 0 gives NaN rows, as a bad slot does."""
    assert q.dtype == k_suf.dtype == v_suf.dtype == k_cache.dtype == v_cache.dtype == torch.bfloat16
    assert q.dim() == 4 and k_suf.dim() == 4 and k_cache.dim() == 4
    P, m, H, D = q.shape
    Hkv = k_suf.shape[2]
    n_slots, S = k_cache.shape[0], k_cache.shape[1]
    assert D == 128, f"attention_prefix_tail: head dim {D} (128 only)"
    assert 1 <= m <= ATTN_PREFIX_MAX_ROWS, f"attention_prefix_tail: {m} suffix rows per pair (1 .. {ATTN_PREFIX_MAX_ROWS})"
    assert Hkv > 0 and H % Hkv == 0, f"attention_prefix_tail: {H} heads over {Hkv} KV heads"
    assert k_suf.shape == (P, m, Hkv, D) and v_suf.shape == k_suf.shape and k_suf.stride() == v_suf.stride()
    assert k_cache.shape == (n_slots, S, Hkv, D) and v_cache.shape == k_cache.shape and k_cache.stride() == v_cache.stride() and n_slots >= 1
    if out is None:
        out = torch.empty(P, m, H, D, dtype=torch.bfloat16, device=q.device)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    assert all(t.stride(-1) == 1 for t in (q, k_suf, v_suf, k_cache, v_cache, out))
    for t in (slot, pfx_len, suf_len):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == P and t.device == q.device
    max_pfx = S if max_pfx is None else int(max_pfx)
    assert 0 <= max_pfx <= S, f"attention_prefix_tail: max_pfx={max_pfx} outside the cache's {S} rows per slot"
    tail = [k_tail, v_tail, tail_row, tail_len]
    has_tail = tail[0] is not None
    assert all((t is not None) == has_tail for t in tail), "attention_prefix_tail: k_tail, v_tail, tail_row and tail_len come together"
    tp = [0] * 9                                                    # k_tail, v_tail, their three strides, n_tail_rows, tail_row, tail_len, max_tail
    if has_tail:
        assert k_tail.dtype == v_tail.dtype == torch.bfloat16 and k_tail.dim() == 4 and k_tail.device == q.device
        n_tail_rows, T = k_tail.shape[0], k_tail.shape[1]
        assert n_tail_rows >= 1 and k_tail.shape == (n_tail_rows, T, Hkv, D) and v_tail.shape == k_tail.shape and k_tail.stride() == v_tail.stride()
        assert k_tail.stride(-1) == 1
        for t in (tail_row, tail_len):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == P and t.device == q.device
        max_tail = T if max_tail is None else int(max_tail)
        assert 0 <= max_tail <= T, f"attention_prefix_tail: max_tail={max_tail} outside the {T} rows of a tail"
        tp = [k_tail.data_ptr(), v_tail.data_ptr(), k_tail.stride(0), k_tail.stride(1), k_tail.stride(2), n_tail_rows, tail_row.data_ptr(),
              tail_len.data_ptr(), max_tail]
    rc = _lib.lib().ina_attention_prefix_tail(q.data_ptr(), q.stride(0), q.stride(1), q.stride(2), out.data_ptr(), out.stride(0), out.stride(1),
                                              out.stride(2), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.stride(0), k_cache.stride(1),
                                              k_cache.stride(2), n_slots, tp[0] or None, tp[1] or None, tp[2], tp[3], tp[4], tp[5], k_suf.data_ptr(),
                                              v_suf.data_ptr(), k_suf.stride(0), k_suf.stride(1), k_suf.stride(2), slot.data_ptr(), pfx_len.data_ptr(),
                                              tp[6] or None, tp[7] or None, suf_len.data_ptr(), P, m, H, Hkv, D, max_pfx, tp[8],
                                              float(scale) if scale is not None else float(D) ** -0.5, _stream())
    _lib.check(rc, "attention_prefix_tail")
    return out


ATTN_SHARED_MAX_GROUP = 16   # query heads per KV head of ops.attention_shared (one candidate's heads fill a 16-row tile at most)


def attention_shared_plan(prompt_of, G: int):
    """host tile plan of ops.attention_shared: prompt_of int [R] (the prompt of every row) -> (tile_rows int32 [n_tiles, cpt], tile_prompt
    int64 [n_tiles]), cpt = 16 // G. The rows of a prompt, in row order, fill tiles of cpt places; a prompt's last tile keeps -1 in the
    places it cannot fill (rows of two prompts never share a tile: a tile reads ONE prompt's prefix)."""
    if not 1 <= G <= ATTN_SHARED_MAX_GROUP:
        raise ValueError(f"attention_shared: {G} query heads per KV head (1 .. {ATTN_SHARED_MAX_GROUP})")
    cpt = 16 // G
    prompt_of = np.asarray(prompt_of, dtype=np.int64).reshape(-1)
    tiles, owner = [], []
    for b in dict.fromkeys(prompt_of.tolist()):                   # prompts in order of first appearance
        rows = np.nonzero(prompt_of == b)[0]
        for i in range(0, rows.size, cpt):
            t = np.full(cpt, -1, dtype=np.int32)
            t[: min(cpt, rows.size - i)] = rows[i:i + cpt]
            tiles.append(t)
            owner.append(b)
    return np.stack(tiles) if tiles else np.zeros((0, cpt), dtype=np.int32), np.asarray(owner, dtype=np.int64)


def attention_shared(q: torch.Tensor, k_tail: torch.Tensor, v_tail: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                     tile_rows: torch.Tensor, tile_slot: torch.Tensor, tile_pfx: torch.Tensor, tail_len: torch.Tensor,
                     out: Optional[torch.Tensor] = None, scale: Optional[float] = None, max_pfx: Optional[int] = None) -> torch.Tensor:
    """single-token attention of R rows whose prompts stay once in a KV cache (ina_attention_shared): row r of tile t sees rows
    [0, tile_pfx[t]) of cache slot tile_slot[t] and the first tail_len[r] rows of its own tail. Nothing is written to the cache.
    q [R, H, 128], k_tail / v_tail [R, T, Hkv, 128] (equal strides), k_cache / v_cache [slots, S, Hkv, 128] (equal strides), all bf16 with a
    contiguous last dim; tile_rows int32 [n_tiles, 16 // (H // Hkv)] (`attention_shared_plan`; -1 = empty place), tile_slot / tile_pfx int32
    [n_tiles], tail_len int32 [R], all on the device. max_pfx (default S): the largest tile_pfx (longer ones are clipped).
    A row with tail_len <= 0 comes out as zeros, a slot outside the cache as NaN rows; rows no tile names are not written."""
    assert q.dtype == k_tail.dtype == v_tail.dtype == k_cache.dtype == v_cache.dtype == torch.bfloat16
    assert q.dim() == 3 and k_tail.dim() == 4 and k_cache.dim() == 4
    R, H, D = q.shape
    T, Hkv = k_tail.shape[1], k_tail.shape[2]
    n_slots, S = k_cache.shape[0], k_cache.shape[1]
    assert D == 128, f"attention_shared: head dim {D} (128 only)"
    assert Hkv > 0 and H % Hkv == 0 and H // Hkv <= ATTN_SHARED_MAX_GROUP, f"attention_shared: {H} heads over {Hkv} KV heads"
    cpt = 16 // (H // Hkv)
    assert R >= 1 and T >= 1 and k_tail.shape == (R, T, Hkv, D) and v_tail.shape == k_tail.shape and k_tail.stride() == v_tail.stride()
    assert k_cache.shape == (n_slots, S, Hkv, D) and v_cache.shape == k_cache.shape and k_cache.stride() == v_cache.stride() and n_slots >= 1
    if out is None:
        out = torch.empty(R, H, D, dtype=torch.bfloat16, device=q.device)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    assert all(t.stride(-1) == 1 for t in (q, k_tail, v_tail, k_cache, v_cache, out))
    n_tiles = tile_rows.shape[0]
    assert n_tiles >= 1 and tile_rows.shape == (n_tiles, cpt), f"attention_shared: tile table {tuple(tile_rows.shape)} ([n_tiles, {cpt}])"
    for t, n in ((tile_rows, n_tiles * cpt), (tile_slot, n_tiles), (tile_pfx, n_tiles), (tail_len, R)):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n and t.device == q.device
    max_pfx = S if max_pfx is None else int(max_pfx)
    assert 0 <= max_pfx <= S, f"attention_shared: max_pfx={max_pfx} outside the cache's {S} rows per slot"
    rc = _lib.lib().ina_attention_shared(q.data_ptr(), q.stride(0), q.stride(1), out.data_ptr(), out.stride(0), out.stride(1), k_cache.data_ptr(),
                                         v_cache.data_ptr(), k_cache.stride(0), k_cache.stride(1), k_cache.stride(2), n_slots, k_tail.data_ptr(),
                                         v_tail.data_ptr(), k_tail.stride(0), k_tail.stride(1), k_tail.stride(2), T, tile_rows.data_ptr(),
                                         tile_slot.data_ptr(), tile_pfx.data_ptr(), tail_len.data_ptr(), n_tiles, R, H, Hkv, D, max_pfx,
                                         float(scale) if scale is not None else float(D) ** -0.5, _stream())
    _lib.check(rc, "attention_shared")
    return out


def drop_params(p: float, seed: int):
    """(seed, threshold, scale) of the counter-based dropout mask: keep iff hash(seed, index) >= p * 2^32, kept values scaled by 1 / (1 - p)."""
    assert 0.0 < p < 1.0
    return seed & 0xFFFFFFFF, max(1, min(0xFFFFFFFF, int(p * 4294967296.0))), 1.0 / (1.0 - p)


def _rowmap(m) -> _lib.RowMap:
    r = _lib.RowMap()
    if m is not None:
        r.seg_len, r.seg_stride, r.off = int(m[0]), int(m[1]), int(m[2])
    return r


def norm(x: torch.Tensor, gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None,
         eps: float = 1e-5, rms: bool = False, mod_scale: Optional[torch.Tensor] = None,
         gate: Optional[torch.Tensor] = None, base: Optional[torch.Tensor] = None, mod_div: int = 1,
         pos: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
         out32: Optional[torch.Tensor] = None, rows: Optional[int] = None, in_map=None, out_map=None,
         out2: Optional[torch.Tensor] = None, gamma2: Optional[torch.Tensor] = None, mod_scale2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm / RMSNorm over the last dim of x (bf16 or f32) -> out (bf16) and/or out32 (f32).

    t = norm(x) * gamma + beta; t *= 1 + mod_scale[r // mod_div]; t *= tanh(gate[r // mod_div]); t += base[r]; t += pos[r % len(pos)].
    in_map / out_map = (seg_len, seg_stride, off) gather / scatter logical rows; `rows` = number of logical rows (default: all of x).
    out2 (bf16): chained pre-norm of the produced row, out2 = norm(t) * gamma2 * (1 + mod_scale2[r // mod_div]) (same rms / eps).
    """
    assert x.dtype in _DT
    x2 = _as2d(x)
    Cdim = x2.shape[1]
    if rows is None:
        rows = x2.shape[0]
    if out is None and out32 is None:
        out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    a = NormArgs()
    a.X, a.x_dtype, a.ldx = x2.data_ptr(), _DT[x2.dtype], x2.stride(0)
    a.rows, a.C = rows, Cdim
    if out is not None:
        y2 = _as2d(out)
        assert y2.dtype == torch.bfloat16 and y2.shape[1] == Cdim
        a.Y, a.ldy = y2.data_ptr(), y2.stride(0)
    if out32 is not None:
        z2 = _as2d(out32)
        assert z2.dtype == torch.float32 and z2.shape[1] == Cdim
        a.Y32, a.ldy32 = z2.data_ptr(), z2.stride(0)
    a.gamma, a.beta = _ptr(_f32(gamma)), _ptr(_f32(beta))
    if mod_scale is not None:
        assert mod_scale.dtype == torch.float32 and mod_scale.stride(-1) == 1
        a.mod_scale, a.mod_ld = mod_scale.data_ptr(), mod_scale.stride(0)
    if gate is not None:
        assert gate.dtype == torch.float32 and gate.stride(-1) == 1
        a.gate, a.mod_ld = gate.data_ptr(), gate.stride(0)
        if mod_scale is not None:
            assert mod_scale.stride(0) == gate.stride(0)
    if base is not None:
        g2 = _as2d(base)
        a.G, a.ldg, a.g_dtype = g2.data_ptr(), g2.stride(0), _DT[g2.dtype]
    if pos is not None:
        assert pos.dtype == torch.float32 and pos.is_contiguous() and pos.shape[-1] == Cdim
        a.P, a.p_mod = pos.data_ptr(), pos.numel() // Cdim
    if out2 is not None:
        w2 = _as2d(out2)
        assert w2.dtype == torch.bfloat16 and w2.shape[1] == Cdim
        a.Y2, a.ldy2, a.gamma2 = w2.data_ptr(), w2.stride(0), _ptr(_f32(gamma2))
        if mod_scale2 is not None:
            assert mod_scale2.dtype == torch.float32 and mod_scale2.stride(-1) == 1 and (a.mod_ld in (0, mod_scale2.stride(0)))
            a.mod_scale2, a.mod_ld = mod_scale2.data_ptr(), mod_scale2.stride(0)
    a.in_map, a.out_map = _rowmap(in_map), _rowmap(out_map)
    a.mod_div = mod_div
    a.rms = 1 if rms else 0
    a.eps = eps
    _lib.check(_lib.lib().ina_norm_bf16(C.byref(a), _stream()), "norm_bf16")
    return out if out is not None else out32


def patchify(img: torch.Tensor, out: torch.Tensor, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), ps: int = 14) -> torch.Tensor:
    """img [n, H, W, C] (f32|bf16, C in 1, 3, 4, 6, 7) -> out bf16 [n * (H/ps) * (W/ps), ldo] im2col rows (k = c*ps*ps + y*ps + x; C = 1 is
    replicated to 3 channels; C > 3 takes mean 0 / std 1 only)."""
    assert img.is_contiguous() and img.dim() == 4 and out.dtype == torch.bfloat16 and out.stride(1) == 1
    a = _lib.PatchifyArgs()
    a.img, a.out = img.data_ptr(), out.data_ptr()
    for i in range(3):
        a.mean[i], a.inv_std[i] = float(mean[i]), 1.0 / float(std[i])
    a.n, a.H, a.W, a.C = img.shape
    assert out.shape[0] == a.n * (a.H // ps) * (a.W // ps)
    a.ps, a.ldo, a.in_dtype = ps, out.stride(0), _DT[img.dtype]
    _lib.check(_lib.lib().ina_patchify(C.byref(a), _stream()), "patchify")
    return out


def embed3(x: Optional[torch.Tensor], w: Optional[torch.Tensor], bias: Optional[torch.Tensor], out: torch.Tensor,
           pos: Optional[torch.Tensor] = None, rows: Optional[int] = None, out_map=None, x_div: int = 1) -> torch.Tensor:
    """out[out_map(r)] = w @ x[r // x_div] + bias + pos[r % len(pos)]  (nn.Linear(3, C); x None = table fill)."""
    o2 = _as2d(out)
    a = _lib.Embed3Args()
    if x is not None:
        assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] == 3 and w is not None
        a.X = x.data_ptr()
        if rows is None:
            rows = (x.numel() // 3) * x_div
    if w is not None:
        assert w.dtype == torch.float32 and w.is_contiguous() and w.shape == (o2.shape[1], 3)
        a.W = w.data_ptr()
    a.b = _ptr(_f32(bias))
    if pos is not None:
        assert pos.dtype == torch.float32 and pos.is_contiguous()
        a.P, a.p_mod = pos.data_ptr(), pos.numel() // o2.shape[1]
    assert rows is not None
    a.Y, a.ldy, a.out_dtype = o2.data_ptr(), o2.stride(0), _DT[o2.dtype]
    a.rows, a.C, a.x_div = rows, o2.shape[1], x_div
    a.out_map = _rowmap(out_map)
    _lib.check(_lib.lib().ina_embed3(C.byref(a), _stream()), "embed3")
    return out


def kv_copy(layer_base: torch.Tensor, seq: torch.Tensor, engine_rows: int, row_bytes: int, max_rows: int, to_engine: bool) -> None:
    """row ranges of a KV cache between engine cache slots and caller tensors, every layer and sequence in one launch (bit copy).
    layer_base: int64 [layers] on the device = address of each layer's cache (engine_rows rows of row_bytes bytes); seq: int64 [n, 4]
    on the device = (caller address of layer 0's first row, caller layer stride in bytes, first engine row, rows) per sequence.
    to_engine False: engine -> caller (export), True: caller -> engine (import). The caller checks the caller-side ranges."""
    assert layer_base.dtype == seq.dtype == torch.int64 and layer_base.is_contiguous() and seq.is_contiguous() and seq.dim() == 2 and seq.shape[1] == 4
    rc = _lib.lib().ina_kv_copy(int(bool(to_engine)), layer_base.data_ptr(), layer_base.numel(), seq.data_ptr(), seq.shape[0], int(engine_rows),
                                int(row_bytes), int(max_rows), _stream())
    _lib.check(rc, "kv_copy")


def memory_gather(out: torch.Tensor, ring: torch.Tensor, fresh: torch.Tensor, blank: torch.Tensor, pe: torch.Tensor, env: torch.Tensor,
                  head: torch.Tensor, count: torch.Tensor, stride: int = 1) -> torch.Tensor:
    """visual-memory token rows of n stepped envs from the per-env ring of cached frame tokens, and the new frame into the ring (one launch).
    out bf16 [n, rows_per_env >= M * ntok, C] (contiguous rows): out[i, j * ntok + p] = bf16(src + pe[j * ntok + p]); ring f32 [max_envs, depth,
    ntok, C] with depth = (M - 1) * stride + 1; fresh f32 [n, ntok, C]; blank f32 [ntok, C]; pe f32 [M * ntok, C]; env / head / count int32 [n]
    on the device (include/internnav_amd.h: ina_memory_gather). The env ids of one launch must be distinct."""
    n, ntok, Cd = fresh.shape
    max_envs, depth = ring.shape[0], ring.shape[1]
    M = pe.shape[0] // ntok
    assert out.dtype == torch.bfloat16 and out.dim() == 3 and out.shape[0] == n and out.shape[2] == Cd and out.stride(2) == 1 and out.stride(1) == Cd
    assert out.shape[1] >= M * ntok and (n == 1 or out.stride(0) >= M * ntok * Cd)
    for t in (ring, fresh, blank, pe):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert ring.shape == (max_envs, depth, ntok, Cd) and blank.shape == (ntok, Cd) and pe.shape == (M * ntok, Cd) and depth == (M - 1) * stride + 1
    for t in (env, head, count):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n and t.device == out.device
    rc = _lib.lib().ina_memory_gather(out.data_ptr(), out.stride(0) if n > 1 else max(out.stride(0), M * ntok * Cd), ring.data_ptr(),
                                      fresh.data_ptr(), blank.data_ptr(), pe.data_ptr(), env.data_ptr(), head.data_ptr(), count.data_ptr(), n,
                                      max_envs, M, ntok, Cd, depth, stride, _stream())
    _lib.check(rc, "memory_gather")
    return out


def traj_actions(traj: torch.Tensor, n_env: int, max_actions: int = 4, traj_out: Optional[torch.Tensor] = None,
                 scale_in_place: bool = False):
    """the action table of n_env envs from their sampled trajectories in one launch: what policy.traj_to_actions computes per env on the host
    (include/internnav_amd.h: ina_traj_actions). traj f32|bf16 [n_env * S, T, 3] (generate_traj's layout, the S samples of an env contiguous) or
    [n_env, S, T, 3]. Returns (actions int32 [n_env, max_actions] = the first max_actions entries of each env's list, zero-padded;
    count int32 [n_env]), both on the device - nothing here waits for the GPU. traj_out f64 [n_env, T + 1, 2] receives the mean trajectory;
    scale_in_place writes x / 4, y / 4 back into traj as the host function does."""
    assert traj.is_cuda and traj.is_contiguous() and traj.dtype in _DT and traj.dim() in (3, 4) and traj.shape[-1] == 3
    rows = traj.shape[0] if traj.dim() == 3 else traj.shape[0] * traj.shape[1]
    assert n_env >= 1 and rows % n_env == 0 and (traj.dim() == 3 or traj.shape[0] == n_env), (tuple(traj.shape), n_env)
    S, T = rows // n_env, traj.shape[-2]
    if traj_out is not None:
        assert traj_out.dtype == torch.float64 and traj_out.is_contiguous() and traj_out.shape == (n_env, T + 1, 2) and traj_out.device == traj.device
    actions = torch.empty((n_env, max(int(max_actions), 0)), dtype=torch.int32, device=traj.device)
    count = torch.empty((n_env,), dtype=torch.int32, device=traj.device)
    rc = _lib.lib().ina_traj_actions(traj.data_ptr(), _DT[traj.dtype], n_env, S, T, actions.data_ptr(), int(max_actions), count.data_ptr(),
                                     _ptr(traj_out), int(bool(scale_in_place)), _stream())
    _lib.check(rc, "traj_actions")
    return actions, count


def goal_slots(out: torch.Tensor, L: int, kind: torch.Tensor, row: torch.Tensor, pos: Optional[torch.Tensor] = None, slot0: int = 1,
               nslots: int = 3, embed: Optional[torch.Tensor] = None, point=None, image=None, pixel=None) -> torch.Tensor:
    """goal embedding e of every env b by its kind (0 none: 0, 1 point: w @ point[row[b]] + bias, 2 image / 3 pixel: w @ mean of the
    tower tokens tok[row[b]*ntok : (row[b]+1)*ntok] + bias) -> out[b*L + slot0 + j] = e + pos[slot0 + j] (j < nslots); embed f32 [B, D]
    receives e. kind / row: int32 [B] on the device. point = (x f32 [n, 3], w f32 [D, 3], bias f32 [D]); image / pixel = (tok f32
    [n * ntok, E], w f32 [D, E], bias f32 [D], ntok); n = rows of that input (0 or None: the kind is absent)."""
    o2 = _as2d(out)
    B, D = kind.numel(), o2.shape[1]
    assert kind.dtype == row.dtype == torch.int32 and kind.is_contiguous() and row.is_contiguous() and row.numel() == B
    assert o2.shape[0] >= B * L and (embed is None or (embed.dtype == torch.float32 and embed.is_contiguous() and embed.numel() >= B * D))
    assert pos is None or (pos.dtype == torch.float32 and pos.is_contiguous() and pos.shape[-1] == D and pos.numel() >= (slot0 + nslots) * D)
    px, pw, pb, n_point = None, None, None, 0
    if point is not None:
        x, w, b = point
        assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] == 3 and w.shape == (D, 3)
        px, pw, pb, n_point = x, _f32(w), _f32(b), x.numel() // 3
    towers, ntok, E = [], 0, 0
    for t in (image, pixel):
        if t is None:
            towers.append((None, None, None, 0))
            continue
        tok, w, b, nt = t
        assert tok.dtype == torch.float32 and tok.is_contiguous() and tok.dim() == 2 and tok.shape[0] % nt == 0 and w.shape == (D, tok.shape[1])
        assert (ntok, E) in ((0, 0), (nt, tok.shape[1])), "image and pixel towers must agree on tokens per frame and width"
        ntok, E = nt, tok.shape[1]
        towers.append((tok, _f32(w), _f32(b), tok.shape[0] // nt))
    (it, iw, ib, n_image), (qt, qw, qb, n_pixel) = towers
    rc = _lib.lib().ina_goal_slots(o2.data_ptr(), o2.stride(0), _DT[o2.dtype], L, slot0, nslots, _ptr(pos), B, D, kind.data_ptr(),
                                   row.data_ptr(), _ptr(embed), _ptr(px), n_point, _ptr(pw), _ptr(pb), _ptr(it), n_image, _ptr(iw),
                                   _ptr(ib), _ptr(qt), n_pixel, _ptr(qw), _ptr(qb), ntok, E, _stream())
    _lib.check(rc, "goal_slots")
    return out


def head3(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, gamma=None, beta=None, eps: float = 1e-5, mode: int = 0,
          sample: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, eps_out: Optional[torch.Tensor] = None,
          coef=(0.0, 0.0, 0.0, 0.0, 0.0), clip: float = 1.0, mod_scale: Optional[torch.Tensor] = None, mod_div: int = 1):
    """final norm + Linear(C,3) + sampler update (mode 0: write eps_out; 1: DDPM step; 2: Euler step) on f32 samples [rows,3]."""
    x2 = _as2d(x)
    a = _lib.Head3Args()
    a.X, a.ldx, a.x_dtype = x2.data_ptr(), x2.stride(0), _DT[x2.dtype]
    a.rows, a.C = x2.shape
    a.gamma, a.beta = _ptr(_f32(gamma)), _ptr(_f32(beta))
    assert w.dtype == torch.float32 and w.is_contiguous() and w.shape == (3, a.C) and b.dtype == torch.float32
    a.W, a.b = w.data_ptr(), b.data_ptr()
    for t in (sample, noise, eps_out):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == a.rows * 3)
    a.sample, a.noise, a.eps_out = _ptr(sample), _ptr(noise), _ptr(eps_out)
    for i in range(5):
        a.coef[i] = float(coef[i])
    a.clip, a.eps, a.mode = clip, eps, mode
    if mod_scale is not None:
        assert mod_scale.dtype == torch.float32 and mod_scale.stride(-1) == 1
        a.mod_scale, a.mod_ld = mod_scale.data_ptr(), mod_scale.stride(0)
    a.mod_div = mod_div
    _lib.check(_lib.lib().ina_head3(C.byref(a), _stream()), "head3")


def seqpool_head(x: torch.Tensor, T: int, gamma, beta, w: torch.Tensor, b: torch.Tensor, out: torch.Tensor, eps: float = 1e-5):
    """out[s] = w . mean_t(LayerNorm(x[s*T + t])) + b."""
    x2 = _as2d(x)
    a = _lib.SeqpoolArgs()
    a.X, a.ldx, a.x_dtype = x2.data_ptr(), x2.stride(0), _DT[x2.dtype]
    a.nseq, a.T, a.C = x2.shape[0] // T, T, x2.shape[1]
    a.gamma, a.beta, a.w, a.b = _ptr(_f32(gamma)), _ptr(_f32(beta)), _f32(w.reshape(-1)).data_ptr(), _f32(b).data_ptr()
    assert out.dtype == torch.float32 and out.numel() == a.nseq
    a.out, a.eps = out.data_ptr(), eps
    _lib.check(_lib.lib().ina_seqpool_head(C.byref(a), _stream()), "seqpool_head")
    return out


def select_traj(critic: torch.Tensor, sample: torch.Tensor, neg: torch.Tensor, pos: torch.Tensor, k: int = 8, scale: float = 0.25):
    """critic [B,S], sample [B,S,T,3] -> neg/pos [B,k,T,3] cumulative trajectories of the k lowest / highest critic samples."""
    B, S, T, _ = sample.shape
    for t in (critic, sample, neg, pos):
        assert t.dtype == torch.float32 and t.is_contiguous()
    a = _lib.SelectArgs()
    a.critic, a.sample, a.neg, a.pos = critic.data_ptr(), sample.data_ptr(), neg.data_ptr(), pos.data_ptr()
    a.scale, a.B, a.S, a.T, a.k = scale, B, S, T, k
    _lib.check(_lib.lib().ina_select_traj(C.byref(a), _stream()), "select_traj")


def pool_act(x: torch.Tensor, out: torch.Tensor, T: int = 1, pos: Optional[torch.Tensor] = None, act=None) -> torch.Tensor:
    """out[s] = act(mean_t x[s*T + t] + pos[s % len(pos)]); x bf16|f32 [nseq*T, C] -> out bf16|f32 [nseq, C]."""
    x2, o2 = _as2d(x), _as2d(out)
    a = _lib.PoolActArgs()
    a.X, a.ldx, a.x_dtype = x2.data_ptr(), x2.stride(0), _DT[x2.dtype]
    a.Y, a.ldy, a.out_dtype = o2.data_ptr(), o2.stride(0), _DT[o2.dtype]
    a.nseq, a.T, a.C = x2.shape[0] // T, T, x2.shape[1]
    assert o2.shape == (a.nseq, a.C)
    if pos is not None:
        assert pos.dtype == torch.float32 and pos.is_contiguous() and pos.shape[-1] == a.C
        a.P, a.p_mod = pos.data_ptr(), pos.numel() // a.C
    a.act = ACT[act]
    _lib.check(_lib.lib().ina_pool_act(C.byref(a), _stream()), "pool_act")
    return out


def gather_rows(x: torch.Tensor, out: torch.Tensor, src: Optional[torch.Tensor] = None, dst: Optional[torch.Tensor] = None,
                rows: Optional[int] = None) -> torch.Tensor:
    """out[dst[r] or r] = x[src[r] or r] (2-D tensors of equal dtype / width, int32 index vectors on the device)."""
    assert x.dim() == 2 and out.dim() == 2 and x.dtype == out.dtype and x.shape[1] == out.shape[1] and x.stride(1) == 1 and out.stride(1) == 1
    a = _lib.GatherArgs()
    es = x.element_size()
    a.X, a.Y = x.data_ptr(), out.data_ptr()
    a.ldx_bytes, a.ldy_bytes, a.row_bytes = x.stride(0) * es, out.stride(0) * es, x.shape[1] * es
    for t in (src, dst):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous())
    a.src, a.dst = _ptr(src), _ptr(dst)
    a.rows = rows if rows is not None else (src.numel() if src is not None else (dst.numel() if dst is not None else x.shape[0]))
    _lib.check(_lib.lib().ina_gather_rows(C.byref(a), _stream()), "gather_rows")
    return out


def rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, heads: int, D: int, col0: int = 0, rows: Optional[int] = None,
         row_map=None, tab: Optional[torch.Tensor] = None, kv_out: Optional[torch.Tensor] = None, kv_dst: Optional[torch.Tensor] = None,
         kv_head0: int = 0, v_heads: int = 0) -> torch.Tensor:
    """in-place rotary embedding on `heads` heads of width D at columns [col0, col0 + heads*D) of bf16 rows x[row_map(r)].
    kv_out (fused KV-cache append of a decoder layer): heads [kv_head0, heads) are key heads - their rotated values go to cache row
    kv_dst[r] of kv_out (not back into x) together with the v_heads value heads that follow them in x: one launch instead of rope +
    gather."""
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.stride(1) == 1
    assert cos.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous() and cos.shape[-1] == D
    a = _lib.RopeArgs()
    a.X, a.cos, a.sin, a.tab = x.data_ptr(), cos.data_ptr(), sin.data_ptr(), _ptr(tab)
    a.map = _rowmap(row_map)
    a.rows = rows if rows is not None else x.shape[0]
    a.heads, a.D, a.ldx, a.col0 = heads, D, x.stride(0), col0
    if kv_out is not None:
        assert kv_out.dtype == torch.bfloat16 and kv_out.stride(1) == 1 and kv_dst.dtype == torch.int32 and kv_dst.is_contiguous()
        assert kv_out.shape[1] >= (heads - kv_head0 + v_heads) * D
        a.KV, a.kv_dst, a.kv_head0, a.v_heads, a.ldkv = kv_out.data_ptr(), kv_dst.data_ptr(), kv_head0, v_heads, kv_out.stride(0)
    _lib.check(_lib.lib().ina_rope_bf16(C.byref(a), _stream()), "rope_bf16")
    return x


def mrope_table(pos: torch.Tensor, inv_freq: torch.Tensor, axis_of: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor):
    """pos int32 [3, n] -> cos/sin f32 [n, D] of the multimodal rope (section axis per frequency in axis_of int32 [D/2])."""
    assert pos.dtype == torch.int32 and pos.is_contiguous() and pos.shape[0] == 3
    n, D = pos.shape[1], cos.shape[-1]
    assert cos.is_contiguous() and sin.is_contiguous() and cos.numel() >= n * D and inv_freq.numel() == D // 2 and axis_of.dtype == torch.int32
    a = _lib.MropeTableArgs()
    a.pos, a.inv_freq, a.axis_of, a.cos, a.sin = pos.data_ptr(), _f32(inv_freq).data_ptr(), axis_of.data_ptr(), cos.data_ptr(), sin.data_ptr()
    a.n, a.D = n, D
    _lib.check(_lib.lib().ina_mrope_table(C.byref(a), _stream()), "mrope_table")


def argmax_rows(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[r] = argmax of f32 row r (first maximum), out int32 [rows]."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and out.dtype == torch.int32 and out.numel() == x.shape[0]
    a = _lib.ArgmaxArgs()
    a.X, a.out, a.rows, a.n, a.ldx = x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], x.stride(0)
    _lib.check(_lib.lib().ina_argmax_rows(C.byref(a), _stream()), "argmax_rows")
    return out


def token_seen_set(seen: torch.Tensor, ids: torch.Tensor, lens: torch.Tensor, n: int) -> torch.Tensor:
    """seen[r] (uint32 [rows, ld_words], token t = bit t & 31 of word t >> 5) = the set of ids[r, :lens[r]] inside [0, n):
    the tokens a repetition penalty acts on. Stale bits are cleared in the same launch; ids int32 [rows, ld_ids], lens int32 [rows]."""
    assert seen.dtype in (torch.uint32, torch.int32) and seen.dim() == 2 and seen.stride(1) == 1 and ids.dtype == torch.int32 and ids.dim() == 2 and ids.stride(1) == 1
    rows = ids.shape[0]
    assert lens.dtype == torch.int32 and lens.is_contiguous() and lens.numel() == rows and seen.shape[0] >= rows and seen.shape[1] * 32 >= n
    rc = _lib.lib().ina_token_seen_set(seen.data_ptr(), seen.stride(0), ids.data_ptr(), ids.stride(0), lens.data_ptr(), rows, int(n), _stream())
    _lib.check(rc, "token_seen_set")
    return seen


def argmax_penalty_rows(x: torch.Tensor, seen: torch.Tensor, penalty: float, out: torch.Tensor, mark: bool = True) -> torch.Tensor:
    """out[r] = argmax_rows of the repetition-penalised f32 row r (HF RepetitionPenaltyLogitsProcessor: a seen token's logit is divided by the
    penalty when >= 0, multiplied when < 0); x is not modified. mark: the chosen token's bit is set in seen[r] by the same launch."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and out.dtype == torch.int32 and out.numel() == x.shape[0]
    assert seen.dtype in (torch.uint32, torch.int32) and seen.dim() == 2 and seen.stride(1) == 1 and seen.shape[0] >= x.shape[0] and seen.shape[1] * 32 >= x.shape[1]
    rc = _lib.lib().ina_argmax_penalty_rows(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], seen.data_ptr(), seen.stride(0), float(penalty),
                                            int(bool(mark)), out.data_ptr(), _stream())
    _lib.check(rc, "argmax_penalty_rows")
    return out


def logprob_rows(x: torch.Tensor, tok: torch.Tensor, logprob: torch.Tensor, margin: Optional[torch.Tensor] = None, seen: Optional[torch.Tensor] = None,
                 penalty: float = 1.0, mark: bool = False, target: Optional[torch.Tensor] = None) -> torch.Tensor:
    """logprob[r] = log_softmax(y[r])[tok[r]] of the f32 rows of x (not modified), y = x or, with `seen`, the repetition-penalised row of
    argmax_penalty_rows. target None: tok[r] = the selection of argmax_rows / argmax_penalty_rows over y (bit-equal; mark sets the chosen bit in
    seen[r]); target int32 [rows]: tok[r] = target[r] (teacher forcing; a target outside [0, n) is ignored: logprob 0, margin 0).
    margin[r] (optional) = y[tok] - the largest y at any other index. tok int32 [rows], logprob / margin f32 [rows], contiguous."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    rows, n = x.shape
    assert tok.dtype == torch.int32 and tok.numel() == rows and tok.is_contiguous()
    for t in (logprob, margin):
        assert t is None or (t.dtype == torch.float32 and t.numel() == rows and t.is_contiguous())
    if seen is not None:
        assert seen.dtype in (torch.uint32, torch.int32) and seen.dim() == 2 and seen.stride(1) == 1 and seen.shape[0] >= rows and seen.shape[1] * 32 >= n
    if target is not None:
        assert target.dtype == torch.int32 and target.numel() == rows and target.is_contiguous()
    rc = _lib.lib().ina_logprob_rows(x.data_ptr(), x.stride(0), rows, n, seen.data_ptr() if seen is not None else None,
                                     seen.stride(0) if seen is not None else 0, float(penalty), int(bool(mark)),
                                     target.data_ptr() if target is not None else None, tok.data_ptr(), logprob.data_ptr(),
                                     margin.data_ptr() if margin is not None else None, _stream())
    _lib.check(rc, "logprob_rows")
    return logprob


def sample_rows(x: torch.Tensor, u: torch.Tensor, tok: torch.Tensor, logprob: torch.Tensor, temperature: float = 1.0, top_k: int = 0,
                top_p: float = 1.0, seen: Optional[torch.Tensor] = None, penalty: float = 1.0, mark: bool = False, src: Optional[torch.Tensor] = None,
                n_kept: Optional[torch.Tensor] = None, thr: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One sampling step of HF generate(do_sample=True) per output row, in one launch: y = the f32 row of x (not modified) or, with `seen`, its
    repetition-penalised row; z = y / temperature; top-k (0 = off, ties at the k-th value stay); top-p over what top-k kept (1 = off; a value
    stays iff the softmax mass at or below it is > 1 - top_p, the maximum always); tok[r] = the first kept id whose inclusive cumulative
    probability exceeds u[r] (f32 uniforms in [0, 1) drawn by the caller - nothing random happens on the device); logprob[r] = the log of
    the drawn token's renormalised probability. src int32 [rows]: output row r reads x[src[r]] (K draws from one logits row; an entry
    outside the rows of x gives tok 0 / logprob NaN); without it rows = x.shape[0]. mark sets the drawn bit in seen[r]. n_kept int32 /
    thr f32 [rows] (optional): the size of the kept set and its smallest value. Deterministic: the same inputs give the same bits."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    x_rows, n = x.shape
    rows = x_rows if src is None else src.numel()
    assert tok.dtype == torch.int32 and tok.numel() == rows and tok.is_contiguous()
    for t in (u, logprob, thr):
        assert t is None or (t.dtype == torch.float32 and t.numel() == rows and t.is_contiguous())
    assert n_kept is None or (n_kept.dtype == torch.int32 and n_kept.numel() == rows and n_kept.is_contiguous())
    assert src is None or (src.dtype == torch.int32 and src.is_contiguous())
    if seen is not None:
        assert seen.dtype in (torch.uint32, torch.int32) and seen.dim() == 2 and seen.stride(1) == 1 and seen.shape[0] >= rows and seen.shape[1] * 32 >= n
    p = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    rc = _lib.lib().ina_sample_rows(x.data_ptr(), x.stride(0), x_rows, rows, n, p(seen), seen.stride(0) if seen is not None else 0, float(penalty),
                                    int(bool(mark)), float(temperature), int(top_k), float(top_p), u.data_ptr(), p(src), tok.data_ptr(),
                                    logprob.data_ptr(), p(n_kept), p(thr), _stream())
    _lib.check(rc, "sample_rows")
    return tok


def automaton_mask_rows(x: torch.Tensor, tables, state_in: torch.Tensor, prev_tok: Optional[torch.Tensor], state_out: torch.Tensor) -> torch.Tensor:
    """Constrained decoding in front of a selection launch: per f32 row r of x (modified IN PLACE) advance the row's automaton state -
    s = state_in[r] without prev_tok, else next[state_in[r]][class(prev_tok[r])], or -1 when the state is outside the automaton, the token
    outside [0, n) or not allowed - write it to state_out[r], and set x[r, i] = -inf wherever class(i) is not allowed in s. Allowed entries are
    not written; a row whose s is outside the automaton is left as it is. tables: what TokenAutomaton.to(device) returns (token_class u8
    [vocab >= n], allow 32-bit [S, 8], next u8 [S, 256]). state_in / state_out int32 [rows], distinct buffers; prev_tok int32 [rows] or None."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    rows, n = x.shape
    cls, allow, nxt = tables.token_class, tables.allow, tables.next
    assert cls.dtype == torch.uint8 and cls.is_contiguous() and nxt.dtype == torch.uint8 and nxt.is_contiguous()
    S = nxt.numel() // 256
    assert allow.dtype in (torch.uint32, torch.int32) and allow.is_contiguous() and allow.numel() == S * 8 and nxt.numel() == S * 256
    for t in (state_in, prev_tok, state_out):
        assert t is None or (t.dtype == torch.int32 and t.numel() == rows and t.is_contiguous())
    if rows == 0:
        return x
    rc = _lib.lib().ina_automaton_mask_rows(x.data_ptr(), x.stride(0) if rows > 1 else max(x.stride(0), n), rows, n, cls.data_ptr(), cls.numel(),
                                            allow.data_ptr(), nxt.data_ptr(), S, state_in.data_ptr(), prev_tok.data_ptr() if prev_tok is not None else None,
                                            state_out.data_ptr(), _stream())
    _lib.check(rc, "automaton_mask_rows")
    return x


BEAM_MAX_CANDIDATES = 32      # M of beam_topm_rows / beam_step: max(2, 1 + n_eos) * num_beams
BEAM_EARLY = {False: 0, True: 1, "never": 2}


def beam_topm_rows(x: torch.Tensor, run_score: torch.Tensor, cand_score: torch.Tensor, cand_tok: torch.Tensor, seen: Optional[torch.Tensor] = None,
                   penalty: float = 1.0, src: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The candidates of one beam-search step per output row, in one launch: y = log_softmax of the f32 row of x (not modified), with `seen`
    the repetition penalty ON y (HF's beam search processes log-probabilities: seen ? (y < 0 ? y * p : y / p) : y), acc = y + run_score[r];
    cand_score f32 / cand_tok int32 [rows, M] = the M best entries by (acc descending, token id ascending), M = cand_score.shape[1] in
    [2, min(32, n)]. src int32 [rows]: output row r reads x[src[r]] (an entry outside the rows of x: scores -inf, ids 0 .. M-1, no access).
    A NaN logit counts as -inf; -inf entries fill up in id order. Deterministic: the same inputs give the same bits."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    x_rows, n = x.shape
    rows = x_rows if src is None else src.numel()
    assert cand_score.dtype == torch.float32 and cand_score.dim() == 2 and cand_score.is_contiguous() and cand_score.shape[0] == rows
    assert cand_tok.dtype == torch.int32 and cand_tok.shape == cand_score.shape and cand_tok.is_contiguous()
    assert run_score.dtype == torch.float32 and run_score.numel() == rows and run_score.is_contiguous()
    assert src is None or (src.dtype == torch.int32 and src.is_contiguous())
    if seen is not None:
        assert seen.dtype in (torch.uint32, torch.int32) and seen.dim() == 2 and seen.stride(1) == 1 and seen.shape[0] >= rows and seen.shape[1] * 32 >= n
    rc = _lib.lib().ina_beam_topm_rows(x.data_ptr(), x.stride(0) if x_rows > 1 else max(x.stride(0), n), x_rows, rows, n,
                                       seen.data_ptr() if seen is not None else None, seen.stride(0) if seen is not None else 0, float(penalty),
                                       run_score.data_ptr(), src.data_ptr() if src is not None else None, cand_score.shape[1], cand_score.data_ptr(),
                                       cand_tok.data_ptr(), _stream())
    _lib.check(rc, "beam_topm_rows")
    return cand_score


def beam_step(cand_score: torch.Tensor, cand_tok: torch.Tensor, st, step: int, max_new_tokens: int, length_penalty: float = 1.0, early_stopping=False,
              flip: Optional[int] = None) -> None:
    """The bookkeeping of one beam-search step, one workgroup per prompt (include/internnav_amd.h, tests/beam_ref.py): merges the K rows' candidate
    lists of every prompt, applies transformers' rules in its fp32 arithmetic and writes the next running set and the finished set into `st`,
    a namespace of device buffers: K, eos int32 [n_eos] (or None), run_score f32 / next_tok / parent int32 [B * K], hist int32 and ts f32
    [2, B * K, T] (ping-pong pairs, a tensor or two tensors: this step reads half flip, default step & 1, and writes the other), fin_tok int32 / fin_ts f32 [B * K, T],
    fin_score f32 / fin_len / fin_flag int32 [B * K], heur / done int32 [B]. step 0 initialises the prompts; a done prompt is frozen."""
    R, M = cand_score.shape
    K = int(st.K)
    assert R % K == 0 and cand_score.dtype == torch.float32 and cand_score.is_contiguous()
    assert cand_tok.dtype == torch.int32 and cand_tok.shape == cand_score.shape and cand_tok.is_contiguous()
    B, T = R // K, st.hist[0].shape[1]
    for t, dt, shape in ((st.run_score, torch.float32, (R,)), (st.next_tok, torch.int32, (R,)), (st.parent, torch.int32, (R,)),
                         (st.hist[0], torch.int32, (R, T)), (st.hist[1], torch.int32, (R, T)), (st.ts[0], torch.float32, (R, T)),
                         (st.ts[1], torch.float32, (R, T)), (st.fin_tok, torch.int32, (R, T)),
                         (st.fin_ts, torch.float32, (R, T)), (st.fin_score, torch.float32, (R,)), (st.fin_len, torch.int32, (R,)),
                         (st.fin_flag, torch.int32, (R,)), (st.heur, torch.int32, (B,)), (st.done, torch.int32, (B,))):
        assert t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous(), (t.dtype, tuple(t.shape), dt, shape)
    eos = getattr(st, "eos", None)
    assert eos is None or (eos.dtype == torch.int32 and eos.is_contiguous())
    f = (step & 1) if flip is None else int(flip)
    rc = _lib.lib().ina_beam_step(cand_score.data_ptr(), cand_tok.data_ptr(), B, K, M, T, int(step), int(max_new_tokens), float(length_penalty),
                                  BEAM_EARLY[early_stopping], eos.data_ptr() if eos is not None else None, eos.numel() if eos is not None else 0,
                                  st.run_score.data_ptr(), st.next_tok.data_ptr(), st.parent.data_ptr(), st.hist[f].data_ptr(), st.hist[1 - f].data_ptr(),
                                  st.ts[f].data_ptr(), st.ts[1 - f].data_ptr(), st.fin_tok.data_ptr(), st.fin_ts.data_ptr(), st.fin_score.data_ptr(),
                                  st.fin_len.data_ptr(), st.fin_flag.data_ptr(), st.heur.data_ptr(), st.done.data_ptr(), _stream())
    _lib.check(rc, "beam_step")


def beam_reorder(parent: torch.Tensor, src_base: Optional[torch.Tensor] = None, dst_base: Optional[torch.Tensor] = None, T: int = 1, t: int = 0,
                 row_bytes: int = 16, seen_src: Optional[torch.Tensor] = None, seen_dst: Optional[torch.Tensor] = None,
                 next_tok: Optional[torch.Tensor] = None, n: int = 0, state_src: Optional[torch.Tensor] = None,
                 state_dst: Optional[torch.Tensor] = None) -> None:
    """Re-parents the per-row state of a beam search in front of the next pass, one launch: for every layer the first t rows of row r's T-row tail
    in the destination set come from row parent[r] of the source set (src_base / dst_base: int64 device tables of the layers' tail addresses,
    two sets that do not overlap); seen_dst[r] = seen_src[parent[r]] | bit next_tok[r] (n = vocabulary); state_dst[r] = state_src[parent[r]].
    A parent outside [0, rows) leaves its row unwritten. Bit copies."""
    rows = parent.numel()
    assert parent.dtype == torch.int32 and parent.is_contiguous()
    n_layers = 0 if src_base is None else src_base.numel()
    if n_layers:
        assert src_base.dtype == torch.int64 and dst_base.dtype == torch.int64 and dst_base.numel() == n_layers and src_base.is_contiguous() and dst_base.is_contiguous()
    ld = 0
    if seen_src is not None:
        ld = seen_src.shape[1]
        for s in (seen_src, seen_dst):
            assert s.dtype in (torch.uint32, torch.int32) and s.dim() == 2 and s.is_contiguous() and s.shape[0] >= rows and s.shape[1] == ld
        assert next_tok.dtype == torch.int32 and next_tok.is_contiguous() and next_tok.numel() >= rows
    for s in (state_src, state_dst):
        assert s is None or (s.dtype == torch.int32 and s.is_contiguous() and s.numel() >= rows)
    p = lambda v: v.data_ptr() if v is not None else None      # noqa: E731
    rc = _lib.lib().ina_beam_reorder(p(src_base), p(dst_base), n_layers, parent.data_ptr(), rows, int(T), int(t), int(row_bytes), p(seen_src), p(seen_dst),
                                     ld, p(next_tok), int(n), p(state_src), p(state_dst), _stream())
    _lib.check(rc, "beam_reorder")


def logit_rules_rows(x: torch.Tensor, tables, col: int, hist: torch.Tensor, len0: torch.Tensor, prev_tok: Optional[torch.Tensor] = None,
                     eos_first: Optional[torch.Tensor] = None, ld_hist: Optional[int] = None) -> torch.Tensor:
    """transformers' logits-processor keys in front of a selection launch (and behind automaton_mask_rows): per f32 row r of x (modified IN
    PLACE) at answer column `col` - append prev_tok[r] to the row's history (col > 0), add the finite sequence biases, store -inf over the
    n-gram, bad-word, EOS (col < eos_first[r]), suppress and begin-suppress bans, and at the forced column make the row -inf with 0.0 at the
    forced ids (contract: `ina_logit_rules_rows` in include/internnav_amd.h). tables: what CompiledRules.to(device) returns. hist int32
    [>= rows, hist_cap] (row stride ld_hist elements, default its own: a larger stride reads every K-th history), len0 int32 [rows] the
    rows' prompt lengths, prev_tok int32 [rows] (required behind column 0), eos_first int32 [rows] (default: the tables')."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    rows, n = x.shape
    assert hist.dtype == torch.int32 and hist.dim() == 2 and hist.stride(1) == 1
    ld = hist.stride(0) if ld_hist is None else int(ld_hist)
    assert (rows - 1) * ld + hist.shape[1] <= (hist.shape[0] - 1) * hist.stride(0) + hist.shape[1] or rows == 0, (rows, ld, tuple(hist.shape))
    eos_first = tables.eos_first if eos_first is None else eos_first
    for t in (len0, prev_tok, eos_first):
        assert t is None or (t.dtype == torch.int32 and t.numel() == rows and t.is_contiguous()), "len0 / prev_tok / eos_first: contiguous int32 [rows]"
    assert col == 0 or prev_tok is not None
    if rows == 0:
        return x
    p = lambda t: None if t is None else t.data_ptr()     # noqa: E731
    cnt = lambda t: 0 if t is None else t.numel()         # noqa: E731
    tb = tables
    rc = _lib.lib().ina_logit_rules_rows(x.data_ptr(), x.stride(0) if rows > 1 else max(x.stride(0), n), rows, n, int(col), hist.data_ptr(), ld, hist.shape[1],
                                         len0.data_ptr(), p(prev_tok), tb.ngram, p(tb.grp_tok), p(tb.grp_base), p(tb.grp_ptr), tb.n_bias, tb.n_groups,
                                         p(tb.seq_ptr), p(tb.seq_ids), p(tb.seq_bias), tb.n_seqs, tb.n_ids, p(tb.ban_tok), cnt(tb.ban_tok), p(tb.begin_tok),
                                         cnt(tb.begin_tok), p(tb.eos_tok), cnt(tb.eos_tok), p(eos_first), p(tb.forced_tok), cnt(tb.forced_tok),
                                         tb.forced_col, _stream())
    _lib.check(rc, "logit_rules_rows")
    return x


def dit_v2t(kv2: torch.Tensor, heads: int, v2t: torch.Tensor) -> torch.Tensor:
    """condition V of a NextDiT block -> the transposed key-permuted image dit_attention consumes.
    kv2 bf16 [envs, Lz, 2, heads, 64] (K | V as produced by the fused kv projection); v2t bf16 [envs, heads, 64, 64]."""
    envs, Lz = kv2.shape[0], kv2.shape[1]
    assert kv2.dtype == torch.bfloat16 and kv2.stride(-1) == 1 and v2t.dtype == torch.bfloat16 and v2t.is_contiguous()
    assert v2t.numel() >= envs * heads * 64 * 64
    v = kv2[:, :, 1]
    a = _lib.DitAttnArgs()
    a.X, a.V2T, a.V2T_src = None, v2t.data_ptr(), v.data_ptr()
    a.v2_bs, a.v2_rs = v.stride(0), v.stride(1)
    a.nseq, a.seq_per_env, a.T, a.heads, a.Lz = envs, 1, 1, heads, Lz
    a.ldx, a.ldo, a.k2_bs, a.k2_rs = 8, 8, 8, 8
    _lib.check(_lib.lib().ina_dit_attention(C.byref(a), _stream()), "dit_attention(v2t)")
    return v2t


def dit_attention(x: torch.Tensor, out: torch.Tensor, norms, kv2: torch.Tensor, v2t: torch.Tensor, head_gate: Optional[torch.Tensor],
                  T: int, seq_per_env: int, heads: int, eps: float = 1e-5, scale: Optional[float] = None,
                  stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """NextDiT attention stage in one launch: out = SDPA(LN(q1), LN(k1), v1) + tanh(gate) * SDPA(LN(q2), K2, V2).

    x bf16 [rows, 4*heads*64] = [q1 | k1 | v1 | q2] per token, rows = nseq * T; norms = ((g_q1, b_q1), (g_k1, b_k1), (g_q2, b_q2)) f32;
    kv2 bf16 [envs, Lz, 2, heads, 64]; v2t from dit_v2t(kv2); out bf16 [rows, heads*64]. stats f32 [rows, 4, 2]: (mean, rstd) of the four
    segments of every x row from the producer (dit_rowchain(seg_stats=)); None = the kernel computes them itself."""
    D = heads * 64
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] == 4 * D and x.stride(1) == 1 and x.shape[0] % T == 0
    assert out.dtype == torch.bfloat16 and out.shape == (x.shape[0], D) and out.stride(1) == 1
    nseq = x.shape[0] // T
    assert kv2.shape[0] * seq_per_env >= nseq and kv2.stride(-1) == 1 and kv2.stride(-2) == 64
    a = _lib.DitAttnArgs()
    a.X, a.O = x.data_ptr(), out.data_ptr()
    (a.g_q1, a.b_q1), (a.g_k1, a.b_k1), (a.g_q2, a.b_q2) = [(_f32(g).data_ptr(), _f32(b).data_ptr()) for g, b in norms]
    k = kv2[:, :, 0]
    a.K2, a.V2T, a.V2T_src, a.head_gate = k.data_ptr(), v2t.data_ptr(), None, _ptr(head_gate)
    a.k2_bs, a.k2_rs = k.stride(0), k.stride(1)
    a.nseq, a.T, a.heads, a.seq_per_env, a.Lz, a.ldx, a.ldo = nseq, T, heads, seq_per_env, kv2.shape[1], x.stride(0), out.stride(0)
    a.scale, a.eps = (scale if scale is not None else 64 ** -0.5), eps
    if stats is not None:
        assert stats.dtype == torch.float32 and stats.shape == (x.shape[0], 4, 2) and stats.is_contiguous()
        a.stats, a.stats_ld = stats.data_ptr(), 8
    _lib.check(_lib.lib().ina_dit_attention(C.byref(a), _stream()), "dit_attention")
    return out


def dit_rowchain(a_in: torch.Tensor, w1: torch.Tensor, gamma1: torch.Tensor, x: torch.Tensor, gate: Optional[torch.Tensor] = None,
                 gamma2: Optional[torch.Tensor] = None, mod_scale2: Optional[torch.Tensor] = None, h: Optional[torch.Tensor] = None,
                 w2: Optional[torch.Tensor] = None, c2: Optional[torch.Tensor] = None, glu2: bool = False, mod_div: int = 0, eps: float = 1e-5,
                 seg_stats: Optional[torch.Tensor] = None, seg_eps: float = 1e-5) -> torch.Tensor:
    """the row-local chain of a NextDiT block in one launch (csrc/dit_rowchain.hip):
        x += tanh(gate[r // mod_div]) * rmsnorm(bf16(a_in @ w1.T)) * gamma1
        H  = rmsnorm(x) * gamma2 * (1 + mod_scale2[r // mod_div])
        c2 = H @ w2.T   (glu2: silu(H @ wg.T) * (H @ wu.T) with w2's rows interleaved [gate16 | up16])
    a_in bf16 [M, K1] (K1 = 384 | 1024; M a multiple of 128), w1 bf16 [384, K1], x f32 [M, 384] (in place); w2 bf16 [N2, 384] -> c2 bf16 [M, N2 (/ 2)], or w2 None
    (then h bf16 [M, 384] may be given to receive H). The projection and H never leave the chip.
    seg_stats f32 [M, N2 // 384, 2] (plain second GEMM): receives (mean, rstd) of every 384-wide segment of the c2 rows = the LayerNorm
    statistics dit_attention(stats=) consumes."""
    assert a_in.dtype == torch.bfloat16 and w1.dtype == torch.bfloat16 and a_in.dim() == 2 and a_in.stride(1) == 1 and w1.stride(1) == 1
    M, K1 = a_in.shape
    assert w1.shape == (384, K1) and x.dtype == torch.float32 and x.shape == (M, 384) and x.stride(1) == 1
    a = _lib.DitRowchainArgs()
    a.A, a.W1, a.gamma1, a.X = a_in.data_ptr(), w1.data_ptr(), _f32(gamma1).data_ptr(), x.data_ptr()
    a.M, a.K1, a.lda, a.ldw1, a.ldx = M, K1, a_in.stride(0), w1.stride(0), x.stride(0)
    if gate is not None:
        assert gate.dtype == torch.float32 and gate.stride(-1) == 1
        a.gate, a.mod_ld = gate.data_ptr(), gate.stride(0)
    a.gamma2 = _ptr(_f32(gamma2))
    if mod_scale2 is not None:
        assert mod_scale2.dtype == torch.float32 and mod_scale2.stride(-1) == 1 and a.mod_ld in (0, mod_scale2.stride(0))
        a.mod_scale2, a.mod_ld = mod_scale2.data_ptr(), mod_scale2.stride(0)
    if h is not None:
        assert w2 is None and h.dtype == torch.bfloat16 and h.shape == (M, 384) and h.stride(1) == 1
        a.H, a.ldh = h.data_ptr(), h.stride(0)
    if w2 is not None:
        N2 = w2.shape[0]
        assert w2.dtype == torch.bfloat16 and w2.shape == (N2, 384) and w2.stride(1) == 1 and c2 is not None
        assert c2.dtype == torch.bfloat16 and c2.shape == (M, N2 // 2 if glu2 else N2) and c2.stride(1) == 1
        a.W2, a.C2, a.N2, a.ldw2, a.ldc2, a.glu2 = w2.data_ptr(), c2.data_ptr(), N2, w2.stride(0), c2.stride(0), int(glu2)
    if seg_stats is not None:
        assert w2 is not None and not glu2 and N2 % 384 == 0
        assert seg_stats.dtype == torch.float32 and seg_stats.shape == (M, N2 // 384, 2) and seg_stats.is_contiguous()
        a.seg_stats, a.seg_eps = seg_stats.data_ptr(), seg_eps
    a.mod_div, a.eps = mod_div, eps
    _lib.check(_lib.lib().ina_dit_rowchain(C.byref(a), _stream()), "dit_rowchain")
    return x


def resize_u8(x: torch.Tensor, out: torch.Tensor, bounds: torch.Tensor, coefs: torch.Tensor, axis: int) -> torch.Tensor:
    """one axis of PIL's 8-bit bicubic resample: x u8 contiguous, out the same shape with `axis` resized to bounds.shape[0];
    bounds int32 [n_out, 2], coefs int32 [n_out, ksize] (internnav_amd.preprocess builds PIL's tables)."""
    assert x.dtype == torch.uint8 and out.dtype == torch.uint8 and x.is_contiguous() and out.is_contiguous()
    assert bounds.dtype == torch.int32 and coefs.dtype == torch.int32 and bounds.is_contiguous() and coefs.is_contiguous()
    n_out = bounds.shape[0]
    outer = 1
    for d in x.shape[:axis]:
        outer *= d
    inner = 1
    for d in x.shape[axis + 1:]:
        inner *= d
    assert out.shape[axis] == n_out and out.numel() == outer * n_out * inner and coefs.shape[0] == n_out
    a = _lib.ResizeU8Args()
    a.in_, a.out, a.bounds, a.coefs = x.data_ptr(), out.data_ptr(), bounds.data_ptr(), coefs.data_ptr()
    a.outer, a.n_in, a.n_out, a.inner, a.ksize = outer, x.shape[axis], n_out, inner, coefs.shape[1]
    _lib.check(_lib.lib().ina_resize_u8(C.byref(a), _stream()), "resize_u8")
    return out


def qwen_patchify_u8(img: torch.Tensor, out: torch.Tensor, lut: torch.Tensor, ps: int = 14, merge: int = 2, tdup: int = 2) -> torch.Tensor:
    """img u8 [n, H, W, 3] -> out bf16 [n * (H/ps) * (W/ps), 3*tdup*ps*ps] in the HF Qwen2-VL patch layout; lut f32 [3, 256]."""
    assert img.dtype == torch.uint8 and img.is_contiguous() and img.dim() == 4 and img.shape[3] == 3
    assert out.dtype == torch.bfloat16 and out.dim() == 2 and out.stride(1) == 1 and lut.dtype == torch.float32 and lut.is_contiguous() and lut.numel() == 768
    n, H, W = img.shape[:3]
    assert out.shape[0] == n * (H // ps) * (W // ps) and out.shape[1] == 3 * tdup * ps * ps
    a = _lib.QwenPatchifyArgs()
    a.img, a.out, a.lut = img.data_ptr(), out.data_ptr(), lut.data_ptr()
    a.n, a.H, a.W, a.ps, a.merge, a.tdup, a.ldo = n, H, W, ps, merge, tdup, out.stride(0)
    _lib.check(_lib.lib().ina_qwen_patchify_u8(C.byref(a), _stream()), "qwen_patchify_u8")
    return out


def u8_lut(x: torch.Tensor, out: torch.Tensor, lut: torch.Tensor) -> torch.Tensor:
    """out[i] = bf16(lut[x[i]]); x u8, lut f32 [256]."""
    assert x.dtype == torch.uint8 and x.is_contiguous() and out.dtype == torch.bfloat16 and out.is_contiguous() and out.numel() == x.numel()
    assert lut.dtype == torch.float32 and lut.is_contiguous() and lut.numel() == 256
    a = _lib.U8LutArgs()
    a.in_, a.out, a.lut, a.n = x.data_ptr(), out.data_ptr(), lut.data_ptr(), x.numel()
    _lib.check(_lib.lib().ina_u8_lut(C.byref(a), _stream()), "u8_lut")
    return out


def resize_f32(x: torch.Tensor, out: torch.Tensor, bounds: torch.Tensor, coefs: torch.Tensor, axis: int) -> torch.Tensor:
    """one axis of PIL's float ("F" mode) bicubic resample: x f32 contiguous, coefs f64 [n_out, ksize], bounds int32 [n_out, 2]."""
    assert x.dtype == torch.float32 and out.dtype == torch.float32 and x.is_contiguous() and out.is_contiguous()
    assert bounds.dtype == torch.int32 and coefs.dtype == torch.float64 and bounds.is_contiguous() and coefs.is_contiguous()
    n_out = bounds.shape[0]
    outer = 1
    for d in x.shape[:axis]:
        outer *= d
    inner = 1
    for d in x.shape[axis + 1:]:
        inner *= d
    assert out.shape[axis] == n_out and out.numel() == outer * n_out * inner and coefs.shape[0] == n_out
    a = _lib.ResizeF32Args()
    a.in_, a.out, a.bounds, a.coefs = x.data_ptr(), out.data_ptr(), bounds.data_ptr(), coefs.data_ptr()
    a.outer, a.n_in, a.n_out, a.inner, a.ksize = outer, x.shape[axis], n_out, inner, coefs.shape[1]
    _lib.check(_lib.lib().ina_resize_f32(C.byref(a), _stream()), "resize_f32")
    return out


def gn_mish(x: torch.Tensor, out: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, seqs: int, T: int, pad: int, in_seq_stride: int,
            groups: int = 8, residual: Optional[torch.Tensor] = None, film_env: Optional[torch.Tensor] = None, film_step: Optional[torch.Tensor] = None,
            film_off: int = 0, seq_per_env: int = 1, eps: float = 1e-5) -> torch.Tensor:
    """GroupNorm(groups) -> Mish [-> scale * y + bias (FiLM)] [-> + residual] of one ConditionalUnet1D Conv1dBlock.
    x bf16|f32 [rows, C]: conv output, row (b, t) at b * in_seq_stride + t; out / residual bf16 padded [seqs * (T + 2 pad), C]."""
    assert x.dtype in (torch.bfloat16, torch.float32) and out.dtype == torch.bfloat16 and x.stride(1) == 1 and out.stride(1) == 1
    C_ = out.shape[1]
    a = _lib.GnMishArgs()
    a.x_f32 = 1 if x.dtype == torch.float32 else 0
    a.X, a.Y, a.gamma, a.beta = x.data_ptr(), out.data_ptr(), _f32(gamma).data_ptr(), _f32(beta).data_ptr()
    a.seqs, a.T, a.C, a.groups, a.pad, a.in_seq_stride, a.ldx, a.ldy = seqs, T, C_, groups, pad, in_seq_stride, x.stride(0), out.stride(0)
    if residual is not None:
        assert residual.dtype == torch.bfloat16 and residual.stride(1) == 1
        a.R, a.ldr = residual.data_ptr(), residual.stride(0)
    if film_env is not None:
        assert film_env.dtype == torch.float32 and film_step.dtype == torch.float32 and film_env.stride(1) == 1 and film_step.is_contiguous()
        a.film_env, a.film_step, a.film_ld, a.film_off, a.seq_per_env = film_env.data_ptr(), film_step.data_ptr(), film_env.stride(0), film_off, seq_per_env
    a.eps = eps
    _lib.check(_lib.lib().ina_gn_mish(C.byref(a), _stream()), "gn_mish")
    return out


def pad_rows(x: torch.Tensor, seqs: int, T: int, pad: int, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """zero the pad rows of a padded bf16 buffer [seqs * (T + 2 pad), C] (+ optional per-channel bias on the valid rows)."""
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1
    a = _lib.PadRowsArgs()
    a.X, a.bias, a.seqs, a.T, a.pad, a.C, a.ldx = x.data_ptr(), _ptr(_f32(bias)), seqs, T, pad, x.shape[1], x.stride(0)
    _lib.check(_lib.lib().ina_pad_rows(C.byref(a), _stream()), "pad_rows")
    return x


def ddim_step(eps: torch.Tensor, sample: torch.Tensor, xin: torch.Tensor, seqs: int, T: int, D: int, pad: int, coefs, clip: float = 1.0,
              use_clipped_model_output: bool = False):
    """DDIMScheduler.step (eta 0) on the fp32 sample [seqs * T, D]; eps f32 in padded row indexing; xin bf16 padded network input.
    use_clipped_model_output as diffusers' step() argument (default False: the direction term keeps the network's eps)."""
    assert eps.dtype == torch.float32 and sample.dtype == torch.float32 and sample.is_contiguous() and xin.dtype == torch.bfloat16
    a = _lib.DdimStepArgs()
    a.eps, a.sample, a.Xin, a.seqs, a.T, a.D, a.pad, a.lde, a.ldx = eps.data_ptr(), sample.data_ptr(), xin.data_ptr(), seqs, T, D, pad, eps.stride(0), xin.stride(0)
    a.inv_sqrt_a, a.sqrt_b, a.sqrt_ap, a.sqrt_bp, a.clip = [float(c) for c in coefs] + [float(clip)]
    a.use_clipped_model_output = int(bool(use_clipped_model_output))
    _lib.check(_lib.lib().ina_ddim_step(C.byref(a), _stream()), "ddim_step")
    return sample
