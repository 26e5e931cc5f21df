"""Op-level GPU tests of the SFT-step kernels (internnav_amd/csrc/train.hip: ew, ew_vec, colsum, colsum_vec x 6, colsum_final, norm_bwd,
norm_bwd_vec x 4, transpose, sparse_rows, small_linear, mse, adamw, gemm_nn<8|16>), each against the float64 restatement of tests/train_ops_ref.py
on the same (bf16 / fp32) inputs, at the shapes where the launchers switch kernels, chunk sizes or take a second trip through a grid-stride loop.
The argument sets live in tests/train_ops_cases.py; tests/test_train_ops_ref_cpu.py runs the same sets through the CPU stand-ins.

Tolerance model (that of test_s1_head_ops_gpu.py), per element and all-or-nothing:
  fp32 results: |err| <= 16 * 2^-24 * (sqrt(n) + 4) * scale, n the reduction length (1 for element-wise ops), scale the float64 sum of |terms|;
  bf16 results: + 2^-8 * |ref|;
  transpose, the bf16 working copy of AdamW, zero_grad and zero padding: torch.equal.
LayerNorm backward carries |x|max * rstd in `scale` (train_ops_ref.norm_bwd; the model is checked against fp32 torch on the CPU).

Activations (`__expf`, `erff`, `tanhf` inside act_grad / ina_act / ina_silu): the constant is not guessed. test_activation_error_table prints
the worst |err| / (2^-24 * scale) against the float64 reference over x in [-12, 12] (step 2^-10) plus +-{20, 50, 88, 100}; the bound of every
activation case is 4 x the value measured on an MI355X (train_ops_cases.ACT_WORST) and never looser than 2e-6 (forward) / 2e-5 (backward) of max|ref|.
Measured (MI355X, ROCm 7, fp32 in / fp32 out):
    gelu_erf   forward 2.000   backward 1.898
    gelu_tanh  forward 1.889   backward 1.898
    relu       forward 0       backward 0        (exact)
    silu       forward 2.020   backward 2.605
    tanh       forward 1.273   backward 1.227
All outputs finite at +-{20, 50, 88, 100}. The scalar and the vector element-wise kernel gave the same bits on every activation; norm_bwd's two
kernels did not (different summation order), they share the bound.
"""
import pytest
import torch

from tests import train_ops_cases as CASES
from tests import train_ops_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U, BF = R.U, R.BF
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def T(built_lib):
    from internnav_amd import train_ops

    return train_ops


def _impl(T):
    return {k: getattr(T, k) for k in ("affine", "act_fwd", "act_bwd", "glu_fwd", "glu_bwd", "colsum", "norm_bwd", "transpose", "sparse_rows",
                                       "small_linear", "mse_masked", "gemm_nn")}


def _run_all(T, cases):
    impl = _impl(T)
    worst = {}
    for c in cases:
        w = CASES.run_case(impl, c)
        worst[c["op"]] = max(worst.get(c["op"], 0.0), w)
    print("worst |err| / bound per op:", {k: round(v, 3) for k, v in worst.items()}, f"({len(cases)} cases)")


# ------------------------------------------------------------------------------------------------ element-wise
def _act_grid():
    x = torch.arange(-12 * 1024, 12 * 1024 + 1, dtype=torch.float64) / 1024
    x = torch.cat([x, torch.tensor([-100.0, -88.0, -50.0, -20.0, 20.0, 50.0, 88.0, 100.0], dtype=torch.float64)])
    pad = (-x.numel()) % 4
    return torch.cat([x, x[:pad]]).float().view(-1, 4).to(DEV)            # [rows, 4]: the vector kernel; the scalar one is run on a [n, 1] view


def test_activation_error_table(T):
    """the measurement the activation bounds are derived from (printed), and the derived bound itself on the same grid."""
    x = _act_grid()
    dy = torch.ones_like(x)
    for act in R.ACTS:
        for which in ("fwd", "bwd"):
            ref, scale = R.act_value(x, act) if which == "fwd" else R.act_slope(x, act)
            worst = 0.0
            for xv in (x, x.reshape(-1, 1)):
                out = T.act_fwd(xv, act) if which == "fwd" else T.act_bwd(xv, dy.view_as(xv), act)
                assert torch.isfinite(out).all(), f"{act} {which}: non-finite output"
                ratio = ((out.double().view_as(ref) - ref).abs() / (U * scale + R.TINY)).max().item()
                worst = max(worst, ratio)
            print(f"ACT_TABLE {act:9s} {which}: worst |err| / (2^-24 * scale) = {worst:.3f}   (bound constant in use: 4 x {CASES.ACT_WORST[(act, which)]})")
            cap = (2e-6 if which == "fwd" else 2e-5) * ref.abs().max().item()
            assert worst <= 4.0 * CASES.ACT_WORST[(act, which)], f"{act} {which}: {worst} above 4 x the recorded worst"
            bound = torch.minimum(4.0 * CASES.ACT_WORST[(act, which)] * U * scale + R.TINY, torch.full_like(scale, cap))
            CASES.check(out.view_as(ref), ref, bound, f"{act} {which} (capped at the earlier whole-tensor tolerance)")


def test_ew_every_op_dtype_layout(T):
    _run_all(T, CASES.ew_cases(DEV))


def test_ew_second_grid_stride_trip(T):
    _run_all(T, CASES.ew_big_cases(DEV))


def test_ew_scalar_and_vector_kernel_same_values(T):
    """both kernels evaluate the same expressions; whether they give the same bits is reported, not asserted (no comment in train.hip promises it)."""
    g = torch.Generator().manual_seed(7)
    x, dy = CASES.randn((75, 384), g, 3.0, dev=DEV), CASES.randn((75, 384), g, dev=DEV)
    for act in R.ACTS:
        a = T.act_bwd(x, dy, act)
        b = T.act_bwd(CASES.misaligned(x), dy, act)
        ref, scale = R.act_bwd(x, dy, act)
        bound = R.fp32_bound(scale, 1, CASES.act_k(act, "bwd"))
        CASES.check(a, ref, bound, f"{act} vec")
        CASES.check(b, ref, bound, f"{act} scalar")
        print(f"act_bwd {act}: scalar and vector kernel bit-equal: {torch.equal(a, b)}")


def test_dropout_large_shape_bf16_out(T):
    """second grid-stride trip of both kernels with a bf16 output, against the host replica of the mask."""
    from tests.test_train_ops_gpu import _keep_mask

    g = torch.Generator().manual_seed(9)
    p, seed = 0.1, 4242
    for rows, C in ((8200, 1028), (2100, 1001)):
        x = CASES.randn((rows, C), g, dev=DEV)
        keep = _keep_mask(seed, torch.arange(rows * C, dtype=torch.int64, device=DEV).view(rows, C), p)
        y = T.dropout(x, p, seed, out_dtype=BF16)
        assert torch.equal(y, torch.where(keep, x * (1.0 / (1.0 - p)), torch.zeros_like(x)).to(BF16)), f"{rows} x {C}"


# ------------------------------------------------------------------------------------------------ column sums
def test_colsum_chunkings_instances_strides(T):
    _run_all(T, CASES.colsum_cases(DEV))


def test_colsum_95232_rows_and_determinism(T):
    c = CASES.colsum_big_case(DEV)
    _run_all(T, [c])
    a, b = T.colsum(*c["args"]), T.colsum(*c["args"])
    assert torch.equal(a, b), "two runs of the two-stage reduction differ"
    g = torch.Generator().manual_seed(11)
    x = CASES.randn((3 * 2049, 203), g, dev=DEV)
    assert torch.equal(T.colsum(x, group_rows=2049), T.colsum(x, group_rows=2049)), "scalar kernel: two runs differ"


@pytest.mark.parametrize("g", [33, 2048, 2049, 4096, 4097, 8192, 8193])
def test_colsum_partial_buffer_count_is_the_librarys(T, g):
    """train_ops.colsum_chunks is the library's count: a partial buffer of exactly that many chunks is accepted, one float fewer is refused."""
    import ctypes as C

    from internnav_amd import _lib

    Cd, groups = 8, 2
    x = torch.ones(groups * g, Cd, device=DEV)
    out = torch.full((groups, Cd), float("nan"), device=DEV)
    need = groups * T.colsum_chunks(g) * Cd

    def call(n_part):
        part = torch.empty(need, device=DEV)
        a = _lib.ColsumArgs()
        a.X, a.x_dt, a.ldx, a.x_cs = x.data_ptr(), 1, Cd, 1
        a.out, a.out_cs, a.ldo = out.data_ptr(), 1, Cd
        a.rows, a.C, a.group_rows, a.scale = groups * g, Cd, g, 1.0
        a.partial, a.partial_elems = part.data_ptr(), n_part
        return _lib.lib().ina_colsum(C.byref(a), torch.cuda.current_stream().cuda_stream)

    assert call(need) == 0
    assert torch.equal(out, torch.full_like(out, float(g)))
    assert call(need - 1) != 0
    assert b"needs a partial buffer" in _lib.lib().ina_last_error()


# ------------------------------------------------------------------------------------------------ norm backward
def test_norm_bwd_every_kernel_and_trigger(T):
    _run_all(T, CASES.norm_bwd_cases(DEV))


@pytest.mark.parametrize("rms", [False, True])
def test_norm_bwd_scalar_and_vector_kernel_same_values(T, rms):
    g = torch.Generator().manual_seed(13)
    x, dy = CASES.randn((70, 384), g, 2.0, dev=DEV, shift=0.6), CASES.randn((70, 384), g, dev=DEV)
    ga = CASES.randn(384, g, 0.2, dev=DEV, shift=1.0)
    (ref, scale), (xh, xs) = R.norm_bwd(x, dy, ga, rms=rms)
    dv, hv = T.norm_bwd(x, dy, ga, rms=rms, want_xhat=True)
    ds, hs = T.norm_bwd(CASES.misaligned(x), dy, ga, rms=rms, want_xhat=True)
    for d, h, name in ((dv, hv, "vec"), (ds, hs, "scalar")):
        CASES.check(d, ref, R.fp32_bound(scale, 384), f"dx {name}")
        CASES.check(h, xh, R.out_bound(xh, R.fp32_bound(xs, 384), BF16), f"xhat {name}")
    CASES.check(hs, hv.double(), BF * xh.abs() + 2 * R.fp32_bound(xs, 384), "xhat scalar vs vec")
    print(f"norm_bwd rms={rms}: scalar and vector kernel bit-equal: dx {torch.equal(dv, ds)}, xhat {torch.equal(hv, hs)}")


# ------------------------------------------------------------------------------------------------ the small ones
def test_transpose_exact_with_zero_tail(T):
    _run_all(T, CASES.transpose_cases(DEV))


def test_sparse_rows(T):
    _run_all(T, CASES.sparse_rows_cases(DEV))


def test_small_linear(T):
    _run_all(T, CASES.small_linear_cases(DEV))


def test_mse_masked(T):
    _run_all(T, CASES.mse_cases(DEV))


# ------------------------------------------------------------------------------------------------ AdamW
@pytest.mark.parametrize("var", CASES.ADAMW_VARIANTS, ids=[v["id"] for v in CASES.ADAMW_VARIANTS])
def test_adamw_four_steps_per_element(T, var):
    w = CASES.adamw_run(T.adamw, T.sumsq_parts, DEV, var)
    print(f"adamw {var['id']}: worst |err| / bound {w:.3f}")


# ------------------------------------------------------------------------------------------------ skinny dX
def _nn_splits(N, mr):
    return [s for s in (None, 1, 3, 7) if s is None or (N + s - 1) // s * mr * 4 <= 48 * 1024]


NN_CASES = [(M, N, K) for M in (1, 8, 9, 16) for N, K in ((16, 8), (520, 1000), (3584, 3584))]


@pytest.mark.parametrize("M,N,K", NN_CASES)
def test_gemm_nn_rows_splits_views(T, M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N)
    mr = 8 if M <= 8 else 16
    xw = CASES.randn((M, N + 8), g, dtype=BF16, dev=DEV)                      # x as a column slice (ldx = N + 8), values outside it large
    xw[:, N:] = 1000.0
    x = xw[:, :N]
    ww = CASES.randn((N, K + 16), g, N ** -0.5, dtype=BF16, dev=DEV)
    ww[:, :8], ww[:, 8 + K:] = 1000.0, 1000.0
    w = ww[:, 8: 8 + K]                                                      # ldw = K + 16, base 16 bytes into the row
    assert w.stride(0) % 8 == 0 and w.data_ptr() % 16 == 0
    ref, scale = R.gemm_nn(x, w)
    bound = R.fp32_bound(scale, N)
    for splits in _nn_splits(N, mr):
        for xx, wv, tag in ((x, w, "views"), (x.contiguous(), w.contiguous(), "dense")):
            out = T.gemm_nn(xx, wv, splits=splits)
            assert out.shape == (M, K)
            CASES.check(out, ref, bound, f"gemm_nn {tag} splits={splits}")
        ob = T.gemm_nn(x, w, out_dtype=BF16, splits=splits)
        CASES.check(ob, ref, R.out_bound(ref, bound, BF16), f"gemm_nn bf16 out splits={splits}")


def test_gemm_nn_refusals(T):
    g = torch.Generator().manual_seed(3)
    x, w = CASES.randn((16, 3584), g, dtype=BF16, dev=DEV), CASES.randn((3584, 64), g, dtype=BF16, dev=DEV)
    with pytest.raises(RuntimeError, match="raise splits"):
        T.gemm_nn(x, w, splits=3)                                            # 1195 rows x 16 x 4 bytes > 48 KiB
    with pytest.raises(RuntimeError, match="multiples of 8"):
        T.gemm_nn(x, CASES.randn((3584, 72), g, dtype=BF16, dev=DEV)[:, 4:68])    # base 8 bytes into the row
    with pytest.raises(RuntimeError, match="multiples of 8"):
        T.gemm_nn(x, CASES.randn((3584, 68), g, dtype=BF16, dev=DEV)[:, :64])     # ldw = 68
    with pytest.raises(RuntimeError, match="gemm_nn"):
        T.gemm_nn(x, w, splits=0)


# ------------------------------------------------------------------------------------------------ refusals
def test_launchers_refuse_bad_arguments(T):
    """every INA_REQUIRE of the launchers a wrapper can reach: an error code before any launch."""
    import ctypes as C

    from internnav_amd import _lib

    x = torch.ones(8, 8, device=DEV)
    e = torch.empty(0, 8, device=DEV)
    E = RuntimeError
    with pytest.raises(E, match="ew: empty"):
        T.affine(e)
    stream = torch.cuda.current_stream().cuda_stream
    y = torch.full((8, 8), 7.0, device=DEV)
    for field, msg in (("s_div", b"s_div must be positive"), ("tab_mod", b"ew: tab_mod must be positive")):      # the wrapper never passes these zeros
        a = _lib.EwArgs()
        a.op, a.rows, a.C = T.EW_AFFINE, 8, 8
        a.A, a.a_dt, a.lda, a.Y, a.y_dt, a.ldy = x.data_ptr(), 1, 8, y.data_ptr(), 1, 8
        a.S, a.s_dt, a.lds, a.s_div = x.data_ptr(), 1, 8, 1
        a.tab, a.tab_mod = x.data_ptr(), 8
        setattr(a, field, 0)
        assert _lib.lib().ina_ew(C.byref(a), stream) != 0 and msg in _lib.lib().ina_last_error()
    a = _lib.SmallLinearArgs()
    a.X, a.x_dt, a.ldx, a.W, a.w_ns, a.w_ks, a.Y, a.y_dt, a.ldy = x.data_ptr(), 1, 8, x.data_ptr(), 8, 1, y.data_ptr(), 1, 8
    a.rows, a.N, a.K, a.tab, a.tab_mod = 8, 8, 8, x.data_ptr(), 0
    assert _lib.lib().ina_small_linear(C.byref(a), stream) != 0 and b"small_linear: tab_mod must be positive" in _lib.lib().ina_last_error()
    assert bool((y == 7.0).all()), "a refused call wrote its output"
    with pytest.raises(E, match="colsum: empty"):
        T.colsum(torch.empty(8, 0, device=DEV))
    with pytest.raises(E, match="not a multiple of group_rows"):
        T.colsum(x, group_rows=3, out=torch.empty(2, 8, device=DEV))
    with pytest.raises(E, match="norm_bwd: empty"):
        T.norm_bwd(e, e)
    with pytest.raises(E, match="transpose: bad problem"):
        T.transpose(e)
    a = _lib.TransposeArgs()
    y = torch.empty(8, 8, dtype=BF16, device=DEV)
    a.X, a.Y, a.rows, a.cols, a.x_dt, a.ldx, a.ldy = x.data_ptr(), y.data_ptr(), 8, 8, 1, 8, 7          # ldy < rows
    assert _lib.lib().ina_transpose(C.byref(a), torch.cuda.current_stream().cuda_stream) != 0
    assert b"transpose: bad problem" in _lib.lib().ina_last_error()
    with pytest.raises(E, match="sparse_rows: empty"):
        T.sparse_rows(x, torch.empty(0, 4, dtype=torch.int32, device=DEV), torch.empty(0, 4, device=DEV))
    with pytest.raises(E, match="small_linear: empty"):
        T.small_linear(e, x)
    with pytest.raises(E, match="mse: empty"):
        T.mse_masked(e, torch.empty(0, 8, device=DEV), torch.empty(0, device=DEV), 1)
    f = torch.ones(16, device=DEV)
    with pytest.raises(E, match="adamw: empty"):
        T.adamw(f[:0], f[:0], f[:0], f[:0], step=1, **CASES.HP)
    with pytest.raises(E, match="bias corrections must be positive"):
        T.adamw(f.clone(), f.clone(), f.clone(), f.clone(), step=0, **CASES.HP)
    xb = x.to(BF16)
    with pytest.raises((E, AssertionError)):
        T.gemm_nn(torch.ones(17, 8, dtype=BF16, device=DEV), xb)
    a = _lib.GemmNnArgs()
    x17, part = torch.ones(17, 8, dtype=BF16, device=DEV), torch.empty(4 * 32 * 8, device=DEV)
    a.X, a.W, a.partial, a.partial_elems = x17.data_ptr(), xb.data_ptr(), part.data_ptr(), part.numel()
    a.M, a.N, a.K, a.ldx, a.ldw, a.splits = 17, 8, 8, 8, 8, 1
    assert _lib.lib().ina_gemm_nn_bf16(C.byref(a), torch.cuda.current_stream().cuda_stream) != 0
    assert b"gemm_nn: bad problem M=17" in _lib.lib().ina_last_error()
    a.M, a.partial_elems = 16, 4 * 16 * 8 - 1
    assert _lib.lib().ina_gemm_nn_bf16(C.byref(a), torch.cuda.current_stream().cuda_stream) != 0
    assert b"partial buffer too small" in _lib.lib().ina_last_error()
    torch.cuda.synchronize()
