"""CPU side of the GEMM fp64 tests (tests/gemm_ref.py; the kernels' side is tests/test_gemm_fp64_gpu.py):
  * every exact case of the shared tables: fp32 torch (the stand-in of tests/_cpu_kernels.py, run through the same sentinel buffers and both
    layouts as the kernels) is `torch.equal` to the float64 reference - the proof that the inputs have the property the zero tolerance rests on;
  * the stand-in against the reference on the epilogue cases with random values, under the bound model; the worst ratio
    |err| / (2^-24 (sqrt(K) + 4) scale) of fp32 torch is recorded here for comparison with the kernels' (docstring of the GPU file):
        relu 0.102, tanh 0.040, gelu 0.021, gelu_tanh 0.021, silu 0.019, mish 0.023 (printed by test_standin_random_values_within_the_model;
        the smooth activations shrink the accumulator's error where their slope is below 1, and the model charges them the slope 1.13)
  * the fragment-order index formula against a direct restatement;
  * what ina_plan_gemm refuses (host arithmetic, through ina_gemm_select): an activation code outside the table, GLU with a residual, GLU with a
    colscale."""
import ctypes as C

import pytest
import torch

from tests import _cpu_kernels as CK
from tests import gemm_ref as G

F32, BF16 = G.F32, G.BF16
DEV = "cpu"


def _exact(cases):
    for c in cases:
        want = G.expected_exact(c)
        for layout in ("aligned", "unaligned"):
            out = G.run_case(CK.linear, c, layout, DEV)
            assert out.dtype == c["out_dtype"] and torch.equal(out, want), f"{c['id']} [{layout}]"


@pytest.mark.parametrize("cfg", sorted(G.REG_TILES))
def test_exact_register_staged(cfg):
    for K in (8, 64, 72, 128, 136, 200):
        _exact(G.reg_cases(cfg, K, DEV))


@pytest.mark.parametrize("cfg", sorted(G.DMA_TILES))
def test_exact_lds_dma(cfg):
    for K in (64, 128, 192, 256):
        _exact(G.dma_cases(cfg, K, DEV))
    _exact(G.group_m_cases(cfg, DEV))


@pytest.mark.parametrize("cfg", [39, 40])
def test_exact_four_wave(cfg):
    for K in (64, 128, 192):
        _exact(G.w4_cases(cfg, K, DEV))
    _exact(G.group_m_cases(cfg, DEV))


def test_exact_rowpanel():
    _exact(G.rowpanel_cases(34, DEV))
    _exact(G.rowpanel_cases(35, DEV, Ns=(384, 768), variants=(("plain", BF16),)))


@pytest.mark.parametrize("K", [8, 128, 136, 256, 512, 1024, 1032])
def test_exact_weight_streaming(K):
    _exact(G.skinny_cases(K, DEV))


def test_exact_weight_streaming_wide():
    _exact(G.skinny_wide_cases(DEV))


@pytest.mark.parametrize("K", [136, 512, 520, 1024, 4096])
def test_exact_prenorm(K):
    _exact(G.prenorm_cases(K, DEV))


@pytest.mark.parametrize("cfg", sorted(G.FEATURE_SHAPES))
def test_exact_epilogue_features(cfg):
    _exact(G.feature_cases(cfg, DEV))
    if cfg != 32:
        _exact(G.batched_cases(cfg, DEV))


def test_standin_random_values_within_the_model(capsys):
    worst = {}
    for cfg in (1, 32):
        for act in G.ACTS:
            for glu in (False, True):
                c = G.random_case(cfg, act, F32, DEV, glu=glu)
                ref, scale, aerr = G.case_ref(c)
                out = G.run_case(CK.linear, c, "aligned", DEV)
                # torch's activations are libm-grade: the kernels' measured allowance (fast exp) covers them
                r = G.check(out, ref, scale, aerr, c["K"], 1.0, c["id"])
                worst[act] = max(worst.get(act, 0.0), r)
    with capsys.disabled():
        print("\nGEMM_K fp32 torch (CPU): " + "  ".join(f"{a} {v:.3f}" for a, v in worst.items()))


def test_standin_refuses_what_it_does_not_compute():
    x, w = torch.zeros(4, 8, dtype=BF16), torch.zeros(32, 8, dtype=BF16)
    with pytest.raises(AssertionError):
        CK.linear(x, w, glu=True, residual=torch.zeros(4, 16))
    with pytest.raises(AssertionError):
        CK.linear(x, w, seg_stats=(torch.zeros(4, 1, 2), 1e-5))
    with pytest.raises(TypeError):
        CK.linear(x, w, no_such_operand=1)


def test_colscale_follows_the_activation():
    """relu(-3) * -2 = 0, not relu(-3 * -2) = 6: the order the reference and the stand-in share with the kernels."""
    x, w = torch.ones(1, 8, dtype=BF16), torch.zeros(4, 8, dtype=BF16)
    kw = dict(bias=torch.full((4,), -3.0), act="relu", colscale=torch.full((4,), -2.0))
    assert float(G.linear_ref(x, w, **kw)[0].abs().max()) == 0.0
    assert float(CK.linear(x, w, out_dtype=F32, **kw).abs().max()) == 0.0


@pytest.mark.parametrize("N,K", [(16, 32), (48, 96), (48, 32), (16, 96)])
def test_preshuffle_index_formula(N, K):
    idx = G.preshuffle_index(N, K)
    assert sorted(idx.reshape(-1).tolist()) == list(range(N * K))            # a permutation
    for n, k in ((0, 0), (N - 1, K - 1), (5, 9), (15, 31), (N - 16, K - 32)):
        frag, lane = (n // 16) * (K // 32) + k // 32, (k % 32) // 8 * 16 + n % 16
        assert int(idx[n, k]) == frag * 512 + lane * 8 + k % 8


# ---------------------------------------------------------------------------------------------------------------- planner refusals
@pytest.fixture(scope="module")
def select(built_lib):
    from internnav_amd import _lib

    h = _lib.lib()

    def sel(M, N, K, **kw):
        a = _lib.GemmArgs()
        a.A = a.W = a.C = 0x1000
        a.M, a.N, a.K = M, N, K
        a.lda = a.ldw = K
        a.ldc = a.ldr = N
        for k, v in kw.items():
            setattr(a, k, v)
        out = C.c_int(0)
        rc = h.ina_gemm_select(C.byref(a), C.byref(out))
        return out.value if rc == 0 else ("error", h.ina_last_error().decode())
    return sel


SHAPES = [(300, 256, 64, {}), (300, 256, 72, {}), (7, 512, 256, {}), (4096, 4096, 2048, {}), (300, 256, 128, dict(force_cfg=22)), (7, 512, 256, dict(force_cfg=32))]


@pytest.mark.parametrize("M,N,K,kw", SHAPES)
def test_planner_refuses_unknown_activation_codes(select, M, N, K, kw):
    for act in range(0, 7):
        assert isinstance(select(M, N, K, act=act, **kw), int), act
    for act in (-1, 7, 100):
        bad = select(M, N, K, act=act, **kw)
        assert isinstance(bad, tuple) and bad[1].startswith("gemm") and "act" in bad[1], (act, bad)


def test_four_wave_tile_takes_the_staged_activations_only(select):
    """39 / 40 have the LDS-transposed epilogue only (activations none .. silu): mish / tanh stay on the ping-pong tile, a forced 39 refuses them."""
    assert select(4096, 4096, 2048, act=4) == 39 and select(4096, 4096, 2048, act=5) == 18 and select(4096, 4096, 2048, act=6) == 18
    for act in (5, 6):
        bad = select(4096, 4096, 2048, act=act, force_cfg=39)
        assert isinstance(bad, tuple) and "39 / 40" in bad[1] and "act" in bad[1], bad


@pytest.mark.parametrize("M,N,K,kw", SHAPES)
def test_planner_refuses_glu_with_residual_or_colscale(select, M, N, K, kw):
    assert isinstance(select(M, N, K, glu=1, act=4, bias=0x3000, rowscale=0x4000, ldc=N // 2, **kw), int)
    for ldr in (N // 2, N // 2 + 4):                 # whatever the alignment of the residual rows
        bad = select(M, N, K, glu=1, act=4, R=0x2000, ldc=N // 2, ldr=ldr, **kw)
        assert isinstance(bad, tuple) and "glu" in bad[1] and "residual" in bad[1], bad
    bad = select(M, N, K, glu=1, act=4, colscale=0x3000, ldc=N // 2, **kw)
    assert isinstance(bad, tuple) and "glu" in bad[1] and "colscale" in bad[1], bad
    assert isinstance(select(M, N, K, R=0x2000, colscale=0x3000, **kw), int)          # both are fine without GLU
