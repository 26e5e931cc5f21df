"""Op-level GPU tests of the GEMM family behind ina_gemm_bf16 (csrc/gemm.hip, gemm_glds.hip, gemm_w4.hip, gemm_rowpanel.hip, gemm_skinny.hip and
the two epilogues of gemm_epilogue.h) against the float64 restatement of tests/gemm_ref.py, every tile forced through force_cfg.

Exact cases (zero tolerance): integer operands whose every partial sum is an exact fp32 number in any summation order (gemm_ref docstring), so
fp32 results must be `torch.equal` to the reference and bf16 results to its single rounding - at both sides of every BM / BN edge, with fewer /
as many / more K steps than ring stages, K tails, every optional operand of the epilogue alone and together, GLU, batches, the residual
aliasing the output, row-strided operands. Every launch writes into sentinel-filled buffers (3 rows and >= 8 columns larger than the result)
in two layouts: 16-byte aligned rows (the LDS-transposed epilogue runs where the kernel has it) and bf16 rows of ld % 8 == 4 / fp32 rows on a
base 8 bytes past a 16-byte boundary (the direct epilogue). Tiles whose contract refuses the second layout (39 / 40, 34 / 35) must refuse it.
tests/test_gemm_ref_cpu.py proves on the CPU that fp32 torch equals the reference on the same tables.

Random-value cases (N(0,1) activations, K^-0.5 weights, N(0,1) bias; one per family and activation - mish and tanh run on the direct epilogue
in either layout, the launchers route them there, and the four-wave tile, which has the other epilogue only, refuses them), per element, every
element checked:
  fp32 results: |err| <= k * 2^-24 * (sqrt(K) + 4) * scale + act_err,   bf16 results: + 2^-8 * |ref|
  act_err = 4 x the measured worst error of the activation as ina_act evaluates it (train_ops_cases.ACT_WORST; mish below), capped at 2e-6 max|act|.
k is measured: every check records the worst |err| / (2^-24 (sqrt(K) + 4) scale) of the fp32 results, the last test prints it per family;
k = 4 x the value measured on an MI355X (ROCm 7), capped at 16:
    register-staged 1-5   worst 0.079  -> k = 0.316
    LDS-DMA               worst 0.084  -> k = 0.336
    four-wave             worst 0.078  -> k = 0.312
    row-panel             worst 0.011  -> k = 0.044   (bf16 results only: the least fp32 error that explains a stored value, see _random)
    row-panel seg_stats   worst 0.084  -> k = 0.336   (mean, rstd of the exact rows)
    weight-streaming      worst 0.029  -> k = 0.116
(fp32 torch on the CPU against the same reference: tests/test_gemm_ref_cpu.py.)
Mish as ina_act evaluates it (v * tanhf(log1pf(__expf(v)))), fp32 in / out through pool_act, x in [-12, 12] step 2^-10 plus +-{20, 50, 88, 100}:
    worst |err| / (2^-24 * scale) = 2.733 at x = -0.0654      (gemm_ref.MISH_WORST; the other activations: train_ops_cases.ACT_WORST)
    (scale = |y| (1 + |x|) + |x| 2^-126 / 2^-24: __expf(x) below the smallest normal is flushed, which alone is the whole result at x = -88;
     without that term the same grid gives 45.3, all of it from that one point)
"""
import pytest
import torch

from tests import gemm_ref as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
LAYOUTS = ("aligned", "unaligned")
# measured worst ratios (see above); a family that needs more than the cap is a finding
MEASURED = {"register-staged": 0.079, "LDS-DMA": 0.084, "four-wave": 0.078, "row-panel": 0.011, "row-panel seg_stats": 0.084, "weight-streaming": 0.029}
KFAM = {f: min(16.0, 4.0 * v) for f, v in MEASURED.items()}
WORST = {f: 0.0 for f in MEASURED}
REFUSED = {39: "39 / 40", 40: "39 / 40", 34: "34 / 35", 35: "34 / 35"}           # tiles whose contract wants 16-byte output rows


@pytest.fixture(scope="module")
def ops(built_lib):
    from internnav_amd import ops

    return ops


def _exact(ops, cases):
    for c in cases:
        want = G.expected_exact(c)
        for layout in LAYOUTS:
            if layout == "unaligned" and c["cfg"] in REFUSED:
                with pytest.raises(Exception, match=REFUSED[c["cfg"]]):
                    G.run_case(ops.linear, c, layout, DEV)
                continue
            out = G.run_case(ops.linear, c, layout, DEV)
            assert out.dtype == c["out_dtype"]
            if not torch.equal(out, want):
                bad = out != want
                i = int(bad.reshape(-1).float().argmax())
                raise AssertionError(f"{c['id']} [{layout}]: {int(bad.sum())}/{bad.numel()} elements differ from the exact result; first at flat index {i}: "
                                     f"out {out.reshape(-1)[i].item()} want {want.reshape(-1)[i].item()}")


# ---------------------------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("K", [8, 64, 72, 128, 136, 200])
@pytest.mark.parametrize("cfg", sorted(G.REG_TILES))
def test_exact_register_staged(ops, cfg, K):
    _exact(ops, G.reg_cases(cfg, K, DEV))


@pytest.mark.parametrize("K", [64, 128, 192, 256])
@pytest.mark.parametrize("cfg", sorted(G.DMA_TILES))
def test_exact_lds_dma(ops, cfg, K):
    _exact(ops, G.dma_cases(cfg, K, DEV))


@pytest.mark.parametrize("cfg", sorted(G.DMA_TILES) + [39])
def test_exact_group_m(ops, cfg):
    _exact(ops, G.group_m_cases(cfg, DEV))


@pytest.mark.parametrize("K", [64, 128, 192])
def test_exact_four_wave(ops, K):
    _exact(ops, G.w4_cases(39, K, DEV))


@pytest.mark.parametrize("K", [64, 128, 192])
def test_exact_four_wave_fragment_ordered(ops, K):
    """cfg 40 (B fragments from the fragment-ordered copy of W) equals cfg 39 and the reference."""
    for c in G.w4_cases(40, K, DEV):
        c["w_frag"] = ops.gemm_preshuffle(c["w"].contiguous())
        _exact(ops, [c])
        a = G.run_case(ops.linear, c, "aligned", DEV)
        b = G.run_case(ops.linear, dict(c, cfg=39, w_frag=None), "aligned", DEV)
        assert torch.equal(a, b), c["id"]


@pytest.mark.parametrize("K", [32, 96])
@pytest.mark.parametrize("N", [16, 48])
def test_preshuffle_is_the_documented_fragment_order(ops, N, K):
    g = torch.Generator(device=DEV).manual_seed(N + K)
    w = G.strided_rows(torch.randn(N, K, generator=g, device=DEV).to(BF16), 24)
    assert w.stride(0) > K
    buf = torch.full((N * K + 64,), G.SENT, dtype=BF16, device=DEV)
    ops.gemm_preshuffle(w, out=buf[:N * K])
    want = torch.empty(N * K, dtype=BF16, device=DEV)
    want[G.preshuffle_index(N, K, DEV).reshape(-1)] = w.reshape(-1)
    assert torch.equal(buf[:N * K], want) and bool((buf[N * K:] == G.SENT).all())


@pytest.mark.parametrize("cfg", [34, 35])
def test_exact_rowpanel(ops, cfg):
    _exact(ops, G.rowpanel_cases(cfg, DEV))


@pytest.mark.parametrize("cfg", [34, 35])
def test_rowpanel_seg_stats_of_exact_rows(ops, cfg):
    """the accumulators are exact, so (mean, rstd) of every 384-wide segment are those of known fp32 rows: fp32 bound against float64 statistics.
    scale: mean - mean|x|; rstd = (var + eps)^-1/2 with var = E[x^2] - mean^2 - rstd * (E[x^2] + mean^2) / (var + eps)."""
    eps = 1e-5
    for c in G.rowpanel_cases(cfg, DEV, Ns=(384, 768), variants=(("plain", BF16),)):
        M, N = c["x"].shape[0], c["w"].shape[0]
        st = torch.full((M + 1, N // 384, 2), float("nan"), device=DEV)
        out = G.Buf(M, N, BF16, "aligned", DEV)
        if M <= 64:                                       # the planner keeps seg_stats away from the weight-streaming row counts
            with pytest.raises(Exception, match="seg_stats"):
                ops.linear(c["x"], c["w"], out=out.v, force_cfg=cfg, seg_stats=(st[:M], eps))
            continue
        ops.linear(c["x"], c["w"], out=out.v, force_cfg=cfg, seg_stats=(st[:M], eps))
        torch.cuda.synchronize()
        assert torch.equal(out.v, G.expected_exact(c)) and out.outside_untouched() and bool(st[M].isnan().all()), c["id"]
        seg = c["acc"][0].reshape(M, N // 384, 384)
        mean, msq = seg.mean(-1), seg.pow(2).mean(-1)
        var = msq - mean * mean
        rstd = torch.rsqrt(var + G.R.f32(eps))
        zero = torch.zeros_like(mean)
        k = KFAM["row-panel seg_stats"]
        r0 = G.check(st[:M, :, 0], mean, seg.abs().mean(-1), zero, 384, k, c["id"] + " mean")
        r1 = G.check(st[:M, :, 1], rstd, rstd * (msq + mean * mean) / (var + eps), zero, 384, k, c["id"] + " rstd")
        WORST["row-panel seg_stats"] = max(WORST["row-panel seg_stats"], r0, r1)


@pytest.mark.parametrize("K", [8, 128, 136, 256, 512, 1024, 1032])
def test_exact_weight_streaming(ops, K):
    _exact(ops, G.skinny_cases(K, DEV))


def test_exact_weight_streaming_wide(ops):
    _exact(ops, G.skinny_wide_cases(DEV))


@pytest.mark.parametrize("K", [136, 512, 520, 1024, 4096])
def test_exact_fused_input_rmsnorm(ops, K):
    _exact(ops, G.prenorm_cases(K, DEV))


@pytest.mark.parametrize("cfg", sorted(G.FEATURE_SHAPES))
def test_exact_epilogue_features(ops, cfg):
    _exact(ops, G.feature_cases(cfg, DEV))


@pytest.mark.parametrize("cfg", sorted(c for c in G.FEATURE_SHAPES if c != 32))
def test_exact_batched(ops, cfg):
    _exact(ops, G.batched_cases(cfg, DEV))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refuses_unknown_activation_and_glu_with_residual_or_colscale(ops):
    pool = G.Pool(67, 160, 64, 7, DEV)
    c = pool.case("refuse", 67, 160, "glu", BF16)
    for cfg in (0, 1, 22):
        with pytest.raises(Exception, match="act"):
            ops.linear(c["x"], c["w"], act=7, force_cfg=cfg)
        with pytest.raises(Exception, match="colscale"):
            ops.linear(c["x"], c["w"], act="relu", glu=True, colscale=pool.colscale, force_cfg=cfg)
        for layout in LAYOUTS:
            for dt in (BF16, F32):
                res, out = G.Buf(67, 80, dt, layout, DEV), G.Buf(67, 80, BF16, layout, DEV)
                with pytest.raises(Exception, match="residual"):
                    ops.linear(c["x"], c["w"], act="relu", glu=True, residual=res.v, out=out.v, force_cfg=cfg)
                assert out.outside_untouched() and bool((out.v == G.SENT).all())          # refused, not launched


# ---------------------------------------------------------------------------------------------------------------- random values
def test_mish_error_table(ops):
    """the measurement gemm_ref.MISH_WORST comes from (printed), by the method of test_train_kernels_fp64_gpu.py::test_activation_error_table."""
    x = torch.cat([torch.arange(-12 * 1024, 12 * 1024 + 1, dtype=F64) / 1024, torch.tensor([20.0, 50.0, 88.0, 100.0, -20.0, -50.0, -88.0, -100.0], dtype=F64)])
    x = torch.cat([x, x[: (-len(x)) % 4]]).float().view(-1, 4).to(DEV)
    out = ops.pool_act(x, torch.full_like(x, float("nan")), T=1, act="mish")
    torch.cuda.synchronize()
    ref, scale = G.act_value(x, "mish")
    assert bool(torch.isfinite(out).all())
    err = (out.double() - ref).abs()
    rel = err / (G.U * scale + G.TINY)
    worst = float(rel.max())
    print(f"MISH_TABLE worst |err| / (2^-24 * scale) = {worst:.3f} at x = {x.reshape(-1)[int(rel.reshape(-1).argmax())].item():.6g}"
          f"   (bound constant in use: 4 x {G.MISH_WORST})")
    assert worst <= 4.0 * G.MISH_WORST
    bound = torch.minimum(4.0 * G.MISH_WORST * G.U * scale + G.TINY, torch.full_like(scale, G.ACT_CAP * float(ref.abs().max())))
    assert bool((err <= bound).all()), "mish: outside 4 x the recorded worst capped at 2e-6 of max|ref|"


def _random(ops, cfg, act, glu=False):
    fam = G.FAMILY[cfg]
    if cfg in (39, 40) and act in ("mish", "tanh"):
        # the four-wave tile has the LDS-transposed epilogue only, whose activations are none .. silu (gemm_epilogue.h): refused, not mis-computed
        c = G.random_case(cfg, act, BF16, DEV)
        with pytest.raises(Exception, match="39 / 40"):
            G.run_case(ops.linear, c, "aligned", DEV)
        return
    for dt in (F32, BF16):
        if cfg in (34, 35) and dt == F32:
            continue                                      # the row-panel kernels write bf16 only (their contract)
        c = G.random_case(cfg, act, dt, DEV, glu=glu)
        ref, scale, aerr = G.case_ref(c)
        for layout in LAYOUTS:
            if layout == "unaligned" and cfg in REFUSED:
                continue                                  # refused (asserted by the exact cases)
            out = G.run_case(ops.linear, c, layout, DEV)
            r = G.check(out, ref, scale, aerr, c["K"], KFAM[fam], f"{c['id']} [{layout}]")
            if dt == F32:
                WORST[fam] = max(WORST[fam], r)
            elif cfg in (34, 35):
                # bf16 only: the fp32 value behind a stored number lies within half a bf16 ulp of it, so |out - ref| - ulp(out) / 2 is the least
                # fp32 error that explains the element (it shows where value and reference round to different sides)
                half = torch.ldexp(torch.ones_like(ref), torch.frexp(out.float().abs()).exponent - 9)
                r = G.ratio(out, ref, scale, aerr + half, c["K"])
                WORST[fam] = max(WORST[fam], r)
            print(f"GEMM_RATIO {fam:16s} {c['id']:28s} {layout:9s} {r:.3f}")


@pytest.mark.parametrize("act", G.ACTS)
@pytest.mark.parametrize("cfg", sorted(G.RANDOM_SHAPES))
def test_random_values_every_family_and_activation(ops, cfg, act):
    _random(ops, cfg, act)


@pytest.mark.parametrize("cfg", sorted(G.RANDOM_SHAPES))
def test_random_values_silu_glu(ops, cfg):
    _random(ops, cfg, "silu", glu=True)


def test_zz_print_measured_k(ops):
    """the table of the docstring: worst |err| / (2^-24 (sqrt(K) + 4) scale) of the fp32 results of this file, per kernel family."""
    for fam, w in WORST.items():
        print(f"GEMM_K {fam:22s} worst {w:.3f}   (k in use: {KFAM[fam]:.3f} = min(16, 4 x {MEASURED[fam]}))")
        assert w <= KFAM[fam]
