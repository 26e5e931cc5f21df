"""GPU: the ops of the training tape (internnav_amd/tape.py: the backward closures, the `_acc` accumulation rule, the weight-transpose cache) and the
layers of internnav_amd/train_layers.py on the HIP kernels, against float64 autograd - the case table, references and bounds of tests/tape_cases.py
(read its docstring for the groups and the bound model; tests/test_tape_ops_cpu.py runs the same table on the CPU stand-ins).

What the whole-step tests (test_sft_gpu.py and siblings: per-tensor relative NORM error against a bf16-autocast yardstick) cannot see and this file
does: a closure wrong by a few percent of one tensor, a contribution that overwrites instead of adding, a stale W^T, a gradient written to the wrong
slice, and the views the real wrappers receive (column slices of a cat_cols buffer, spans at offsets that are no multiple of 8).

Measured on an MI355X (ROCm 7), worst |err| / bound per op over its cases, all results / the fp32-stored results alone (a bf16-stored result
sits near 1.0 by construction: half a bf16 spacing against 2^-8 |ref|); the exact cases count as 0:
    act            0.918 / 0.025      glu            0.937 / -          modulate       0.937 / 0.008      col_scale      0.930 / 0.002
    norm           0.944 / 0.904      attention      0.813 / -          small_linear   0.962 / 0.011      mse_head       0.970 / 0.005
    (attention: dq / dk / dv against attn_bwd_ref.reference at the stored o, attn_bwd_ref's own bound; the stored o against the float64 forward apart)
    linear         0.995 / 0.252      (dX through the GEMMs, dW through gemm_dw in one launch, in row ranges and through the five-launch fallback,
                                       and the second dX after adamw_step)
    add, span / rows / cols, cat_tokens, cat_cols, repeat_seq, mean_tokens, pair_goal_current, broadcast_param, add_table, col_scale and
    modulate ('id', 'one_plus'), the `_acc` rule, linear with integer operands on every dW route, dropout: exact (torch.equal).
Layers, worst per-tensor (engine error) / (error of the float32 module under bf16 autocast), both against the float64 module; the bar is 1.25:
    mha-self-d96-residual 0.86   mha-self-d128-causal 0.85   mha-split-d128-residual 0.88   mha-split-d96 0.93   mha-self-d96-no-attn-dropout 0.86
    ffn-d96 0.83   encoder_layer-d96 1.03   encoder_layer-d128 0.95   decoder_layer-d128 1.00   decoder_layer-d96 1.13
    decoder_layer_prenorm-causal-d96 0.99   decoder_layer_prenorm-causal-d128 1.13   rgbd_former 1.04   dino-depth1 1.06
These ratios are for CONDITIONED inputs: every ReLU layer case shifts its linear1 bias until no pre-activation of the float64 reference lies within
2^-5 of zero (tape_cases._open_relu_gap), so no ReLU unit is exercised near its kink - there a unit that flips in one precision only moves
engine and yardstick alike by several times their error (seen at 1.5 - 3 x on decoder_layer-d96 before the conditioning). The GELU cases
(decoder_layer_prenorm, dino) and the mha cases are not conditioned.
The whole file takes 3 s; the slowest case 0.2 s.

Finding fixed with this file: `Tape.linear`'s backward handed a bf16 gradient that is a column slice of a cat_cols buffer (row stride 20, base 8 bytes
past a 16-byte boundary) straight to the dX GEMM and to the fallback's transpose + GEMM; the launcher refuses it ("gemm: K/lda/ldw must be multiples of
8"). The stand-ins take any stride, so the CPU tests never saw it. The tape now makes the aligned copy; the wrapper is as strict as before.

Mutation table: single edits of a scratch copy of tape.py / train_layers.py (never committed), each run against this file on the MI355X and against
tests/test_tape_ops_cpu.py; the committed code passes every case. Failing cases (the same on the CPU stand-ins unless noted; L: = test_layer):
    add without the second _acc                 acc-dtype-then-f32-sum, acc-non-owned-add-first / -add-last, norm-*-x-also-residual*, plumb-cat-mixed,
                                                plumb-spans-fanout                                                    [whole-graph CPU tests: pass]
    _acc's third branch without base=           acc-dtype-then-f32-sum, acc-non-owned-add-last, norm-*-x-also-residual*, plumb-cat-mixed, 11 layers [w-g: fail]
    _acc in place into a non-owned buffer       acc-non-owned-add-last, norm-ln-x-also-residual, norm-rms-x-also-residual-bf16x       [w-g: pass]
    modulate 'tanh' without act_bwd             modulate-tanh-div1, modulate-tanh-div4-base                                           [w-g: fail]
    modulate with group_rows=1                  modulate-id-div4-base, modulate-one_plus-div4, modulate-tanh-div4-base                [w-g: fail]
    col_scale without (1 - tanh^2)              col_scale-tanh-heads                                                                  [w-g: fail]
    add_table summing over the wrong axis       add_table-x2, add_table-x3, L:rgbd_former                                             [w-g: fail]
    attention: torch.empty for a partial source attention-partial-blocks-d48, -d64 (NaN where 0 is due, thanks to the NaN-filled allocations) [w-g: pass]
    span without the copy in _own_f32_grad      plumb-spans-fanout                                                                    [w-g: pass]
    linear without the residual's gradient      linear-residual-f32, linear-residual-bf16, 10 layers                                  [w-g: fail]
    _w_transposed without the version check     wt-cache-after-adamw                                                                  [w-g: pass]
    mean_tokens without / L                     plumb-repeat-mean-pair                                                                [w-g: fail]
    pair_goal_current without the goal sum      plumb-repeat-mean-pair                                                                [w-g: fail]
    mse_head without loss_scale on x's gradient mse_head-2blocks-masked-scaled, mse_head-f32x-masked-scaled                           [w-g: fail]
    _mha's rows=(d, 3*d) as (0, 2*d)            L:mha-split-d96, L:mha-split-d128-residual, both decoder layers x 2, L:rgbd_former    [w-g: fail]
    bias gradient to rows [0, N) of a packed b  linear-rows-tail, the same 7 layers                                                   [w-g: fail]
    linear without the aligned copy of dy       linear-dw-fallback-bf16, linear-rand-dw-fallback-bf16, the bf16 twins test - GPU only [w-g: pass]
"whole-graph CPU tests" = tests/test_sft_tape_cpu.py and tests/test_navdp_train_cpu.py: 6 of the 17 edits pass them.
"""
import pytest
import torch

from tests import tape_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORST = {}
OPS = C.CASES


@pytest.fixture(scope="module")
def lib(built_lib):
    import internnav_amd  # noqa: F401

    return built_lib


@pytest.mark.parametrize("case", OPS, ids=[c.id for c in OPS])
def test_op(lib, case):
    got = C.run(case, DEV)
    torch.cuda.synchronize()
    w = C.check(case, got, WORST)
    print(f"{case.id}: worst |err| / bound {w:.3f}")


@pytest.mark.parametrize("fallback,aligned", C.DW_TWINS)
def test_dw_routes_agree_bit_for_bit(lib, monkeypatch, fallback, aligned):
    """the five-launch fallback (a gradient that is a misaligned column slice of a cat_cols buffer) and gemm_dw (its aligned twin) on the same exact
    values: the same dW, db and dX bits - and each route really is the one taken."""
    from internnav_amd import train_ops

    taken = []
    real_ok = train_ops.gemm_dw_ok
    monkeypatch.setattr(train_ops, "gemm_dw_ok", lambda *a: taken.append(real_ok(*a)) or taken[-1])
    a, b = C.run(C.by_id(fallback), DEV), C.run(C.by_id(aligned), DEV)
    assert taken[:2] == [False, True] and all(taken[1:]), f"routes offered (gemm_dw?): {taken}"          # (gemm_dw asks once more itself)
    for k in ("p.w", "p.b", "x.x"):
        assert torch.equal(a[k], b[k]), k


def test_frozen_linear_has_no_gradient_entry_and_no_dw_launch(lib, monkeypatch):
    """a linear whose weight lives in the frozen store: the trainable store has no entry for it and the backward never reaches the dW routes."""
    from internnav_amd import ops, train_ops

    calls = []
    for mod, name in ((train_ops, "gemm_dw_ok"), (train_ops, "gemm_dw"), (train_ops, "transpose"), (train_ops, "colsum"), (ops, "linear")):
        monkeypatch.setattr(mod, name, (lambda f, n: lambda *a, **kw: calls.append(n) or f(*a, **kw))(getattr(mod, name), name))
    case = C.by_id("linear-frozen")
    got = C.run(case, DEV)
    store = got["_tape"].store
    assert "w" not in store.index and "b" not in store.index and set(store.index) == {"dummy"} and "p.w" not in got
    assert calls == ["linear", "transpose", "linear"], calls          # forward, W^T for dX, dX: no dW GEMM, no bias column sum
    C.check(case, got)


def test_dw_row_ranges_are_taken(lib):
    from internnav_amd import train_ops

    assert train_ops.gemm_dw_splits(2049) == 2 and train_ops.gemm_dw_splits(390) == 1


@pytest.mark.parametrize("lc", C.LAYERS, ids=[c.id for c in C.LAYERS])
def test_layer(lib, lc):
    table = []
    got = C.layer_run(lc, DEV)
    torch.cuda.synchronize()
    w = C.layer_check(lc, got, table)
    print("\n".join(table))
    print(f"{lc.id}: worst engine / bf16-autocast ratio {w:.2f}")


def test_zz_worst_per_op(lib):
    """the table of the docstring: worst |err| / bound per op over the cases above (run the whole file)."""
    for k, v in sorted(WORST.items()):
        print(f"TAPE_WORST {k:30s} {v:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
