"""TEST INFRASTRUCTURE: the case table of the training tape (internnav_amd/tape.py) and of the layers built on it (internnav_amd/train_layers.py),
their float64 references, their bounds and the runner, shared by tests/test_tape_ops_cpu.py (torch stand-ins of tests/_cpu_kernels.py) and
tests/test_tape_ops_fp64_gpu.py (the HIP kernels).

A case builds a small ParamStore and Tape, runs forward and backward and yields EVERY gradient (`run`): of the inputs (`x.<name>`), of every
tensor of the store (`p.<name>`), of the intermediate values it names (`w.<name>`), and the forward values it names (`v.<name>`).

The reference of a case (`reference`) is plain torch in float64 with torch.autograd. Each forward value is rounded straight-through (`st`) to the
dtype the tape stores it in - bf16 weights as `ParamStore.w16` gives them, bf16 or f32 activations as the op's docstring says - so the derivative
is taken at the values the tape's backward closures read. It is never the tape and never the stand-ins. Seed gradients are bf16-representable:
`Tape.bf16(dy)` is exact and the error of a single op is the error of its kernels.

Groups
  exact    dyadic / small-integer values (as tests/gemm_ref.py builds them): every partial sum of every summation order is exact, the gradient must be
           `torch.equal` to the float64 result cast (one rounding) to the gradient's dtype, on the stand-ins and on the kernels alike.
  bounded  random values; per element, all-or-nothing:
             element-wise ops and reductions: 16 * 2^-24 * (sqrt(n) + 4) * scale (+ 2^-8 |ref| for a bf16-stored result), `scale` the float64 sum of
               |terms| in closed form (tests/train_ops_ref.py), activations with train_ops_cases.ACT_WORST (`act_k`) and the caps of train_ops_cases.case;
             GEMM results: k * 2^-24 * (sqrt(K) + 4) * scale with the largest test_gemm_fp64_gpu.KFAM (the tape does not pin the tile);
             attention: the unmodified bound of tests/attn_bwd_ref.py against its reference, the function the kernel defines (delta from the GIVEN
               bf16 o), evaluated at the o the tape stored (`attention_check`); that o is checked against the float64 forward on its own, and
               `attention_autograd_gap` ties the closed form to float64 autograd (its `delta_f64` variant equals autograd to 1e-12).
           Where a gradient is a chain of two kernels the first one's bound is carried through the second one's (exact) arithmetic; this is stated
           where it happens. A key without a bound must be exact (unused column blocks, masked-out batches).
  layer    train_layers at small width against the torch module itself in float64 (nn.MultiheadAttention, nn.TransformerEncoderLayer,
           nn.TransformerDecoderLayer with norm_first False / True, dropout = 0) loaded with the store's own (bf16-representable) weights. Per tensor -
           output, every parameter gradient, every input gradient: relative norm error <= 1.25 x the error of the SAME module in float32 under
           torch.autocast("cpu", bfloat16), measured at test time. (autocast leaves float64 tensors alone, so the yardstick runs the float32 copy.)
           Tensors whose reference norm is below 1e-6 of the largest follow test_sft_tape_cpu._check's floor (norm below 1e-4 of the largest).
"""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import torch
import torch.nn as nn
import torch.nn.functional as Fn

from tests import attn_bwd_ref as AB
from tests import train_ops_cases as TC
from tests import train_ops_ref as R
from tests.test_gemm_fp64_gpu import KFAM

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
K_GEMM = max(KFAM.values())          # the tape does not pin the GEMM family of a dX / dW product
MARGIN = 1.25                        # layers: the margin of tests/test_unet1d_gpu.py on the bf16-autocast yardstick
CASES = []


# ---------------------------------------------------------------------------------------------------------------- values
def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, *shape, lo=-4, hi=4, dtype=F32):
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype)


def dyad(g, *shape, dtype=F32):
    return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, shape, generator=g)].to(dtype)


def rnd(g, *shape, scale=1.0, dtype=F32, shift=0.0):
    """N(shift, scale) rounded to bf16 (exact in either dtype), stored as `dtype`."""
    return (torch.randn(shape, generator=g) * scale + shift).to(BF16).to(dtype)


def rnd32(g, *shape, scale=1.0, shift=0.0):
    return torch.randn(shape, generator=g) * scale + shift


def st(t, dtype):
    """straight-through rounding: the value a kernel stores (fp32 arithmetic, one rounding to `dtype`), the derivative of the identity."""
    return t + (t.detach().to(F32).to(dtype).to(F64) - t.detach())


class RefParams:
    """float64 leaves of the store's tensors; w16 is the straight-through bf16 working copy."""

    def __init__(self, params, frozen):
        self.leaf = {k: t.to(F64).requires_grad_(True) for k, t in params.items()}
        self.leaf.update({k: t.to(F64) for k, t in frozen.items()})

    def w32(self, name):
        return self.leaf[name]

    def w16(self, name):
        return st(self.leaf[name], BF16)


def case(id, op, group, cpu_skip=None, real_dw_ok=False, nan_fill=False):
    def deco(fn):
        CASES.append(NS(id=id, op=op, group=group, build=fn, cpu_skip=cpu_skip, real_dw_ok=real_dw_ok, nan_fill=nan_fill))
        return fn
    return deco


def prob(params, vars, tape, ref, seeds, frozen=None, prefill=None, bounds=None, watch=(), values=(), ref_loss=None, drop_p=0.0, tape_seed=0, dtypes=None):
    """vars: name -> (tensor, req) (req None: a plain tensor, not a Var). tape(tp, V) / ref(P, V) -> name -> output; seeds: name -> dy."""
    return NS(params=params, vars=vars, tape=tape, ref=ref, seeds=seeds, frozen=frozen or {}, prefill=prefill or {}, bounds=bounds, watch=tuple(watch),
              values=tuple(values), ref_loss=ref_loss, drop_p=drop_p, tape_seed=tape_seed, custom=None, dtypes=dtypes or {})


# ---------------------------------------------------------------------------------------------------------------- runner
_BUILT, _REFS = {}, {}


def built(case):
    """the case's problem, built once per process; its tensors are never modified (the runner hands clones to the tape)."""
    if case.id not in _BUILT:
        _BUILT[case.id] = case.build()
    return _BUILT[case.id]


def _nan_fill(grad_shapes, device):
    """allocate and free NaN-filled buffers of the gradient buffers' sizes: a torch.empty where torch.zeros is needed then shows (the caching
    allocator hands the same blocks out again)."""
    bufs = [torch.full(s, float("nan"), dtype=dt, device=device) for s, dt in grad_shapes for _ in range(4)]
    del bufs


def run(case, device):
    """forward + backward of the case on `device` through internnav_amd.tape (kernels, or whatever is installed in their place) -> every gradient."""
    from internnav_amd.tape import ParamStore, Tape, Var

    pb = built(case)
    if pb.custom is not None:
        return pb.custom(device)
    store = ParamStore(pb.params, device)
    frozen = ParamStore(pb.frozen, device, trainable=False) if pb.frozen else None
    for k, t in pb.prefill.items():
        store.grad(k).copy_(t)
    tp = Tape(store, frozen, drop_p=pb.drop_p, seed=pb.tape_seed)
    V = {k: (t.clone().to(device) if req is None else Var(t.clone().to(device), req=req)) for k, (t, req) in pb.vars.items()}
    outs = pb.tape(tp, V)
    for n, dy in pb.seeds.items():
        Tape.accumulate(outs[n], dy.clone().to(device))
    if case.nan_fill:
        vs = [o for o in list(outs.values()) + list(V.values()) if isinstance(o, Var)]
        _nan_fill([(tuple(o.v.shape), BF16) for o in vs], device)
    tp.backward()
    got = {}
    for k, (t, req) in pb.vars.items():
        if req is not None:
            got["x." + k] = V[k].g
    for k in pb.params:
        got["p." + k] = store.grad(k).clone()
    for k in pb.watch:
        got["w." + k] = outs[k].g
    for k in pb.values:
        got["v." + k] = outs[k].v if isinstance(outs[k], Var) else outs[k]
    got["_tape"] = tp
    return got


def reference(case):
    """(refs, bounds): name -> float64 tensor (None: no gradient), name -> bound tensor (bounded cases; a missing name is exact)."""
    pb = built(case)
    if pb.custom is not None:
        return pb.custom_ref()
    if case.id in _REFS:
        return _REFS[case.id]
    P = RefParams(pb.params, pb.frozen)
    V = {k: (t.to(F64).requires_grad_(bool(req)) if t.is_floating_point() else t) for k, (t, req) in pb.vars.items()}
    outs = pb.ref(P, V)
    for k in pb.watch:
        outs[k].retain_grad()
    loss = sum((outs[n] * dy.to(F64)).sum() for n, dy in pb.seeds.items())
    if pb.ref_loss is not None:
        loss = loss + pb.ref_loss(outs)
    loss.backward()
    refs = {}
    for k, (t, req) in pb.vars.items():
        if req is not None:
            refs["x." + k] = V[k].grad if req else None
    for k, t in pb.params.items():
        g = P.leaf[k].grad
        g = torch.zeros_like(P.leaf[k]) if g is None else g
        refs["p." + k] = g + pb.prefill[k].to(F64) if k in pb.prefill else g
    for k in pb.watch:
        refs["w." + k] = outs[k].grad
    for k in pb.values:
        refs["v." + k] = outs[k].detach()
    bounds = pb.bounds(NS(P=P, V=V, outs=outs, refs=refs, seeds={k: v.to(F64) for k, v in pb.seeds.items()})) if pb.bounds else {}
    _REFS[case.id] = (refs, bounds)
    return refs, bounds


def _check_elem(out, ref, bound, what):
    """train_ops_cases.check where the bound is positive, `== ref` where it is 0 (unused blocks, masked rows); NaN never passes."""
    err = (out.double() - ref).abs()
    bad = ~(err <= bound)
    pos = bound > 0
    ratio = torch.where(pos, err / torch.where(pos, bound, torch.ones_like(bound)), torch.zeros_like(err)).nan_to_num(nan=float("inf"))
    if bool(bad.any()):
        i = int(torch.where(bad, ratio + 1.0, torch.zeros_like(ratio)).reshape(-1).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())}/{err.numel()} elements out of bound; worst at flat index {i}: out "
                             f"{out.reshape(-1)[i].item():.9g} ref {ref.reshape(-1)[i].item():.9g} bound {bound.reshape(-1)[i].item():.3g}")
    return float(ratio.max()) if ratio.numel() else 0.0


def check(case, got, worst=None):
    """every gradient of `got` against the reference: exact keys with torch.equal, bounded keys per element. Returns the worst |err| / bound."""
    refs, bounds = reference(case)
    got = {k: v for k, v in got.items() if not k.startswith("_")}
    w = w32 = 0.0
    if case.op == "attention":          # the gradients: attention_check; below: the stored o against the float64 forward
        assert {k for k in got if k.startswith("x.")} == {k for k in refs if k.startswith("x.")}
        w = attention_check(case, got)
        refs, got = ({k: v for k, v in d.items() if k.startswith("v.")} for d in (refs, got))
    assert set(got) == set(refs), f"{case.id}: gradients {sorted(set(got) ^ set(refs))} on one side only"
    for k, ref in refs.items():
        g = got[k]
        what = f"{case.id} {k}"
        if ref is None:
            assert g is None, f"{what}: a gradient where none is due"
            continue
        assert g is not None, f"{what}: no gradient"
        g = g.detach().cpu()
        want_dt = built(case).dtypes.get(k) if built(case).custom is None else None
        assert want_dt is None or g.dtype == want_dt, f"{what}: kept as {g.dtype}, due {want_dt}"
        assert g.shape == ref.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(ref.shape)}"
        if case.group == "exact" or k not in bounds:
            want = ref.to(F32).to(g.dtype)
            if not torch.equal(g, want):
                bad = (g.double() != want.double())
                i = int(bad.reshape(-1).nonzero()[0])
                raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements differ from the exact result; first at flat index {i}: "
                                     f"got {g.reshape(-1)[i].item()!r} want {want.reshape(-1)[i].item()!r}")
        else:
            r = _check_elem(g, ref, bounds[k], what)
            w = max(w, r)
            if g.dtype == F32:          # a bf16-stored result sits near 1.0 by construction (half a bf16 spacing against 2^-8 |ref|): kept apart
                w32 = max(w32, r)
    if worst is not None:
        worst[case.op] = max(worst.get(case.op, 0.0), w)
        worst[case.op + " (f32 results)"] = max(worst.get(case.op + " (f32 results)", 0.0), w32)
    return w


# ---------------------------------------------------------------------------------------------------------------- exact group: plumbing
@case("plumb-spans-fanout", "span", "exact")
def _():
    """overlapping column spans (offsets 3 and 4: neither a multiple of 8), overlapping row spans, a fan-out of x into an add whose (non-owned)
    gradient is there BEFORE the spans accumulate into theirs (spans are created first, so they run last in backward)."""
    g = gen(1)
    x, z = ints(g, 6, 24), ints(g, 6, 24)

    def tape(tp, V):
        a, b = tp.cols(V["x"], 3, 19), tp.cols(V["x"], 4, 20)
        r1, r2 = tp.rows(V["x"], 1, 5), tp.rows(V["x"], 2, 6)
        return dict(c=tp.add(a, b), r1=r1, r2=r2, s=tp.add(V["x"], V["z"]))

    def ref(P, V):
        x = V["x"]
        return dict(c=x[:, 3:19] + x[:, 4:20], r1=x[1:5], r2=x[2:6], s=x + V["z"])
    return prob({}, dict(x=(x, True), z=(z, True)), tape, ref, dict(c=ints(g, 6, 16), r1=ints(g, 4, 24), r2=ints(g, 4, 24), s=ints(g, 6, 24)))


@case("plumb-spans-bf16-first", "span", "exact")
def _():
    """a bf16 x whose only gradients come through spans: the first span makes the fp32 buffer from nothing."""
    g = gen(2)
    x = ints(g, 5, 16, dtype=BF16)

    def tape(tp, V):
        return dict(a=tp.cols(V["x"], 1, 9), b=tp.rows(V["x"], 0, 3))

    def ref(P, V):
        return dict(a=V["x"][:, 1:9], b=V["x"][0:3])
    return prob({}, dict(x=(x, True)), tape, ref, dict(a=ints(g, 5, 8, dtype=BF16), b=ints(g, 3, 16, dtype=BF16)))


@case("plumb-cat-mixed", "cat", "exact")
def _():
    """cat_tokens and cat_cols with mixed bf16 / f32 parts; the column slices of cat_cols's gradient go on through an add (non-owned views)."""
    g = gen(3)
    N, C = 2, 8
    a, b, c = ints(g, N * 2, C, dtype=BF16), ints(g, N * 3, C), ints(g, N * 1, C, dtype=BF16)
    u0, u1, w = ints(g, 5, 4, dtype=BF16), ints(g, 5, 4, dtype=BF16), ints(g, 5, 8)

    def tape(tp, V):
        u = tp.add(V["u0"], V["u1"])
        return dict(t=tp.cat_tokens([(V["a"], 2), (V["b"], 3), (V["c"], 1)], N), k=tp.cat_cols(u, V["w"]), k2=tp.cat_cols(V["w"], u))

    def ref(P, V):
        t = torch.cat([V["a"].view(N, 2, C), V["b"].view(N, 3, C), V["c"].view(N, 1, C)], 1).reshape(-1, C)
        u = V["u0"] + V["u1"]
        return dict(t=t, k=torch.cat([u, V["w"]], 1), k2=torch.cat([V["w"], u], 1))
    return prob({}, {k: (v, True) for k, v in dict(a=a, b=b, c=c, u0=u0, u1=u1, w=w).items()}, tape, ref,
                dict(t=ints(g, N * 6, C), k=ints(g, 5, 12, dtype=BF16), k2=ints(g, 5, 12)))


@case("plumb-repeat-mean-pair", "shape", "exact")
def _():
    """repeat_seq, mean_tokens with L = 4, pair_goal_current."""
    g = gen(4)
    B, L, C, times, Tn = 2, 4, 8, 3, 3
    x, f = ints(g, B * L, C, dtype=BF16), ints(g, B * Tn * L, C)

    def tape(tp, V):
        return dict(r=tp.repeat_seq(V["x"], B, L, times), m=tp.mean_tokens(V["x"], L), p=tp.pair_goal_current(V["f"], B, Tn, L))

    def ref(P, V):
        x, f4 = V["x"], V["f"].view(B, Tn, L, C)
        return dict(r=x.view(B, 1, L, C).expand(B, times, L, C).reshape(-1, C), m=x.view(B, L, C).mean(1),
                    p=torch.cat([f4[:, :1].expand(B, Tn, L, C), f4], 2).reshape(-1, C))
    return prob({}, dict(x=(x, True), f=(f, True)), tape, ref,
                dict(r=ints(g, B * times * L, C, dtype=BF16), m=ints(g, B, C), p=ints(g, B * Tn * 2 * L, C)), values=("r", "m", "p"))


@case("plumb-broadcast-param", "broadcast_param", "exact")
def _():
    """a sum of two tables broadcast over n = 3 sequences, two gradient sinks."""
    g = gen(5)
    L, C, n = 3, 8, 3
    params = dict(q=ints(g, L, C), t=ints(g, L, C), other=ints(g, 4))

    def tape(tp, V):
        P = tp.P
        return dict(y=tp.broadcast_param(P.w32("q") + P.w32("t"), [P.grad("q"), P.grad("t")], n))

    def ref(P, V):
        return dict(y=(P.w32("q") + P.w32("t")).unsqueeze(0).expand(n, L, C).reshape(n * L, C))
    return prob(params, {}, tape, ref, dict(y=ints(g, n * L, C)), prefill=dict(q=ints(g, L, C)), values=("y",))


for _n in (1, 2, 3):
    @case(f"add_table-x{_n}", "add_table", "exact")
    def _(n=_n):
        """rows = n x mod; the table is the head of a larger parameter, whose other rows keep their (prefilled) gradient."""
        g = gen(10 + n)
        mod, C = 3, 8
        params = dict(tab=ints(g, 1, 5, C))
        x = ints(g, n * mod, C)

        def tape(tp, V):
            return dict(y=tp.add_table(V["x"], "tab", mod))

        def ref(P, V):
            return dict(y=V["x"] + P.w32("tab").reshape(-1, C)[:mod].repeat(n, 1))
        return prob(params, dict(x=(x, True)), tape, ref, dict(y=ints(g, n * mod, C)), prefill=dict(tab=ints(g, 1, 5, C)), values=("y",))


for _base in (False, True):
    @case("col_scale-plain" + ("-base" if _base else ""), "col_scale", "exact")
    def _(base=_base):
        g = gen(20 + base)
        rows, C = 7, 16
        params = dict(gamma=dyad(g, C))
        vars = dict(x=(ints(g, rows, C, dtype=BF16), True))
        if base:
            vars["b"] = (ints(g, rows, C), True)

        def tape(tp, V):
            return dict(y=tp.col_scale(V["x"], "gamma", base=V.get("b")))

        def ref(P, V):
            y = V["x"] * P.w32("gamma")
            return dict(y=y + V["b"] if base else y)
        return prob(params, vars, tape, ref, dict(y=ints(g, rows, C, dtype=F32 if base else BF16)), prefill=dict(gamma=ints(g, C)), values=("y",))


for _f, _div, _base in (("id", 1, False), ("id", 4, True), ("one_plus", 1, True), ("one_plus", 4, False)):
    @case(f"modulate-{_f}-div{_div}" + ("-base" if _base else ""), "modulate", "exact")
    def _(f=_f, div=_div, base=_base):
        g = gen(30 + div + 2 * base + (7 if f == "id" else 0))
        rows, C = 8, 16
        vars = dict(x=(ints(g, rows, C, dtype=BF16), True), s=(ints(g, rows // div, C, lo=-2, hi=2), True))
        if base:
            vars["b"] = (ints(g, rows, C), True)

        def tape(tp, V):
            return dict(y=tp.modulate(V["x"], V["s"], f, div, base=V.get("b")))

        def ref(P, V):
            s = V["s"].repeat_interleave(div, 0)
            y = V["x"] * (1.0 + s if f == "one_plus" else s)
            return dict(y=y + V["b"] if base else y)
        return prob({}, vars, tape, ref, dict(y=ints(g, rows, C, dtype=F32 if base else BF16)), values=("y",))


# ---------------------------------------------------------------------------------------------------------------- exact group: _acc
@case("acc-dtype-then-f32-sum", "_acc", "exact")
def _():
    """three consumers of a bf16 x seeded 512, 1, 1: the first contribution stays bf16 (w.only), the second makes an fp32 sum, the third adds in
    place - a sum kept in bf16 would give 512 (514 ties to 512), the fp32 one 514; y1 has one consumer: its gradient stays bf16."""
    g = gen(40)
    x, y1 = ints(g, 5, 8, dtype=BF16), ints(g, 5, 8, dtype=BF16)
    z = [ints(g, 5, 8, dtype=BF16) for _ in range(4)]

    def tape(tp, V):
        return dict(a=tp.add(V["x"], V["z0"]), b=tp.add(V["x"], V["z1"]), c=tp.add(V["x"], V["z2"]), only=tp.add(V["y1"], V["z3"]))

    def ref(P, V):
        return dict(a=V["x"] + V["z0"], b=V["x"] + V["z1"], c=V["x"] + V["z2"], only=V["y1"] + V["z3"])
    one = torch.ones(5, 8, dtype=BF16)
    vars = dict(x=(x, True), y1=(y1, True), **{f"z{i}": (t, True) for i, t in enumerate(z)})
    return prob({}, vars, tape, ref, dict(a=one * 512, b=one, c=one, only=ints(g, 5, 8, dtype=BF16)),
                dtypes={"x.y1": BF16, "x.x": F32})


for _order in ("add-first", "add-last"):
    @case(f"acc-non-owned-{_order}", "_acc", "exact")
    def _(order=_order):
        """y = add(a, b) and a second consumer of a (a col_scale), in either creation order: b.g must still equal y.g afterwards - a non-owned first
        contribution (y.g itself) is never added into."""
        g = gen(41)
        a, b = ints(g, 5, 8), ints(g, 5, 8)
        params = dict(gamma=dyad(g, 8))

        def tape(tp, V):
            if order == "add-first":
                y = tp.add(V["a"], V["b"])
                z = tp.col_scale(V["a"], "gamma")
            else:
                z = tp.col_scale(V["a"], "gamma")
                y = tp.add(V["a"], V["b"])
            return dict(y=y, z=z)

        def ref(P, V):
            return dict(y=V["a"] + V["b"], z=V["a"] * P.w32("gamma"))
        return prob(params, dict(a=(a, True), b=(b, True)), tape, ref, dict(y=ints(g, 5, 8), z=ints(g, 5, 8)), watch=("y",))


# ---------------------------------------------------------------------------------------------------------------- exact group: linear
def _linear_case(id, rows, N, K, bias=True, wrows=None, residual=None, x_req=True, frozen=False, x_dtype=BF16, Nfull=None, seed=50, **kw):
    @case(id, "linear", "exact", **kw)
    def _():
        g = gen(seed)
        Nf = Nfull or N
        wt = dict(w=ints(g, Nf, K), b=ints(g, Nf))
        params = dict(dummy=ints(g, 8)) if frozen else dict(wt)
        vars = dict(x=(ints(g, rows, K, dtype=x_dtype), x_req))
        if residual is not None:
            vars["r"] = (ints(g, rows, N, dtype=residual), True)
        ydt = residual if residual is not None else BF16

        def tape(tp, V):
            return dict(y=tp.linear(V["x"], "w", "b" if bias else None, rows=wrows, residual=V.get("r")))

        def ref(P, V):
            W, b = P.w16("w"), P.w32("b")
            if wrows:
                W, b = W[wrows[0]:wrows[1]], b[wrows[0]:wrows[1]]
            y = st(V["x"], BF16) @ W.t()
            if bias:
                y = y + b
            return dict(y=y + V["r"] if residual is not None else y)
        prefill = {} if frozen else dict(w=ints(g, Nf, K), b=ints(g, Nf))
        return prob(params, vars, tape, ref, dict(y=ints(g, rows, N, dtype=ydt)), frozen=wt if frozen else None, prefill=prefill)


_linear_case("linear-bias", 5, 16, 8)
_linear_case("linear-nobias", 7, 8, 16, bias=False)
_linear_case("linear-f32-x", 6, 8, 8, x_dtype=F32)
_linear_case("linear-rows-head", 5, 8, 16, wrows=(0, 8), Nfull=24)
_linear_case("linear-rows-tail", 5, 16, 16, wrows=(8, 24), Nfull=24)
_linear_case("linear-residual-f32", 5, 8, 8, residual=F32)
_linear_case("linear-residual-bf16", 5, 8, 8, residual=BF16)
_linear_case("linear-x-noreq", 5, 8, 8, x_req=False)
_linear_case("linear-frozen", 5, 8, 8, frozen=True)
# the one-launch gemm_dw: 1, 4, 5, 8, 9 and 13 32-row slabs (131, 259 and 390 rows: not multiples of 4), then the row ranges at 2049 rows
for _rows in (32, 128, 131, 256, 259, 390):
    _linear_case(f"linear-dw-slabs-{_rows}", _rows, 8, 16, seed=60 + _rows)
_linear_case("linear-dw-ranges-2049", 2049, 8, 8, seed=59)


def _fallback_case(id, dt, ca, op="linear", group="exact", **kw):
    @case(id, op, group, **kw)
    def _():
        """the gradient of a linear arrives as a column slice of a cat_cols buffer: with ca = 4 leading columns its base (8 bytes bf16, 16 bytes f32)
        and row stride (20) break gemm_dw_ok's alignment rule, the five-launch fallback runs and the dX GEMM must get an aligned operand; ca = 8
        (row stride 24) is the aligned twin on the same values, which gemm_dw takes."""
        g = gen(70)
        rows, N, K = 13, 16, 8
        exact = group == "exact"
        mk = ints if exact else rnd
        params = dict(w=mk(g, N, K), b=mk(g, N))
        x, a_full, dy_full = mk(g, rows, K, dtype=BF16), mk(g, rows, 8, dtype=dt), mk(g, rows, 8 + N, dtype=dt)
        a, dy = a_full[:, :ca].contiguous(), dy_full[:, 8 - ca:].contiguous()

        def tape(tp, V):
            return dict(y=tp.cat_cols(V["a"], tp.linear(V["x"], "w", "b")))

        def ref(P, V):
            return dict(y=torch.cat([V["a"], st(V["x"] @ P.w16("w").t() + P.w32("b"), BF16)], 1))
        return prob(params, dict(x=(x, True), a=(a, True)), tape, ref, dict(y=dy), bounds=None if exact else (lambda c: _linear_bounds(c, dy[:, ca:])))


_fallback_case("linear-dw-fallback-f32", F32, 4, real_dw_ok=True)
_fallback_case("linear-dw-fallback-bf16", BF16, 4, real_dw_ok=True)
_fallback_case("linear-dw-aligned-f32", F32, 8, real_dw_ok=True)
_fallback_case("linear-dw-aligned-bf16", BF16, 8, real_dw_ok=True)
DW_TWINS = (("linear-dw-fallback-f32", "linear-dw-aligned-f32"), ("linear-dw-fallback-bf16", "linear-dw-aligned-bf16"))      # same values: same dW bits


# ---------------------------------------------------------------------------------------------------------------- bounds of the bounded group
def _ew_bound(ref, scale, dtype, n=1, k=16.0, cap=None):
    fb = R.fp32_bound(scale, n, k)
    if cap is not None and ref.numel():
        fb = torch.minimum(fb, torch.full_like(fb, cap * float(ref.abs().max())))
    return R.out_bound(ref, fb, dtype)


def _gemm_bound(ref, scale, K, dtype):
    return R.out_bound(ref, R.fp32_bound(scale, K, K_GEMM), dtype)


def _linear_bounds(c, dy, x="x", w="w", b="b", x_dtype=BF16):
    """dX = dy W (reduction over N), dW = dy^T x and db (reductions over the rows); operands exact (bf16 seeds, bf16 x, bf16 W)."""
    dy = dy.to(F64)
    xv, W = c.V[x].detach().to(F32).to(BF16).to(F64), c.P.w16(w).detach()
    out = {"x." + x: _gemm_bound(c.refs["x." + x], dy.abs() @ W.abs(), W.shape[0], x_dtype),
           "p." + w: _gemm_bound(c.refs["p." + w], dy.abs().t() @ xv.abs(), dy.shape[0], F32)}
    if b:
        out["p." + b] = _ew_bound(c.refs["p." + b], dy.abs().sum(0), F32, n=dy.shape[0])
    return out


# ---------------------------------------------------------------------------------------------------------------- bounded group: element-wise
_TACT = {"gelu_erf": Fn.gelu, "gelu_tanh": lambda t: Fn.gelu(t, approximate="tanh"), "relu": Fn.relu, "silu": Fn.silu}
for _kind in ("gelu_tanh", "silu", "relu", "gelu_erf"):          # every kind the heads pass (sft.py, navdp_train.py, train_layers.py)
    for _dt in (BF16, F32):
        @case(f"act-{_kind}-{TC.DTN[_dt]}", "act", "bounded")
        def _(kind=_kind, dt=_dt):
            g = gen(100)
            x, dy = rnd(g, 9, 24, scale=2.0, dtype=dt), rnd(g, 9, 24, dtype=dt)

            def bounds(c):
                ref, scale = R.act_bwd(x, dy, kind)
                return {"x.x": _ew_bound(ref, scale, dt, k=TC.act_k(kind, "bwd"), cap=2e-5)}
            return prob({}, dict(x=(x, True)), lambda tp, V: dict(y=tp.act(V["x"], kind)), lambda P, V: dict(y=_TACT[kind](V["x"])), dict(y=dy), bounds=bounds)


@case("glu", "glu", "bounded")
def _():
    g = gen(101)
    a, b, dy = rnd(g, 9, 24, scale=2.0, dtype=BF16), rnd(g, 9, 24, dtype=BF16), rnd(g, 9, 24, dtype=BF16)

    def bounds(c):
        k = max(TC.act_k("silu", "fwd"), TC.act_k("silu", "bwd"))
        (da, sa), (db, sb) = R.glu_bwd(a, b, dy)
        return {"x.a": _ew_bound(da, sa, BF16, k=k, cap=2e-5), "x.b": _ew_bound(db, sb, BF16, k=k, cap=2e-5)}
    return prob({}, dict(a=(a, True), b=(b, True)), lambda tp, V: dict(y=tp.glu(V["a"], V["b"])), lambda P, V: dict(y=Fn.silu(V["a"]) * V["b"]),
                dict(y=dy), bounds=bounds)


for _div, _base in ((1, False), (4, True)):
    @case(f"modulate-tanh-div{_div}" + ("-base" if _base else ""), "modulate", "bounded")
    def _(div=_div, base=_base):
        """ds = act_bwd(s, colsum(dy * x, groups of div rows), tanh): the column sum's bound times the slope's magnitude (1 + t^2 >= |1 - t^2|),
        plus the slope evaluation on the exact sum."""
        g = gen(110 + div)
        rows, C = 8, 16
        x, s = rnd(g, rows, C, dtype=BF16), rnd32(g, rows // div, C, scale=0.5)
        ydt = F32 if base else BF16
        dy = rnd(g, rows, C, dtype=ydt)
        vars = dict(x=(x, True), s=(s, True))
        if base:
            vars["b"] = (rnd32(g, rows, C), True)

        def ref(P, V):
            y = V["x"] * torch.tanh(V["s"]).repeat_interleave(div, 0)
            return dict(y=y + V["b"] if base else y)

        def bounds(c):
            dx, mag = R.affine(dy, scale=s, s_div=div, s_f="tanh")
            cs, cm = R.colsum(dy, x, group_rows=div)
            t = torch.tanh(s.to(F64))
            ds = R.fp32_bound(cm, div) * (1.0 + t * t) + R.fp32_bound(cs.abs() * (1.0 + t * t), 1, TC.act_k("tanh", "bwd"))
            return {"x.x": _ew_bound(dx, mag, BF16), "x.s": ds}
        return prob({}, vars, lambda tp, V: dict(y=tp.modulate(V["x"], V["s"], "tanh", div, base=V.get("b"))), ref, dict(y=dy), bounds=bounds)


@case("col_scale-tanh-heads", "col_scale", "bounded")
def _():
    """gamma[c] = tanh(gate[c // (C / H)]); d gate[h] = (1 - tanh^2) * sum over the head's columns of colsum(dy * x): one fp32 reduction over
    rows * C / H terms in the model (a column sum, a torch sum, one product)."""
    g = gen(120)
    rows, C, H = 7, 32, 4
    x, base, dy = rnd(g, rows, C, dtype=BF16), rnd32(g, rows, C), rnd(g, rows, C)
    params = dict(gate=rnd32(g, H, scale=0.5))

    def ref(P, V):
        return dict(y=V["x"] * torch.tanh(P.w32("gate")).repeat_interleave(C // H) + V["b"])

    def bounds(c):
        gate = params["gate"].to(F64)
        gv = gate.repeat_interleave(C // H).view(1, C)
        dx, mag = R.affine(dy, scale=gv, s_div=rows, s_f="tanh")
        m = (dy.to(F64) * x.to(F64)).abs().sum(0).view(H, -1).sum(1)
        t = torch.tanh(gate)
        return {"x.x": _ew_bound(dx, mag, BF16), "p.gate": R.fp32_bound(m * (1.0 + t * t), rows * (C // H))}
    return prob(params, dict(x=(x, True), b=(base, True)), lambda tp, V: dict(y=tp.col_scale(V["x"], "gate", base=V["b"], tanh_heads=H)), ref,
                dict(y=dy), bounds=bounds)


# ---------------------------------------------------------------------------------------------------------------- bounded group: norm
def _norm_case(id, rms, out_dtype, gamma, beta, x_dtype=F32, also_residual=False, rows=11, C=24):
    """gamma / beta: 'train' | 'frozen' | None."""
    @case(id, "norm", "bounded")
    def _():
        """dx: train_ops_ref.norm_bwd's model over C terms; d gamma = colsum(dy * bf16(xhat)) over the rows: the reduction's fp32 bound, 2^-8 of the
        |terms| for the bf16 xhat, and xhat's own fp32 error weighted with |dy|; d beta = colsum(dy). With `also_residual` x is consumed by an add
        as well: its gradient is the fp32 sum of the two contributions (one more fp32 addition)."""
        g = gen(130)
        eps = 1e-5
        x, dy = rnd(g, rows, C, scale=2.0, dtype=x_dtype, shift=0.5), rnd(g, rows, C, dtype=out_dtype)
        tens = {}
        if gamma:
            tens["gamma"] = rnd32(g, C, scale=0.2, shift=1.0)
        if beta:
            tens["beta"] = rnd32(g, C, scale=0.2)
        train = {k: v for k, v in tens.items() if (gamma if k == "gamma" else beta) == "train"}
        params = train or dict(dummy=torch.zeros(8))
        frozen = {k: v for k, v in tens.items() if k not in train}
        vars = dict(x=(x, True))
        seeds = dict(y=dy)
        if also_residual:
            vars["z"] = (rnd32(g, rows, C), True)
            seeds["r"] = rnd(g, rows, C)

        def tape(tp, V):
            out = dict(y=tp.norm(V["x"], "gamma" if gamma else None, "beta" if beta else None, eps, rms=rms, out_dtype=out_dtype))
            if also_residual:
                out["r"] = tp.add(V["x"], V["z"])
            return out

        def ref(P, V):
            xv = V["x"]
            d = xv if rms else xv - xv.mean(1, keepdim=True)
            y = d * torch.rsqrt((d * d).mean(1, keepdim=True) + R.f32(eps))
            if gamma:
                y = y * P.w32("gamma")
            if beta:
                y = y + P.w32("beta")
            out = dict(y=y)
            if also_residual:
                out["r"] = xv + V["z"]
            return out

        def bounds(c):
            (dx, sc), (xh, xs) = R.norm_bwd(x, dy, tens.get("gamma"), eps, rms)
            b = _ew_bound(dx, sc, x_dtype, n=C)
            if also_residual:
                tot = c.refs["x.x"]
                b = b + R.fp32_bound(dx.abs() + seeds["r"].to(F64).abs(), 1)
                assert torch.allclose(tot, dx + seeds["r"].to(F64), rtol=1e-9, atol=1e-12)
            out = {"x.x": b}
            ady = dy.to(F64).abs()
            if gamma == "train":
                terms = (ady * xh.abs()).sum(0)
                out["p.gamma"] = R.fp32_bound(terms, rows) + R.BF * terms + (ady * R.fp32_bound(xs, C)).sum(0)
                if beta:
                    out["p.beta"] = R.fp32_bound(ady.sum(0), rows)
            return out
        return prob(params, vars, tape, ref, seeds, frozen=frozen, bounds=bounds)


_norm_case("norm-ln-bf16-train", False, BF16, "train", "train")
_norm_case("norm-ln-f32-train", False, F32, "train", "train")
_norm_case("norm-ln-bf16x-train", False, BF16, "train", "train", x_dtype=BF16)
_norm_case("norm-rms-bf16-train", True, BF16, "train", None)
_norm_case("norm-rms-f32-frozen", True, F32, "frozen", None)
_norm_case("norm-ln-frozen", False, BF16, "frozen", "frozen")
_norm_case("norm-ln-absent", False, F32, None, None)
_norm_case("norm-ln-x-also-residual", False, BF16, "train", "train", also_residual=True)
_norm_case("norm-rms-x-also-residual-bf16x", True, BF16, "train", None, x_dtype=BF16, also_residual=True)


# ---------------------------------------------------------------------------------------------------------------- bounded group: attention
def attention_autograd_gap(q, k, v, do, causal):
    """max |closed form (delta from the float64 o) - float64 autograd| over dq, dk, dv, relative to the largest gradient: ties attn_bwd_ref's
    restatement to torch.autograd (the kernel's own definition takes delta from the stored bf16 o, which autograd does not know)."""
    D = q.shape[-1]
    qr, kr, vr = (t.to(F64).requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bqhd,bkhd->bhqk", qr, kr) * AB.f32(D ** -0.5)
    if causal:
        Lq, Lk = q.shape[1], k.shape[1]
        s = s.masked_fill(~(torch.arange(Lk)[None, :] <= torch.arange(Lq)[:, None] + (Lk - Lq)), float("-inf"))
    o = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), vr)
    gq, gk, gv = torch.autograd.grad(o, (qr, kr, vr), do.to(F64))
    r = AB.reference(q, k, v, o.detach().to(BF16), do, scale=D ** -0.5, causal=causal, mut="delta_f64", bounds=False)
    top = max(float(t.abs().max()) for t in (gq, gk, gv))
    return max(float((r[n][0] - t).abs().max()) for n, t in (("dq", gq), ("dk", gk), ("dv", gv))) / top


def _attn_case(id, B, Lq, Lk, H, D, layout, causal=False, **kw):
    """layout: 'packed' (q | k | v of one buffer), 'split' (q of its own, k | v packed, as _mha builds it), 'partial' (q the middle block of a
    3-block buffer, k | v blocks 0 and 2 of another 3-block buffer: the unused blocks' gradient is exactly zero)."""
    @case(id, "attention", "bounded", **kw)
    def _():
        g = gen(140 + Lq + D)
        Cd = H * D
        if layout == "packed":
            assert Lq == Lk
            vars = dict(qkv=(rnd(g, B * Lq, 3 * Cd, dtype=BF16), True))
            src = dict(q=("qkv", 0), k=("qkv", Cd), v=("qkv", 2 * Cd))
        elif layout == "split":
            vars = dict(qp=(rnd(g, B * Lq, Cd, dtype=BF16), True), kvp=(rnd(g, B * Lk, 2 * Cd, dtype=BF16), True))
            src = dict(q=("qp", 0), k=("kvp", 0), v=("kvp", Cd))
        else:
            vars = dict(qb=(rnd(g, B * Lq, 3 * Cd, dtype=BF16), True), kvb=(rnd(g, B * Lk, 3 * Cd, dtype=BF16), True))
            src = dict(q=("qb", Cd), k=("kvb", 0), v=("kvb", 2 * Cd))
        do = rnd(g, B * Lq, Cd, dtype=BF16)

        def tape(tp, V):
            s = {n: (V[a], c0) for n, (a, c0) in src.items()}
            return dict(o=tp.attention(s["q"], s["k"], s["v"], B, Lq, Lk, H, D, causal=causal))

        def blocks(T):
            return {n: T[a][:, c0:c0 + Cd].view(B, Lq if n == "q" else Lk, H, D) for n, (a, c0) in src.items()}

        def ref(P, V):
            b = blocks(V)
            s = torch.einsum("bqhd,bkhd->bhqk", b["q"], b["k"]) * AB.f32(D ** -0.5)
            if causal:
                s = s.masked_fill(~(torch.arange(Lk)[None, :] <= torch.arange(Lq)[:, None] + (Lk - Lq)), float("-inf"))
            return dict(o=torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), b["v"]).reshape(B * Lq, Cd))
        pb = prob({}, vars, tape, ref, dict(o=do), values=("o",))

        def bounds(c):
            """the stored o, after attn_fwd_ref's model: P is rounded to bf16 before P V and o once more (2^-8 (A + |o|), A = sum_k P |v|); the fp32
            logits (f T per key, T = scale sum_d |q||k|), exponentials and sums add A (f (1 + T) + 4 2^-24 (|M| + 8)), doubled for the normaliser."""
            b = blocks({k: t.to(F64) for k, (t, _) in vars.items()})
            sc = AB.f32(D ** -0.5)
            s = torch.einsum("bqhd,bkhd->bhqk", b["q"], b["k"]) * sc
            Tm = torch.einsum("bqhd,bkhd->bhqk", b["q"].abs(), b["k"].abs()) * sc
            if causal:
                s = s.masked_fill(~(torch.arange(Lk)[None, :] <= torch.arange(Lq)[:, None] + (Lk - Lq)), float("-inf"))
            A = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), b["v"].abs()).reshape(B * Lq, Cd)
            f = 16.0 * R.U * (math.sqrt(max(Lk, D)) + 4.0)
            eps = f * (1.0 + float(Tm.max())) + 4.0 * R.U * (float(s[torch.isfinite(s)].abs().max()) + 8.0)
            o64 = c.refs["v.o"]
            return {"v.o": R.BF * (A + o64.abs()) * (1.0 + 2.0 ** -6) + 2.0 * A * eps}
        pb.bounds = bounds
        pb.attn = NS(src=src, blocks=blocks, do=do, B=B, Lq=Lq, Lk=Lk, H=H, D=D, causal=causal)
        return pb


def attention_check(case, got):
    """dq / dk / dv of an attention case against attn_bwd_ref.reference - the function the kernel defines - evaluated at the tape's own stored bf16 o
    (`v.o`, the GIVEN o of that function, as in tests/test_attention_bwd_fp64_gpu.py), with attn_bwd_ref's bound unmodified; column blocks no
    operand uses carry bound 0: exactly zero. Returns the worst |err| / bound."""
    pb = built(case)
    a = pb.attn
    T = {k: t for k, (t, _) in pb.vars.items()}
    b = a.blocks(T)
    o = got["v.o"].detach().cpu().view(a.B, a.Lq, a.H, a.D)
    r = AB.reference(b["q"], b["k"], b["v"], o, a.do.view(a.B, a.Lq, a.H, a.D), scale=a.D ** -0.5, causal=a.causal)
    Cd = a.H * a.D
    want = {k: (torch.zeros(t.shape, dtype=F64), torch.zeros(t.shape, dtype=F64)) for k, t in T.items()}
    for n, (src, c0) in a.src.items():
        ref, bound = r["d" + n]
        want[src][0][:, c0:c0 + Cd] = ref.reshape(-1, Cd)
        want[src][1][:, c0:c0 + Cd] = bound.reshape(-1, Cd)
    worst = 0.0
    for k, (ref, bound) in want.items():
        g = got["x." + k].detach().cpu()
        assert g.dtype == BF16 and g.shape == ref.shape, f"{case.id} x.{k}: {g.dtype} {tuple(g.shape)}"
        worst = max(worst, _check_elem(g, ref, bound, f"{case.id} x.{k}"))
    return worst


_attn_case("attention-packed-d48", 2, 7, 7, 2, 48, "packed")
_attn_case("attention-packed-causal-d64", 2, 6, 6, 2, 64, "packed", causal=True)
_attn_case("attention-split-d64", 2, 5, 9, 2, 64, "split")
_attn_case("attention-split-causal-d48", 2, 3, 8, 2, 48, "split", causal=True)
_attn_case("attention-partial-blocks-d48", 2, 4, 6, 2, 48, "partial", nan_fill=True)
_attn_case("attention-partial-blocks-d64", 1, 5, 3, 2, 64, "partial", nan_fill=True)


# ---------------------------------------------------------------------------------------------------------------- bounded group: small linears
def _small_linear_case(id, rows, N, K, xkind, tab):
    """xkind: 'bf16' | 'f32' (a Var) | 'plain' (a tensor, an input of the step)."""
    @case(id, "small_linear", "bounded")
    def _():
        """dW[n, k] = sum_r dy[r, n] x[r, k] and db over the rows, dx = dy W over N: one fp32 reduction each."""
        g = gen(150 + K)
        xdt = BF16 if xkind == "bf16" else F32
        x, dy = rnd(g, rows, K, dtype=xdt), rnd(g, rows, N)
        params = {"h.weight": rnd32(g, N, K, scale=K ** -0.5), "h.bias": rnd32(g, N)}
        tb = rnd32(g, 3, N) if tab else None

        def tape(tp, V):
            return dict(y=tp.small_linear(V["x"], "h", tab=None if tb is None else tb.to(tp.store.p32.device)))

        def ref(P, V):
            y = V["x"].to(F64) @ P.w32("h.weight").t() + P.w32("h.bias")
            return dict(y=y + tb.to(F64).repeat((rows + 2) // 3, 1)[:rows] if tab else y)

        def bounds(c):
            d, xv, W = dy.to(F64).abs(), x.to(F64).abs(), params["h.weight"].to(F64).abs()
            out = {"p.h.weight": R.fp32_bound(d.t() @ xv, rows), "p.h.bias": R.fp32_bound(d.sum(0), rows)}
            if xkind != "plain":
                out["x.x"] = _ew_bound(c.refs["x.x"], d @ W, xdt, n=N)
            return out
        return prob(params, dict(x=(x, None if xkind == "plain" else True)), tape, ref, dict(y=dy), bounds=bounds)


_small_linear_case("small_linear-K3-plain-tab", 9, 16, 3, "plain", True)
_small_linear_case("small_linear-K2-f32", 9, 8, 2, "f32", False)
_small_linear_case("small_linear-K16-bf16", 11, 3, 16, "bf16", False)
_small_linear_case("small_linear-K24-f32-tab", 6, 1, 24, "f32", True)


def _mse_case(id, blocks, mask, loss_scale, x_dtype=BF16):
    @case(id, "mse_head", "bounded")
    def _():
        """out = x W^T + b (fp32, error e_out <= the small_linear bound over K) -> dout = 2 m (out - t) ls / den (mse_masked's bound + 2 m ls / den * e_out)
        -> dW, db (reductions over the rows, dout's error carried with |x| weights) and dx = dout W (over D, carried with |W| weights, bf16-stored
        for a bf16 x). The reported losses are unscaled; an all-zero mask gives loss 0 and every gradient exactly 0 (no bound: exact)."""
        g = gen(160 + blocks)
        nseq, T, D, K = len(mask), 3, 3, 16
        n = nseq * T
        x, target = rnd(g, blocks * n, K, dtype=x_dtype), rnd32(g, blocks * n, D)
        m = torch.tensor(mask, dtype=F32)
        params = {"h.weight": rnd32(g, D, K, scale=K ** -0.5), "h.bias": rnd32(g, D)}

        def tape(tp, V):
            losses = tp.mse_head(V["x"], "h", target.to(tp.store.p32.device), m.to(tp.store.p32.device), T, loss_scale, blocks=blocks)
            return {f"loss{i}": l for i, l in enumerate(losses)}

        def losses64(P, V):
            out = V["x"] @ P.w32("h.weight").t() + P.w32("h.bias")
            res = {}
            for i in range(blocks):
                e = out[i * n:(i + 1) * n] - target.to(F64)[i * n:(i + 1) * n]
                den = m.to(F64).sum() * T * D
                w = m.to(F64).repeat_interleave(T)[:, None]
                res[f"loss{i}"] = ((w * e * e).sum() / den if den > 0 else (e * 0).sum()).view(1)
            return res

        def bounds(c):
            if not any(mask):
                return {}
            W, b, xv = params["h.weight"].to(F64), params["h.bias"].to(F64), x.to(F64)
            out = xv @ W.t() + b
            e_out = R.fp32_bound(xv.abs() @ W.abs().t() + b.abs(), K)
            bl, dout, e_d = {}, [], []
            for i in range(blocks):
                sl = slice(i * n, (i + 1) * n)
                (loss, ls_), (d, ds_) = R.mse_masked(out[sl], target[sl], m, T, loss_scale)
                den = float(m.sum()) * T * D
                w = m.to(F64).repeat_interleave(T)[:, None]
                e_d.append(R.fp32_bound(ds_, 1) + 2.0 * w * abs(R.f32(loss_scale)) / den * e_out[sl])
                dout.append(d)
                bl[f"v.loss{i}"] = R.fp32_bound(ls_, n * D) + (2.0 * w * (out[sl] - target[sl].to(F64)).abs() * e_out[sl]).sum().view(1) / den
            d, e_d = torch.cat(dout), torch.cat(e_d)
            bl["p.h.weight"] = R.fp32_bound(d.abs().t() @ xv.abs(), blocks * n) + e_d.t() @ xv.abs()
            bl["p.h.bias"] = R.fp32_bound(d.abs().sum(0), blocks * n) + e_d.sum(0)
            bl["x.x"] = _ew_bound(c.refs["x.x"], d.abs() @ W.abs(), x_dtype, n=D) + e_d @ W.abs()
            return bl
        return prob(params, dict(x=(x, True)), tape, losses64, {}, bounds=bounds, values=tuple(f"loss{i}" for i in range(blocks)),
                    ref_loss=lambda outs: loss_scale * sum(o.sum() for o in outs.values()))


_mse_case("mse_head-1block", 1, (1.0, 1.0, 1.0), 1.0)
_mse_case("mse_head-2blocks-masked-scaled", 2, (1.0, 0.0, 1.0, 0.0), 0.4)
_mse_case("mse_head-f32x-masked-scaled", 1, (0.0, 1.0), 2.5, x_dtype=F32)
_mse_case("mse_head-all-masked", 2, (0.0, 0.0), 0.4)


# ---------------------------------------------------------------------------------------------------------------- bounded group: linear, N(0,1)
def _linear_rand(id, rows, N, K, **kw):
    @case(id, "linear", "bounded", **kw)
    def _():
        g = gen(170 + rows)
        params = dict(w=rnd(g, N, K, scale=K ** -0.5), b=rnd32(g, N))
        x, dy = rnd(g, rows, K, dtype=BF16), rnd(g, rows, N, dtype=BF16)
        return prob(params, dict(x=(x, True)), lambda tp, V: dict(y=tp.linear(V["x"], "w", "b")),
                    lambda P, V: dict(y=V["x"] @ P.w16("w").t() + P.w32("b")), dict(y=dy), bounds=lambda c: _linear_bounds(c, dy))


_linear_rand("linear-rand-dw-one-launch", 37, 16, 24)
_linear_rand("linear-rand-dw-ranges", 2049, 8, 8)
_fallback_case("linear-rand-dw-fallback-bf16", BF16, 4, group="bounded", real_dw_ok=True)
_fallback_case("linear-rand-dw-fallback-f32", F32, 4, group="bounded", real_dw_ok=True)


# ---------------------------------------------------------------------------------------------------------------- the transpose cache
@case("wt-cache-after-adamw", "linear", "bounded")
def _():
    """backward, adamw_step (lr 0.5: every weight moves by about 0.5), a second forward and backward on the SAME tape: the second dX must be
    dy @ (the store's new bf16 weights) - a W^T cached from before the step is off by far more than the GEMM bound. The new weights are READ from
    the store (the only independent check on them: each moved by more than 0.1): this case is about which W^T the second backward uses, not about the
    optimiser update, which tests/test_train_kernels_fp64_gpu.py checks."""
    g = gen(180)
    rows, N, K = 9, 16, 8
    w, b, x = rnd(g, N, K, scale=K ** -0.5), rnd32(g, N), rnd(g, rows, K, dtype=BF16)
    dy1, dy2 = rnd(g, rows, N, dtype=BF16), rnd(g, rows, N, dtype=BF16)
    pb = prob(dict(w=w, b=b), {}, None, None, {})
    state = {}

    def custom(device):
        from internnav_amd.tape import ParamStore, Tape, Var

        store = ParamStore(dict(w=w, b=b), device)
        tp = Tape(store)
        got = {}
        for i, dy in enumerate((dy1, dy2)):
            xv = Var(x.to(device))
            y = tp.linear(xv, "w", "b")
            Tape.accumulate(y, dy.to(device))
            tp.backward()
            got[f"x.pass{i}"] = xv.g
            if i == 0:
                store.adamw_step(0.5, max_norm=0.0)
                state["w16"] = store.w16("w").detach().cpu().clone()
        assert float((state["w16"].float() - w).abs().min()) > 0.1, "the optimiser step did not move the weights"
        return got

    def custom_ref():
        refs, bounds = {}, {}
        for i, (dy, W) in enumerate(((dy1, w.to(BF16)), (dy2, state["w16"]))):
            refs[f"x.pass{i}"] = dy.to(F64) @ W.to(F64)
            bounds[f"x.pass{i}"] = _gemm_bound(refs[f"x.pass{i}"], dy.to(F64).abs() @ W.to(F64).abs(), N, BF16)
        return refs, bounds
    pb.custom, pb.custom_ref = custom, custom_ref
    return pb


# ---------------------------------------------------------------------------------------------------------------- dropout
@case("dropout-p0.5", "dropout", "exact", cpu_skip="the stand-ins cover the eval-mode graph: they draw no dropout mask")
def _():
    """p = 0.5: the output is exactly 0 or 2 x, the gradient exactly 0 where the output is 0 and exactly 2 dy elsewhere; the same tape seed gives the
    same mask again, the next site of a tape another one."""
    g = gen(190)
    x, dy = ints(g, 24, 32, lo=1, hi=4, dtype=BF16), ints(g, 24, 32, lo=1, hi=4, dtype=BF16)
    pb = prob({}, {}, None, None, {})

    def custom(device):
        from internnav_amd.tape import ParamStore, Tape, Var

        store = ParamStore(dict(dummy=torch.zeros(8)), device)
        res = []
        for seed in (5, 5):
            tp = Tape(store, drop_p=0.5, seed=seed)
            xs = [Var(x.to(device)), Var(x.to(device))]
            ys = [tp.dropout(v) for v in xs]
            for y in ys:
                Tape.accumulate(y, dy.to(device))
            tp.backward()
            assert tp.sites == {"dropout": 2, "attention": 0}
            res.append([(y.v.cpu(), v.g.cpu()) for y, v in zip(ys, xs)])
        for y, gx in res[0]:
            keep = y != 0
            assert 0.3 < float(keep.float().mean()) < 0.7
            assert torch.equal(y, torch.where(keep, 2 * x, torch.zeros_like(x))), "dropout output is not 0 | 2 x"
            assert torch.equal(gx, torch.where(keep, 2 * dy, torch.zeros_like(dy))), "dropout gradient is not 0 | 2 dy under the forward's mask"
        assert torch.equal(res[0][0][0], res[1][0][0]) and torch.equal(res[0][1][0], res[1][1][0]), "the same seed drew another mask"
        assert not torch.equal(res[0][0][0] != 0, res[0][1][0] != 0), "the second dropout site drew the first one's mask"
        return {}
    pb.custom, pb.custom_ref = custom, lambda: ({}, {})
    return pb


# ---------------------------------------------------------------------------------------------------------------- layers
LAYERS = []


def layer(id, **kw):
    def deco(fn):
        LAYERS.append(NS(id=id, build=fn, op="layer", group="layer", **kw))
        return fn
    return deco


def bf16_weights(sd):
    """matrices bf16-representable (the store's bf16 working copy then IS the fp32 master weight the module is loaded with), vectors left fp32."""
    return {k: (v.to(BF16).to(F32) if v.dim() >= 2 else v) for k, v in sd.items()}


def _rand_module_params(mod, g, prefix):
    sd = {}
    for k, v in mod.state_dict().items():
        if v.dim() == 1 and k.endswith("weight"):          # the LayerNorm weights (every other weight here is a matrix)
            t = rnd32(g, *v.shape, scale=0.2, shift=1.0)
        elif v.dim() == 1:
            t = rnd32(g, *v.shape, scale=0.2)
        else:
            t = rnd32(g, *v.shape, scale=v.shape[-1] ** -0.5)
        sd[prefix + k] = t
    return bf16_weights(sd)


RELU_GAP = 2.0 ** -5          # 8 x the bf16 spacing at 1: an order of magnitude above the error of a pre-activation of size ~1 in either precision


def _open_relu_gap(z, bias):
    """ReLU's derivative jumps at 0: a pre-activation within rounding error of 0 switches its unit's whole gradient on or off in one precision and
    not in the other - in the engine and in the bf16-autocast yardstick alike (~1 % of N(0,1) values lie that close), which is noise on the bar, not
    wiring. The layer cases therefore shift each linear1 bias by the smallest multiple of RELU_GAP / 2 after which no row of the float64
    REFERENCE's pre-activations z [rows, F] is within RELU_GAP of 0. Only the reference is consulted; what feeds linear1 does not depend on its bias."""
    z = z.reshape(-1, z.shape[-1]).to(F64)
    out = bias.to(F64).clone()
    for j in range(z.shape[1]):
        s = next(s for m in range(4 * z.shape[0] + 4) for s in (m * RELU_GAP / 2, -m * RELU_GAP / 2) if float((z[:, j] + s).abs().min()) >= RELU_GAP)
        out[j] += s
    return out.to(F32)


def _gap_linear1(mod, params, prefix, ref, inputs):
    """apply _open_relu_gap to `mod.linear1` (parameters under `prefix`) from a float64 run of the reference `ref(P, X, dtype)`."""
    zs = []
    h = mod.linear1.register_forward_hook(lambda m, i, o: zs.append(o.detach()))
    with torch.no_grad():
        ref({k: v.to(F64) for k, v in params.items()}, {k: v.to(F64) for k, v in inputs.items()}, F64)
    h.remove()
    params[prefix + "linear1.bias"] = _open_relu_gap(zs[0], params[prefix + "linear1.bias"])


def _causal(L):
    return torch.triu(torch.ones(L, L, dtype=torch.bool), 1)          # True: masked


def layer_run(lc, device):
    """the layer on the tape -> name -> tensor (v.*: outputs, x.*: input gradients, p.*: every parameter gradient)."""
    from internnav_amd.tape import ParamStore, Tape, Var

    pb = built(lc)
    store = ParamStore(pb.params, device)
    tp = Tape(store, drop_p=pb.drop_p, seed=3)
    V = {k: Var(t.clone().to(device)) for k, t in pb.inputs.items()}
    out = pb.tape(tp, V)
    Tape.accumulate(out, pb.dy.clone().to(device))
    tp.backward()
    got = {"v.out": out.v.float().cpu()}
    got.update({"x." + k: v.g.float().cpu() for k, v in V.items()})
    got.update({"p." + k: store.grad(k).clone().cpu() for k in pb.params})
    if pb.expect_sites is not None:
        assert tp.sites == pb.expect_sites, (tp.sites, pb.expect_sites)
    return got


def layer_reference(lc, dtype, autocast):
    """the torch module in `dtype` (float64: the reference; float32 under bf16 autocast: the yardstick) on the same weights, inputs and seed."""
    pb = built(lc)
    P = {k: v.to(dtype).requires_grad_(True) for k, v in pb.params.items()}
    X = {k: v.to(dtype).requires_grad_(True) for k, v in pb.inputs.items()}
    with torch.autocast("cpu", dtype=BF16, enabled=autocast):
        out = pb.ref(P, X, dtype)
    (out.to(dtype) * pb.dy.to(dtype)).sum().backward()
    res = {"v.out": out.detach().to(F64)}
    res.update({"x." + k: v.grad.to(F64) for k, v in X.items()})
    res.update({"p." + k: (torch.zeros_like(v) if v.grad is None else v.grad).to(F64) for k, v in P.items()})
    return res


def layer_check(lc, got, table=None):
    """per tensor: rel. norm error against float64 <= 1.25 x that of the float32 module under bf16 autocast (tensors below 1e-6 of the largest
    norm: norm below 1e-4 of it). Returns the worst engine / yardstick ratio."""
    ref, yard = layer_reference(lc, F64, False), layer_reference(lc, F32, True)
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))
    top = max(float(v.norm()) for k, v in ref.items() if k[0] != "v")
    worst, fails = 0.0, []
    for k, r in ref.items():
        g = got[k].to(F64).view_as(r)
        if k[0] != "v" and float(r.norm()) < 1e-6 * top:
            assert float(g.norm()) < 1e-4 * top, f"{lc.id} {k}: a gradient where (almost) none is due"
            continue
        e, y = float((g - r).norm() / r.norm()), float((yard[k] - r).norm() / r.norm())
        ratio = e / y if y > 0 else (0.0 if e == 0 else float("inf"))
        worst = max(worst, ratio)
        if table is not None:
            table.append(f"{lc.id:34s} {k:48s} engine {e:.3e}  bf16-autocast {y:.3e}  ratio {ratio:.2f}")
        if not e <= MARGIN * y:
            fails.append(f"{k}: engine {e:.3e} vs {MARGIN} x bf16-autocast {y:.3e}")
    assert not fails, f"{lc.id}: " + "; ".join(fails)
    return worst


def _lprob(params, inputs, tape, ref, dy, drop_p=0.0, expect_sites=None):
    return NS(params=params, inputs=inputs, tape=tape, ref=ref, dy=dy, drop_p=drop_p, expect_sites=expect_sites)


def _load(mod, P, prefix, dtype):
    """the module's forward as a function of the leaves P (torch.func.functional_call keeps the graph to them)."""
    sd = {k[len(prefix):]: v for k, v in P.items() if k.startswith(prefix)}
    return lambda *a, **kw: torch.func.functional_call(mod.to(dtype), sd, a, kw)


def _mha_case(id, d, H, B, Lq, Lk, self_attn, residual, causal=False, no_attn_dropout=False):
    @layer(id)
    def _():
        from internnav_amd import train_layers as TL

        g = gen(200 + Lq + d)
        mod = nn.MultiheadAttention(d, H, dropout=0.0, batch_first=True)
        params = _rand_module_params(mod, g, "a.")
        inputs = dict(x=rnd32(g, B * Lq, d))
        if not self_attn:
            inputs["mem"] = rnd32(g, B * Lk, d)

        def tape(tp, V):
            kv = V["x"] if self_attn else V["mem"]
            return TL._mha(tp, V["x"], kv, "a", B, Lq, Lk, H, d, residual=V["x"] if residual else None, causal=causal,
                           attn_dropout=not no_attn_dropout)

        def ref(P, X, dtype):
            x = X["x"].view(B, Lq, d)
            kv = x if self_attn else X["mem"].view(B, Lk, d)
            y = _load(mod, P, "a.", dtype)(x, kv, kv, need_weights=False, attn_mask=_causal(Lq) if causal else None)[0]
            return ((x + y) if residual else y).reshape(B * Lq, d)
        # attn_dropout=False on a tape that trains with dropout and no residual: no mask anywhere, the eval-mode module is the reference
        return _lprob(params, inputs, tape, ref, rnd(g, B * Lq, d, dtype=F32 if residual else BF16), drop_p=0.5 if no_attn_dropout else 0.0,
                      expect_sites={"dropout": 0, "attention": 0})


_mha_case("mha-self-d96-residual", 96, 2, 2, 5, 5, True, True)
_mha_case("mha-self-d128-causal", 128, 2, 2, 6, 6, True, False, causal=True)
_mha_case("mha-split-d128-residual", 128, 2, 2, 4, 7, False, True)
_mha_case("mha-split-d96", 96, 2, 2, 3, 6, False, False)
_mha_case("mha-self-d96-no-attn-dropout", 96, 2, 2, 5, 5, True, False, no_attn_dropout=True)


@layer("ffn-d96")
def _():
    from internnav_amd import train_layers as TL

    g = gen(210)
    d, rows = 96, 11
    mod = nn.TransformerEncoderLayer(d, 2, 64, 0.0, batch_first=True)
    params = {k: v for k, v in _rand_module_params(mod, g, "f.").items() if ".linear" in k}
    inputs = dict(x=rnd32(g, rows, d))

    def ref(P, X, dtype):
        h = Fn.relu(Fn.linear(X["x"], P["f.linear1.weight"], P["f.linear1.bias"]))
        return X["x"] + Fn.linear(h, P["f.linear2.weight"], P["f.linear2.bias"])
    z = inputs["x"].to(F64) @ params["f.linear1.weight"].to(F64).t() + params["f.linear1.bias"].to(F64)
    params["f.linear1.bias"] = _open_relu_gap(z, params["f.linear1.bias"])
    return _lprob(params, inputs, lambda tp, V: TL._ffn(tp, V["x"], "f", "relu", V["x"]), ref, rnd(g, rows, d), expect_sites={"dropout": 0, "attention": 0})


def _tlayer_case(id, kind, d, B, Lq, Lm):
    @layer(id)
    def _():
        from internnav_amd import train_layers as TL

        g = gen(220 + d + Lq)
        H = 2
        if kind == "encoder":
            mod = nn.TransformerEncoderLayer(d, H, 64, 0.0, batch_first=True, norm_first=False)
        else:
            mod = nn.TransformerDecoderLayer(d, H, 64, 0.0, activation="gelu" if kind == "prenorm" else "relu", batch_first=True, norm_first=kind == "prenorm")
        params = _rand_module_params(mod, g, "L.")
        inputs = dict(x=rnd32(g, B * Lq, d))
        if kind != "encoder":
            inputs["mem"] = rnd32(g, B * Lm, d)

        def tape(tp, V):
            if kind == "encoder":
                return TL.encoder_layer(tp, V["x"], "L", B, Lq, H, d)
            if kind == "decoder":
                return TL.decoder_layer(tp, V["x"], V["mem"], "L", B, Lq, Lm, H, d)
            return TL.decoder_layer_prenorm(tp, V["x"], V["mem"], "L", B, Lq, Lm, H, d, causal=True)

        def ref(P, X, dtype):
            f, x = _load(mod, P, "L.", dtype), X["x"].view(B, Lq, d)
            if kind == "encoder":
                return f(x).reshape(B * Lq, d)
            mem = X["mem"].view(B, Lm, d)
            return f(x, mem, tgt_mask=_causal(Lq) if kind == "prenorm" else None).reshape(B * Lq, d)
        if kind != "prenorm":
            _gap_linear1(mod, params, "L.", ref, inputs)
        return _lprob(params, inputs, tape, ref, rnd(g, B * Lq, d))


_tlayer_case("encoder_layer-d96", "encoder", 96, 2, 7, 0)
_tlayer_case("encoder_layer-d128", "encoder", 128, 2, 3, 0)
_tlayer_case("decoder_layer-d128", "decoder", 128, 2, 5, 7)
_tlayer_case("decoder_layer-d96", "decoder", 96, 2, 4, 3)
_tlayer_case("decoder_layer_prenorm-causal-d96", "prenorm", 96, 2, 6, 4)
_tlayer_case("decoder_layer_prenorm-causal-d128", "prenorm", 128, 2, 3, 5)


@layer("rgbd_former")
def _():
    """fixed at H = 8, d = 384; n = 2 sequences of Lf = 6 tokens, Lm = 3 queries; the positional table has 8 rows (2 unused: zero gradient)."""
    from internnav_amd import train_layers as TL

    g = gen(230)
    n, Lf, Lm, d, tok_dim = 2, 6, 3, 384, 32
    mods = [nn.TransformerDecoderLayer(d, 8, 64, 0.0, batch_first=True) for _ in range(2)]
    params = {}
    for i, m in enumerate(mods):
        params.update(_rand_module_params(m, g, f"rgbd_encoder.former_net.layers.{i}."))
    params.update(bf16_weights({"rgbd_encoder.project_layer.weight": rnd32(g, tok_dim, d, scale=d ** -0.5),
                                "rgbd_encoder.project_layer.bias": rnd32(g, tok_dim, scale=0.2)}))
    params["rgbd_encoder.former_pe.weight"] = rnd32(g, 8, d, scale=0.5)
    params["rgbd_encoder.former_query.weight"] = rnd32(g, Lm, d)
    inputs = dict(tok=rnd32(g, n * Lf, d))

    def ref(P, X, dtype):
        tok = (X["tok"].view(n, Lf, d) + P["rgbd_encoder.former_pe.weight"][:Lf])
        q = P["rgbd_encoder.former_query.weight"].unsqueeze(0).expand(n, Lm, d)
        for i, m in enumerate(mods):
            q = _load(m, P, f"rgbd_encoder.former_net.layers.{i}.", dtype)(q, tok)
        return Fn.linear(q, P["rgbd_encoder.project_layer.weight"], P["rgbd_encoder.project_layer.bias"]).reshape(n * Lm, tok_dim)
    for i, m in enumerate(mods):          # in order: layer 1's input depends on layer 0's bias
        _gap_linear1(m, params, f"rgbd_encoder.former_net.layers.{i}.", ref, inputs)
    return _lprob(params, inputs, lambda tp, V: TL.rgbd_former(tp, V["tok"], n, Lf, Lm, "former_pe.weight", "former_query.weight"), ref,
                  rnd(g, n * Lm, tok_dim, dtype=BF16))


@layer("dino-depth1")
def _():
    """DinoTrain with DEPTH = 1 on one 224 x 224 frame (257 tokens) against a restatement of DinoVisionTransformer in the test: F.conv2d patch
    embed, the dinov2 bicubic pos-embed interpolation (scale (16 + 0.1) / 37), cls token, one block with LayerScale, the final norm, cls dropped."""
    from internnav_amd import train_layers as TL

    g = gen(240)
    D, Hh, p = 384, 6, "rgb."
    sd = {p + "patch_embed.proj.weight": rnd32(g, D, 3, 14, 14, scale=588 ** -0.5), p + "patch_embed.proj.bias": rnd32(g, D, scale=0.2),
          p + "pos_embed": rnd32(g, 1, 1370, D, scale=0.5), p + "cls_token": rnd32(g, 1, 1, D, scale=0.5),
          p + "norm.weight": rnd32(g, D, scale=0.2, shift=1.0), p + "norm.bias": rnd32(g, D, scale=0.2)}
    b = p + "blocks.0."
    for nm, shape in (("attn.qkv", (3 * D, D)), ("attn.proj", (D, D)), ("mlp.fc1", (4 * D, D)), ("mlp.fc2", (D, 4 * D))):
        sd[b + nm + ".weight"], sd[b + nm + ".bias"] = rnd32(g, *shape, scale=shape[1] ** -0.5), rnd32(g, shape[0], scale=0.2)
    for nm in ("norm1", "norm2"):
        sd[b + nm + ".weight"], sd[b + nm + ".bias"] = rnd32(g, D, scale=0.2, shift=1.0), rnd32(g, D, scale=0.2)
    sd[b + "ls1.gamma"], sd[b + "ls2.gamma"] = rnd32(g, D, scale=0.3, shift=0.5), rnd32(g, D, scale=0.3, shift=0.5)
    params = bf16_weights(sd)
    params[p + "pos_embed"], params[p + "cls_token"] = sd[p + "pos_embed"], sd[p + "cls_token"]          # fp32 tables, not GEMM operands
    frames = torch.rand(1, 224, 224, 3, generator=g)
    pb = _lprob(params, {}, None, None, rnd(g, 256, D))

    def ref(P, X, dtype):
        mean, std = (torch.tensor(v, dtype=dtype).view(1, 3, 1, 1) for v in (TL.RESNET_MEAN, TL.RESNET_STD))
        img = ((frames.to(dtype).permute(0, 3, 1, 2) - mean) / std)
        img = img.to(F32).to(BF16).to(dtype) if dtype == F64 else img        # the im2col rows are stored in bf16 (an input, no gradient)
        x = Fn.conv2d(img, P[p + "patch_embed.proj.weight"], P[p + "patch_embed.proj.bias"], stride=14).flatten(2).transpose(1, 2)      # [1, 256, D]
        pos = P[p + "pos_embed"]
        with torch.autocast("cpu", enabled=False):
            grid = Fn.interpolate(pos[:, 1:].reshape(1, 37, 37, D).permute(0, 3, 1, 2), scale_factor=(16.1 / 37, 16.1 / 37), mode="bicubic", antialias=False)
        x = torch.cat([P[p + "cls_token"].expand(1, -1, -1) + pos[:, :1], x + grid.permute(0, 2, 3, 1).reshape(1, 256, D)], 1)
        ln = lambda t, nm: Fn.layer_norm(t, (D,), P[nm + ".weight"], P[nm + ".bias"], 1e-6)      # noqa: E731
        qkv = Fn.linear(ln(x, b + "norm1"), P[b + "attn.qkv.weight"], P[b + "attn.qkv.bias"]).view(1, 257, 3, Hh, D // Hh).permute(2, 0, 3, 1, 4)
        a = Fn.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2]).transpose(1, 2).reshape(1, 257, D)
        x = x + Fn.linear(a, P[b + "attn.proj.weight"], P[b + "attn.proj.bias"]) * P[b + "ls1.gamma"]
        h = Fn.gelu(Fn.linear(ln(x, b + "norm2"), P[b + "mlp.fc1.weight"], P[b + "mlp.fc1.bias"]))
        x = x + Fn.linear(h, P[b + "mlp.fc2.weight"], P[b + "mlp.fc2.bias"]) * P[b + "ls2.gamma"]
        return ln(x, p + "norm")[:, 1:].reshape(256, D)

    def tape(tp, V):
        dino = TL.DinoTrain(p, tp.store.p32.device)
        dino.DEPTH = 1
        return dino.forward(tp, frames.to(tp.store.p32.device))
    pb.tape, pb.ref = tape, ref
    return pb


def by_id(id):
    return next(c for c in CASES + LAYERS if c.id == id)
