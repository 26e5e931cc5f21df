"""Attention forward (ina_attention_bf16 through ops.attention: the six kernels of internnav_amd/csrc/attention.hip and attention_wide.hip) against
the float64 restatement of tests/attn_fwd_ref.py at its kernel, tile and mask edges. The reference, the per-element bound (derived from the number
formats, limit 1.0) and the case table live in tests/attn_fwd_ref.py; tests/test_attn_fwd_ref_cpu.py checks them without a GPU (SDPA equality,
an emulation of the kernels' rounding points, the thirteen mutations that must leave the bound).

Every pinned kernel is compared with float64 on its own, element by element. Outputs are pre-filled with NaN (with the random base under
`accumulate`): rows without an allowed key must come back exactly 0 (exactly the base), their bound is 0. Strided and packed outputs sit inside a
sentinel-filled buffer with guard rows and columns that must stay untouched. Inputs carry planted edges (attn_fwd_ref.make_inputs): a mask that
is off by one key moves the result by hundreds to thousands of bounds.

Measured worst |err| / bound per group (MI355X, ROCm 7):
    row16    kernel 1 (attn_fwd_kernel)                                  0.954   (30 cases; the gate + accumulate cases, else <= 0.66)
    dropout  kernel 1 (attn_fwd_kernel, DROP build), salted and unsalted 0.640
    decode   kernel 0 (8-wave at d 128, else 4-wave / the pair > 1024)   0.764
             kernel 1 (split + combine)                                  0.764
             kernel 3 (4-wave at d 128)                                  0.764
    wide     kernel 2 and kernel 0 (attn_fwd_wide_kernel<D, 4>)          0.702
    window   kernel 0 / 2 (attn_fwd_wide_kernel<80, 2, 1>) and kernel 1  0.580
(the float32 / bf16 emulation of tests/test_attn_fwd_ref_cpu.py gives the same figures: the two bf16 roundings dominate; the rope + append cache
rows are bit-equal to the reference, every other cache row untouched).
With these single edits of a scratch copy of the kernels (never committed) the suite fails as follows, and passes in every other case:
    row16    attn_fwd_kernel, `causal_shift = len_k - len_q` taken from p.Lk: the two causal row16 cases whose len_k is below Lk fail (k_len
             [65, 37, 0] and the packed causal case);
    dropout  `row = (...) * p.Lk` of the DROP build with len_k for p.Lk: the two k_len cases fail, salted and unsalted;
    decode   `kv <= qpos + causal_shift` as `<` in `dec_mask` (attention.hip), the one mask of the split, the 4-wave and the 8-wave kernel: every
             causal decode run fails on every kernel (all 23, rope + append included), no non-causal one, and nothing in the prefix / shared
             suites, whose kernels hand the shared chunk step (attention_chunk.h) a mask of their own (`kv <= qpos` as `<` in
             attn_prefix_kernel: the seven cases of tests/test_attention_prefix_gpu.py fail and nothing here);
    wide     `l_run *= alpha` of the deferred rescale removed: 34 of the 42 wide runs fail, both ramp cases among them;
    window   `ub = min(len_k - 1, ...)` one key later in the single-buffer build only: the four window runs on kernel 0 / 2 fail, kernel 1 passes.
"""
import pytest
import torch

from tests import attn_fwd_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
NAN = float("nan")
SENTINEL = -7.0


@pytest.fixture(scope="module")
def ops(built_lib):
    from internnav_amd import ops

    return ops


def _views(c, inp):
    """device views of the inputs in the case's layout and the output view (NaN, or the base under accumulate). Returns (args, kwargs, out, after):
    after() checks what must not have been written (guard rows / columns, the rope launch's cache and projection buffer)."""
    B, Lq, Lk, H, Hkv, D = c["dims"]
    kw, checks = {}, []
    if c["layout"] == "varlen":             # packed rows; the output inside a sentinel buffer: a guard row above and below, 8 guard columns on each side
        q, k, v = (inp[n].to(DEV) for n in ("q", "k", "v"))
        T = q.shape[0]
        buf = torch.full((T + 2, H * D + 16), SENTINEL, dtype=BF16, device=DEV)
        out = buf[1:-1, 8:8 + H * D].view(T, H, D)
        kw.update(cu_q=inp["cu_q"].to(DEV), cu_k=inp["cu_k"].to(DEV), max_q=Lq, max_k=Lk)
    elif c["layout"] == "strided":          # q | k | v column slices of one [B, L, (H + 2 Hkv) D] projection, the output inside a sentinel buffer
        assert Lq == Lk and c["kv_bdiv"] == 1
        qkv = torch.cat([inp[n].reshape(B, Lq, -1) for n in ("q", "k", "v")], 2).to(DEV)
        q, k, v = qkv[..., :H * D].view(B, Lq, H, D), qkv[..., H * D:(H + Hkv) * D].view(B, Lk, Hkv, D), qkv[..., (H + Hkv) * D:].view(B, Lk, Hkv, D)
        buf = torch.full((B, Lq + 2, H * D + 16), SENTINEL, dtype=BF16, device=DEV)
        out = buf[:, 1:-1, 8:8 + H * D].view(B, Lq, H, D)
        before = qkv.clone()
        checks.append(lambda: torch.equal(qkv, before) or "the projection buffer was written")
    elif c["rope"]:                         # the decoder's buffers: q | k_new | v_new in one projection, k / v the two halves of a longer KV cache
        qkv = torch.cat([inp[n].reshape(B * Lq, -1) for n in ("q", "k_new", "v_new")], 1).to(DEV)
        q = qkv[:, :H * D].view(B, Lq, H, D)
        k_new, v_new = qkv[:, H * D:(H + Hkv) * D].view(B, Lq, Hkv, D), qkv[:, (H + Hkv) * D:].view(B, Lq, Hkv, D)
        cache = torch.randn(B, Lk + 5, 2, Hkv, D, generator=torch.Generator().manual_seed(5)).to(BF16).to(DEV)
        cache[:, :Lk, 0], cache[:, :Lk, 1] = inp["k"].to(DEV), inp["v"].to(DEV)
        k, v = cache[:, :Lk, 0], cache[:, :Lk, 1]
        kw.update(rope=(inp["cos"].to(DEV), inp["sin"].to(DEV), k_new, v_new))
        want, before = cache.clone(), qkv.clone()
        _, k_ref, v_ref = R.rope_apply(c, inp)
        want[:, :Lk, 0], want[:, :Lk, 1] = k_ref.to(DEV), v_ref.to(DEV)
        checks.append(lambda: torch.equal(cache, want) or f"KV cache: {(cache != want).sum().item()} elements differ from the appended reference")
        checks.append(lambda: torch.equal(qkv, before) or "the projection buffer was written")
    else:
        q, k, v = (inp[n].to(DEV) for n in ("q", "k", "v"))
    if c["layout"] in ("varlen", "strided"):
        out.fill_(NAN)

        def guard():
            mask = torch.ones_like(buf, dtype=torch.bool)
            mask[..., 1:-1, 8:8 + H * D] = False
            return torch.equal(buf[mask], torch.full_like(buf[mask], SENTINEL)) or "wrote outside the output view"
        checks.append(guard)
    else:
        out = inp["base"].to(DEV).clone() if c["acc"] else torch.full((B, Lq, H, D), NAN, dtype=BF16, device=DEV)
    if inp["k_len"] is not None:
        kw["k_len"] = inp["k_len"].to(DEV)
    if inp["gate"] is not None:
        kw["head_gate"] = inp["gate"].to(DEV)

    def after():
        for chk in checks:
            res = chk()
            assert res is True, f"{c['name']}: {res}"
    return (q, k, v), kw, out, after


def _run(ops, c, kernel, salted=False):
    """one case on one pinned kernel: a single launch, every element against its bound."""
    inp, ref, bound = R.case_reference(c, R.SALT if salted else 0)
    args, kw, out, after = _views(c, inp)
    if c["drop"] is not None:
        kw.update(drop_p=c["drop"][0], drop_seed=c["drop"][1], drop_salt=torch.tensor([R.SALT], dtype=torch.int32, device=DEV) if salted else None)
    res = ops.attention(*args, scale=c["scale"], causal=c["causal"], kv_start=c["kv_start"], kv_bdiv=c["kv_bdiv"], out=out, accumulate=c["acc"],
                        kernel=kernel, **kw)
    torch.cuda.synchronize()
    assert res is out
    after()
    worst, ok = R.ratio(out.cpu(), R.pack(c, inp, ref), R.pack(c, inp, bound))
    print(f"{c['name']} kernel {kernel}{' (salted)' if salted else ''}: worst |err|/bound {worst:.3f}")
    assert ok, f"{c['name']} kernel {kernel}: outside the bound (or not exactly 0 / the base where the bound is 0): {worst:.3f}"
    return worst


def _group(name):
    runs = [(c, kern) for c in R.GROUPS[name] for kern in c["kernels"]]
    return pytest.mark.parametrize("c,kernel", runs, ids=[f"{c['name']}-kernel{kern}" for c, kern in runs])


@_group("row16")
def test_row16(ops, c, kernel):
    """attn_fwd_kernel: 4 head dims, the Lq 16 | 17 | 32 | 33 workgroup widths, the Lk 48 | 49 key blocks, kv_start, k_len, causal Lq > Lk, gate +
    accumulate, packed sequences of length 0 and 1."""
    _run(ops, c, kernel)


@_group("dropout")
@pytest.mark.parametrize("salted", [False, True], ids=["nosalt", "salt"])
def test_dropout(ops, c, kernel, salted):
    """the forward's own mask: index with the full Lk, applied after the row sum, the salt word added to the seed."""
    _run(ops, c, kernel, salted=salted)


@_group("decode")
def test_decode(ops, c, kernel):
    """the split + combine pair (1), the one-launch kernels (0; 3 = four waves at d 128): row packing G * Lq 16 | 17 | 48, Lk 1024 | 1025, k_len down
    to 0; rope + append: the cache rows bit for bit, every other cache row untouched, then the output against its bound."""
    B, Lq, Lk, H, Hkv, D = c["dims"]
    assert Lk >= 256 and Lq <= 8 and (H // Hkv) * Lq <= 48 and not (c["kv_start"] or c["gate"] or c["acc"] or c["lens_q"]), "outside the decode contract"
    if c["rope"]:
        assert ops.attention_rope_ok(Lq, Lk, H, Hkv, D) and all(n >= Lq for n in (c["k_len"] or [Lk]))
    _run(ops, c, kernel)


@_group("wide")
def test_wide(ops, c, kernel):
    """attn_fwd_wide_kernel pinned (2) and through the automatic rule (0): end-aligned tiles with a first tile of one row, clamped staging at
    k_len 40 / 0, kv_start inside a block, the deferred running maximum, packed and strided layouts."""
    _run(ops, c, kernel)


@_group("window")
def test_window(ops, c, kernel):
    """packed d-80 windows of at most 64 tokens: the single-buffer build of the 32-row kernel (0, 2) and the 16-row kernel (1)."""
    _run(ops, c, kernel)


def _dense(B, Lq, Lk, H, Hkv, D):
    q = torch.zeros(B, Lq, H, D, dtype=BF16, device=DEV)
    k, v = (torch.zeros(B, Lk, Hkv, D, dtype=BF16, device=DEV) for _ in range(2))
    return q, k, v


def _rope(B, Lq, Hkv, D):
    cs = torch.zeros(B * Lq, 128, device=DEV)
    return cs, cs.clone(), torch.ones(B, Lq, Hkv, D, dtype=BF16, device=DEV), torch.ones(B, Lq, Hkv, D, dtype=BF16, device=DEV)


REFUSALS = {
    "kernel3_outside_decode": ((1, 16, 32, 2, 2, 128), lambda: dict(kernel=3)),
    "kernel2_with_gate": ((1, 128, 128, 2, 2, 64), lambda: dict(kernel=2, head_gate=torch.zeros(2, device=DEV))),
    "rope_D64": ((1, 1, 256, 4, 4, 64), lambda: dict(causal=True, rope=_rope(1, 1, 4, 64))),
    "rope_kernel1": ((1, 1, 256, 4, 4, 128), lambda: dict(causal=True, kernel=1, rope=_rope(1, 1, 4, 128))),
    "dropout_D80": ((1, 16, 32, 2, 2, 80), lambda: dict(drop_p=0.1, drop_seed=1)),
    "D72": ((1, 16, 32, 2, 2, 72), lambda: dict()),
    "H3_Hkv2": ((1, 16, 32, 3, 2, 64), lambda: dict()),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(ops, name):
    """rejected by the library's argument checks before any launch, reported through _lib.check; output and KV cache are left as they were."""
    from internnav_amd import _lib

    dims, kw = REFUSALS[name]
    q, k, v = _dense(*dims)
    out = torch.full(q.shape, NAN, dtype=BF16, device=DEV)
    with pytest.raises(_lib.EngineError, match="attention_bf16"):
        ops.attention(q, k, v, out=out, **kw())
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and not k.any() and not v.any()
