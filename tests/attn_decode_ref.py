"""TEST INFRASTRUCTURE: float64 restatement of the three single-token attention entries built on csrc/attention_chunk.h - ops.attention_prefix and
ops.attention_prefix_tail (attn_prefix_kernel / attn_prefix_tail_kernel, csrc/attention_prefix.hip) and ops.attention_shared (attn_shared_kernel,
csrc/attention_shared.hip) -, their per-element error bound, a float32 / bf16 emulation of the kernels' chunk walk, and the case tables shared by
tests/test_attn_decode_ref_cpu.py and tests/test_attention_decode_fp64_gpu.py. Plain torch on the CPU; of internnav_amd only
ops.attention_shared_plan (host code) is used, as tests/attn_shared_ref.py does.

All three entries are "row r attends an explicit list of keys" (include/internnav_amd.h):
  prefix       query row i < suf' of pair p sees cache rows [0, pfx') of slot slot[p], then suffix keys j <= i of pair p;
  prefix_tail  ... cache rows [0, pfx'), then rows [0, tl') of tail tail_row[p], then suffix keys j <= i;
  shared       row r, named by tile t, sees cache rows [0, pfx') of slot tile_slot[t], then rows [0, tl') of its own tail;
with pfx' = min(max(pfx_len, 0), max_pfx), suf' = min(max(suf_len, 0), m), tl' = min(max(tail_len, 0), max_tail | T). Rows at or behind suf',
rows with tl' = 0 (shared) are exactly 0; a slot outside the cache, or (prefix_tail) a tail row outside the buffer under tl' > 0, gives NaN in the
live rows; tl' = 0 never looks at tail_row; a tile place < 0 or >= n_rows is empty; rows no tile names are not written.
`pair_problems` / `shared_problems` reduce a launch to problems (Q rows of one KV group, their key segments gathered by SLICING, so NaN in a row
the mask does not admit cannot enter) and `attend` is softmax(Q K^T scale) V on them in float64.

Bound: tests/attn_fwd_ref.py's, unchanged in form (its docstring derives it) and computed by the same functions -
    bound = u8 (A + |ref|)(1 + 2^-6) + fK (A + |o|) + E_S,   0 where A = 0 (checked with ==),   limit 1.0
- because the kernels have that module's rounding points: fp32 logits, exp2 in fp32 against the wave's running maximum, P rounded to bf16 before
P V, the row sum of the un-rounded P, fp32 rescales, fp32 partials merged in wave order with exp2(m_w - m) weights, one bf16 store. Lk in
fK = 16 u24 (sqrt(Lk) + 4) is the row's admitted key count rounded up to whole 64-key chunks of each segment (what the waves accumulate over).

Emulation (`emulate`): the chunk walk as the kernels do it. Chunks are 64 keys of ONE segment, in the order prefix, tail, suffix; chunk c of
that list belongs to wave c mod 4 (the prefix kernels' rule; for the shared kernel prefix chunk c -> wave c mod 4 and tail chunk t of any place
-> wave (nc + t) mod 4, the same function of the row's own chunk index - and a chunk of another place leaves the row's state as it was). A wave
keeps (m, l, O) in the exp2 domain over its chunks in order; the four partials are merged as ac_combine does. It shows on the CPU that a
faithful implementation stays inside the bound, and hosts the arithmetic mutations.

Inputs (`make_inputs`): seeded bf16 buffers as the engine passes them (one fused q|k|v projection, one cache, one tail buffer), NaN in everything
the launch must not read (cache rows at or behind pfx' and every unnamed slot, tail rows at or behind tl' and every unnamed tail, fused rows at or
behind suf', the k|v columns of the shared entry's projection, the q and tail of its unnamed row). Planted edges in the EVEN KV heads, in
attn_fwd_ref.make_inputs' style: a planted key is 3 * q of the KV group's first head of the last live row of the pair (shared: of the row
itself; for a prefix, of the last pair / row that names the slot). Planted: the last key of every segment (pfx' - 1, tl' - 1), both sides of
every 64-key chunk edge inside a segment, prefix key 0, and in the suffix the diagonal and the key after it of a mid-tile row (that row's q).
A mask that is off by one key there moves the result by many bounds whatever the prefix length. Odd KV heads keep a spread softmax.
Ramp cases: for one row (a head of KV head 1, where nothing else is planted) one key of each chunk (key 10, or the chunk's last) is a multiple of
the row's q that puts the chunk's exp2-domain maximum at a chosen level, so that the maxima rise along one wave's walk (+4, +10: the rescale
inside a wave carries the result) and the four waves end 8 - 20 apart (the combine's weights carry it)."""
from __future__ import annotations

import zlib

import numpy as np
import torch

from tests import attn_fwd_ref as RF
from tests.attn_fwd_ref import BF16, F32, F64, f32, ratio  # noqa: F401  (ratio is re-exported to the two test modules)

D = 128
CHUNK, WAVES = 64, 4
LOG2E = 1.4426950408889634
S_CACHE, N_SLOTS = 840, 4
T_TAIL, N_TAILS = 130, 5
SENTINEL = -7.0
ALT_SCALE = 0.11          # the non-default scale (d^-0.5 = 0.0884): make_inputs asserts that every planted logit stays inside fp32's exp2 range
RESTATEMENT_MUTATIONS = ("pfx_minus", "pfx_plus", "tail_minus", "tail_plus", "diag_minus", "diag_plus", "tail_of_neighbour", "kv_head_mod",
                         "scale_ignored", "clamp_missing")
EMULATION_MUTATIONS = ("chunk_skip", "stale_prefetch", "no_rescale", "combine_unweighted")
MUTATIONS = RESTATEMENT_MUTATIONS + EMULATION_MUTATIONS


def _clamp(v, hi):
    return min(max(int(v), 0), int(hi))


def _cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------------------ problems
def _prefix_rows(raw, max_pfx, mut):
    """the cache rows a mask admits (a slice)"""
    pf = _clamp(raw, max_pfx)
    if mut == "clamp_missing" and int(raw) < 0:
        return slice(None, int(raw))                        # a negative length used as is
    return slice(0, max(pf + (1 if mut == "pfx_plus" else -1 if mut == "pfx_minus" else 0), 0))


def _tail_rows(tl, mut):
    return slice(0, max(tl + (1 if mut == "tail_plus" else -1 if mut == "tail_minus" else 0), 0))


def _heads(kh, H, Hkv, mut):
    G = H // Hkv
    return [h for h in range(H) if (h % Hkv if mut == "kv_head_mod" else h // G) == kh]


def pair_problems(q, k, v, kc, vc, slot, pfx_len, suf_len, kt=None, vt=None, tail_row=None, tail_len=None, max_pfx=None, max_tail=None, mut=None):
    """ops.attention_prefix / ops.attention_prefix_tail (kt .. tail_len given) as problems. q [P, m, H, D], k / v [P, m, Hkv, D], kc / vc
    [slots, S, Hkv, D], kt / vt [tails, T, Hkv, D] (torch, any float dtype), tables of ints [P].
    -> (problems, nan [P, m] bool: the live rows of a pair with a bad slot / tail row). A problem: Q [G * n, D] (head-major), segs
    [(K, V, allowed bool [G * n, keys] | None)], dst [(index of out, rows)] per head."""
    P, m, H, _ = q.shape
    Hkv = k.shape[2]
    n_slots, S = kc.shape[:2]
    max_pfx = S if max_pfx is None else max_pfx
    has_tail = kt is not None
    if has_tail:
        n_tails, T = kt.shape[:2]
        max_tail = T if max_tail is None else max_tail
    probs, nan = [], torch.zeros(P, m, dtype=torch.bool)
    for p in range(P):
        sl, n = int(slot[p]), _clamp(suf_len[p], m)
        tl = _clamp(tail_len[p], max_tail) if has_tail else 0
        tr = int(tail_row[p]) if tl > 0 else 0
        if not 0 <= sl < n_slots or (tl > 0 and not 0 <= tr < n_tails):
            nan[p, :n] = True
            continue
        if n == 0:
            continue
        rows = _prefix_rows(pfx_len[p], max_pfx, mut)
        i = torch.arange(n)
        for kh in range(Hkv):
            heads = _heads(kh, H, Hkv, mut)
            segs = [(kc[sl, rows, kh], vc[sl, rows, kh], None)]
            if tl > 0:
                segs.append((kt[tr, _tail_rows(tl, mut), kh], vt[tr, _tail_rows(tl, mut), kh], None))
            diag = i + (1 if mut == "diag_plus" else -1 if mut == "diag_minus" else 0)
            segs.append((k[p, :n, kh], v[p, :n, kh], (i.view(1, n) <= diag.view(n, 1)).repeat(len(heads), 1)))
            probs.append(dict(Q=torch.cat([q[p, :n, h] for h in heads], 0), segs=[s for s in segs if s[0].shape[0]],
                              dst=[((p, slice(0, n), h), n) for h in heads]))
    return probs, nan


def shared_problems(q, kt, vt, kc, vc, tile_rows, tile_slot, tile_pfx, tail_len, max_pfx=None, mut=None):
    """ops.attention_shared as problems. q [R, H, D], kt / vt [R, T, Hkv, D], kc / vc [slots, S, Hkv, D], tile_rows ints [n_tiles, cpt],
    tile_slot / tile_pfx [n_tiles], tail_len [R]. -> (problems, nan [R] bool, written [R] bool: the rows some tile names)."""
    R, H, _ = q.shape
    T, Hkv = kt.shape[1:3]
    n_slots, S = kc.shape[:2]
    max_pfx = S if max_pfx is None else max_pfx
    probs, nan, written = [], torch.zeros(R, dtype=torch.bool), torch.zeros(R, dtype=torch.bool)
    for t in range(len(tile_rows)):
        sl = int(tile_slot[t])
        for r in (int(x) for x in tile_rows[t]):
            if not 0 <= r < R:
                continue
            written[r] = True
            tl = _clamp(tail_len[r], T)
            if not 0 <= sl < n_slots:
                nan[r] = tl > 0
                continue
            if tl == 0:
                continue
            rows = _prefix_rows(tile_pfx[t], max_pfx, mut)
            src = (r + 1 if r + 1 < R else r - 1) if mut == "tail_of_neighbour" else r
            for kh in range(Hkv):
                heads = _heads(kh, H, Hkv, mut)
                segs = [(kc[sl, rows, kh], vc[sl, rows, kh], None), (kt[src, _tail_rows(tl, mut), kh], vt[src, _tail_rows(tl, mut), kh], None)]
                probs.append(dict(Q=torch.stack([q[r, h] for h in heads], 0), segs=[s for s in segs if s[0].shape[0]], dst=[((r, h), 1) for h in heads]))
    return probs, nan, written


# ------------------------------------------------------------------------------------------------------------ float64 and the bound
def attend(prob, scale, bounds=True):
    """(ref, bound) float64 [rows, D] of one problem: softmax over the admitted keys of all segments, jointly. `scale` is used as it is:
    `reference` passes the float32 value the kernel receives."""
    Q = prob["Q"].to(F64)
    n = Q.shape[0]
    if not prob["segs"]:
        z = torch.zeros(n, D, dtype=F64)
        return z, z.clone()
    K, V = (torch.cat([s[i].to(F64) for s in prob["segs"]], 0) for i in (0, 1))
    masks = [torch.ones(n, s[0].shape[0], dtype=torch.bool) if s[2] is None else s[2] for s in prob["segs"]]
    allowed = torch.cat(masks, 1)
    sc = scale
    S = (Q @ K.T) * sc
    P = RF._softmax(S, allowed)
    o = P @ V
    if not bounds:
        return o, None
    A = P @ V.abs()
    T = (Q.abs() @ K.abs().T) * sc
    M = S.masked_fill(~allowed, float("-inf")).amax(-1, keepdim=True)
    eps = RF.exponent_eps(T, M, D)
    ES = (P * eps) @ V.abs() + o.abs() * (P * eps).sum(-1, keepdim=True)
    Lk = sum(((mk.sum(-1) + CHUNK - 1) // CHUNK) * CHUNK for mk in masks).to(F64).view(n, 1)
    return o, RF.bound_of(A, o, o, ES, RF.fp32_factor(Lk))


def _chunks(prob):
    out = []
    for K, V, al in prob["segs"]:
        for k0 in range(0, K.shape[0], CHUNK):
            out.append((K[k0:k0 + CHUNK].to(F32), V[k0:k0 + CHUNK].to(F32), None if al is None else al[:, k0:k0 + CHUNK]))
    return out


def walk(prob, scale, mut=None, trace=None):
    """the kernels' arithmetic on one problem: fp32, chunk c -> wave c mod 4, per wave a running (m, l, O) in the exp2 domain with P rounded to
    bf16 before P V and the un-rounded row sum, the four partials merged in wave order as ac_combine does, one bf16 result. `trace` (a list)
    receives per wave the list of its chunks' maxima, each [rows]."""
    Q = prob["Q"].to(F32)
    n = Q.shape[0]
    chunks = _chunks(prob)
    sc2 = torch.tensor(f32(scale), dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    parts = []
    for w in range(WAVES):
        own = list(range(w, len(chunks), WAVES))
        if mut == "chunk_skip" and len(own) >= 2:
            own = own[:-1]
        m_run, l_run, acc = torch.full((n,), float("-inf"), dtype=F32), torch.zeros(n, dtype=F32), torch.zeros(n, D, dtype=F32)
        seen = []
        for t, ci in enumerate(own):
            K, V, al = chunks[ci]
            if mut == "stale_prefetch" and t == 2:          # the registers still hold the wave's second chunk (zeros behind its keys)
                K2, V2, _ = chunks[own[1]]
                pad = torch.zeros(max(K.shape[0] - K2.shape[0], 0), D, dtype=F32)
                K, V = torch.cat([K2, pad], 0)[:K.shape[0]], torch.cat([V2, pad], 0)[:K.shape[0]]
            s = (Q @ K.T) * sc2
            if al is not None:
                s = s.masked_fill(~al, float("-inf"))
            mx = s.amax(-1)
            seen.append(mx)
            m_new = torch.maximum(m_run, mx)
            m_use = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
            alpha = torch.where(torch.isinf(m_run), torch.zeros_like(m_run), torch.exp2(m_run - m_use))
            e = torch.exp2(s - m_use[:, None])
            l_run = l_run * alpha + e.sum(-1)
            acc = (acc if mut == "no_rescale" else acc * alpha[:, None]) + e.to(BF16).to(F32) @ V
            m_run = m_new
        parts.append((m_run, l_run, acc))
        if trace is not None:
            trace.append(seen)
    m = torch.stack([p[0] for p in parts]).amax(0)
    m_use = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    l, o = torch.zeros(n, dtype=F32), torch.zeros(n, D, dtype=F32)
    for ms, lw, ow in parts:
        wl = torch.ones(n, dtype=F32) if mut == "combine_unweighted" else torch.where(torch.isinf(ms), torch.zeros_like(ms), torch.exp2(ms - m_use))
        l = l + lw * wl
        o = o + ow * wl[:, None]
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    return (o * inv[:, None]).to(BF16)


def _scatter(probs, shape, fn, dtype):
    outs = [torch.zeros(shape, dtype=dtype) for _ in range(2)]
    for prob in probs:
        res, r0 = fn(prob), 0
        for idx, rows in prob["dst"]:
            for o, t in zip(outs, res):
                if t is not None:
                    o[idx] = t[r0:r0 + rows].reshape(o[idx].shape)
            r0 += rows
    return outs


# ------------------------------------------------------------------------------------------------------------ cases
def pair_case(entry, name, H, Hkv, m, pairs, pfx_of, scale=None, max_pfx=None, max_tail=None, ramp=None):
    """entry "prefix": pairs [(slot, suf_len)]; "prefix_tail": pairs [(slot, tail_row, tail_len, suf_len)]. pfx_of {slot: pfx_len}. All table
    values are RAW (what the launch receives): the clamps are the kernel's and the reference's business. ramp: (pair, row, {chunk: level})."""
    if entry == "prefix":
        pairs = [(s, -1, 0, n) for s, n in pairs]
    return dict(entry=entry, name=f"{entry}-{name}", H=H, Hkv=Hkv, m=m, pairs=pairs, pfx_of=pfx_of, scale=scale if scale else D ** -0.5,
                max_pfx=max_pfx, max_tail=max_tail, ramp=ramp)


def shared_case(name, H, Hkv, prompts, scale=None, max_pfx=None, bad_places=False, ramp=None):
    """prompts [(slot, tile_pfx, [tail_len of every candidate])], RAW values. bad_places: two empty places of the tile table name row n_rows and
    a row far above it. ramp: (row, {chunk: level})."""
    return dict(entry="shared", name=f"shared-{name}", H=H, Hkv=Hkv, prompts=prompts, scale=scale if scale else D ** -0.5, max_pfx=max_pfx,
                bad_places=bad_places, ramp=ramp)


# ramp levels (exp2 domain) per chunk of the ramp row's chunk list; wave w walks chunks w, w + 4, ...
# 13 prefix chunks (769 keys; chunk 12 is key 768 alone and keeps a random logit) + the suffix chunk 13 / the tail chunks 13, 14:
#   wave 0: 16 -> 20 -> 30 (+4, +10)   wave 1: 10 -> 14 -> 22   wave 2: 12 -> 16 -> 38 (+4, +22)   wave 3: 8 -> 18 -> 18
#   final maxima 30, 22, 38, 18: 8, 16 and 20 below the row maximum
RAMP_769 = {0: 16, 4: 20, 8: 30, 1: 10, 5: 14, 9: 22, 2: 12, 6: 16, 10: 38, 3: 8, 7: 18, 11: 18}
# prefix 257 (chunks 0 - 4, chunk 4 is key 256 alone), tail 130 (chunks 5 - 7), the suffix chunk 8. A tail of T = 130 rows has three chunks, so no
# wave owns a prefix, a tail AND the suffix chunk (that takes four tail chunks); the steps cross the segments wave by wave instead:
#   wave 0: prefix 16 -> prefix 20 -> suffix 30 (+4, +10)   wave 1: prefix 10 -> tail 22   wave 2: prefix 12 -> tail 38   wave 3: prefix 8 -> tail 18
RAMP_257_130 = {0: 16, 4: 20, 8: 30, 1: 10, 5: 22, 2: 12, 6: 38, 3: 8, 7: 18}

P_ = lambda *a, **k: pair_case("prefix", *a, **k)            # noqa: E731
T_ = lambda *a, **k: pair_case("prefix_tail", *a, **k)       # noqa: E731
# ---- prefix: (H, Hkv) 28/4, 4/4, 16/2; m 1 / 3 / 16 / 17 / 64; pfx_len 0 / 1 / 63 / 64 / 65 / 256 / 257 / 769 (13 chunks: every wave walks >= 3,
#      the last holds one key) / 832 (13 full chunks, the suffix chunk falls to wave 1); suf_len 0 / 1 / m and ragged; slot 3 is never named
PREFIX = [
    P_("m3", 28, 4, 3, [(1, 3), (1, 1), (0, 2), (1, 3), (2, 0)], {0: 0, 1: 769, 2: 63}),
    P_("m1", 28, 4, 1, [(1, 1), (0, 1), (2, 1), (0, 0)], {0: 64, 1: 1, 2: 257}),
    P_("m16", 16, 2, 16, [(2, 16), (0, 1), (1, 7)], {0: 65, 1: 256, 2: 832}),
    P_("m17", 4, 4, 17, [(0, 17), (1, 1), (2, 16), (1, 0)], {0: 257, 1: 63, 2: 769}),
    P_("m64", 4, 4, 64, [(1, 64), (0, 1), (2, 33)], {0: 1, 1: 65, 2: 64}),
    P_("m64-H28", 28, 4, 64, [(1, 64), (0, 1)], {0: 0, 1: 832}),
    # table values that need the clamps: pfx_len -2, -200 (a length below -63 is where an unclamped chunk count goes negative) and 300 > max_pfx,
    # suf_len m + 3 and -1
    P_("clamps", 4, 4, 3, [(0, 6), (1, 3), (2, 2), (3, -1), (1, 1)], {0: -2, 1: 300, 2: -200, 3: 64}, max_pfx=257),
    P_("scale", 16, 2, 17, [(0, 17), (2, 5)], {0: 257, 2: 65}, scale=ALT_SCALE),
    P_("ramp", 16, 2, 16, [(1, 16), (0, 9)], {0: 256, 1: 769}, ramp=(0, 12, {**RAMP_769, 13: 26})),
]
# ---- prefix_tail: pfx_len % 64 in 0 / 1 / 63 x tail_len 0 / 1 / 63 / 64 / 65 / 130 (all 18, over the first two cases), tails named out of order
PREFIX_TAIL = [
    T_("m5", 28, 4, 5, [(0, 4, 130, 5), (1, 0, 1, 5), (2, 2, 64, 3), (0, 1, 63, 5), (1, 3, 65, 1), (2, -1, 0, 4), (0, 3, 65, 0), (1, 2, 64, 5), (2, 4, 130, 5)],
       {0: 64, 1: 65, 2: 63}),
    T_("m17", 4, 4, 17, [(2, 0, 1, 17), (0, -1, 0, 5), (1, 1, 63, 16), (2, 3, 65, 1), (0, 2, 64, 17), (1, 4, 130, 9), (0, 0, 1, 3), (1, -1, 0, 17), (2, 1, 63, 2)],
       {0: 128, 1: 1, 2: 127}),
    T_("long", 16, 2, 3, [(1, 2, 65, 3), (0, 0, 130, 3), (1, 1, 1, 1)], {0: 832, 1: 769}),
    T_("m64", 4, 4, 64, [(0, 3, 130, 64), (2, 1, 64, 33), (0, 1, 64, 1)], {0: 256, 2: 1}),
    T_("m1", 28, 4, 1, [(3, 2, 63, 1), (0, 0, 130, 1), (3, 4, 65, 1), (0, -1, 0, 1)], {0: 0, 3: 257}),
    # tail_len above max_tail (100 -> 70) and negative; tail_len <= 0 with a tail_row outside the buffer (ignored); tail_len > 0 with one
    # (NaN live rows, zeros behind them); suf_len above m
    T_("clamps", 4, 4, 3, [(0, 1, 100, 3), (1, 1 << 30, 0, 3), (0, -9, -3, 2), (1, N_TAILS, 5, 2), (0, -1, 1, 7), (1, 3, 64, 3)], {0: 65, 1: 300},
       max_pfx=257, max_tail=70),
    T_("scale", 16, 2, 5, [(2, 1, 65, 5), (0, 0, 130, 2)], {0: 63, 2: 257}, scale=ALT_SCALE),
    T_("ramp", 16, 2, 16, [(1, 2, 130, 16), (0, 0, 64, 9)], {0: 64, 1: 257}, ramp=(0, 12, RAMP_257_130)),
]
# ---- shared: (H, Hkv) gives 2 / 4 / 1 / 8 rows per tile; tile_pfx 0 / 1 / 63 / 64 / 65 / 769; tail_len 1 / 2 / 63 / 64 / 65 / 128 / 130 / 200 (-> T)
#      / -1 (-> a zero row); candidate counts that leave half-filled tiles; one row no tile names (tail_len 9, everything of it NaN)
SHARED = [
    shared_case("H28", 28, 4, [(3, 769, [1, 65, 2]), (0, 63, [64, 128, 63, 2, 1]), (2, 0, [65])]),
    shared_case("H8", 8, 2, [(2, 64, [128, 1, 64, 63, 2]), (0, 1, [2, 65]), (1, 65, [63, 130, 200, -1])]),
    shared_case("H16", 16, 1, [(1, 65, [2, 64]), (3, 0, [1, 130, 63])]),
    shared_case("H2", 2, 2, [(0, 769, [1, 2, 63, 64, 65, 130, 128, 5, 3]), (1, 1, [128, 5, 3])]),
    shared_case("bad-places", 8, 2, [(1, 257, [65, 1, 130, 2, 64]), (3, 64, [3])], bad_places=True),
    shared_case("scale", 28, 4, [(1, 257, [65, 3]), (0, 64, [130])], scale=ALT_SCALE),
    shared_case("clamps", 2, 2, [(0, 300, [3, 64, 200]), (1, -5, [65, 1, -1]), (2, -200, [2])], max_pfx=257),
    # the ramp row (row 1, tail 65) shares its tile with rows whose tails are longer than its own
    shared_case("ramp", 8, 2, [(2, 769, [130, 65, 128, 130]), (0, 1, [2])], ramp=(1, {**RAMP_769, 13: 26, 14: 12})),
]
GROUPS = {"prefix": PREFIX, "prefix_tail": PREFIX_TAIL, "shared": SHARED}
ALL = [c for g in GROUPS.values() for c in g]
BY_NAME = {c["name"]: c for c in ALL}
assert len(BY_NAME) == len(ALL)


def pair_views(c, fused, cache, tails=None):
    """(q, k_suf, v_suf, k_cache, v_cache, k_tail, v_tail) views of a pair case's buffers (any device); the tail views are None without tails"""
    H, Hkv, m = c["H"], c["Hkv"], c["m"]
    P = fused.shape[0] // m
    q = fused[:, : H * D].view(P, m, H, D)
    k = fused[:, H * D:(H + Hkv) * D].view(P, m, Hkv, D)
    v = fused[:, (H + Hkv) * D:].view(P, m, Hkv, D)
    c5 = cache.view(N_SLOTS, S_CACHE, 2, Hkv, D)
    t5 = None if tails is None else tails.view(N_TAILS, T_TAIL, 2, Hkv, D)
    return q, k, v, c5[:, :, 0], c5[:, :, 1], None if t5 is None else t5[:, :, 0], None if t5 is None else t5[:, :, 1]


def shared_views(c, fused, tail, cache):
    """(q, k_tail, v_tail, k_cache, v_cache) views of a shared case's buffers (any device)"""
    H, Hkv = c["H"], c["Hkv"]
    rows = fused.shape[0]
    t5 = tail.view(rows, T_TAIL, 2, Hkv, D)
    c5 = cache.view(N_SLOTS, S_CACHE, 2, Hkv, D)
    return fused[:, : H * D].view(rows, H, D), t5[:, :, 0], t5[:, :, 1], c5[:, :, 0], c5[:, :, 1]


def _edges(n):
    """the planted keys of a segment of n keys: key 0, both sides of every chunk edge inside it, the last key"""
    keys = {0, n - 1} | {e + d for e in range(CHUNK, n, CHUNK) for d in (-1, 0)}
    return sorted(x for x in keys if 0 <= x < n)


def _plant(K, keys, qrow, G):
    """K [rows, Hkv, D] (a view): the even KV heads of `keys` become 3 * q of their group's first head; qrow [H, D]"""
    val = (3.0 * qrow[::G].float()).to(BF16)
    for j in keys:
        K[j, 0::2] = val[0::2]


def _ramp(c, qr, chunk_key, levels, worst):
    """key `chunk_key(chunk)` (a [D] view of KV head 1) becomes the multiple of qr whose exp2-domain logit is the chunk's level"""
    sc2 = f32(c["scale"]) * LOG2E
    nq = float(qr.float() @ qr.float())
    for ch, level in levels.items():
        chunk_key(ch)[:] = (qr.float() * (level / (sc2 * nq))).to(BF16)
    worst.append(max(levels.values()))


def make_inputs(c, seed=0):
    """the case's buffers and int32 tables (CPU), the effective lengths the poison and the planting use, and `planted_max`: the largest
    exp2-domain logit a planted key gives (asserted to stay inside fp32's exp2 range, also at the non-default scale)."""
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()) + 7919 * seed)
    rnd = lambda *s: torch.randn(s, generator=g).to(BF16)                        # noqa: E731
    i32 = lambda x: torch.tensor(list(x), dtype=torch.int32)                      # noqa: E731
    H, Hkv = c["H"], c["Hkv"]
    G, W = H // Hkv, 2 * Hkv * D
    nan = float("nan")
    worst = []
    cache = rnd(N_SLOTS * S_CACHE, W)
    c5 = cache.view(N_SLOTS, S_CACHE, 2, Hkv, D)
    max_pfx = S_CACHE if c["max_pfx"] is None else c["max_pfx"]
    if c["entry"] == "shared":
        prompts = c["prompts"]
        from internnav_amd import ops

        prompt_of = [b for b, (_, _, tl) in enumerate(prompts) for _ in tl]
        raw_tl = [n for _, _, tl in prompts for n in tl]
        R = len(raw_tl)
        tiles, owner = ops.attention_shared_plan(prompt_of, G)
        tiles = np.array(tiles, dtype=np.int64)
        if c["bad_places"]:
            empty = np.argwhere(tiles < 0)
            assert len(empty) >= 2
            tiles[tuple(empty[0])], tiles[tuple(empty[1])] = R + 1, 1 << 20     # n_rows = R + 1 (the unnamed row included)
        fused = rnd(R + 1, (H + 2 * Hkv) * D)
        tail = rnd((R + 1) * T_TAIL, W)
        t5 = tail.view(R + 1, T_TAIL, 2, Hkv, D)
        q = fused[:, :H * D].view(R + 1, H, D)
        eff_tl = [_clamp(n, T_TAIL) for n in raw_tl]
        pfx_eff = {s: _clamp(p, max_pfx) for s, p, _ in prompts}
        for b, (s, _, tl) in enumerate(prompts):                       # the prompt's prefix: planted for its last row with a tail
            rows = [r for r in range(R) if prompt_of[r] == b and eff_tl[r] > 0]
            _plant(c5[s, :, 0], _edges(pfx_eff[s]), q[rows[-1]], G)
        for r in range(R):
            _plant(t5[r, :, 0], _edges(eff_tl[r]), q[r], G)
        if c["ramp"]:
            r, levels = c["ramp"]
            s, nc = prompts[prompt_of[r]][0], _cdiv(pfx_eff[prompts[prompt_of[r]][0]], CHUNK)

            def chunk_key(ch):
                if ch < nc:
                    return c5[s, ch * CHUNK + min(10, pfx_eff[s] - ch * CHUNK - 1), 0, 1]
                return t5[r, (ch - nc) * CHUNK + min(10, eff_tl[r] - (ch - nc) * CHUNK - 1), 0, 1]
            _ramp(c, q[r, G], chunk_key, levels, worst)
        worst.append(3.0 * float((q[:R].float() ** 2).sum(-1).max()) * f32(c["scale"]) * LOG2E)
        fused[:, H * D:] = nan
        fused[R] = nan
        for r, n in enumerate(eff_tl + [0]):
            t5[r, n:] = nan
        for s in range(N_SLOTS):
            c5[s, pfx_eff.get(s, 0):] = nan
        out = dict(fused=fused, tail=tail, cache=cache, R=R, tile_rows=torch.tensor(tiles, dtype=torch.int32), tile_slot=i32(prompts[b][0] for b in owner),
                   tile_pfx=i32(prompts[b][1] for b in owner), tail_len=i32(raw_tl + [9]))
    else:
        m, pairs = c["m"], c["pairs"]
        P = len(pairs)
        has_tail = c["entry"] == "prefix_tail"
        max_tail = T_TAIL if c["max_tail"] is None else c["max_tail"]
        fused = rnd(P * m, (H + 2 * Hkv) * D)
        tails = rnd(N_TAILS * T_TAIL, W)
        t5 = tails.view(N_TAILS, T_TAIL, 2, Hkv, D)
        q = fused[:, :H * D].view(P, m, H, D)
        k = fused[:, H * D:(H + Hkv) * D].view(P, m, Hkv, D)
        pfx_eff = {s: _clamp(p, max_pfx) for s, p in c["pfx_of"].items()}
        suf_eff = [_clamp(n, m) for _, _, _, n in pairs]
        tl_eff = [_clamp(tl, max_tail) if has_tail else 0 for _, _, tl, _ in pairs]
        tail_eff = {}
        for p, (s, tr, _, _) in enumerate(pairs):
            assert s in pfx_eff
            if tl_eff[p] > 0 and 0 <= tr < N_TAILS:
                assert tail_eff.setdefault(tr, tl_eff[p]) == tl_eff[p], "the pairs that name a tail agree on its length"
        assert len(set(s for s, _, _, _ in pairs)) < N_SLOTS or c["name"].endswith("clamps")
        for p, (s, tr, _, _) in enumerate(pairs):                       # a later pair re-plants a shared prefix / tail with its own q
            if suf_eff[p] == 0:
                continue
            last = q[p, suf_eff[p] - 1]
            _plant(c5[s, :, 0], _edges(pfx_eff[s]), last, G)
            if tr in tail_eff and tl_eff[p] > 0:
                _plant(t5[tr, :, 0], _edges(tail_eff[tr]), last, G)
            _plant(k[p], [suf_eff[p] - 1], last, G)
            qm = RF.mid_query(suf_eff[p])
            if qm is not None:
                _plant(k[p], [qm, qm + 1], q[p, qm], G)
        if c["ramp"]:
            p, i, levels = c["ramp"]
            s, tr = pairs[p][0], pairs[p][1]
            nc, nt = _cdiv(pfx_eff[s], CHUNK), _cdiv(tl_eff[p], CHUNK)
            assert i < suf_eff[p] - 1

            def chunk_key(ch):
                if ch < nc:
                    return c5[s, ch * CHUNK + min(10, pfx_eff[s] - ch * CHUNK - 1), 0, 1]
                if ch < nc + nt:
                    return t5[tr, (ch - nc) * CHUNK + min(10, tl_eff[p] - (ch - nc) * CHUNK - 1), 0, 1]
                assert ch == nc + nt
                return k[p, min(10, i), 1]
            _ramp(c, q[p, i, G], chunk_key, levels, worst)
        worst.append(3.0 * float((q.float() ** 2).sum(-1).max()) * f32(c["scale"]) * LOG2E)
        for s in range(N_SLOTS):
            c5[s, pfx_eff.get(s, 0):] = nan
        for t in range(N_TAILS):
            t5[t, tail_eff.get(t, 0):] = nan
        f3 = fused.view(P, m, -1)
        for p in range(P):
            f3[p, suf_eff[p]:] = nan
        out = dict(fused=fused, cache=cache, tails=tails if has_tail else None, P=P, slot=i32(s for s, _, _, _ in pairs),
                   pfx_len=i32(c["pfx_of"][s] for s, _, _, _ in pairs), suf_len=i32(n for _, _, _, n in pairs),
                   tail_row=i32(t for _, t, _, _ in pairs), tail_len=i32(t for _, _, t, _ in pairs), suf_eff=suf_eff)
    out["planted_max"] = max(worst)
    assert out["planted_max"] < 110.0, f"{c['name']}: a planted logit of 2^{out['planted_max']:.0f} leaves fp32's exp2 range"
    return out


def problems(c, inp, mut=None):
    """(problems, nan mask, written mask, output shape) of a case of this module"""
    if c["entry"] == "shared":
        q, kt, vt, kc, vc = shared_views(c, inp["fused"], inp["tail"], inp["cache"])
        probs, nan, written = shared_problems(q, kt, vt, kc, vc, inp["tile_rows"].tolist(), inp["tile_slot"].tolist(), inp["tile_pfx"].tolist(),
                                              inp["tail_len"].tolist(), c["max_pfx"], mut)
        return probs, nan, written, (inp["R"] + 1, c["H"], D)
    q, k, v, kc, vc, kt, vt = pair_views(c, inp["fused"], inp["cache"], inp["tails"])
    tail = {} if kt is None else dict(kt=kt, vt=vt, tail_row=inp["tail_row"].tolist(), tail_len=inp["tail_len"].tolist(), max_tail=c["max_tail"])
    probs, nan = pair_problems(q, k, v, kc, vc, inp["slot"].tolist(), inp["pfx_len"].tolist(), inp["suf_len"].tolist(), max_pfx=c["max_pfx"], mut=mut, **tail)
    return probs, nan, torch.ones(inp["P"], dtype=torch.bool), (inp["P"], c["m"], c["H"], D)


def _scale(c, mut):
    return D ** -0.5 if mut == "scale_ignored" else c["scale"]


def reference(c, inp, mut=None, bounds=True):
    """(ref, bound, nan, written): float64 [P, m, H, D] / [R + 1, H, D]; nan [P, m] / [R + 1]: rows that must be NaN (ref holds 0 there);
    written [P] / [R + 1]: what the launch writes at all. bound is 0 where the result must be exactly 0."""
    probs, nan, written, shape = problems(c, inp, mut)
    ref, bound = _scatter(probs, shape, lambda pr: attend(pr, f32(_scale(c, mut)), bounds), F64)
    return ref, bound if bounds else None, nan, written


def emulate(c, inp, mut=None, trace=None):
    """bf16 result of the emulated chunk walk, same shape as the reference (0 in NaN rows and in rows that are not written)"""
    probs, _, _, shape = problems(c, inp)
    return _scatter(probs, shape, lambda pr: (walk(pr, c["scale"], mut, trace), None), BF16)[0]


def check(out, ref, bound, nan, written=None):
    """(worst |err| / bound, ok): every written element inside its bound (== where it is 0), NaN exactly in the NaN rows"""
    out = out.to(F64)
    rows = nan.view(nan.shape + (1,) * (out.dim() - nan.dim())).expand(out.shape)
    keep = ~rows if written is None else ~rows & written.view(written.shape + (1,) * (out.dim() - written.dim())).expand(out.shape)
    ok_nan = bool(torch.isnan(out[rows]).all())
    w, ok = ratio(out[keep], ref[keep], bound[keep])
    return w, ok and ok_nan


_CACHE = {}


def case_reference(c, seed=0):
    """(inputs, ref, bound, nan, written) of a case, computed once per process and never modified"""
    key = (c["name"], seed)
    if key not in _CACHE:
        inp = make_inputs(c, seed)
        _CACHE[key] = (inp,) + reference(c, inp)
    return _CACHE[key]
