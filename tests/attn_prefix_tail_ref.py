"""TEST INFRASTRUCTURE: float64 restatement of ops.attention_prefix_tail (internnav_amd/csrc/attention_prefix.hip), the poisoned test cases shared
by tests/test_attn_prefix_tail_ref_cpu.py and tests/test_attention_prefix_tail_gpu.py, and the tolerance of tests/attn_prefix_ref.py.

Mask (include/internnav_amd.h, ina_attention_prefix_tail): query row i of pair p, i < suf_len[p], sees cache rows [0, min(pfx_len[p], max_pfx))
of slot slot[p], then rows [0, min(tail_len[p], max_tail)) of tail tail_row[p], then suffix keys j <= i of pair p. Rows i >= suf_len[p] are
zeros; a slot outside the cache, or a tail row outside the buffer with tail_len > 0, gives NaN in the rows i < suf_len[p]; tail_len <= 0 does
not look at tail_row."""
import numpy as np
import torch

from attn_prefix_ref import ATOL, RTOL, D, tolerance  # noqa: F401  (the bound of the 16-row attention kernels: 1.5e-2 + |ref| / 128)


def attention_prefix_tail_ref(q, k_suf, v_suf, k_cache, v_cache, slot, pfx_len, suf_len, k_tail=None, v_tail=None, tail_row=None, tail_len=None,
                              scale=None, max_pfx=None, max_tail=None):
    """float64 numpy. q [P, m, H, D], k_suf / v_suf [P, m, Hkv, D], k_cache / v_cache [slots, S, Hkv, D], k_tail / v_tail [tails, T, Hkv, D] or
    None (no tail), tables int [P] -> out [P, m, H, D]. Only the rows the mask admits are ever read (slices, no multiplication by a mask): NaN
    anywhere else cannot reach the result."""
    q, k_suf, v_suf, k_cache, v_cache = (np.asarray(t, dtype=np.float64) for t in (q, k_suf, v_suf, k_cache, v_cache))
    P, m, H, d = q.shape
    Hkv = k_suf.shape[2]
    G = H // Hkv
    n_slots, S = k_cache.shape[:2]
    scale = d ** -0.5 if scale is None else scale
    max_pfx = S if max_pfx is None else max_pfx
    has_tail = k_tail is not None
    if has_tail:
        k_tail, v_tail = np.asarray(k_tail, dtype=np.float64), np.asarray(v_tail, dtype=np.float64)
        n_tails, T = k_tail.shape[:2]
        max_tail = T if max_tail is None else max_tail
    out = np.zeros((P, m, H, d))
    for p in range(P):
        sl, n = int(slot[p]), min(max(int(suf_len[p]), 0), m)
        tl = min(max(int(tail_len[p]), 0), max_tail) if has_tail else 0
        tr = int(tail_row[p]) if tl > 0 else 0
        if not 0 <= sl < n_slots or (tl > 0 and not 0 <= tr < n_tails):
            out[p, :n] = np.nan
            continue
        pf = min(max(int(pfx_len[p]), 0), max_pfx)
        for h in range(H):
            kh = h // G
            ks, vs = [k_cache[sl, :pf, kh]], [v_cache[sl, :pf, kh]]
            if tl > 0:
                ks.append(k_tail[tr, :tl, kh])
                vs.append(v_tail[tr, :tl, kh])
            for i in range(n):
                k = np.concatenate(ks + [k_suf[p, : i + 1, kh]], 0)
                v = np.concatenate(vs + [v_suf[p, : i + 1, kh]], 0)
                s = (k @ q[p, i, h]) * scale
                e = np.exp(s - s.max())
                out[p, i, h] = (e / e.sum()) @ v
    return out


def sdpa_ref(q, k_suf, v_suf, k_cache, v_cache, slot, pfx_len, suf_len, k_tail, v_tail, tail_row, tail_len, scale=None):
    """the same through torch SDPA in float64 on the per-pair concatenation [cache[slot, :pfx_len] | tail[tail_row, :tail_len] | suffix[:suf_len]]
    with a bottom-right-aligned causal mask (query i of suf_len sees keys <= pfx_len + tail_len + i)."""
    P, m, H, d = q.shape
    Hkv = k_suf.shape[2]
    out = np.zeros((P, m, H, d))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    for p in range(P):
        n, pf, sl, tl = int(suf_len[p]), int(pfx_len[p]), int(slot[p]), max(int(tail_len[p]), 0)
        if n == 0:
            continue
        kp, vp = [t(k_cache[sl, :pf])], [t(v_cache[sl, :pf])]
        if tl:
            kp.append(t(k_tail[int(tail_row[p]), :tl]))
            vp.append(t(v_tail[int(tail_row[p]), :tl]))
        k = torch.cat(kp + [t(k_suf[p, :n])], 0).permute(1, 0, 2).repeat_interleave(H // Hkv, 0)     # [H, pf + tl + n, D]
        v = torch.cat(vp + [t(v_suf[p, :n])], 0).permute(1, 0, 2).repeat_interleave(H // Hkv, 0)
        mask = torch.ones(n, pf + tl + n, dtype=torch.bool).tril(diagonal=pf + tl)
        o = torch.nn.functional.scaled_dot_product_attention(t(q[p, :n]).permute(1, 0, 2), k, v, attn_mask=mask, scale=scale)
        out[p, :n] = o.permute(1, 0, 2).numpy()
    return out


# ---- the cases: (H, Hkv, m, pairs [(slot, tail_row, suf_len)], {slot: pfx_len}, {tail_row: tail_len}); 5 cache slots of S_CACHE rows and 5 tails
#      of T rows. In every case one slot and one tail are named by no pair (wholly NaN), slots and tails are named out of order, and one tail is
#      shared by two pairs. m covers 1 / 5 (the real 1 + N_QUERY) / 16 / 17 / 64 with ragged suf_len including 0; pfx_len covers 0 / 1 / 63 / 64 /
#      65 (chunk edges) and 256 / 300 (what four waves hold at once, and more); tail_len covers 0 / 1 / 63 / 64 / 65 / 130 (none, chunk edges,
#      three chunks). tail_row -1 stands for "no tail": its tail_len is 0. Pairs with pfx_len % 64 == 0 (0, 64 and 256) and a tail are in cases
#      0 - 4: there the kernel walks the chunks ops.attention_prefix walks on a slot that holds [prefix | tail] (bit equality).
S_CACHE, N_SLOTS, T_TAIL, N_TAILS = 448, 5, 136, 5
CASES = [
    (28, 4, 5, [(3, 1, 5), (0, 0, 5), (1, 1, 3), (2, 2, 5), (2, 3, 1), (0, -1, 0), (1, -1, 4)], {0: 256, 1: 64, 2: 0, 3: 300}, {0: 65, 1: 130, 2: 1, 3: 0}),
    (4, 4, 1, [(2, 4, 1), (0, 1, 1), (3, 0, 1), (1, 1, 1), (3, 2, 1), (1, -1, 0)], {0: 1, 1: 63, 2: 65, 3: 64}, {0: 63, 1: 64, 2: 0, 4: 130}),
    (28, 4, 16, [(1, 2, 16), (0, 0, 7), (2, 3, 1), (3, 1, 16), (1, 0, 9), (0, -1, 0)], {0: 0, 1: 256, 2: 63, 3: 1}, {0: 64, 1: 63, 2: 130, 3: 65}),
    (4, 4, 17, [(0, 4, 17), (1, 2, 5), (2, 1, 16), (3, 4, 1), (2, 0, 17), (3, -1, 0)], {0: 64, 1: 300, 2: 0, 3: 65}, {0: 0, 1: 1, 2: 65, 4: 130}),
    (4, 4, 64, [(0, 0, 64), (2, 1, 33), (1, 2, 64), (0, 1, 17), (2, -1, 1), (1, 2, 0)], {0: 256, 1: 1, 2: 64}, {0: 130, 1: 64, 2: 63}),
    (28, 4, 64, [(1, 3, 64), (0, 3, 1)], {0: 0, 1: 300}, {3: 130}),
]
CASE_IDS = [f"H{c[0]}_kv{c[1]}_m{c[2]}_{i}" for i, c in enumerate(CASES)]


def make_case(case, seed=0):
    """-> dict of bf16 torch tensors (CPU) laid out as the engine passes them - q / k_suf / v_suf strided views of ONE fused [P * m, (H + 2 Hkv) D]
    projection buffer, k_cache / v_cache views of one [slots * S, 2 Hkv D] cache, k_tail / v_tail views of one [tails * T, 2 Hkv D] tail buffer - and
    the int32 tables. N(0, 1) values; every row the mask must not read is NaN: cache rows at or behind pfx_len, tail rows at or behind tail_len,
    every row of an unnamed slot or tail, fused rows (q, k and v) at or behind suf_len."""
    H, Hkv, m, pairs, pfx_of, tail_of = case
    P = len(pairs)
    g = torch.Generator().manual_seed(2000 + seed)
    fused = torch.randn(P * m, (H + 2 * Hkv) * D, generator=g).to(torch.bfloat16)
    cache = torch.randn(N_SLOTS * S_CACHE, 2 * Hkv * D, generator=g).to(torch.bfloat16)
    tails = torch.randn(N_TAILS * T_TAIL, 2 * Hkv * D, generator=g).to(torch.bfloat16)
    c3, t3, f3 = cache.view(N_SLOTS, S_CACHE, -1), tails.view(N_TAILS, T_TAIL, -1), fused.view(P, m, -1)
    named_slots, named_tails = {s for s, _, _ in pairs}, {t for _, t, _ in pairs if t >= 0}
    assert named_slots == set(pfx_of) and named_tails == set(tail_of) and len(named_slots) < N_SLOTS and len(named_tails) < N_TAILS
    for s in range(N_SLOTS):
        c3[s, pfx_of.get(s, 0):] = float("nan")
    for t in range(N_TAILS):
        t3[t, tail_of.get(t, 0):] = float("nan")
    for p, (_, _, suf) in enumerate(pairs):
        f3[p, suf:] = float("nan")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    return dict(fused=fused, cache=cache, tails=tails, H=H, Hkv=Hkv, m=m, P=P, slot=i32([s for s, _, _ in pairs]),
                pfx_len=i32([pfx_of[s] for s, _, _ in pairs]), tail_row=i32([t for _, t, _ in pairs]),
                tail_len=i32([tail_of[t] if t >= 0 else 0 for _, t, _ in pairs]), suf_len=i32([n for _, _, n in pairs]))


def views(fused, cache, tails, H, Hkv, m):
    """(q, k_suf, v_suf, k_cache, v_cache, k_tail, v_tail) views of the three buffers (any device)"""
    P = fused.shape[0] // m
    q = fused[:, : H * D].view(P, m, H, D)
    k = fused[:, H * D:(H + Hkv) * D].view(P, m, Hkv, D)
    v = fused[:, (H + Hkv) * D:].view(P, m, Hkv, D)
    c5 = cache.view(-1, S_CACHE, 2, Hkv, D)
    t5 = tails.view(-1, T_TAIL, 2, Hkv, D)
    return q, k, v, c5[:, :, 0], c5[:, :, 1], t5[:, :, 0], t5[:, :, 1]


def reference_of(c):
    q, k, v, kc, vc, kt, vt = (t.double().numpy() for t in views(c["fused"], c["cache"], c["tails"], c["H"], c["Hkv"], c["m"]))
    return attention_prefix_tail_ref(q, k, v, kc, vc, c["slot"].numpy(), c["pfx_len"].numpy(), c["suf_len"].numpy(), kt, vt, c["tail_row"].numpy(),
                                     c["tail_len"].numpy())


def materialised(c):
    """a cache of P slots, slot p = [prefix of pair p | tail of pair p] and NaN behind (bf16 CPU [P * S_CACHE, 2 Hkv D]), with the tables
    (slot = 0 .. P - 1, pfx_len + tail_len) ops.attention_prefix takes for it: the same keys in the same order without a tail segment"""
    P, w = c["P"], c["cache"].shape[1]
    c3, t3 = c["cache"].view(N_SLOTS, S_CACHE, w), c["tails"].view(N_TAILS, T_TAIL, w)
    mat = torch.full((P, S_CACHE, w), float("nan"), dtype=torch.bfloat16)
    for p in range(P):
        pf, tl = int(c["pfx_len"][p]), int(c["tail_len"][p])
        mat[p, :pf] = c3[int(c["slot"][p]), :pf]
        if tl:
            mat[p, pf:pf + tl] = t3[int(c["tail_row"][p]), :tl]
    return mat.view(P * S_CACHE, w), torch.arange(P, dtype=torch.int32), (c["pfx_len"] + c["tail_len"]).to(torch.int32)


# ---- the argument sets ina_attention_prefix_tail must refuse before any HIP call (dummy pointers, no GPU); keys name the argument that is replaced.
#      Defaults of the caller: P = 2 pairs x m = 5 rows x H = 28 / Hkv = 4 heads of D = 128 in the engine's layout, 5 tails of 136 rows.
def abi_refusal_cases():
    return [dict(D=64), dict(m=0), dict(m=65), dict(H=30), dict(Hkv=0), dict(P=-1), dict(max_pfx=-1), dict(n_slots=0), dict(q_rs=4612), dict(c_rs=1028),
            dict(s_hs=100), dict(o_rs=3586), dict(slot=None), dict(pfx_len=None), dict(suf_len=None), dict(Q=None), dict(k_cache=None), dict(v_suf=None),
            dict(Q_off=8), dict(O_off=4), dict(scale=float("nan")),
            # the tail: some of its four arguments missing, no tails, a negative limit, unaligned strides and pointers
            dict(k_tail=None), dict(v_tail=None), dict(tail_row=None), dict(tail_len=None), dict(k_tail=None, v_tail=None), dict(tail_row=None, tail_len=None),
            dict(k_tail=None, v_tail=None, tail_row=None), dict(n_tail_rows=0), dict(max_tail=-1), dict(t_ps=1028), dict(t_rs=1028), dict(t_hs=100),
            dict(k_tail_off=8), dict(v_tail_off=4)]
