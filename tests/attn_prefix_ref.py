"""TEST INFRASTRUCTURE: float64 restatement of ops.attention_prefix (internnav_amd/csrc/attention_prefix.hip), the poisoned test cases shared by
tests/test_attn_prefix_ref_cpu.py and tests/test_attention_prefix_gpu.py, and the tolerance the project uses for its 16-row attention kernels.

Mask (include/internnav_amd.h, ina_attention_prefix): query row i of pair p, i < suf_len[p], sees cache rows [0, min(pfx_len[p], max_pfx)) of
slot slot[p] and suffix keys j <= i of pair p. Rows i >= suf_len[p] are zeros; a slot outside the cache gives NaN in the rows i < suf_len[p]."""
import numpy as np
import torch

D = 128
ATOL, RTOL = 1.5e-2, 1.0 / 128          # test_attention_wide_gpu._check: |err| <= 1.5e-2 + |ref| / 128 on N(0, 1) inputs (bf16 P and bf16 output)


def tolerance(ref):
    return ATOL + RTOL * np.abs(ref)


def attention_prefix_ref(q, k_suf, v_suf, k_cache, v_cache, slot, pfx_len, suf_len, scale=None, max_pfx=None):
    """float64 numpy. q [P, m, H, D], k_suf / v_suf [P, m, Hkv, D], k_cache / v_cache [slots, S, Hkv, D], tables int [P] -> out [P, m, H, D].
    Only the rows the mask admits are ever read (slices, no multiplication by a mask): NaN anywhere else cannot reach the result."""
    q, k_suf, v_suf, k_cache, v_cache = (np.asarray(t, dtype=np.float64) for t in (q, k_suf, v_suf, k_cache, v_cache))
    P, m, H, d = q.shape
    Hkv = k_suf.shape[2]
    G = H // Hkv
    n_slots, S = k_cache.shape[:2]
    scale = d ** -0.5 if scale is None else scale
    max_pfx = S if max_pfx is None else max_pfx
    out = np.zeros((P, m, H, d))
    for p in range(P):
        sl, n = int(slot[p]), min(max(int(suf_len[p]), 0), m)
        if not 0 <= sl < n_slots:
            out[p, :n] = np.nan
            continue
        pf = min(max(int(pfx_len[p]), 0), max_pfx)
        for h in range(H):
            kh = h // G
            for i in range(n):
                k = np.concatenate([k_cache[sl, :pf, kh], k_suf[p, : i + 1, kh]], 0)
                v = np.concatenate([v_cache[sl, :pf, kh], v_suf[p, : i + 1, kh]], 0)
                s = (k @ q[p, i, h]) * scale
                e = np.exp(s - s.max())
                out[p, i, h] = (e / e.sum()) @ v
    return out


def sdpa_ref(q, k_suf, v_suf, k_cache, v_cache, slot, pfx_len, suf_len, scale=None):
    """the same through torch SDPA in float64 on the per-pair concatenation [cache[slot, :pfx_len] | suffix[:suf_len]] with a bottom-right-aligned
    causal mask (query i of suf_len sees keys <= pfx_len + i)."""
    P, m, H, d = q.shape
    Hkv = k_suf.shape[2]
    out = np.zeros((P, m, H, d))
    for p in range(P):
        n, pf, sl = int(suf_len[p]), int(pfx_len[p]), int(slot[p])
        if n == 0:
            continue
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
        k = torch.cat([t(k_cache[sl, :pf]), t(k_suf[p, :n])], 0).permute(1, 0, 2).repeat_interleave(H // Hkv, 0)     # [H, pf + n, D]
        v = torch.cat([t(v_cache[sl, :pf]), t(v_suf[p, :n])], 0).permute(1, 0, 2).repeat_interleave(H // Hkv, 0)
        mask = torch.ones(n, pf + n, dtype=torch.bool).tril(diagonal=pf)
        o = torch.nn.functional.scaled_dot_product_attention(t(q[p, :n]).permute(1, 0, 2), k, v, attn_mask=mask, scale=scale)
        out[p, :n] = o.permute(1, 0, 2).numpy()
    return out


# ---- the cases: (H, Hkv, m, slot [P], suf_len [P], {slot: pfx_len}); 4 cache slots of S rows, slot 3 is named by no pair.
#      m covers 1 / 3 / 16 / 17 / 64 (one row, a partial tile, a full tile, one row more, the contract's limit), suf_len is ragged with 1 and m
#      in every case, pfx_len covers 0 / 1 / 63 / 64 / 65 (chunk edges) and 256 / 257 / 300 (what four waves hold at once, and one chunk more:
#      a wave walks a second chunk), the slot table is non-monotonic and slot 1 is shared by three pairs.
S_CACHE, N_SLOTS = 320, 4
CASES = [
    (28, 4, 3, [1, 1, 0, 1, 2], [3, 1, 2, 3, 3], {0: 0, 1: 300, 2: 63}),
    (28, 4, 1, [1, 1, 0, 1, 2], [1, 1, 1, 1, 1], {0: 64, 1: 1, 2: 257}),
    (28, 4, 16, [1, 1, 0, 1, 2], [16, 1, 7, 16, 9], {0: 65, 1: 256, 2: 0}),
    (4, 4, 17, [1, 1, 0, 1, 2], [17, 1, 16, 5, 17], {0: 257, 1: 63, 2: 300}),
    (4, 4, 64, [1, 1, 0, 1, 2], [64, 1, 33, 64, 17], {0: 1, 1: 65, 2: 64}),
    (28, 4, 64, [1, 0], [64, 1], {0: 300, 1: 0}),
    (4, 4, 3, [1, 1, 0, 1, 2], [3, 2, 1, 0, 3], {0: 256, 1: 64, 2: 1}),          # a pair with nothing to score: zeros
]
CASE_IDS = [f"H{c[0]}_kv{c[1]}_m{c[2]}_{i}" for i, c in enumerate(CASES)]


def make_case(case, seed=0):
    """-> dict of bf16 torch tensors (CPU) laid out as the engine passes them - q / k_suf / v_suf strided views of ONE fused [P * m, (H + 2 Hkv) D]
    projection buffer, k_cache / v_cache views of one [slots * S, 2 Hkv D] cache - and the int32 tables. N(0, 1) values; every row the mask must
    not read is NaN: cache rows at or behind pfx_len, every row of an unnamed slot, fused rows (q, k and v) at or behind suf_len."""
    H, Hkv, m, slot, suf, pfx_of = case
    P = len(slot)
    g = torch.Generator().manual_seed(1000 + seed)
    fused = torch.randn(P * m, (H + 2 * Hkv) * D, generator=g).to(torch.bfloat16)
    cache = torch.randn(N_SLOTS * S_CACHE, 2 * Hkv * D, generator=g).to(torch.bfloat16)
    c3 = cache.view(N_SLOTS, S_CACHE, 2 * Hkv * D)
    for s in range(N_SLOTS):
        c3[s, pfx_of.get(s, 0):] = float("nan")
    f3 = fused.view(P, m, -1)
    for p in range(P):
        f3[p, suf[p]:] = float("nan")
    return dict(fused=fused, cache=cache, H=H, Hkv=Hkv, m=m, P=P, slot=torch.tensor(slot, dtype=torch.int32),
                pfx_len=torch.tensor([pfx_of[s] for s in slot], dtype=torch.int32), suf_len=torch.tensor(suf, dtype=torch.int32))


def views(fused, cache, H, Hkv, m):
    """(q, k_suf, v_suf, k_cache, v_cache) views of the two buffers (any device)"""
    P = fused.shape[0] // m
    q = fused[:, : H * D].view(P, m, H, D)
    k = fused[:, H * D:(H + Hkv) * D].view(P, m, Hkv, D)
    v = fused[:, (H + Hkv) * D:].view(P, m, Hkv, D)
    c5 = cache.view(N_SLOTS, S_CACHE, 2, Hkv, D)
    return q, k, v, c5[:, :, 0], c5[:, :, 1]


def reference_of(c):
    q, k, v, kc, vc = (t.double().numpy() for t in views(c["fused"], c["cache"], c["H"], c["Hkv"], c["m"]))
    return attention_prefix_ref(q, k, v, kc, vc, c["slot"].numpy(), c["pfx_len"].numpy(), c["suf_len"].numpy())


# ---- the argument sets ina_attention_prefix must refuse before any HIP call (dummy pointers, no GPU); keys name the argument that is replaced.
#      Defaults of the caller: P = 2 pairs x m = 3 rows x H = 28 / Hkv = 4 heads of D = 128 in the engine's layout.
def abi_refusal_cases():
    return [dict(D=64), dict(m=0), dict(m=65), dict(H=30), dict(Hkv=0), dict(P=-1), dict(max_pfx=-1), dict(n_slots=0), dict(q_rs=4612), dict(c_rs=1028),
            dict(s_hs=100), dict(o_rs=3586), dict(slot=None), dict(pfx_len=None), dict(suf_len=None), dict(Q=None), dict(k_cache=None), dict(v_suf=None),
            dict(Q_off=8), dict(O_off=4), dict(scale=float("nan"))]
