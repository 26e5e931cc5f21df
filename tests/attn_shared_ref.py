"""TEST INFRASTRUCTURE: float64 restatement of ops.attention_shared (internnav_amd/csrc/attention_shared.hip), a brute-force model of its host
tile plan and the poisoned test cases shared by tests/test_attn_shared_ref_cpu.py and tests/test_attention_shared_gpu.py.

Mask (include/internnav_amd.h, ina_attention_shared): row r, named by tile t, sees cache rows [0, min(tile_pfx[t], max_pfx)) of slot tile_slot[t]
and the first min(tail_len[r], T) rows of its own tail. tail_len <= 0: a zero row; a slot outside the cache: NaN in the tile's rows that have a
tail; a row no tile names is not written. The tolerance is the project's for its 16-row attention kernels, attn_prefix_ref.tolerance."""
import numpy as np
import torch

from attn_prefix_ref import tolerance  # noqa: F401  (1.5e-2 + |ref| / 128 on N(0, 1) inputs)

D = 128
FILL = 7.0          # what the output buffer holds before a launch: a row the launch skips keeps it


def attention_shared_ref(q, k_tail, v_tail, k_cache, v_cache, tile_rows, tile_slot, tile_pfx, tail_len, scale=None, max_pfx=None, fill=FILL):
    """float64 numpy. q [R, H, D], k_tail / v_tail [R, T, Hkv, D], k_cache / v_cache [slots, S, Hkv, D], tile_rows int [n_tiles, cpt], tile_slot /
    tile_pfx int [n_tiles], tail_len int [R] -> out [R, H, D] (rows no tile names: `fill`). Mask and softmax restated on the two key ranges
    WITHOUT concatenating them: a joint maximum, two exponential sums. Only admitted rows are read (slices): NaN elsewhere cannot reach the result."""
    q, k_tail, v_tail, k_cache, v_cache = (np.asarray(t, dtype=np.float64) for t in (q, k_tail, v_tail, k_cache, v_cache))
    R, H, d = q.shape
    T, Hkv = k_tail.shape[1:3]
    G = H // Hkv
    n_slots, S = k_cache.shape[:2]
    scale = d ** -0.5 if scale is None else scale
    max_pfx = S if max_pfx is None else max_pfx
    out = np.full((R, H, d), float(fill))
    for t in range(len(tile_rows)):
        sl, pf = int(tile_slot[t]), min(max(int(tile_pfx[t]), 0), max_pfx)
        for r in (int(x) for x in tile_rows[t]):
            if not 0 <= r < R:
                continue
            n = min(max(int(tail_len[r]), 0), T)
            if not 0 <= sl < n_slots:
                out[r] = np.nan if n > 0 else 0.0
                continue
            out[r] = 0.0
            if n == 0:
                continue
            for h in range(H):
                kh = h // G
                sp = (k_cache[sl, :pf, kh] @ q[r, h]) * scale                # the prompt, in place
                st = (k_tail[r, :n, kh] @ q[r, h]) * scale                   # the row's own tail
                m = max(sp.max() if pf else -np.inf, st.max())
                ep, et = np.exp(sp - m), np.exp(st - m)
                out[r, h] = (ep @ v_cache[sl, :pf, kh] + et @ v_tail[r, :n, kh]) / (ep.sum() + et.sum())
    return out


def brute_force(q, k_tail, v_tail, k_cache, v_cache, row_slot, row_pfx, tail_len):
    """per live row softmax(q K^T) V on the concatenated [prefix | tail] keys, through torch in float64 -> {row: [H, D]}"""
    R, H, d = q.shape
    Hkv = k_tail.shape[2]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    out = {}
    for r in range(R):
        n = int(tail_len[r])
        if r not in row_slot or n <= 0:
            continue
        sl, pf = row_slot[r], row_pfx[r]
        k = torch.cat([t(k_cache[sl, :pf]), t(k_tail[r, :n])], 0).permute(1, 0, 2).repeat_interleave(H // Hkv, 0)      # [H, pf + n, D]
        v = torch.cat([t(v_cache[sl, :pf]), t(v_tail[r, :n])], 0).permute(1, 0, 2).repeat_interleave(H // Hkv, 0)
        p = torch.softmax(torch.einsum("hd,hkd->hk", t(q[r]), k) * d ** -0.5, dim=-1)
        out[r] = torch.einsum("hk,hkd->hd", p, v).numpy()
    return out


def brute_force_plan(prompt_of, G):
    """the tile plan written down row by row: a row joins the open tile of its prompt, a full tile (16 // G rows) is closed"""
    cpt = 16 // G
    open_tile, tiles = {}, []
    for r, b in enumerate(prompt_of):
        if b not in open_tile or len(tiles[open_tile[b]][1]) == cpt:
            open_tile[b] = len(tiles)
            tiles.append((b, []))
        tiles[open_tile[b]][1].append(r)
    return tiles


# ---- the cases: (H, Hkv, [(slot, pfx_len, [tail_len of every candidate]) per prompt]). 5 cache slots of S_CACHE rows, tails of T rows.
#      (H, Hkv) gives 2 / 4 / 1 / 16 candidates per tile; pfx_len covers 0 / 1 / 63 / 64 / 65 / 200 (chunk edges; 200 = four chunks: every wave owns
#      one and the tail chunks wrap round), tail_len 1 / 2 / 63 / 64 / 65 / 128, the candidates per prompt 1 / 2 / 3 / 5 (odd counts leave a half-filled
#      tile at 2 per tile); the prompts' slots are named out of order and at least one slot is named by no tile.
S_CACHE, N_SLOTS, T = 208, 5, 128
CASES = [
    (28, 4, [(3, 200, [1, 65, 2]), (0, 63, [64, 128, 63, 2, 1]), (2, 0, [65])]),
    (8, 2, [(2, 64, [128, 1, 64, 63, 2]), (0, 1, [2, 65]), (4, 65, [63])]),
    (16, 1, [(1, 65, [2, 64]), (3, 0, [1, 128, 63])]),
    (2, 2, [(4, 200, [1, 2, 63, 64, 65]), (1, 1, [128, 5, 3]), (0, 63, [64, 1])]),
]
CASE_IDS = [f"H{c[0]}_kv{c[1]}_{i}" for i, c in enumerate(CASES)]


def make_case(case, seed=0):
    """-> dict of bf16 torch tensors (CPU) laid out as the engine passes them - q a strided view of a fused [rows, (H + 2 Hkv) D] projection
    buffer, the tails views of one [rows * T, 2 Hkv D] buffer, k_cache / v_cache views of one [slots * S, 2 Hkv D] cache - and the int32 tables
    (the tile table from ops.attention_shared_plan). N(0, 1) values; NaN in everything the launch must not read: cache rows at or behind pfx_len,
    every unnamed slot, tail rows at or behind tail_len, the k|v columns of the fused buffer, and the whole tail and q of one extra row that no
    tile names (row R: its tail_len says 9)."""
    from internnav_amd import ops

    H, Hkv, prompts = case
    prompt_of = [b for b, (_, _, tl) in enumerate(prompts) for _ in tl]
    tails = [n for _, _, tl in prompts for n in tl]
    R = len(tails)
    g = torch.Generator().manual_seed(2000 + seed)
    fused = torch.randn(R + 1, (H + 2 * Hkv) * D, generator=g).to(torch.bfloat16)
    fused[:, H * D:] = float("nan")
    fused[R] = float("nan")
    tail = torch.randn((R + 1) * T, 2 * Hkv * D, generator=g).to(torch.bfloat16)
    t3 = tail.view(R + 1, T, -1)
    for r, n in enumerate(tails + [0]):
        t3[r, n:] = float("nan")
    cache = torch.randn(N_SLOTS * S_CACHE, 2 * Hkv * D, generator=g).to(torch.bfloat16)
    c3 = cache.view(N_SLOTS, S_CACHE, -1)
    pfx_of = {s: p for s, p, _ in prompts}
    for s in range(N_SLOTS):
        c3[s, pfx_of.get(s, 0):] = float("nan")
    tiles, owner = ops.attention_shared_plan(prompt_of, H // Hkv)
    i32 = lambda v: torch.tensor(np.asarray(v), dtype=torch.int32)
    return dict(fused=fused, tail=tail, cache=cache, H=H, Hkv=Hkv, R=R, prompt_of=prompt_of, tile_rows=i32(tiles),
                tile_slot=i32([prompts[b][0] for b in owner]), tile_pfx=i32([prompts[b][1] for b in owner]), tail_len=i32(tails + [9]),
                row_slot={r: prompts[b][0] for r, b in enumerate(prompt_of)}, row_pfx={r: prompts[b][1] for r, b in enumerate(prompt_of)})


def views(fused, tail, cache, H, Hkv):
    """(q, k_tail, v_tail, k_cache, v_cache) views of the three buffers (any device)"""
    rows = fused.shape[0]
    q = fused[:, : H * D].view(rows, H, D)
    t5 = tail.view(rows, T, 2, Hkv, D)
    c5 = cache.view(N_SLOTS, S_CACHE, 2, Hkv, D)
    return q, t5[:, :, 0], t5[:, :, 1], c5[:, :, 0], c5[:, :, 1]


def reference_of(c, **tables):
    """float64 reference of a case, any of its tables replaced (tile_rows=, tile_slot=, tile_pfx=, tail_len=)"""
    q, kt, vt, kc, vc = (t.double().numpy() for t in views(c["fused"], c["tail"], c["cache"], c["H"], c["Hkv"]))
    tb = {n: (tables[n] if n in tables else c[n]).numpy() for n in ("tile_rows", "tile_slot", "tile_pfx", "tail_len")}
    return attention_shared_ref(q, kt, vt, kc, vc, tb["tile_rows"], tb["tile_slot"], tb["tile_pfx"], tb["tail_len"])


# ---- the argument sets ina_attention_shared must refuse before any HIP call (dummy pointers, no GPU); keys name the argument that is replaced.
#      Defaults of the caller: 3 tiles of 2 places over 5 rows x H = 28 / Hkv = 4 heads of D = 128 in the engine's layout, tails of 8 rows.
def abi_refusal_cases():
    return [dict(D=64), dict(H=30), dict(Hkv=0), dict(H=0), dict(H=34, Hkv=2), dict(n_tiles=0), dict(n_tiles=-1), dict(n_rows=0), dict(n_rows=-3),
            dict(T=0), dict(max_pfx=-1), dict(n_slots=0), dict(q_rs=4612), dict(c_rs=1028), dict(t_hs=100), dict(t_ps=8196), dict(o_rs=3586),
            dict(tile_rows=None), dict(tile_slot=None), dict(tile_pfx=None), dict(tail_len=None), dict(Q=None), dict(O=None), dict(k_cache=None),
            dict(v_tail=None), dict(Q_off=8), dict(O_off=4), dict(k_tail_off=8), dict(scale=float("nan"))]
