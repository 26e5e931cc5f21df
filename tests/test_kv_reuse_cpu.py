"""CPU: host logic of System-2 KV reuse (EngineKVCache, generate(past_key_values=...), InternVLAN1Net(kv_reuse=True)).

The longest-common-prefix rule with its two cuts (image boundary, more than SKINNY_GEMM_MAX_ROWS rows left to run), the rectangle fit,
the agent's reuse-aware chunking, the image-identity check of the policy and the handle's crop / row selection / deepcopy on CPU
tensors. No GPU: handles here hold their own tensors, nothing is a view of an engine."""
import copy
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

from internnav_amd import synthetic as S
from internnav_amd.agent import plan_s2_chunks
from internnav_amd.qwen_vl import ATTN_WIDE_MIN_ROWS, SKINNY_GEMM_MAX_ROWS, EngineKVCache, kv_image_cut, kv_reuse_fit, kv_reuse_lengths

ROOT = Path(__file__).resolve().parent.parent
CFG = S.QWEN_TEST_CFG
IMG, VS, VE = CFG["image_token_id"], CFG["vision_start_id"], CFG["vision_end_id"]


def _prompt(text, *parts):
    """text ids, then for each part either an int (an image of that many tokens) or a list (text)."""
    ids = list(text)
    for p in parts:
        ids += [VS] + [IMG] * p + [VE] if isinstance(p, int) else list(p)
    return np.asarray(ids, dtype=np.int64)


def test_skinny_row_bound_mirrors_the_gemm_planner():
    """the reuse cut keeps more than SKINNY_GEMM_MAX_ROWS rows because ina_plan_gemm sends M <= that bound to the weight-streaming
    kernel (32): read the bound off csrc/gemm.hip."""
    src = (ROOT / "internnav_amd" / "csrc" / "gemm.hip").read_text()
    m = re.search(r"p\.force_cfg <= 0 && p\.M <= (\d+) && p\.batch == 1 && p\.N >= 256\)\s*\{\s*kernel = 32;", src)
    assert m, "automatic weight-streaming rule not found in gemm.hip"
    assert int(m.group(1)) == SKINNY_GEMM_MAX_ROWS


def test_wide_attention_bound_mirrors_its_contract():
    """a run narrower than ATTN_WIDE_MIN_ROWS query rows would take the narrow attention kernel: read the bound off attention_wide.hip."""
    src = (ROOT / "internnav_amd" / "csrc" / "attention_wide.hip").read_text()
    m = re.search(r"if \(\(p\.Lq < (\d+) \|\| p\.Lk < (\d+)\) && !window_shape\(p\)\) return false;", src)
    assert m, "query / key bound of the wide attention kernel not found in attention_wide.hip"
    assert int(m.group(1)) == int(m.group(2)) == ATTN_WIDE_MIN_ROWS


def test_lcp_look_down_mid_text_and_image_cut():
    prev = _prompt(range(10, 50), 100, list(range(60, 70)), 100, [7, 8])
    # look-down turn: the whole previous prompt, then answer + template + a new frame
    new = np.concatenate([prev, _prompt([1, 2, 3], 150, [9])])
    pl = kv_reuse_lengths(new[None], [new.size], [prev], IMG)
    assert pl.tolist() == [prev.size]
    # diverging in the text behind the first image: reuse ends mid-text
    other = prev.copy()
    other[40 + 102 + 4] = 999
    pl = kv_reuse_lengths(new[None], [new.size], [other], IMG)
    assert pl.tolist() == [40 + 102 + 4]
    # a cache that ends inside an image: cut back to that image's first token (its <vision_start> stays in the prefix)
    half = prev[: 40 + 102 + 10 + 1 + 30]
    pl = kv_reuse_lengths(new[None], [new.size], [half], IMG)
    assert pl.tolist() == [40 + 102 + 10 + 1]
    assert kv_image_cut(new, 40 + 50, IMG) == 41 and kv_image_cut(new, 41, IMG) == 41 and kv_image_cut(new, 40 + 102, IMG) == 142
    # nothing cached / identical prompt: at least one token runs
    assert kv_reuse_lengths(new[None], [new.size], [None], IMG).tolist() == [0]
    pl = kv_reuse_lengths(prev[None], [prev.size], [prev], IMG)
    assert 0 < pl[0] and prev.size - pl[0] >= ATTN_WIDE_MIN_ROWS


def test_more_than_skinny_rows_stay_in_the_run_rectangle():
    prev = _prompt(range(10, 50), 100)
    new = np.concatenate([prev, np.arange(200, 230)])        # 30 new text tokens: too narrow a run -> cut
    pl = kv_reuse_lengths(new[None], [new.size], [prev], IMG)
    assert new.size - pl[0] >= ATTN_WIDE_MIN_ROWS
    assert pl[0] == 41                                       # 128 rows back lands inside the image: cut to its first token
    # the rectangle is as wide as the shortest reuse leaves it: only that row is cut
    ids2 = np.stack([new, new])
    pl2 = kv_reuse_lengths(ids2, [new.size] * 2, [prev, prev], IMG)
    assert pl2.tolist() == [41, prev.size]
    long = np.concatenate([prev, np.arange(200, 200 + ATTN_WIDE_MIN_ROWS)])
    assert kv_reuse_lengths(np.stack([long] * 3), [long.size] * 3, [prev] * 3, IMG).tolist() == [prev.size] * 3


def test_ragged_rows_and_rectangle_fit():
    a = _prompt(range(10, 50), 100, list(range(60, 160)))
    b = _prompt(range(10, 50), 100, list(range(60, 300)))
    ids = np.zeros((2, b.size), dtype=np.int64)
    ids[0, : a.size], ids[1] = a, b
    pl = kv_reuse_lengths(ids, [a.size, b.size], [a[:150], b[:200]], IMG)
    assert pl.tolist() == [150, 200]
    fit, dropped = kv_reuse_fit(pl, b.size, 100, s_max=b.size + 100 + 50)
    assert fit.tolist() == [150, 200] and dropped == 0
    fit, dropped = kv_reuse_fit(pl, b.size, 100, s_max=b.size + 100 + 40)
    assert fit.tolist() == [0, 0] and dropped == 2           # once a row runs whole, every other prefix widens the rectangle by itself
    fit, dropped = kv_reuse_fit(np.asarray([30, 200]), b.size, 100, s_max=b.size + 100 + 40)
    assert fit.tolist() == [30, 0] and dropped == 1          # the longest prefix goes first


def test_agent_groups_look_down_rows_apart_from_fresh_ones():
    lens = [2327, 2000, 2300, 1990]
    reuse = [1910, 300, 1900, 296]                           # two look-down turns, two fresh calls
    chunks = plan_s2_chunks(lens, reuse, cap=4, s_max=2944, tail=132)
    assert sorted(map(sorted, chunks)) == [[0, 2], [1, 3]]
    for c in chunks:
        p = [reuse[i] for i in c]
        assert max(p) + max(lens[i] for i in c) - min(p) + 132 <= 2944
    assert plan_s2_chunks(lens, [0] * 4, cap=2, s_max=4000, tail=132) == [[3, 1], [2, 0]]   # no reuse: by length, cap rows per chunk
    assert sum(len(c) for c in plan_s2_chunks(list(range(100, 110)), [5] * 10, cap=3, s_max=10_000, tail=0)) == 10


def _cache(n_rows, layers=3, w=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    toks = [torch.randint(0, 100, (n,), generator=g) if n else None for n in n_rows]
    kv = [torch.randn(layers, n, w, generator=g).to(torch.bfloat16) if n else None for n in n_rows]
    return EngineKVCache(toks, kv)


def test_engine_kv_cache_crop_select_deepcopy_on_cpu():
    c = _cache([12, 7, 0])
    assert len(c) == 3 and [c.get_seq_length(b) for b in range(3)] == [12, 7, 0] and not c.is_view
    d = copy.deepcopy(c)
    assert d.kv[0] is not c.kv[0] and torch.equal(d.kv[0], c.kv[0]) and torch.equal(d.token_ids[1], c.token_ids[1]) and d.kv[2] is None
    s = c.select([1, 0])
    assert s.get_seq_length(0) == 7 and torch.equal(s.kv[1], c.kv[0])
    c.crop(9)
    assert [c.get_seq_length(b) for b in range(3)] == [9, 7, 0] and c.kv[0].shape == (3, 9, 16)
    assert torch.equal(c.kv[0], d.kv[0][:, :9]) and torch.equal(c.token_ids[0], d.token_ids[0][:9])
    c.crop(-2)                                               # HF: a negative length removes that many tokens from the end
    assert [c.get_seq_length(b) for b in range(3)] == [7, 5, 0]
    c.crop(0)
    assert c.get_seq_length(0) == 0 and c.kv[0] is None
    d.batch_select_indices([1])
    assert len(d) == 1 and d.get_seq_length() == 7


def _net(prev_ids, prev_keys, new_keys):
    from internnav_amd.policy import InternVLAN1Net

    net = object.__new__(InternVLAN1Net)
    net.kv_reuse, net.model = True, SimpleNamespace(qwen=SimpleNamespace(cfg=CFG))
    net._kv = (EngineKVCache([torch.as_tensor(prev_ids)], [torch.zeros(1, len(prev_ids), 16, dtype=torch.bfloat16)]), list(prev_keys))
    net.image_keys = list(new_keys)
    return net


def test_policy_reuse_stops_where_image_identities_differ():
    t = list(range(10, 50))
    hist = _prompt(t, [5, 6], 100, [1], 100, [1], 100, [2, 3])          # frames 0, 3, 6 + current
    # look-down turn: same images + a look-down frame with a key of its own -> the whole previous prompt
    ld = np.concatenate([hist, _prompt([4, 4], 150, [5])])
    net = _net(hist, [0, 3, 6], [0, 3, 6, ("look_down", 4)])
    assert net.kv_request({"input_ids": torch.as_tensor(ld)[None]}).get_seq_length() == hist.size
    # next call: the linspace sample repeats frame 0 and 3, then frame 5 replaces 6 - the token ids agree, the images do not
    nxt = _prompt(t, [5, 6], 100, [1], 100, [1], 100, [1], 100, [2, 3])
    net = _net(hist, [0, 3, 6], [0, 3, 5, 8])
    third = 40 + 2 + (102 + 1) * 2 + 1                       # first token of the third image
    assert net.kv_request({"input_ids": torch.as_tensor(nxt)[None]}).get_seq_length() == third
    # a diverging first frame (a new episode's frame 0 under the same key would be reset() first): only the text is reused
    net = _net(hist, [7, 3, 6], [0, 3, 5, 8])
    assert net.kv_request({"input_ids": torch.as_tensor(nxt)[None]}).get_seq_length() == 43
    # nothing in common
    net = _net(hist, [0], [0])
    assert net.kv_request({"input_ids": torch.as_tensor(np.asarray([1, 2, 3]))[None]}) is None
