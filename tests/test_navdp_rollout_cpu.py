"""Host side of the NavDPNet rollout session (internnav_amd.navdp_rollout), no GPU: the ring plan against a plain deque model, the
ina_memory_gather entry through ctypes, the ring-depth / footprint arithmetic, and the noise draws of the ranking rollout against the fp32 oracle."""
import ctypes as C
import random
from collections import deque

import numpy as np
import pytest

from internnav_amd.navdp_rollout import RolloutPlan, ring_bytes, ring_depth

M = 8


def _run_schedule(seed: int, stride: int, envs: int = 5, steps: int = 40):
    """random interleaving of reset / full step / subset step. Model: per env a deque of the ids of the frames pushed since its reset; window
    slot j holds the frame (M - 1 - j) * stride pushes back, or None (the blank frame) - navdp_lerobot_dataset.py:215-222 with
    memory_digit = stride. The plan is checked through a host image of the ring: ring[env][slot] = id of the frame last written there."""
    rng = random.Random(seed)
    plan = RolloutPlan(envs, M, stride)
    depth = ring_depth(M, stride)
    model = [deque(maxlen=depth) for _ in range(envs)]
    ring = [[None] * depth for _ in range(envs)]
    frame = 0
    for _ in range(steps):
        op = rng.random()
        if op < 0.15:
            ids = rng.sample(range(envs), rng.randint(1, envs))
            plan.reset(ids)
            for e in ids:
                model[e].clear()
            continue
        ids = None if op < 0.55 else rng.sample(range(envs), rng.randint(1, envs))
        before = (plan.head.copy(), plan.count.copy())
        table = plan.step(ids)
        order = list(range(envs)) if ids is None else ids
        assert table.dtype == np.int32 and table.shape == (3, len(order)) and table[0].tolist() == order
        untouched = [e for e in range(envs) if e not in order]
        assert (plan.head[untouched] == before[0][untouched]).all() and (plan.count[untouched] == before[1][untouched]).all()
        slots = plan.slots(table)
        for i, e in enumerate(order):
            frame += 1
            model[e].append(frame)
            assert 0 <= table[1, i] < depth and 1 <= table[2, i] <= depth
            ring[e][table[1, i]] = frame
            for j in range(M):
                back = (M - 1 - j) * stride
                want = model[e][-1 - back] if back < len(model[e]) else None
                got = ring[e][slots[i, j]] if slots[i, j] >= 0 else None
                assert got == want, (seed, stride, e, j, got, want)
            assert slots[i, M - 1] == table[1, i]                                  # the newest slot is the one just written ...
            assert all(slots[i, j] != table[1, i] for j in range(M - 1))           # ... and no older slot aliases it


@pytest.mark.parametrize("stride", [1, 2, 4])
def test_plan_equals_deque_model(stride):
    for seed in range(120):
        _run_schedule(seed, stride)


def test_plan_refuses_bad_env_ids():
    from internnav_amd.runtime import CapacityError

    plan = RolloutPlan(4, M, 1)
    with pytest.raises(ValueError):
        plan.step([1, 1])
    with pytest.raises(CapacityError):
        plan.step([4])
    with pytest.raises(ValueError):
        plan.step([])
    assert not plan.count.any() and not plan.head.any()       # a refused step leaves the rings alone


def test_ring_depth_and_footprint():
    assert [ring_depth(8, s) for s in (1, 2, 4)] == [8, 15, 29]
    assert ring_depth(1, 3) == 1
    frame = 256 * 384 * 4
    assert frame == 393216
    assert ring_bytes(64, 8, 1) == 64 * 8 * frame == 201326592                # the 201 MB of the class docstring
    assert ring_bytes(64, 8, 2) == 64 * 15 * frame
    assert ring_bytes(64, 8, 1) < 64 * 8 * 224 * 224 * 3 * 4                   # below the fp32 window the caller held before (308 MB)


def test_memory_gather_entry_visible_through_ctypes(built_lib):
    from internnav_amd import _lib

    h = C.CDLL(str(built_lib))
    assert hasattr(h, "ina_memory_gather")
    res, args = _lib.SYMBOLS["ina_memory_gather"]
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert res is C.c_int and args == [p, i64, p, p, p, p, p, p, p, i32, i32, i32, i32, i32, i32, i32, p]
    # host-side validation runs without a GPU: null tensors and a ring depth that is not (M - 1) * stride + 1 are refused
    fn = _lib.lib().ina_memory_gather
    assert fn(None, 0, None, None, None, None, None, None, None, 1, 1, 8, 256, 384, 8, 1, None) != 0
    assert b"memory_gather" in _lib.lib().ina_last_error()
    assert fn(16, 8 * 256 * 384, 16, 16, 16, 16, 16, 16, 16, 1, 1, 8, 256, 384, 9, 1, None) != 0
    assert b"ring depth" in _lib.lib().ina_last_error()


def test_ranking_draws_keep_the_oracle_within_the_cap():
    """the noise draws of the ranking rollout (tests/navdp_rollout_ref.py: RANK_DRAW) were selected with the fp32 oracle: on the oracle's own
    critic values at most 10 % of the (env, step) pairs have a gap at the bottom-8 or the top-8 cut inside CRITIC_ERR_BUDGET, so the GPU
    ranking test leaves out at most that share as long as the engine's critic error stays inside the budget."""
    import torch

    from internnav_amd import synthetic as S
    from oracle import navdp as o_navdp
    from tests.navdp_rollout_ref import CFG, CRITIC_ERR_BUDGET, RANK_B, cut_gaps, rank_steps

    sd = S.navdpnet_train_state_dict(seed=21, pixel_channel=4)
    pairs = inside = 0
    for st in rank_steps():
        with torch.no_grad():
            _, _, _, critic, _ = o_navdp.navdpnet_pointgoal(sd, st["goal_point"], st["images"], st["depth"], st["x_init"], st["step_noise"], CFG,
                                                            return_all=True)
        for b in range(RANK_B):
            lo, hi = cut_gaps(critic[b])
            print(f"step {st['t']} env {b}: oracle gaps {lo:.3e} / {hi:.3e}")
            pairs += 1
            inside += int(min(lo, hi) <= CRITIC_ERR_BUDGET)
    assert pairs == 12 and inside <= 0.10 * pairs, f"{inside} of {pairs} pairs have an oracle gap inside {CRITIC_ERR_BUDGET}"


def test_session_pass_and_full_call_pass_select_different_tiles(built_lib):
    """the session relies on the GEMM result not depending on the tile config among the TILED kernels (they accumulate K in the same order).
    Pinned here: ina_gemm_select picks another config for the biased qkv GEMM of the session's 5-frame pass (and of the one-frame blank
    pass) than for the full call's 40-frame pass, so the bit-equality tests on the GPU do compare different tiles; and no row count of a
    session or full-call pass selects a kernel outside that family - the row-panel configs 34 / 35 (another K order; selected from 16384
    rows on only WITHOUT a bias, and every ViT-S Linear has one) or the weight-streaming config 32 (64 rows or fewer: a frame has 257)."""
    from internnav_amd import _lib

    def select(rows, N, K, bias=True):
        a = _lib.GemmArgs()
        a.A = a.W = a.C = 4096
        a.bias = 4096 if bias else None
        a.M, a.N, a.K, a.lda, a.ldw, a.ldc, a.batch = rows, N, K, K, K, N, 1
        k = C.c_int(0)
        assert _lib.lib().ina_gemm_select(C.byref(a), C.byref(k)) == 0
        return k.value

    full = select(5 * M * 257, 1152, 384)
    assert select(5 * 257, 1152, 384) != full and select(257, 1152, 384) != full
    for frames in (1, 3, 4, 5, 40, 64, 512):
        for N, K in ((1152, 384), (384, 384), (1536, 384), (384, 1536)):
            assert select(frames * 257, N, K) not in (32, 34, 35), (frames, N, K)
    assert select(512 * 257, 1152, 384, bias=False) == 34          # what a bias-free ViT would get: not bit-equal to the tiled kernels
