"""TEST INFRASTRUCTURE of the rollout-session tests: a scripted rollout (which envs step, which reset), seeded frames / noise / goals, and
the memory window of an env materialised the way the reference dataset does (navdp_lerobot_dataset.py:215-222: newest frame last, slot j
holds the frame (M - 1 - j) * stride steps back, all-zero images in front of the episode)."""
from __future__ import annotations

import torch

from internnav_amd import synthetic as S

CFG = S.NAVDPNET_CFG
M = CFG["memory_size"]

# 12 steps of 5 envs: resets staggered over the rollout, env 2 sits out steps 3, 8 and 9 (and env 4 step 5)
SCRIPT_B5 = [dict(reset=[], skip=[]) for _ in range(12)]
SCRIPT_B5[3]["skip"] = [2]
SCRIPT_B5[4]["reset"] = [1]
SCRIPT_B5[5]["skip"] = [4]
SCRIPT_B5[7]["reset"] = [0, 3]
SCRIPT_B5[8]["skip"] = [2]
SCRIPT_B5[9]["skip"] = [2]
SCRIPT_B5[10]["reset"] = [2]

MODES = {"point": [1, 1, 1, 1, 1], "none": [0, 0, 0, 0, 0], "image": [2, 2, 2, 2, 2], "pixel": [3, 3, 3, 3, 3], "mixed": [0, 1, 2, 3, 1]}


def window(history, stride: int) -> torch.Tensor:
    """history: the frames [224, 224, 3] of one env since its reset, newest last -> [M, 224, 224, 3]."""
    out = torch.zeros(M, 224, 224, 3)
    for j in range(M):
        back = (M - 1 - j) * stride
        if back < len(history):
            out[j] = history[-1 - back]
    return out


class Rollout:
    """seeded inputs of a scripted rollout of B envs; `steps()` yields per step the stepped env ids, the envs reset before it, the newest
    frames, the materialised windows and the other call arguments (CPU tensors)."""

    def __init__(self, B: int, script, kinds, stride: int, seed: int):
        self.B, self.script, self.stride, self.seed = B, script, stride, seed
        self.kinds = torch.tensor(kinds, dtype=torch.int32)
        self.point = S.navdpnet_inputs(B, seed=seed)["goal"]
        g = S.navdpnet_goal_inputs(B, seed=seed, pixel_channel=4)
        self.image, self.pixel = g["goal_image"], g["goal_pixel"]

    def goals(self, ids):
        k = self.kinds[ids]
        sel = torch.tensor(ids)
        return dict(goal_kind=k, goal_point=self.point[sel] if bool((k == 1).any()) else None,
                    goal_image=self.image[sel[k == 2]] if bool((k == 2).any()) else None,
                    goal_pixel=self.pixel[sel[k == 3]] if bool((k == 3).any()) else None)

    def steps(self):
        T, Sn, K = CFG["predict_size"], CFG["sample_num"], CFG["num_train_timesteps"]
        g = torch.Generator().manual_seed(7000 + self.seed)
        hist = [[] for _ in range(self.B)]
        for t, s in enumerate(self.script):
            for e in s["reset"]:
                hist[e] = []
            ids = [e for e in range(self.B) if e not in s["skip"]]
            n = len(ids)
            rgb = torch.rand(n, 224, 224, 3, generator=g)
            for i, e in enumerate(ids):
                hist[e].append(rgb[i])
            yield dict(t=t, ids=ids, reset=s["reset"], rgb=rgb, images=torch.stack([window(hist[e], self.stride) for e in ids]),
                       depth=torch.rand(n, 1, 224, 224, 1, generator=g) * 5.0, x_init=torch.randn(n, Sn, T, 3, generator=g),
                       step_noise=torch.randn(K, n, Sn, T, 3, generator=g), **self.goals(ids))


# ---- the ranking rollout: 3 envs x 4 steps with point goals (the kind the fp32 oracle implements), env 1 reset before step 2.
# The top-8 / bottom-8 selection is discontinuous in the critic values, so it is compared only where the ORACLE's gap at both cuts exceeds
# the critic error. RANK_DRAW[t][e] names the noise draw of env e at step t: the first draw k = 0, 1, .. for which both oracle gaps
# exceed CRITIC_ERR_BUDGET, found with the oracle alone on the CPU (tests/test_navdp_rollout_cpu.py re-checks it), never with the engine.
# CRITIC_ERR_BUDGET: twice the 7.5e-3 max |critic error| of the full call (bf16 operands against the fp32 oracle) on these weights; the oracle's
# critic values span about 0.5 over an env's 32 samples, so an unselected draw clears the budget at both cuts about one time in ten.
RANK_B, RANK_SEED, CRITIC_ERR_BUDGET = 3, 41, 1.5e-2
RANK_SCRIPT = [dict(reset=[], skip=[]), dict(reset=[], skip=[]), dict(reset=[1], skip=[]), dict(reset=[], skip=[])]
RANK_DRAW = [[5, 19, 13], [5, 0, 8], [33, 38, 1], [4, 2, 14]]


def rank_noise(t: int, e: int, k: int):
    """draw k of (x_init [S, T, 3], step_noise [K, S, T, 3]) for env e at step t of the ranking rollout."""
    T, Sn, K = CFG["predict_size"], CFG["sample_num"], CFG["num_train_timesteps"]
    g = torch.Generator().manual_seed(900000 + 10000 * t + 1000 * e + k)
    return torch.randn(Sn, T, 3, generator=g), torch.randn(K, Sn, T, 3, generator=g)


def rank_steps(draws=None):
    """the steps of the ranking rollout (as Rollout.steps) with the noise of every (step, env) replaced by its selected draw."""
    draws = RANK_DRAW if draws is None else draws
    for st in Rollout(RANK_B, RANK_SCRIPT, [1] * RANK_B, 1, seed=RANK_SEED).steps():
        noise = [rank_noise(st["t"], e, draws[st["t"]][e]) for e in st["ids"]]
        st["x_init"] = torch.stack([n[0] for n in noise])
        st["step_noise"] = torch.stack([n[1] for n in noise], dim=1)
        yield st


def cut_gaps(critic: torch.Tensor):
    """critic [S] -> the gaps between the 8th and 9th lowest and between the 8th and 9th highest value."""
    c = critic.sort().values
    return (c[8] - c[7]).item(), (c[-8] - c[-9]).item()
