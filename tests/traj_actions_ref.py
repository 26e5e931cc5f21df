"""Helper of the traj_actions tests (not a test): an instrumented restatement of policy.traj_to_actions, and the seeded inputs both test files use.

`traj_actions_ref` computes what the host function computes - the same roundings in the same order - with `np.linalg.norm` written as
sqrt(x*x + y*y) and `np.mean(axis=0)` as a sequential fp64 sum in sample order (the first sample by copy, as add.reduce does) divided by S.
Beside the action list and the fp64 mean trajectory it returns the MINIMUM DECISION MARGIN of the run: how far the closest of its comparisons
was from falling the other way. The device kernel restates the same arithmetic but its atan2 / cos / sin differ from the host libm by a few ulp
(~1e-15 relative); on an input whose margin exceeds 1e-9 such a difference cannot change a decision, so the lists must be EQUAL there.
Margins (one per decision taken):
  stop      | |pos - goal| - 0.2 |
  argmin    the gap between the two smallest DIFFERENT distances (exact ties go to the lowest index in both implementations)
  degen     | |target_dir| - 1e-6 |
  round     the distance of delta_yaw / turn from a half-integer
  wrap      the distance of target_yaw - yaw + pi from a multiple of 2 pi
  advance   | |next - goal| - |pos - goal| |
"""
import math

import numpy as np
import torch

TURN = float(np.deg2rad(15))
PI, TWO_PI = float(np.pi), float(2 * np.pi)
MARGIN_BOUND = 1e-9


def mean_trajectory(dp_actions: torch.Tensor) -> np.ndarray:
    """fp64 [T + 1, 2]: x, y / 4 in the tensor's dtype, sequential fp32 cumulative sum per sample, sequential fp64 mean over the samples."""
    t = dp_actions.detach().clone()
    t[:, :, :2] /= 4.0
    d = t.float().cpu().numpy()
    S, T = d.shape[:2]
    cum = np.empty((S, T, 2), np.float32)
    run = d[:, 0, :2].copy()
    cum[:, 0] = run
    for k in range(1, T):
        run = run + d[:, k, :2]                  # float32 + float32, one rounding per step
        cum[:, k] = run
    xy = np.zeros((S, T + 1, 2))
    xy[:, 1:] = cum
    acc = xy[0].copy()
    for s in range(1, S):
        acc = acc + xy[s]
    return acc / S


def _norm(x, y):
    return math.sqrt(x * x + y * y)


def _norm_angle(a):
    return (a + PI) % TWO_PI - PI


def traj_actions_ref(dp_actions: torch.Tensor, log=None, tie_last: bool = False):
    """-> (actions, mean trajectory fp64 [T + 1, 2], minimum decision margin). dp_actions [S, T, 3] is not modified. log: a list that receives
    (number of actions before the decision, kind, margin) per decision. tie_last resolves exact argmin ties to the HIGHEST index - the wrong
    rule, only there so that a test can show that its input tells the two rules apart."""
    traj = mean_trajectory(dp_actions)
    pts = traj.tolist()
    actions = []
    margin = math.inf

    def note(kind, m):
        nonlocal margin
        margin = min(margin, m)
        if log is not None:
            log.append((len(actions), kind, m))

    yaw, (px, py), (gx, gy) = 0.0, pts[0], pts[-1]
    while True:
        dgoal = _norm(px - gx, py - gy)
        note("stop", abs(dgoal - 0.2))
        if not dgoal > 0.2:
            break
        dist = [_norm(x - px, y - py) for x, y in pts]
        lo = min(dist)
        nearest = max(i for i, v in enumerate(dist) if v == lo) if tie_last else dist.index(lo)
        others = [v for v in dist if v != lo]
        if others:
            note("argmin", min(others) - lo)
        tx, ty = pts[min(nearest + 4, len(pts) - 1)]
        tx, ty = tx - px, ty - py
        tn = _norm(tx, ty)
        note("degen", abs(tn - 1e-6))
        if tn < 1e-6:
            break
        raw = math.atan2(ty, tx) - yaw
        wrap = (raw + PI) % TWO_PI
        note("wrap", min(wrap, TWO_PI - wrap))
        q = _norm_angle(raw) / TURN
        note("round", abs(abs(q - math.floor(q)) - 0.5))
        n_turns = int(round(q))
        if n_turns > 0:
            actions += [2] * n_turns
        elif n_turns < 0:
            actions += [3] * (-n_turns)
        yaw = _norm_angle(yaw + n_turns * TURN)
        nx, ny = px + 0.25 * math.cos(yaw), py + 0.25 * math.sin(yaw)
        dnext = _norm(nx - gx, ny - gy)
        note("advance", abs(dnext - dgoal))
        if dnext > dgoal:
            break
        actions.append(1)
        px, py = nx, ny
    return actions, traj, margin


# ------------------------------------------------------------------------------------------------ seeded inputs of the CPU and the GPU test
KINDS = ("strong", "behind", "curved", "static", "slow", "tiny")     # env b of a batch is of kind KINDS[b % 6]: B = 1 and B = 3 get the long lists
SHAPES = ((1, 1), (32, 3), (3, 24), (32, 32))                        # (S, T)
N_ENVS = 64
SEED = 20240611


def seeded_batch(S: int, T: int, seed: int = SEED) -> torch.Tensor:
    """f32 [64, S, T, 3] x4-scaled increments. The LENGTH of the mean path depends on the kind, not on T, so every shape reaches the same branches:
    strong 3 m in a random direction, behind 2 m within 0.4 rad of straight back (six or more turns at once), curved 3 m whose heading sweeps up to
    +-2.5 rad, static 0.02 m, slow 0.5 m, tiny 0.1 m (goal inside the stop radius). Per-sample noise of 20 % of a step; the yaw channel is noise."""
    rng = np.random.default_rng(seed + 1000 * S + T)
    out = np.empty((N_ENVS, S, T, 3), np.float32)
    for b in range(N_ENVS):
        kind = KINDS[b % len(KINDS)]
        total = {"strong": 3.0, "behind": 2.0, "curved": 3.0, "static": 0.02, "slow": 0.5, "tiny": 0.1}[kind] * rng.uniform(0.7, 1.3)
        step = total / T
        head = {"behind": math.pi + rng.uniform(-0.4, 0.4)}.get(kind, rng.uniform(-math.pi, math.pi))
        sweep = rng.uniform(-2.5, 2.5) if kind == "curved" else 0.0
        ang = head + sweep * (np.arange(T) / max(T - 1, 1))
        base = step * np.stack([np.cos(ang), np.sin(ang)], -1)                       # [T, 2]
        xy = base[None] + rng.normal(0.0, 0.2 * step, (S, T, 2))
        out[b, :, :, :2] = (4.0 * xy).astype(np.float32)
        out[b, :, :, 2] = rng.normal(0.0, 0.1, (S, T)).astype(np.float32)
    return torch.from_numpy(out)


def tie_case() -> torch.Tensor:
    """f32 [2, 12, 3]: 0.25 m steps along +x whose points the pursuit reaches EXACTLY (cos 0 = 1, sin 0 = 0), a run of zero increments - four
    coincident points, an exact four-way tie of the nearest-point search when the position stands on them - then a bend towards +y. Both samples
    are equal, so the mean is exact. The look-ahead target, and with it the number of turns, depends on which of the tied points wins."""
    inc = [(1.0, 0.0)] * 3 + [(0.0, 0.0)] * 3 + [(0.6, 0.8), (0.6, 0.8)] + [(0.0, 1.0)] * 4
    t = torch.zeros(2, len(inc), 3)
    t[:, :, :2] = torch.tensor(inc)
    return t


def minus_x_case() -> torch.Tensor:
    """f32 [4, 8, 3]: a straight line along -x, 0.25 m per step. The first heading is atan2(+0, -d) = pi, so target_yaw - yaw + pi = 2 pi exactly: the
    wrap margin is ZERO and delta_yaw may come out as -pi (twelve right turns, what the host gives) or +pi (twelve left turns)."""
    t = torch.zeros(4, 8, 3)
    t[:, :, 0] = -1.0
    return t
