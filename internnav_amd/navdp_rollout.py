"""NavDPNet rollout sessions: the visual memory of every env stays on the device as cached frame tokens, a step encodes only the new frame.

`NavDPNet.predict_*_batch_action_vel` takes the whole memory window [B, M, 224, 224, 3] on every call and runs all B * M frames through the
RGB ViT-S. In a rollout the window slides: one frame per env is new, the other M - 1 were tokenised on earlier steps, and their tokens do not
depend on the slot they sit in - `former_pe` is added only where the final LayerNorm writes them (vit_s.DinoV2Encoder.forward, `pos`).
`NavDPRollout` keeps the fp32 final-LayerNorm tokens (before `former_pe`, i.e. before the only rounding that depends on the slot) of each
env's last frames in a ring in HBM; a step runs the RGB tower over the n new frames only and ONE `ina_memory_gather` launch writes the new
tokens into the ring and rebuilds the former's bf16 token rows (ring row + former_pe[slot], rounded once - the arithmetic of the full call).
Memory semantics are the reference dataset's (navdp_lerobot_dataset.py:215-222): the newest frame is the last slot, slots older than the
episode hold an all-zero image (its tokens are computed once at construction by the same ViT path), `stride` is `memory_digit`.

GEMM rows are independent, attention and the norms are per image and per row, and the TILED GEMM kernels all accumulate K in the same
order (gemm.hip, tests/test_ops_gpu.py), so the tokens of a frame do not depend on how many frames share its pass: the n-frame pass of a
step, and the one-frame pass of the blank image, give the bits of the full call's n * M-frame pass although ina_gemm_select picks other
tiles for it, and a session step gives the bits of `predict_mixedgoal_batch_action_vel` on the materialised window. This rests on what
ina_gemm_select does for the ViT-S GEMMs today: the row-panel configs 34 / 35 (another K order, NOT bit-equal; from 16384 rows on, the
full call's range from 8 envs) are selected only without a bias and every ViT-S Linear has one, and the weight-streaming config 32 needs
64 rows or fewer where a frame has 257. Whoever lets the selection take the biased row-panel epilogue must pin the session's tiles to the
full call's (tests/test_navdp_rollout_cpu.py pins the selection; the GPU tests would show the difference).

Host / device split (as QwenVLEngine.plan): `RolloutPlan` does every index computation on the host (no device work, no sync - `reset` only
clears host counters); a step uploads one int32 table and issues a fixed launch sequence, so a step is graph capturable (`capture`).
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .navdp import IMAGENET_MEAN, IMAGENET_STD, GoalPlan, NavDPNet
from .runtime import CapacityError, GraphedCall

TOKENS, WIDTH = 256, 384   # patch tokens per frame and their width (ViT-S/14 on 224 x 224)


def ring_depth(memory_size: int, stride: int) -> int:
    """frames an env's ring holds: slot j of the window is (memory_size - 1 - j) * stride pushes old, the oldest (memory_size - 1) * stride."""
    assert memory_size >= 1 and stride >= 1
    return (memory_size - 1) * stride + 1


def ring_bytes(max_envs: int, memory_size: int, stride: int) -> int:
    """HBM footprint of the token ring: max_envs x depth frames of 256 x 384 fp32 tokens (393216 bytes per frame)."""
    return max_envs * ring_depth(memory_size, stride) * TOKENS * WIDTH * 4


class RolloutPlan:
    """Host state of the rings: per env the ring slot of its last push (`head`) and its pushes since the last reset, saturated at the ring
    depth (`count`). Pure host arithmetic: no torch device, no library."""

    def __init__(self, max_envs: int, memory_size: int, stride: int = 1):
        self.max_envs, self.M, self.stride = int(max_envs), int(memory_size), int(stride)
        self.depth = ring_depth(self.M, self.stride)
        self.head = np.zeros(self.max_envs, dtype=np.int32)
        self.count = np.zeros(self.max_envs, dtype=np.int32)

    def _ids(self, env_ids) -> np.ndarray:
        if env_ids is None:
            ids = np.arange(self.max_envs, dtype=np.int64)
        else:
            ids = np.asarray(env_ids.cpu() if torch.is_tensor(env_ids) else env_ids, dtype=np.int64)
        if ids.ndim != 1 or ids.size == 0:
            raise ValueError(f"env_ids must be a non-empty 1-D list of env indices, got shape {ids.shape}")
        if ids.min() < 0 or ids.max() >= self.max_envs:
            raise CapacityError(f"env_ids {ids.min()} .. {ids.max()} outside the session's {self.max_envs} envs")
        if np.unique(ids).size != ids.size:
            raise ValueError("env_ids holds an env twice: one step pushes one frame per env")
        return ids

    def reset(self, env_ids=None) -> None:
        """the named envs (None: all) start a new episode: their next window holds blank frames in front of the new frame."""
        self.count[self._ids(env_ids)] = 0

    def step(self, env_ids=None) -> np.ndarray:
        """push one frame for the named envs (None: all, in order) -> int32 [3, n]: env, the ring slot the new frame goes to, and the pushes
        since the reset with this one included (what ina_memory_gather reads). Envs not named keep head and count."""
        ids = self._ids(env_ids)
        self.head[ids] = (self.head[ids] + 1) % self.depth
        self.count[ids] = np.minimum(self.count[ids] + 1, self.depth)
        return np.stack([ids.astype(np.int32), self.head[ids], self.count[ids]])

    def slots(self, table: np.ndarray) -> np.ndarray:
        """the kernel's source rule on the host: int32 [n, M], the ring slot window slot j of launch row i reads (j = M - 1: the slot just
        written), or -1 where the blank frame stands in."""
        _, head, count = table
        back = (self.M - 1 - np.arange(self.M, dtype=np.int64)) * self.stride          # [M]
        slot = (head[:, None].astype(np.int64) - back[None, :]) % self.depth
        return np.where(back[None, :] < count[:, None], slot, -1).astype(np.int32)


class NavDPRollout:
    """Stateful rollout over a NavDPNet engine: `step` takes the NEWEST frame of each stepped env and returns what
    `net.predict_mixedgoal_batch_action_vel` returns on that env's whole window, bit for bit.

    HBM footprint: the ring holds (M - 1) * stride + 1 frames per env as fp32 tokens, max_envs * depth * 393216 bytes - 201 MB at 64 envs,
    M = 8, stride 1 (403 MB at stride 2) - plus 393 KB per env for the step's new tokens and one blank frame; see `ring_bytes`.
    The caller no longer holds or uploads the [B, M, 224, 224, 3] window (308 MB of fp32 at B = 64).

    The session shares the engine's workspaces: calls on `net` and session steps may be interleaved, not overlapped."""

    def __init__(self, net: NavDPNet, max_envs: int, stride: int = 1):
        if max_envs > net.b_max:
            raise CapacityError(f"session of {max_envs} envs on an engine built for {net.b_max}")
        self.net, self.max_envs, self.stride = net, int(max_envs), int(stride)
        self.plan = RolloutPlan(max_envs, net.M, stride)
        dev, f32 = net.device, torch.float32
        self.ring = torch.zeros(self.max_envs, self.plan.depth, TOKENS, WIDTH, dtype=f32, device=dev)
        self.fresh = torch.empty(self.max_envs, TOKENS, WIDTH, dtype=f32, device=dev)
        self.blank = torch.empty(TOKENS, WIDTH, dtype=f32, device=dev)
        # [kind | row] of the goal plan (2n, contiguous: encode_goals' plan_dev), then env / head / count at fixed offsets
        self.table = torch.zeros(5 * self.max_envs, dtype=torch.int32, device=dev)
        # two pinned host images of the table, used in turn: a step fills one while the upload of the step before may still read the other;
        # the event of an image is waited for before it is filled again
        self._stage = [torch.zeros(5 * self.max_envs, dtype=torch.int32).pin_memory() for _ in range(2)]
        self._staged = [torch.cuda.Event(), torch.cuda.Event()]
        self._turn = 0
        net.rgb.forward(torch.zeros(1, 224, 224, 3, dtype=f32, device=dev), net.vit_ws, None, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                        extra_outputs=((None, self.blank, None, None),))

    @property
    def ring_bytes(self) -> int:
        return ring_bytes(self.max_envs, self.net.M, self.stride)

    def reset(self, env_ids=None) -> None:
        """start a new episode for these envs (None: all). Host only: no launch, no device sync; the stale ring rows are never read."""
        self.plan.reset(env_ids)

    # ---- host side of a step
    def _check(self, gplan: GoalPlan, env_ids, rgb, depth, x_init, step_noise) -> None:
        """refuse a malformed step before anything advances: row counts, the frame shape and the env ids (RolloutPlan._ids)."""
        n = gplan.B
        n_ids = len(self.plan._ids(env_ids))
        if not (n == n_ids and rgb.shape[0] == n and depth.shape[0] == n and x_init.shape[0] == n and step_noise.shape[1] == n):
            raise ValueError(f"{n} goal kinds, {n_ids} envs, {rgb.shape[0]} frames, {depth.shape[0]} depth frames, {x_init.shape[0]} x_init rows, "
                             f"{step_noise.shape[1]} step-noise rows")
        if tuple(rgb.shape[1:]) != (224, 224, 3):
            raise ValueError(f"rgb must be [n, 224, 224, 3] (the newest frame of each env), got {tuple(rgb.shape)}")

    def _upload_table(self, gplan: GoalPlan, env_ids) -> None:
        """advance the rings of a checked step on the host and upload the step's table (self.table) on the current stream."""
        n, E = gplan.B, self.max_envs
        tab = self.plan.step(env_ids)
        k = self._turn
        self._turn = 1 - k
        self._staged[k].synchronize()               # the upload that last read this image is done (no-op for a fresh event)
        host = self._stage[k]
        host[:n], host[n:2 * n] = gplan.kind, gplan.row
        host[2 * E:].view(3, E)[:, :n] = torch.from_numpy(tab)
        self.table.copy_(host, non_blocking=True)
        self._staged[k].record()

    # ---- device side of a step: a fixed launch sequence over static buffers
    def _run(self, gplan: GoalPlan, table: torch.Tensor, goal_point, goal_image, goal_pixel, rgb, depth, x_init, step_noise):
        net, n, E = self.net, gplan.B, self.max_envs
        M, Lc, D = net.M, net.Lc, net.D
        nt = (M + 1) * TOKENS
        fresh = self.fresh[:n]
        net.rgb.forward(rgb.reshape(n, 224, 224, 3), net.vit_ws, None, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                        extra_outputs=((None, fresh.view(n * TOKENS, WIDTH), None, None),))
        ops.memory_gather(net.former.tokens[: n * nt].view(n, nt, WIDTH), self.ring, fresh, self.blank, net.former.pe[: M * TOKENS],
                          table[2 * E:2 * E + n], table[3 * E:3 * E + n], table[4 * E:4 * E + n], stride=self.stride)
        net.encode_depth_and_former(n, depth)
        net.encode_goals(gplan, table[: 2 * n], goal_point, goal_image, goal_pixel)
        return net._sample_and_rank(n, x_init, step_noise)

    def step(self, goal_kind, goal_point: Optional[torch.Tensor] = None, goal_image: Optional[torch.Tensor] = None,
             goal_pixel: Optional[torch.Tensor] = None, *, rgb: torch.Tensor, depth: torch.Tensor, x_init: torch.Tensor,
             step_noise: torch.Tensor, env_ids: Optional[Sequence[int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """one policy step of the envs `env_ids` (None: all max_envs, in order; otherwise distinct env indices, row i of every input belongs to
        env_ids[i]). rgb f32|bf16 [n, 224, 224, 3] in 0..1: the NEWEST frame only; depth [n, 1, 224, 224, 1] metres; goal arguments, x_init
        [n, S, T, 3], step_noise [K, n, S, T, 3] and the result (negative, positive) f32 [n, 8, T, 3] as predict_mixedgoal_batch_action_vel.
        Envs not named keep their memory untouched."""
        gplan = self.net._plan_goals(goal_kind, goal_point, goal_image, goal_pixel)
        self._check(gplan, env_ids, rgb, depth, x_init, step_noise)
        self._upload_table(gplan, env_ids)
        dev = self.net.device
        return self._run(gplan, self.table, goal_point, goal_image, goal_pixel, rgb.to(dev).contiguous(), depth.to(dev), x_init.to(dev),
                         step_noise.to(dev))

    def capture(self, goal_kind, goal_point: Optional[torch.Tensor] = None, goal_image: Optional[torch.Tensor] = None,
                goal_pixel: Optional[torch.Tensor] = None, *, rgb: torch.Tensor, depth: torch.Tensor, x_init: torch.Tensor,
                step_noise: torch.Tensor, env_ids: Optional[Sequence[int]] = None) -> "CapturedStep":
        """perform this step AND capture its launch sequence into a hipGraph (runtime.GraphedCall: the capture runs with the cyclic garbage
        collector off). The returned object replays it for later steps of the same shape: the same number of envs with the same goal kinds
        per row; the env ids, goal values and frames may change. `.outputs` holds this step's (negative, positive)."""
        return CapturedStep(self, goal_kind, goal_point, goal_image, goal_pixel, rgb, depth, x_init, step_noise, env_ids)


class CapturedStep:
    """A captured session step. Capturing executes the launch sequence three times on the same table and inputs (two warm-up runs and the
    capture); the sequence is idempotent - the ring slot of the new frame is rewritten with the same tokens - so that counts as ONE step."""

    def __init__(self, ses: NavDPRollout, goal_kind, goal_point, goal_image, goal_pixel, rgb, depth, x_init, step_noise, env_ids):
        self.ses = ses
        dev = ses.net.device
        self.kinds = torch.as_tensor(goal_kind).clone()
        gplan = ses.net._plan_goals(self.kinds, goal_point, goal_image, goal_pixel)
        ses._check(gplan, env_ids, rgb, depth, x_init, step_noise)
        ses._upload_table(gplan, env_ids)

        def static(t, dtype=None):
            return None if t is None else t.to(device=dev, dtype=dtype or t.dtype, copy=True).contiguous()

        inputs = dict(table=ses.table, rgb=static(rgb), depth=static(depth), x_init=static(x_init), step_noise=static(step_noise))
        for k, t in (("goal_point", goal_point), ("goal_image", goal_image), ("goal_pixel", goal_pixel)):
            if t is not None:
                inputs[k] = static(t, torch.float32)

        def fn(table, rgb, depth, x_init, step_noise, goal_point=None, goal_image=None, goal_pixel=None):
            return ses._run(gplan, table, goal_point, goal_image, goal_pixel, rgb, depth, x_init, step_noise)

        self.gplan = gplan
        self.call = GraphedCall(fn, inputs)
        self.outputs = self.call.outputs

    def __call__(self, goal_point: Optional[torch.Tensor] = None, goal_image: Optional[torch.Tensor] = None,
                 goal_pixel: Optional[torch.Tensor] = None, *, rgb: torch.Tensor, depth: torch.Tensor, x_init: torch.Tensor,
                 step_noise: torch.Tensor, env_ids: Optional[Sequence[int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        ses = self.ses
        gplan = ses.net._plan_goals(self.kinds, goal_point, goal_image, goal_pixel)
        if not (torch.equal(gplan.kind, self.gplan.kind) and torch.equal(gplan.row, self.gplan.row)):
            raise ValueError("a captured step replays the goal layout it was captured with (the same goal_point form, [n, 3] or compact)")
        ses._check(gplan, env_ids, rgb, depth, x_init, step_noise)
        new = dict(rgb=rgb, depth=depth, x_init=x_init, step_noise=step_noise)
        for k, t in (("goal_point", goal_point), ("goal_image", goal_image), ("goal_pixel", goal_pixel)):
            if t is not None:
                new[k] = t
        for k, v in new.items():
            if v.shape != self.call.inputs[k].shape:
                raise ValueError(f"{k}: captured with shape {tuple(self.call.inputs[k].shape)}, got {tuple(v.shape)}")
        ses._upload_table(gplan, env_ids)            # the rings advance only once the replay is accepted
        return self.call(**new)
