"""GPU tests of the device action table (ina_traj_actions / ops.traj_actions) and of the opt-in `device_actions` paths built on it.

The kernel restates policy.traj_to_actions rounding for rounding; only atan2 / cos / sin come from another libm (a few ulp). Every input here
has decision margins above 1e-9 (tests/test_traj_actions_cpu.py proves that for the same inputs without a GPU), so the action lists must be
EQUAL to the host's on every case, none skipped; the fp64 mean trajectory involves no libm call and must be equal BIT FOR BIT. The one input
with a zero margin (the straight line along -x) is asserted only as far as the margin rule allows."""
import functools
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import traj_actions_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def ops(built_lib):
    from internnav_amd import ops as o, runtime

    runtime.require_gfx950()
    return o


@functools.lru_cache(maxsize=None)
def _seeded(S, T, bf16=False):
    """(batch [64, S, T, 3] on the host, host lists, fp64 mean trajectories [64, T + 1, 2]) - computed once, shared, never modified."""
    batch = R.seeded_batch(S, T)
    if bf16:
        batch = batch.to(torch.bfloat16)
    refs = [R.traj_actions_ref(batch[b]) for b in range(R.N_ENVS)]
    return batch, [r[0] for r in refs], torch.from_numpy(np.stack([r[1] for r in refs]))


def _bits(t):
    return t.contiguous().view(torch.int64)


def _check_table(actions, count, lists, max_actions):
    actions, count = actions.cpu(), count.cpu()
    assert actions.dtype == count.dtype == torch.int32 and actions.shape == (len(lists), max_actions) and count.shape == (len(lists),)
    for b, want in enumerate(lists):
        n = min(len(want), max_actions)
        assert int(count[b]) == n, (b, int(count[b]), n)
        assert actions[b, :n].tolist() == want[:n], (b, actions[b].tolist(), want[:max_actions])
        assert not actions[b, n:].any()                                  # zero padding


def test_reference_executed_cases(ops):
    cases = torch.load(GOLD / "vln_utils.pt", weights_only=True)["cases"]
    batch = torch.stack([c["traj"] for c in cases])
    lists = [c["actions"] for c in cases]
    assert batch.dtype == torch.float32 and max(len(a) for a in lists) <= 256
    t = batch.to(DEV)
    a4, c4 = ops.traj_actions(t, len(cases), 4)
    _check_table(a4, c4, lists, 4)
    assert torch.equal(t.cpu(), batch)                                   # without scale_in_place the input is left alone
    a, c = ops.traj_actions(t, len(cases), 256, scale_in_place=True)
    _check_table(a, c, lists, 256)
    assert torch.equal(t.cpu().view(torch.int32), torch.stack([c["mutated"] for c in cases]).view(torch.int32))    # vln_utils.py:129, bit for bit


@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("S,T", R.SHAPES)
def test_seeded_inputs_equal_the_host_function(ops, S, T, B):
    batch, lists, trajs = _seeded(S, T)
    t = batch[:B].to(DEV)
    rows = t.view(B * S, T, 3)                                            # generate_traj's layout
    for max_actions in (1, 4, 256):
        out = torch.full((B, T + 1, 2), float("nan"), dtype=torch.float64, device=DEV)
        a, c = ops.traj_actions(rows if max_actions == 4 else t, B, max_actions, traj_out=out)
        _check_table(a, c, lists[:B], max_actions)
        assert torch.equal(_bits(out.cpu()), _bits(trajs[:B])), (S, T, B, max_actions)
    assert torch.equal(t.cpu(), batch[:B])


def test_bf16_input_equals_the_host_function_on_the_same_tensor(ops):
    from internnav_amd.policy import traj_to_actions

    batch, lists, trajs = _seeded(32, 32, True)
    assert batch.dtype == torch.bfloat16
    for b in (0, 1, 2):
        assert traj_to_actions(batch[b].clone()) == lists[b]              # the host function itself, on the bf16 tensor
    t = batch.to(DEV)
    out = torch.empty((R.N_ENVS, 33, 2), dtype=torch.float64, device=DEV)
    a, c = ops.traj_actions(t, R.N_ENVS, 256, traj_out=out, scale_in_place=True)
    _check_table(a, c, lists, 256)
    assert torch.equal(_bits(out.cpu()), _bits(trajs))
    want = batch.clone()
    want[..., :2] /= 4.0
    assert torch.equal(t.cpu().view(torch.int16), want.view(torch.int16))


def test_edge_inputs(ops):
    # all zero: count 0, an all-zero table and an all-zero mean trajectory
    z = torch.zeros(2, 5, 7, 3, device=DEV)
    out = torch.full((2, 8, 2), 1.0, dtype=torch.float64, device=DEV)
    a, c = ops.traj_actions(z, 2, 4, traj_out=out)
    assert not c.cpu().any() and not a.cpu().any() and not _bits(out.cpu()).any()
    # exact ties of the nearest-point search (four coincident points under the position): the lowest index wins, as in np.argmin
    t = R.tie_case()
    want, traj, margin = R.traj_actions_ref(t)
    assert margin > R.MARGIN_BOUND and R.traj_actions_ref(t, tie_last=True)[0] != want
    out = torch.empty((1, t.shape[1] + 1, 2), dtype=torch.float64, device=DEV)
    a, c = ops.traj_actions(t.to(DEV), 1, 256, traj_out=out)
    _check_table(a, c, [want], 256)
    assert torch.equal(_bits(out.cpu()[0]), _bits(torch.from_numpy(traj)))
    # the straight line along -x: delta_yaw = -pi or +pi at the first decision (wrap margin 0, the only one at or below the bound - CPU test).
    # Either sign gives twelve equal turns and the heading -pi; every later decision has a clear margin, so the rest of the list is the host's
    t = R.minus_x_case()
    want, traj, _ = R.traj_actions_ref(t)
    out = torch.empty((1, t.shape[1] + 1, 2), dtype=torch.float64, device=DEV)
    a, c = ops.traj_actions(t.to(DEV), 1, 256, traj_out=out)
    got = a.cpu()[0, : int(c.cpu()[0])].tolist()
    print("straight line along -x: first twelve actions", got[:12])
    assert got[:12] in ([3] * 12, [2] * 12) and got[12:] == want[12:] and len(got) == len(want)
    assert torch.equal(_bits(out.cpu()[0]), _bits(torch.from_numpy(traj)))


def test_one_captured_replay(ops, monkeypatch):
    """runtime.GraphedCall around the launch: the library is entered once per call of the function (one kernel node - the wrapper issues nothing
    else), a replay issues none, and replays on refreshed inputs give what the eager launch gives."""
    from internnav_amd import _lib
    from internnav_amd.runtime import GraphedCall

    batch, lists, trajs = _seeded(32, 32)
    B = 8
    first, second = batch[:B].to(DEV), batch[B:2 * B].to(DEV)
    eager = [ops.traj_actions(x, B, 4) for x in (first, second)]
    h, entry, calls = _lib.lib(), _lib.lib().ina_traj_actions, []
    monkeypatch.setattr(h, "ina_traj_actions", lambda *a: (calls.append(1), entry(*a))[1])
    out = torch.empty((B, 33, 2), dtype=torch.float64, device=DEV)
    g = GraphedCall(lambda traj: ops.traj_actions(traj, B, 4, traj_out=out), {"traj": first.clone()}, warmup=2)
    assert len(calls) == 3                                               # two warm-up calls and the capture
    for x, (ea, ec), lo in ((second, eager[1], B), (first, eager[0], 0), (second, eager[1], B)):
        a, c = g(traj=x)
        torch.cuda.synchronize()
        assert torch.equal(a, ea) and torch.equal(c, ec)
        _check_table(a, c, lists[lo:lo + B], 4)
        assert torch.equal(_bits(out.cpu()), _bits(trajs[lo:lo + B]))
    assert len(calls) == 3


# ------------------------------------------------------------------------------------------------ agent level
class _Tok:
    """one token per character; decode() returns the scripted System-2 answers in turn"""

    def __init__(self, answers):
        self.answers, self.n = list(answers), 0

    def __call__(self, texts, return_tensors="pt"):
        return {"input_ids": torch.tensor([[ord(ch) % 3000 for ch in texts[0]]])}

    def decode(self, ids, skip_special_tokens=True):
        self.n += 1
        return self.answers[(self.n - 1) % len(self.answers)]


class _Proc:
    image_token = "<|image_pad|>"

    def __init__(self, answers):
        self.tokenizer = _Tok(answers)

    def apply_chat_template(self, conv, tokenize=False, add_generation_prompt=True):
        return "".join("<|vision_start|><|image_pad|><|vision_end|>" if c["type"] == "image" else c["text"] for m in conv for c in m["content"])

    def __call__(self, text, images, return_tensors="pt"):      # the host pre-processing path: one 2 x 2 patch image per frame
        return {"input_ids": self.tokenizer(text)["input_ids"], "pixel_values": torch.zeros(4 * len(images), 1176),
                "image_grid_thw": torch.tensor([[1, 2, 2]] * len(images))}


class _Model:
    """synthetic model on the GPU: System-2 is scripted (the processor decodes the script), System-1 returns the seeded [32 * n, 32, 3]
    trajectories of its k-th call on the device, as generate_traj does."""
    device = torch.device(DEV)

    def __init__(self):
        self.s1_calls = 0

    def generate(self, input_ids=None, **kw):
        return SimpleNamespace(sequences=torch.cat([input_ids, torch.zeros(input_ids.shape[0], 1, dtype=torch.long)], 1))

    def generate_latents(self, seqs, pv, grid, rows=None, **kw):
        return torch.zeros(seqs.shape[0] if rows is None else len(rows), 4, 8, device=DEV)

    def generate_traj(self, traj_latents=None, images_dp=None, depths_dp=None):
        n = traj_latents.shape[0]
        self.s1_calls += 1
        return R.seeded_batch(32, 32, seed=R.SEED + self.s1_calls)[:n].reshape(n * 32, 32, 3).to(DEV)


ANSWERS = ["12 34", "↑→", "56 78", "12 34", "←", "90 12"]


def _rollout(device_actions, device_pre, built_lib):
    from internnav_amd import dist as D
    from internnav_amd.agent import InternVLAN1Agent
    from internnav_amd.preprocess import FramePreprocessor

    pre = FramePreprocessor(DEV, resize_w=56, resize_h=56) if device_pre else None
    ms = {"infer_mode": "partial_async", "resize_w": 56, "resize_h": 56, "device_actions": device_actions}
    agent = InternVLAN1Agent({"model_settings": ms}, model=_Model(), processor=_Proc(ANSWERS), frame_preprocessor=pre)
    ran, run_s1 = [], agent._run_s1
    agent._run_s1 = lambda jobs: (ran.append([agent.envs.index(e) for e, _ in jobs]), run_s1(jobs))[1]
    agent.reset()
    rng = np.random.default_rng(5)
    trace = []
    for step in range(12):
        obs = [{"rgb": rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), "depth": rng.random((48, 64, 1), dtype=np.float32) * 0.6,
                "instruction": "walk past the sofa and stop at the door"} for _ in range(3)]
        ran.clear()
        out = agent.step(obs)
        trace.append(([o["action"] for o in out], [list(e.s1_output.idx or []) for e in agent.envs], list(ran)))
        if device_actions and ran:
            table = agent.last_action_table
            assert table.is_cuda and table.dtype == torch.int32 and table.shape == (len(ran[0]), 4)
            want = [agent.envs[i].s1_output.idx + [0] * (4 - len(agent.envs[i].s1_output.idx)) for i in ran[0]]
            assert table.tolist() == want
            gathered = D.all_gather_actions(table)                       # one rank: the table itself, still on the device, no round trip
            assert gathered.is_cuda and gathered.shape == (1, len(ran[0]), 4) and torch.equal(gathered[0], table)
        if step == 6:
            agent.reset([1])
    assert device_actions or agent.last_action_table is None
    return trace


@pytest.mark.parametrize("device_pre", [False, True], ids=["host-frames", "device-frames"])
def test_batched_agent_with_device_actions_equals_host_path(built_lib, device_pre):
    """both System-1 branches of the agent (host PIL frames / the device frame pre-processor): the same actions and the same per-env S1Output.idx
    at every step of a scripted rollout (pixel goals, discrete answers, an episode reset) with device_actions on and off."""
    pytest.importorskip("PIL.Image")
    off, on = _rollout(False, device_pre, built_lib), _rollout(True, device_pre, built_lib)
    assert off == on
    assert sum(len(r[2]) for r in on) >= 3 and any(len(j) > 1 for r in on for j in r[2])      # System-1 ran, also for several envs in one call
    assert any(len(idx) == 4 for r in on for idx in r[1])


def test_async_agent_continuous_trajectory_is_bit_equal(built_lib):
    pytest.importorskip("PIL.Image")
    from internnav_amd.async_agent import InternVLAN1AsyncAgent

    rgb, depth = np.zeros((48, 64, 3), np.uint8), np.zeros((48, 64), np.float32)
    outs = []
    for flag in (False, True):
        ag = InternVLAN1AsyncAgent(SimpleNamespace(device=DEV, model_path="unused", resize_w=56, resize_h=56, num_history=4, plan_step_gap=3,
                                                   device_actions=flag), model=_Model(), processor=_Proc(["12 34"]))
        assert ag.device_actions is flag
        outs.append([ag.step(rgb, depth, None, "walk to the door", None).output_trajectory for _ in range(3)])
    for host, dev in zip(*outs):
        assert isinstance(dev, np.ndarray) and dev.dtype == np.float64 and dev.shape == host.shape == (33, 2)
        assert dev.tobytes() == host.tobytes()
    assert outs[0][0].tobytes() != outs[0][1].tobytes()                  # the frames had different trajectories
