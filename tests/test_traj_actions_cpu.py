"""Host side of the device action table (ina_traj_actions), no GPU: the instrumented restatement of tests/traj_actions_ref.py against
policy.traj_to_actions on the reference-executed cases and on every seeded input of the GPU test, the decision margins that let the GPU test
demand equality on all of them, the C-ABI entry through ctypes with its refusals, and the unchanged defaults of the Python surface."""
import ctypes as C
import functools
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import traj_actions_ref as R
from internnav_amd.policy import traj_to_actions

GOLD = Path(__file__).resolve().parent / "golden"


@functools.lru_cache(maxsize=None)
def _golden():
    return torch.load(GOLD / "vln_utils.pt", weights_only=True)["cases"]


def _check(t: torch.Tensor):
    """helper == host function on t [S, T, 3] (list and continuous trajectory, bit for bit); returns (list, margin)."""
    acts, traj, margin = R.traj_actions_ref(t)
    assert acts == traj_to_actions(t.clone())
    host = traj_to_actions(t.clone(), use_discrate_action=False)
    assert host.dtype == np.float64 and host.shape == traj.shape and host.tobytes() == traj.tobytes()      # the sequential fp64 mean IS np.mean
    return acts, margin


def test_restatement_equals_host_function_on_reference_cases():
    lo = math.inf
    for c in _golden():
        keep = c["traj"].clone()
        acts, margin = _check(c["traj"])
        assert torch.equal(c["traj"], keep)                     # the helper leaves its input alone
        assert acts == c["actions"]
        assert margin > R.MARGIN_BOUND, margin
        lo = min(lo, margin)
    print(f"minimum decision margin over the 12 reference-executed cases: {lo:.3e}")


@pytest.mark.parametrize("S,T", R.SHAPES)
def test_restatement_and_margins_on_the_seeded_inputs(S, T):
    """every seeded env of the GPU test, f32 and rounded to bf16: the helper equals the host function and no decision is closer than 1e-9 to
    falling the other way - the condition under which a few ulp of atan2 / cos / sin cannot change the list."""
    batch = R.seeded_batch(S, T)
    lo, longest, kinds = math.inf, 0, {}
    for b in range(R.N_ENVS):
        for t in (batch[b], batch[b].to(torch.bfloat16)):
            acts, margin = _check(t)
            assert margin > R.MARGIN_BOUND, (S, T, b, str(t.dtype), margin)
            lo, longest = min(lo, margin), max(longest, len(acts))
        kinds.setdefault(R.KINDS[b % 6], []).append(R.traj_actions_ref(batch[b])[0])
    print(f"(S, T) = ({S}, {T}): minimum decision margin {lo:.3e}, longest list {longest}")
    # the six kinds reach the branches they are drawn for
    assert all(a == [] for a in kinds["tiny"]) and all(a == [] for a in kinds["static"])           # goal inside the stop radius: count 0
    assert all(len(a) > 4 for a in kinds["strong"])                                                 # longer than the policy's table
    assert all(len(a) >= 6 and len(set(a[:6])) == 1 and a[0] in (2, 3) for a in kinds["behind"])    # six or more turns at once
    assert any(2 in a and 3 in a for a in kinds["curved"]) or T < 3
    assert all(0 < len(a) for a in kinds["slow"])


def test_edge_inputs_of_the_gpu_test():
    # all zero: the goal is the start
    acts, margin = _check(torch.zeros(5, 7, 3))
    assert acts == [] and margin == 0.2
    # exact ties of the nearest-point search: the case tells "lowest index wins" from "highest index wins", and no OTHER decision is close
    t = R.tie_case()
    log = []
    acts, margin = _check(t)
    assert R.traj_actions_ref(t, log=log)[0] == acts and margin > R.MARGIN_BOUND
    assert R.traj_actions_ref(t, tie_last=True)[0] != acts
    pts = R.mean_trajectory(t)
    assert (pts[3:7] == pts[3]).all() and acts[:3] == [1, 1, 1]            # four coincident points, reached exactly by three forward steps
    # the straight line along -x: only the first wrap decision has no margin (delta_yaw = -pi or +pi), every other decision is clear
    t = R.minus_x_case()
    log = []
    acts, _, margin = R.traj_actions_ref(t, log=log)
    assert acts == traj_to_actions(t.clone()) and margin == 0.0
    assert [(n, k) for n, k, m in log if m <= R.MARGIN_BOUND] == [(0, "wrap")]
    assert acts[:12] == [3] * 12 and set(acts[12:]) == {1}


def test_traj_actions_entry_visible_through_ctypes(built_lib):
    from internnav_amd import _lib

    h = C.CDLL(str(built_lib))
    assert hasattr(h, "ina_traj_actions")
    res, args = _lib.SYMBOLS["ina_traj_actions"]
    p, i32 = C.c_void_p, C.c_int32
    assert res is C.c_int and args == [p, i32, i32, i32, i32, p, i32, p, p, i32, p]
    assert _lib.ABI_VERSION == 8 and h.ina_abi_version() == 8                       # plain arguments: no struct, no ABI bump
    # host-side validation runs without a GPU
    fn, err = _lib.lib().ina_traj_actions, _lib.lib().ina_last_error
    F32, BF16 = 1, 0
    ok = dict(traj=16, dt=F32, B=2, S=32, T=32, actions=16, ma=4, count=16)

    def call(**kw):
        a = dict(ok, **kw)
        return fn(a["traj"], a["dt"], a["B"], a["S"], a["T"], a["actions"], a["ma"], a["count"], None, 0, None)

    for bad, word in ((dict(traj=None), b"null"), (dict(actions=None), b"null"), (dict(count=None), b"null"), (dict(T=0), b"T=0"), (dict(S=0), b"S=0"),
                      (dict(T=1024), b"1025 points"), (dict(ma=0), b"max_actions=0"), (dict(ma=257), b"max_actions=257"), (dict(dt=2), b"dtype"),
                      (dict(dt=-1), b"dtype"), (dict(B=0), b"B=0")):
        assert call(**bad) != 0, bad
        assert b"traj_actions" in err() and word in err(), (bad, err())
    assert BF16 == 0


def test_device_actions_is_opt_in_and_defaults_are_unchanged():
    import inspect

    from internnav_amd import ops
    from internnav_amd.agent import InternVLAN1Agent
    from internnav_amd.async_agent import InternVLAN1AsyncAgent
    from internnav_amd.policy import InternVLAN1Net, S1Output

    class _Model:
        device = torch.device("cpu")

    ag = InternVLAN1Agent({"model_settings": {"infer_mode": "partial_async"}}, policy_factory=lambda: None)
    assert ag.device_actions is False and ag.last_action_table is None
    assert InternVLAN1Agent({"model_settings": {"device_actions": True}}, policy_factory=lambda: None).device_actions is True
    assert InternVLAN1AsyncAgent({"device": "cpu"}, model=_Model(), processor=object()).device_actions is False
    assert InternVLAN1AsyncAgent({"device": "cpu", "device_actions": True}, model=_Model(), processor=object()).device_actions is True
    sig = inspect.signature(ops.traj_actions)
    assert list(sig.parameters) == ["traj", "n_env", "max_actions", "traj_out", "scale_in_place"]
    assert [sig.parameters[k].default for k in ("max_actions", "traj_out", "scale_in_place")] == [4, None, False]
    # actions_from_traj: the host path, unchanged on the reference-executed cases (list cut to four, input un-normalised in place)
    net = InternVLAN1Net(_Model(), object())
    for c in _golden():
        t = c["traj"].clone()
        assert net.actions_from_traj(t) == S1Output(idx=c["actions"][:4])
        assert torch.equal(t, c["mutated"])
    # the batch method is for continuous_traj only; the chunk_token branch stays on the host
    with pytest.raises(NotImplementedError):
        InternVLAN1Net(_Model(), object(), continuous_traj=False).actions_from_traj_batch(torch.zeros(32, 32, 3), 1)
