"""GPU tests of the NavDPNet rollout session (internnav_amd.navdp_rollout): the ina_memory_gather kernel against a torch index expression,
session steps against NavDPNet.predict_mixedgoal_batch_action_vel on the materialised windows (bit-equal), the session's top-8 / bottom-8
selection against the fp32 oracle, a captured step against the eager session, and isolation of envs."""
import pytest
import torch

from internnav_amd import synthetic as S
from tests.navdp_rollout_ref import CFG, MODES, RANK_B, SCRIPT_B5, M, Rollout, cut_gaps, rank_steps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def net(built_lib):
    from internnav_amd.navdp import NavDPNet

    return NavDPNet(_weights(), CFG, DEV, max_envs=64)


def _weights():
    return S.navdpnet_train_state_dict(seed=21, pixel_channel=4)


def _dev(d):
    return {k: (v.to(DEV) if torch.is_tensor(v) and k != "goal_kind" else v) for k, v in d.items()}


def _full(net, st):
    neg, pos = net.predict_mixedgoal_batch_action_vel(st["goal_kind"], st["goal_point"], st["goal_image"], st["goal_pixel"],
                                                      input_images=st["images"], input_depths=st["depth"], x_init=st["x_init"],
                                                      step_noise=st["step_noise"])
    return neg.clone(), pos.clone()


def _session_args(st):
    return dict(goal_kind=st["goal_kind"], goal_point=st["goal_point"], goal_image=st["goal_image"], goal_pixel=st["goal_pixel"], rgb=st["rgb"],
                depth=st["depth"], x_init=st["x_init"], step_noise=st["step_noise"])


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize("stride", [1, 2])
def test_memory_gather_kernel(built_lib, stride):
    """random rings; heads that wrap; counts 1, 2, M - 1, M, ring depth (count includes the push of the launch, so 1 is an env straight
    after its reset - "no earlier push"); a subset launch over permuted env ids. A copy, one add and one rounding: bit-equal. A count of 0
    (no push at all: not a state the plan produces) poisons its rows and leaves the ring alone."""
    from internnav_amd import ops

    ntok, C, E = 256, 384, 7
    depth = (M - 1) * stride + 1
    g = torch.Generator().manual_seed(5 + stride)
    ring = torch.randn(E, depth, ntok, C, generator=g).to(DEV)
    blank = torch.randn(ntok, C, generator=g).to(DEV)
    pe = torch.randn(M * ntok, C, generator=g).to(DEV)
    cases = [
        ([0, 1, 2, 3, 4, 5, 6], [0, 1, depth - 1, 3 % depth, depth // 2, 2, 0], [1, 2, M - 1, M, depth, depth, 1]),     # every env
        ([5, 2, 6], [1, 0, depth - 2], [depth, 3, 1]),                                                                   # a permuted subset
        ([3], [0], [depth]),                                                                                             # one env, wrapped
    ]
    for env, head, count in cases:
        n = len(env)
        fresh = torch.randn(n, ntok, C, generator=g).to(DEV)
        out = torch.full((n, (M + 1) * ntok, C), 7.0, dtype=torch.bfloat16, device=DEV)
        e, h, c = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in (env, head, count))
        want_ring = ring.clone()
        want_ring[e.long(), h.long()] = fresh
        back = ((M - 1 - torch.arange(M, device=DEV)) * stride)
        slot = (h.long()[:, None] - back[None, :]) % depth
        src = want_ring[e.long()[:, None], slot]                                       # [n, M, ntok, C]
        src = torch.where((back[None, :] < c.long()[:, None])[:, :, None, None], src, blank)
        want = (src + pe.view(M, ntok, C)).to(torch.bfloat16).view(n, M * ntok, C)
        ops.memory_gather(out, ring, fresh, blank, pe, e, h, c, stride=stride)
        torch.cuda.synchronize()
        assert torch.equal(out[:, : M * ntok], want), (stride, env)
        assert bool((out[:, M * ntok:] == 7.0).all()), "rows past the memory slots were written"
        assert torch.equal(ring, want_ring), "ring: only slot head of every launched env may change"
    # bad table entries: NaN rows, no access outside the ring, ring untouched
    before = ring.clone()
    fresh = torch.randn(3, ntok, C, generator=g).to(DEV)
    out = torch.zeros(3, M * ntok, C, dtype=torch.bfloat16, device=DEV)
    e, h, c = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in ([E, 1, 2], [0, depth, 0], [1, 1, 0]))
    ops.memory_gather(out, ring, fresh, blank, pe, e, h, c, stride=stride)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all()) and torch.equal(ring, before)


# ---------------------------------------------------------------------------------------------- 2. the session against the existing call
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("mode", ["point", "none", "image", "pixel", "mixed"])
def test_session_equals_full_call_b5(net, mode, stride):
    """12 scripted steps of 5 envs (staggered resets, env 2 / env 4 sitting out some steps): every step's (negative, positive) equal the
    full call on the same windows - zero frames in front, the same noise - bit for bit."""
    from internnav_amd.navdp_rollout import NavDPRollout

    ses = NavDPRollout(net, 5, stride=stride)
    for st in Rollout(5, SCRIPT_B5, MODES[mode], stride, seed=31).steps():
        if st["reset"]:
            ses.reset(st["reset"])
        d = _dev(st)
        want = _full(net, d)
        neg, pos = ses.step(**_session_args(d), env_ids=d["ids"])
        torch.cuda.synchronize()
        assert neg.shape == want[0].shape == (len(d["ids"]), 8, CFG["predict_size"], 3)
        assert torch.isfinite(neg).all() and torch.isfinite(pos).all()
        assert torch.equal(neg, want[0]) and torch.equal(pos, want[1]), f"{mode} stride {stride} step {st['t']}: session differs from the full call"


def test_session_equals_full_call_b64(net):
    """64 envs, the four goal kinds interleaved, three steps (env 9 reset before the third)."""
    from internnav_amd.navdp_rollout import NavDPRollout

    script = [dict(reset=[], skip=[]), dict(reset=[], skip=[]), dict(reset=[9], skip=[])]
    ses = NavDPRollout(net, 64)
    for st in Rollout(64, script, [(b * 7 + b // 5) % 4 for b in range(64)], 1, seed=32).steps():
        if st["reset"]:
            ses.reset(st["reset"])
        d = _dev(st)
        want = _full(net, d)
        neg, pos = ses.step(**_session_args(d))
        torch.cuda.synchronize()
        assert torch.equal(neg, want[0]) and torch.equal(pos, want[1]), f"B = 64 step {st['t']}: session differs from the full call"


def test_session_ranking_vs_fp32_oracle(net):
    """the ranking rollout (3 envs x 4 steps, point goals, env 1 reset before step 2; noise draws selected with the oracle alone, see
    tests/navdp_rollout_ref.py): wherever the fp32 oracle's gap at a cut (8th / 9th lowest, 8th / 9th highest critic value) exceeds the
    measured critic error - the largest |session critic - oracle critic| of the rollout - the session selects the oracle's set at that cut.
    An (env, step) pair with a cut that is not compared counts as left out: at most 10 % of the pairs. The returned trajectories are those
    of the session's own critic order."""
    from internnav_amd.navdp_rollout import NavDPRollout
    from oracle import navdp as o_navdp

    sd, Sn, T = _weights(), CFG["sample_num"], CFG["predict_size"]
    ses = NavDPRollout(net, RANK_B)
    rec = []
    for st in rank_steps():
        if st["reset"]:
            ses.reset(st["reset"])
        with torch.no_grad():
            _, _, _, ref, _ = o_navdp.navdpnet_pointgoal(sd, st["goal_point"], st["images"], st["depth"], st["x_init"], st["step_noise"], CFG,
                                                         return_all=True)
        neg, pos = ses.step(**_session_args(_dev(st)))
        torch.cuda.synchronize()
        mine = net.critic[: RANK_B * Sn].view(RANK_B, Sn).float().cpu().clone()
        traj = torch.cumsum(net.sample[: RANK_B * Sn * T].view(RANK_B, Sn, T, 3).float().cpu() / 4.0, dim=2)
        for b in range(RANK_B):
            assert torch.allclose(neg[b].cpu(), traj[b][mine[b].argsort()[:8]], atol=1e-5)
            assert torch.allclose(pos[b].cpu(), traj[b][(-mine[b]).argsort()[:8]], atol=1e-5)
        rec.append((st["t"], ref, mine))
    err = max((mine - ref).abs().max().item() for _, ref, mine in rec)
    mean = sum((mine - ref).abs().mean().item() for _, ref, mine in rec) / len(rec)
    print(f"critic error of the session against the fp32 oracle over {len(rec) * RANK_B} (env, step) pairs: max {err:.3e} mean {mean:.3e}")
    left_out = 0
    for t, ref, mine in rec:
        for b in range(RANK_B):
            lo, hi = cut_gaps(ref[b])
            print(f"step {t} env {b}: oracle gaps {lo:.3e} (bottom cut) {hi:.3e} (top cut)")
            left_out += int(min(lo, hi) <= err)
            if lo > err:
                assert set(mine[b].argsort()[:8].tolist()) == set(ref[b].argsort()[:8].tolist()), f"step {t} env {b}: bottom-8 set differs"
            if hi > err:
                assert set((-mine[b]).argsort()[:8].tolist()) == set((-ref[b]).argsort()[:8].tolist()), f"step {t} env {b}: top-8 set differs"
    print(f"left out: {left_out} of {len(rec) * RANK_B} pairs")
    assert left_out <= 0.10 * len(rec) * RANK_B, f"{left_out} of {len(rec) * RANK_B} (env, step) pairs have an oracle gap below the critic error {err:.3e}"


# -------------------------------------------------------------------------------------------------------------------------- 3. capture
def test_captured_step_equals_eager(net):
    """two sessions on the same frames: one eager, one that captures step 2 and replays it for steps 3 - 6 with refreshed tables (other env
    ids, a reset in between)."""
    from internnav_amd.navdp_rollout import NavDPRollout

    script = [dict(reset=[], skip=[3]), dict(reset=[], skip=[3]), dict(reset=[], skip=[3]), dict(reset=[], skip=[2]), dict(reset=[1], skip=[3]),
              dict(reset=[], skip=[0]), dict(reset=[], skip=[2])]
    kinds = [1, 1, 1, 1]          # one goal layout for every subset of three envs: what a captured step replays
    eager, graphed = NavDPRollout(net, 4), NavDPRollout(net, 4)
    step = None
    for st in Rollout(4, script, kinds, 1, seed=33).steps():
        for s in (eager, graphed):
            if st["reset"]:
                s.reset(st["reset"])
        d = _dev(st)
        a = _session_args(d)
        want = tuple(x.clone() for x in eager.step(**a, env_ids=d["ids"]))
        if st["t"] < 2:
            got = graphed.step(**a, env_ids=d["ids"])
        elif st["t"] == 2:
            step = graphed.capture(**a, env_ids=d["ids"])
            got = step.outputs
        else:
            a.pop("goal_kind")
            got = step(**a, env_ids=d["ids"])
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"step {st['t']}: captured session differs from the eager one"
    assert torch.equal(eager.ring, graphed.ring)


# ------------------------------------------------------------------------------------------------------------------------ 4. isolation
def test_reset_and_subset_steps_leave_other_envs_alone(net):
    from internnav_amd.navdp_rollout import NavDPRollout

    script = [dict(reset=[], skip=[]) for _ in range(5)]
    a, b = NavDPRollout(net, 4), NavDPRollout(net, 4)
    for st in Rollout(4, script, [1, 0, 1, 1], 1, seed=34).steps():
        d = _dev(st)
        if st["t"] == 2:
            b.reset([1])                         # only session b resets env 1
        out_a = tuple(x.clone() for x in a.step(**_session_args(d)))
        out_b = tuple(x.clone() for x in b.step(**_session_args(d)))
        torch.cuda.synchronize()
        others = [0, 2, 3]
        for x, y in zip(out_a, out_b):
            assert torch.equal(x[others], y[others]), f"step {st['t']}: the reset of env 1 changed another env's output"
            assert torch.equal(x[1], y[1]) == (st["t"] < 2), f"step {st['t']}: env 1 after its reset"
    # a stepped subset leaves the other envs' rings (and host state) untouched
    ring, head, count = a.ring.clone(), a.plan.head.copy(), a.plan.count.copy()
    st = next(iter(Rollout(2, [dict(reset=[], skip=[])], [1, 1], 1, seed=35).steps()))
    d = _dev(st)
    a.step(**_session_args(d), env_ids=[3, 1])
    torch.cuda.synchronize()
    assert torch.equal(a.ring[[0, 2]], ring[[0, 2]]) and not torch.equal(a.ring[[1, 3]], ring[[1, 3]])
    assert (a.plan.head[[0, 2]] == head[[0, 2]]).all() and (a.plan.count[[0, 2]] == count[[0, 2]]).all()
