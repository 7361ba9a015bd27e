"""The hive's transition kernel source (roborugby_amd/csrc/rr_hive.hpp: hive_transition) on the CPU: compiled with g++ as lane loops
(tests/hive_transition_lib.py) at the product's lane widths and at 64.

The per-robot reward is this project's definition (the reference has none); it is pinned to the reference where the reference has an
answer: with one robot per team and positive ball 0 it IS the team's reward, bit for bit, on every recorded step of presets T and D.
Elsewhere (G, X: several robots, negative balls) it is held bit for bit to the numpy restatement of the definition, and the next
observation to the kernel source's own observer / the oracle's get_game_state(robot, ball) for the ball that was HELD over the step.

Bars: rewards exact in fp64; observations 1e-9 (the bar of tests/test_hive_emulated.py); fp32 arithmetic within
16 * 2^-24 * diag * mult_ball of the fp64 restatement -- each term is a difference of two distances <= diag rounded to fp32."""
import os

import numpy as np
import pytest

import hive_emu_lib as he
import hive_transition_lib as ht
import oracle_lib as ol

TOL_OBS = 1e-9


def _steps(golden_dir, preset):
    """every recorded step of traj_<preset>.npz as flat arrays: state before / after, the step's outputs"""
    t = np.load(os.path.join(golden_dir, f"traj_{preset}.npz"))
    idx = [(ep, s) for ep in range(len(t["length"])) for s in range(int(t["length"][ep]))]
    ep, s = np.array([i[0] for i in idx]), np.array([i[1] for i in idx])
    d = dict(robots0=t["state_robots"][ep, s], balls0=t["state_balls"][ep, s], robots1=t["state_robots"][ep, s + 1],
             balls1=t["state_balls"][ep, s + 1], robots_i1=t["state_robots_i"][ep, s + 1], inner1=t["state_inner"][ep, s + 1],
             step1=t["state_step"][ep, s + 1], status=(t["naughty"][ep, s].astype(np.int64) << 16).astype(np.int32),
             done=t["done"][ep, s].astype(np.uint8))
    for k in ("reward", "reward_g", "obs", "obs_g"):
        d[k] = t[k][ep, s]
    return d


_cache = {}


def _shared(golden_dir, preset):
    if preset not in _cache:
        _cache[preset] = _steps(golden_dir, preset)
    return _cache[preset]


@pytest.mark.parametrize("preset,vw", [(p, vw) for p in ("T", "D") for vw in he.LANES[p]])
def test_one_robot_per_team_and_ball_0_is_the_references_team_reward_bit_for_bit(golden_dir, preset, vw):
    d = _shared(golden_dir, preset)
    n = len(d["done"])
    assert n == {"T": 4564, "D": 3110}[preset]
    _, nr, _, _ = ht.counts(preset)
    assign = np.zeros((n, nr), np.int32)
    for kind in (0, 1):
        obs, rew, term, val = ht.hive_transition(preset, d["robots0"], d["balls0"], d["robots1"], d["balls1"], (1 << nr) - 1, kind, assign,
                                                 d["status"], d["done"], vw)
        assert np.all(val == 1) and np.array_equal(term, np.repeat(d["done"][:, None], nr, 1))
        assert np.array_equal(rew[:, 0], d["reward"]), (preset, vw, kind, np.abs(rew[:, 0] - d["reward"]).max())
        if nr > 1:
            assert np.array_equal(rew[:, 1], d["reward_g"]), (preset, vw, kind, np.abs(rew[:, 1] - d["reward_g"]).max())
        if kind == 0:  # the recorded observations are SingleBall_6wayLidar_v2's
            err = float(np.abs(obs[:, 0] - d["obs"]).max())
            assert err <= TOL_OBS, (preset, vw, err)
            if nr > 1:
                err = float(np.abs(obs[:, 1] - d["obs_g"]).max())
                assert err <= TOL_OBS, (preset, vw, err)
    if preset == "D":
        assert int((d["status"] != 0).sum()) == 228  # steps that carry NaughtyBots bits
    # the numpy restatement says the same
    want, _, valid = ht.restate(preset, d["robots0"][:, :, :2], d["balls0"][:, :, :2], d["robots1"][:, :, :2], d["balls1"][:, :, :2],
                                (1 << nr) - 1, assign, d["status"], d["done"])
    assert valid.all() and np.array_equal(want, rew)


def _masks(preset):
    nrh, nr, _, _ = ht.counts(preset)
    return ((1 << nrh) - 1, (1 << nr) - 1, 1 << (nr - 1))  # the happy team, every robot, one single (grumpy) robot


@pytest.mark.parametrize("preset,vw", [(p, vw) for p in ("G", "X") for vw in he.LANES[p]])
def test_full_game_rewards_equal_the_restatement_and_the_ball_is_held(golden_dir, preset, vw):
    d = _shared(golden_dir, preset)
    cfg = ol.PRESETS[preset]
    nrh, nr, nbp, nb = ht.counts(preset)
    n = len(d["done"])
    oracle = ol.OracleEnv(preset)
    seen = dict(negative=0, grumpy=0, naughty=0, held=0, reassigned=0)
    for mask in _masks(preset):
        assign, _ = he.greedy_assign_batch(d["robots0"][:, :, :2], d["balls0"][:, :, :2], mask, cfg["W"], cfg["H"])
        want, wterm, wvalid = ht.restate(preset, d["robots0"][:, :, :2], d["balls0"][:, :, :2], d["robots1"][:, :, :2], d["balls1"][:, :, :2],
                                         mask, assign, d["status"], d["done"])
        assert np.array_equal(wvalid, assign >= 0)  # (no ball leaves play in these trajectories, every status is a stepped one)
        for kind in (0, 1):
            obs, rew, term, val = ht.hive_transition(preset, d["robots0"], d["balls0"], d["robots1"], d["balls1"], mask, kind, assign,
                                                     d["status"], d["done"], vw)
            assert np.array_equal(val.astype(bool), wvalid) and np.array_equal(term, wterm)
            assert np.array_equal(rew, want), (preset, vw, mask, kind, np.abs(rew - want).max())
            assert np.all(obs[~wvalid] == 0) and np.all(np.isfinite(obs))
            # the same (robot, ball) on the state after the step: the kernel source's own observer where the greedy assignment there
            # happens to give the same ball, the oracle's get_game_state(robot, ball) for every other row
            assign1, obs1 = he.hive_observe(preset, d["robots1"], d["balls1"], mask, kind, vw)
            same = wvalid & (assign1 == assign)
            assert np.array_equal(obs[same], obs1[same]), (preset, vw, mask, kind)
            rest = np.argwhere(wvalid & ~same)
            for a, r in rest:
                oracle.set_state(d["robots1"][a], d["robots_i1"][a], d["balls1"][a], d["inner1"][a], int(d["step1"][a]))
                team, b = (1 if r < nrh else -1), int(assign[a, r])
                ref = oracle.observe_kind(1, team, int(r), b) if kind else oracle.observe(team, int(r), b)
                err = float(np.abs(obs[a, r] - ref[:11]).max())
                assert err <= TOL_OBS, (preset, vw, mask, kind, a, r, b, err)
            seen["held"] += int(same.sum())
            seen["reassigned"] += len(rest)
        seen["negative"] += int((wvalid & (assign >= nbp)).sum())
        seen["grumpy"] += int(wvalid[:, nrh:].sum())
        seen["naughty"] += int((wvalid & (((d["status"][:, None] >> (16 + np.arange(nr))[None, :]) & 1) != 0)).sum())
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("vw", he.LANES["G"])
def test_rows_that_are_no_transition_are_invalid_and_all_zero(golden_dir, vw):
    d = _shared(golden_dir, "G")
    cfg = ol.PRESETS["G"]
    s = slice(0, 400, 7)
    r0, b0, r1, b1, done = d["robots0"][s], d["balls0"][s], d["robots1"][s], d["balls1"][s], np.ones(len(d["done"][s]), np.uint8)
    n = len(done)
    status = np.full(n, 3 << 16, np.int32)  # (NaughtyBots bits of robots 0 and 1: an invalid row must not carry their penalty either)
    good, _ = he.greedy_assign_batch(r0[:, :, :2], b0[:, :, :2], 15, cfg["W"], cfg["H"])
    assert (good >= 0).all()

    def run(assign=good, mask=15, status=status, balls1=b1, kind=0):
        obs, rew, term, val = ht.hive_transition("G", r0, b0, r1, balls1, mask, kind, assign, status, done, vw)
        assert np.all(np.isfinite(obs)) and np.all(np.isfinite(rew)) and term.max() <= 1 and val.max() <= 1  # every element is written
        dead = val == 0
        assert np.all(obs[dead] == 0) and np.all(rew[dead] == 0) and np.all(term[dead] == 0)
        assert np.all(term[~dead] == 1) and np.all(np.abs(obs[~dead]).sum(axis=1) > 0)
        return val.astype(bool)

    for kind in (0, 1):
        assert run(kind=kind).all()
        for bad in (-1, 8, -7, 1 << 20):  # not a ball: never used as an index
            assert not run(assign=np.full_like(good, bad), kind=kind).any()
            mixed = good.copy()
            mixed[::2, 1] = bad
            v = run(assign=mixed, kind=kind)
            assert not v[::2, 1].any() and v[1::2].all() and v[:, [0, 2, 3]].all()
        for mask in (3, 4, 10):  # a robot outside the mask
            v = run(mask=mask, kind=kind)
            assert np.array_equal(v, np.repeat((((mask >> np.arange(4)) & 1) == 1)[None, :], n, 0))
        for bit in (ht.WAS_RESET, ht.NOT_READY, ht.STEP_AFTER_DONE):
            st = status.copy()
            st[1::3] |= bit
            v = run(status=st, kind=kind)
            assert not v[1::3].any() and v[0::3].all() and v[2::3].all()
        parked = b1.copy()  # a ball the goal bookkeeping consumed during this step (rr_extras.hpp: goal_step parks it at x <= -1000)
        for a in range(0, n, 2):
            b = int(good[a, 2])
            parked[a, b, 0], parked[a, b, 1] = -1000.0 - 40.0 * b, -1000.0
        v = run(balls1=parked, kind=kind)
        assert not v[::2, 2].any() and v[1::2].all() and v[:, [0, 1, 3]].all()


@pytest.mark.parametrize("vw", [8, 64])
def test_fp32_arithmetic_stays_within_the_derived_bound(golden_dir, vw):
    d = _shared(golden_dir, "G")
    cfg = ol.PRESETS["G"]
    bound = ht.fp32_bound(cfg["W"], cfg["H"])
    assert abs(bound - 16 * 2.0 ** -24 * 200000.0) < 1e-12
    assign, _ = he.greedy_assign_batch(d["robots0"][:, :, :2], d["balls0"][:, :, :2], 15, cfg["W"], cfg["H"])
    want, wterm, wvalid = ht.restate("G", d["robots0"][:, :, :2], d["balls0"][:, :, :2], d["robots1"][:, :, :2], d["balls1"][:, :, :2], 15,
                                     assign, d["status"], d["done"])
    for kind in (0, 1):
        _, rew, term, val = ht.hive_transition("G", d["robots0"], d["balls0"], d["robots1"], d["balls1"], 15, kind, assign, d["status"],
                                               d["done"], vw, f32=True)
        assert np.array_equal(val.astype(bool), wvalid) and np.array_equal(term, wterm)
        err = float(np.abs(rew - want).max())
        print(f"fp32 emulation, {vw} lanes, kind {kind}: worst |reward - fp64 restatement| {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (vw, kind, err, bound)
        assert np.array_equal(rew.astype(np.float32).astype(np.float64), rew)  # fp32 values
