"""The shapes at the limits of the one-shape library (oracle_lib.PRESETS: W, R, Q, P) on the host emulation: what the parametrisations
they joined elsewhere do not look at.

  * the second team's outputs.  `_compare` of test_differential_adversarial.py reads `obs` and `reward` only; W and Q are the only
    shapes besides G that take the one-pass two-team observation (observe_both: the grumpy lidar candidates alias per-sub-step ball
    scratch), Q with no slack in its aliasing bound, and R's reward scratch holds 8 robots' terms.  Every step of 40-step episodes,
    state set from the oracle before each step: both observations within 1e-9, both rewards within 1e-6 (`_compare`'s tolerances).
  * the parity build.  W, R and Q run free for 40 steps on the exact-trig emulation next to the oracle: bit for bit where the
    reference's libm is correctly rounded (the claim of test_parity_build.py), and against the oracle's plain libm bit for bit on
    the episodes counted below, within 1e-9 on the others."""
import numpy as np
import pytest

import emu_lib as el
import oracle_lib as ol

STEPS, EPISODES = 40, 6
FATAL = 63


def _start(preset, episode, seed=77):
    """an oracle arena fresh from reset with the balls set rolling (up to 9 px a frame: contacts within the first steps)"""
    o = ol.OracleEnv(preset)
    o.reset(seed, episode, 0)
    o.reset(seed, episode, 1)
    st = o.get_state()
    rng = np.random.RandomState(1000 * seed + episode)
    st["balls"][:, 6:] = rng.uniform(-9, 9, (o.nb, 2))
    o.set_state(st["robots"], st["robots_i"], st["balls"], None, st["step"])
    return o, rng


def _actions(rng, nr, s):
    """mostly forward (robots meet each other, the balls and the walls), every fifth step anything"""
    return np.where(rng.rand(nr) < (0.5 if s % 5 == 0 else 0.85), 0, rng.randint(0, 8, nr)).astype(np.int32)


def _close(a, b, tol):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.array_equal(np.isnan(a), np.isnan(b)) and float(np.nan_to_num(np.abs(a - b)).max()) < tol


@pytest.mark.parametrize("preset,narrow", [(p, nw) for p in "WQR" for nw in (False, True)])
def test_both_teams_observations_and_rewards_every_step(preset, narrow):
    env = el.EmuEnv(preset, narrow=narrow)
    steps = contacts = 0
    for ep in range(EPISODES):
        o, rng = _start(preset, ep)
        for s in range(STEPS):
            st = o.get_state()
            env.set_state(st["robots"], st["robots_i"], st["balls"], st["step"])
            a = _actions(rng, o.nr, s)
            want, got = o.step(a), env.step(a)
            ctx = (preset, narrow, ep, s)
            assert (got["status"] & ~256) == (want["status"] & ~256), ctx
            if want["status"] & FATAL:
                break  # the reference raised: only the flag is defined
            post, mine = o.get_state(), env.get_state()
            assert np.array_equal(mine["robots_i"], post["robots_i"]) and _close(mine["robots"], post["robots"], 1e-9), ctx
            assert _close(mine["balls"], post["balls"], 1e-9), ctx
            assert _close(got["obs"], want["obs"], 1e-9), (ctx, got["obs"] - want["obs"])
            assert _close(got["obs_g"], want["obs_g"], 1e-9), (ctx, got["obs_g"] - want["obs_g"])
            assert abs(got["reward"] - want["reward"]) < 1e-6 and abs(got["reward_g"] - want["reward_g"]) < 1e-6, ctx
            assert got["naughty"] == want["naughty"] and got["done"] == want["done"], ctx
            contacts += int(np.abs(post["balls"][:, 6:] - st["balls"][:, 6:] * 0.995 ** 12).max() > 1e-6)
            steps += 1
    assert steps > 0.8 * EPISODES * STEPS and contacts > 0.1 * steps, (steps, contacts)
    print(f"[{preset} narrow={narrow}] {steps} steps, {contacts} with a contact response: both teams' observations and rewards match the oracle")


def _free_run(preset, ep, correctly_rounded):
    """(steps run, first step after which the states differ in a bit or None, largest difference seen)"""
    ol.lib().rro_debug_attribution(4 if correctly_rounded else 0)
    try:
        o, rng = _start(preset, ep)
        st = o.get_state()
        e = el.EmuEnv(preset, exact=True)
        e.set_state(st["robots"], st["robots_i"], st["balls"], st["step"])
        assert e.set_scratch_rect(st["inner"])
        first, worst = None, 0.0
        for s in range(STEPS):
            a = _actions(rng, o.nr, s)
            want, got = o.step(a), e.step(a)
            if want["status"] & FATAL:
                return s, first, worst
            post, mine = o.get_state(), e.get_state()
            assert np.array_equal(mine["robots_i"], post["robots_i"]) and np.array_equal(np.isnan(mine["robots"]), np.isnan(post["robots"])), (preset, ep, s)
            d = max(float(np.nanmax(np.abs(mine["robots"] - post["robots"]))), float(np.abs(mine["balls"] - post["balls"]).max()))
            worst = max(worst, d)
            if d > 0 and first is None:
                first = s
        return STEPS, first, worst
    finally:
        ol.lib().rro_debug_attribution(0)


# bit-exact episodes of EPISODES against the oracle's plain libm (glibc), measured with the oracle and the emulation of this repository
# (R: episode 3 leaves the oracle at step 30 by 1.1e-13 -- a sin / cos that glibc does not round correctly; with a correctly rounded
# libm on the oracle's side it stays bit for bit like the others)
BIT_EXACT = {"W": 6, "R": 5, "Q": 6}


@pytest.mark.parametrize("preset", ["W", "R", "Q"])
def test_parity_build_runs_free_next_to_the_oracle(preset):
    runs = [_free_run(preset, ep, True) for ep in range(EPISODES)]
    assert all(first is None for _, first, _ in runs), (preset, runs)  # a correctly rounded libm on both sides: every episode, every bit
    runs = [_free_run(preset, ep, False) for ep in range(EPISODES)]
    exact = sum(first is None for _, first, _ in runs)
    print(f"[{preset}] parity build, {EPISODES} free-running episodes of {STEPS} steps against the oracle: {exact} bit for bit; {runs}")
    assert sum(n for n, _, _ in runs) > 0.8 * EPISODES * STEPS
    assert exact == BIT_EXACT[preset] and all(worst < 1e-9 for _, _, worst in runs), (preset, runs)
