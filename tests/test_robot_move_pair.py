"""The robot move, its tail spread over the robot's lane pair by component (csrc/rr_sim.hpp: robot_move_comp_begin), against a fixture
recorded with that tail on ONE lane (robot_move_finish under `part == 0`): tests/golden/robot_move_pin.npz, written by
tools/gen_robot_move_pin.py on the commit before the split.  Every arena of the fixture, every array, bit for bit: at the full wave and
at the narrow width, in the default and in the parity build.  (What the arenas are made of: the tool's docstring; each arm broken once
and the test's verdict: profiles/pair_move/README.md.)
What the fixture does NOT hold: A.wm, the "blocked | clamped" byte the move leaves for the island freeze, is not part of the canonical state,
and every status word and NaughtyBots set in these contact-free arenas is 0.  The move's effect on the rect is pinned here; the byte
itself (`wmv |= 2` for a clamp) only through the suites that compare the shortcuts on and off (test_fixed_point_memo, test_gpu_shortcuts)."""
import os

import numpy as np
import pytest

import emu_lib
import oracle_lib as ol

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robot_move_pin.npz")
PRESETS = ("T", "D", "G", "Dwide")
GROUPS = ("act1", "act3", "thr1")
ARRAYS = ("robots", "robots_i", "balls", "status", "naughty")


@pytest.fixture(scope="module")
def pin():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def bits(a):
    """the array's bytes as integers: NaN == NaN, -0.0 != +0.0"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def run_group(pin, preset, group, exact, narrow):
    key = f"{preset}_{group}_"
    robots, robots_i, balls = pin[key + "robots"], pin[key + "robots_i"], pin[key + "balls"]
    thrust = pin.get(key + "thrust")
    acts = thrust if thrust is not None else pin[key + "actions"]
    steps, n = acts.shape[:2]
    env = emu_lib.EmuEnv(preset, exact=exact, narrow=narrow)
    got = {k: np.zeros_like(pin[f"{key}{'exact' if exact else 'default'}_{k}"]) for k in ARRAYS}
    for a in range(n):
        env.set_state(robots[a], robots_i[a], balls[a], 0)
        for s in range(steps):
            r = env.step_thrust(acts[s, a]) if thrust is not None else env.step(acts[s, a])
            st = env.get_state()
            got["robots"][s, a], got["robots_i"][s, a], got["balls"][s, a] = st["robots"], st["robots_i"], st["balls"]
            got["status"][s, a], got["naughty"][s, a] = r["status"], r["naughty"]
    return got


def test_fixture_covers_the_arms(pin):
    """about 200 arenas per preset, all nine thrust patterns, and robots the step leaves where they were (blocked) next to ones it moves"""
    for preset in PRESETS:
        n = sum(pin[f"{preset}_{g}_robots"].shape[0] for g in GROUPS)
        assert n == 200
        t = pin[f"{preset}_thr1_thrust"]
        pairs = {tuple(p) for p in t.reshape(-1, 2).astype(int).tolist()}
        assert (0, 0) in pairs and len(pairs) == 9, pairs
        assert set(np.unique(pin[f"{preset}_act1_actions"]).tolist()) == set(range(8))
        rot = pin[f"{preset}_act1_robots"][..., 6]
        assert np.any((rot + 720.0) % 360.0 != rot)  # a rotation the restore has to renormalise
        cfg = ol.PRESETS[preset]
        r0 = np.concatenate([pin[f"{preset}_{g}_robots"].reshape(-1, 10) for g in GROUPS])
        # robots across each of the four walls (the clamp's four tests), and on the `<=` walls exactly
        assert np.any(r0[:, 2] < 0) and np.any(r0[:, 3] > cfg["W"]) and np.any(r0[:, 4] <= 0) and np.any(r0[:, 5] >= cfg["H"])
        assert np.any(r0[:, 4] == 0) and np.any(r0[:, 5] == cfg["H"])


@pytest.mark.parametrize("narrow", [False, True], ids=["wave64", "narrow"])
@pytest.mark.parametrize("exact", [False, True], ids=["default", "parity"])
@pytest.mark.parametrize("preset", PRESETS)
def test_move_reproduces_the_single_lane_fixture(pin, preset, exact, narrow):
    build = "exact" if exact else "default"
    for group in GROUPS:
        got = run_group(pin, preset, group, exact, narrow)
        for k in ARRAYS:
            want = pin[f"{preset}_{group}_{build}_{k}"]
            same = bits(got[k]) == bits(want)
            bad = np.argwhere(~same)
            assert same.all(), (f"{preset} {group} {build} narrow={narrow}: {k} differs in {len(bad)} words, first at [step, arena, ...] = "
                                f"{bad[0].tolist()}: {got[k][tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")
