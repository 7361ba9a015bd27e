"""Non-square arenas on the CPU: the oracle and the host-emulated wave at W != H.

Every other preset has W == H, so any of the places that tell width from height -- wall tests and clamps, the ball / wall bounce, the
lidar's walls, the observers' goal corner, the reset ranges, the goal triangles, the reward multiplier -- could have the two swapped
without a test noticing.  Here they are pinned to the reference at 1000 x 640 (`Dwide`: D's counts) and 480 x 720 (`Ttall`: T's), from
vectors the unmodified reference produced with its two arena constants patched at load time (oracle/refgen/load_reference.py), and at
`Gwide` (G's counts, 1000 x 640) to the oracle and the numpy restatement of the hive rule.

The reference itself mixes the two up in one place: a ball beyond the bottom wall is reflected with
`ARENA_HEIGHT - (bottom - ARENA_WIDTH) * 1.1` (RR_TrashyPhysics.py:336).  Kernel and oracle copy that on purpose; the fixtures hold
steps that take that line (counted by the generator, `walls`), so "tidying" it fails here.

The oracle's free-running bit-exact replay of the same fixtures, the reset, and the mixins are further cases of the parametrised tests
in test_oracle_traj.py, test_emulated_wave.py, test_reset_distribution.py, test_oracle_mixins.py and test_mixins_kernel.py."""
import json
import os
import sys

import numpy as np
import pytest

import emu_lib as el
import hive_emu_lib as he
import oracle_lib as ol
from nonsquare_lib import (GOAL_BALLS, GOAL_ROBOTS, GOAL_WANT, H, NEAR_OUT, SWAP_IN, SWAP_OUT, W, clamped_edge, robots_across_the_walls,
                           swap_sensitive_layouts)

TOL = 1e-9  # tests/test_emulated_wave.py's bar


def test_the_ids_have_the_generators_sizes_and_their_shapes_other_constants():
    sys.path.insert(0, os.path.join(ol.REPO, "oracle", "refgen"))
    from load_reference import ARENA, BASE  # (reads no reference code)
    for name in ("Dwide", "Ttall"):
        cfg, shape = ol.PRESETS[name], ol.PRESETS[ol.SHAPE[name]]
        assert (cfg["W"], cfg["H"]) == tuple(float(v) for v in ARENA[name]) and BASE[name] == ol.SHAPE[name]
        assert {k: v for k, v in cfg.items() if k not in "WH"} == {k: v for k, v in shape.items() if k not in "WH"}
    assert {k: v for k, v in ol.PRESETS["Gwide"].items() if k not in "WH"} == {k: v for k, v in ol.PRESETS["G"].items() if k not in "WH"}
    assert ol.PRESETS["Dwide"]["W"] > ol.PRESETS["Dwide"]["H"] and ol.PRESETS["Ttall"]["W"] < ol.PRESETS["Ttall"]["H"]


@pytest.mark.parametrize("preset", ["Dwide", "Ttall"])
def test_fixture_takes_every_wall_and_the_bottom_wall_often(golden_dir, preset):
    """A condition on the input: `walls[episode, step]` = calls of bounce_ball_off_wall in that step that found the ball beyond the
    left / right / top / bottom wall.  The bottom wall (the reference's width-for-height line) and the right wall (the other one a
    swap moves) in at least 5 recorded steps each, the other two at least once."""
    t = np.load(f"{golden_dir}/traj_{preset}.npz")
    meta = json.loads(str(t["meta"]))
    cfg = ol.PRESETS[preset]
    assert meta["arena"] == [cfg["W"], cfg["H"]] and meta["walls"] == "left,right,top,bottom"
    walls = t["walls"]
    assert walls.shape == t["actions"].shape[:2] + (4,) and walls.dtype.kind == "i"
    recorded = np.arange(walls.shape[1])[None, :] < t["length"][:, None]
    assert not walls[~recorded].any()
    left, right, top, bottom = ((walls[..., k] > 0) & recorded for k in range(4))
    print(f"[{preset}] steps with a ball beyond the left / right / top / bottom wall: {left.sum()} / {right.sum()} / {top.sum()} / {bottom.sum()}")
    assert bottom.sum() >= 5 and right.sum() >= 5 and left.sum() >= 1 and top.sum() >= 1
    assert walls.sum() <= meta["coverage"]["bounce_ball_off_wall"] * 2  # (a call finds at most one wall per axis)
    if cfg["nr_h"] + cfg["nr_g"] > 1:
        # NaughtyBots.on_robot_collision fired (RR_ScoreKeepers.py:123-128): needs two robots, so the one-robot Ttall cannot have it
        assert (t["naughty"][recorded] > 0).sum() >= 1 and meta["coverage"]["robot_collision"] > 0
    else:
        assert not t["naughty"].any() and meta["coverage"]["undo_naughty"] > 0  # its robot's blocked moves were undone, though


def _diff(st, ref_r, ref_b):
    assert np.array_equal(np.isnan(st["robots"]), np.isnan(ref_r))
    return max(float(np.nanmax(np.abs(st["robots"] - ref_r))), float(np.abs(st["balls"] - ref_b).max()))


@pytest.mark.parametrize("preset,narrow", [("Dwide", False), ("Dwide", True), ("Ttall", False), ("Ttall", True)])
def test_emulated_wave_follows_every_recorded_step(golden_dir, preset, narrow):
    """Every recorded step from the reference's dumped state (no stride): integer state, done and the NaughtyBots set exact; state and
    both teams' observations within 1e-9, rewards within 1e-7 -- test_emulated_wave.py's bars."""
    t = dict(np.load(f"{golden_dir}/traj_{preset}.npz"))  # (every array once: an NpzFile decompresses on each access)
    env = el.EmuEnv(preset, narrow=narrow)
    has_g = ol.PRESETS[preset]["nr_g"] > 0
    worst, n = 0.0, 0
    for ep in range(t["length"].shape[0]):
        for s in range(int(t["length"][ep])):
            env.set_state(t["state_robots"][ep, s], t["state_robots_i"][ep, s], t["state_balls"][ep, s], t["state_step"][ep, s])
            a = t["actions"][ep, s]
            r = env.step(a[a >= 0])
            st = env.get_state()
            d = _diff(st, t["state_robots"][ep, s + 1], t["state_balls"][ep, s + 1])
            d = max(d, float(np.abs(r["obs"] - t["obs"][ep, s]).max()))
            if has_g:
                d = max(d, float(np.abs(r["obs_g"] - t["obs_g"][ep, s]).max()))
                assert abs(r["reward_g"] - t["reward_g"][ep, s]) < 1e-7, (preset, ep, s)
            assert np.array_equal(st["robots_i"], t["state_robots_i"][ep, s + 1]) and st["step"] == t["state_step"][ep, s + 1], (ep, s)
            assert d < TOL and abs(r["reward"] - t["reward"][ep, s]) < 1e-7, (preset, ep, s, d)
            assert r["done"] == bool(t["done"][ep, s]) and r["naughty"] == t["naughty"][ep, s], (preset, ep, s)
            assert (r["status"] & ~256) == 0
            worst = max(worst, d)
            n += 1
    assert n == int(t["length"].sum()) > 3000
    print(f"[{preset}{' narrow' if narrow else ''}] {n} golden steps through the emulated wave, worst {worst:.2e}")


def test_emulated_wave_flags_the_fault_the_reference_raised_at_dwide(golden_dir):
    t = np.load(f"{golden_dir}/traj_Dwide.npz")
    eps = [ep for ep in range(t["length"].shape[0]) if int(t["exc"][ep])]
    assert eps  # the plan drives one episode into the reference's "unable to resolve" exception
    for ep in eps:
        n = int(t["length"][ep])
        env = el.EmuEnv("Dwide")
        env.set_state(t["state_robots"][ep, n], t["state_robots_i"][ep, n], t["state_balls"][ep, n], t["state_step"][ep, n])
        a = t["actions"][ep, n]
        assert env.step(a[a >= 0])["status"] & int(t["exc"][ep])


@pytest.mark.parametrize("preset", ["Dwide", "Ttall", "Gwide"])
def test_reset_places_every_entity_at_these_sizes(preset):
    """The reference's rejection sampling (and the kernel's copy of it) loops until everything fits: at each size used here every one
    of a few thousand (arena, episode) pairs places all entities, inside the arena's own ranges on both axes."""
    cfg = ol.PRESETS[preset]
    o = ol.OracleEnv(preset)
    R, B = [], []
    for arena in range(400):
        for episode in range(6):
            assert o.reset(7, arena, episode) == 0
            s = o.get_state()
            R.append(s["robots"]); B.append(s["balls"])
    R, B = np.array(R), np.array(B)
    W, H = cfg["W"], cfg["H"]
    assert R[..., 0].min() >= 80 and R[..., 0].max() <= W - 80 and R[..., 1].min() >= 40 and R[..., 1].max() <= H - 40  # RR_EnvBase.py:163-166
    assert B[..., 0].min() >= 40 and B[..., 0].max() <= W - 40 and B[..., 1].min() >= 40 and B[..., 1].max() <= H - 40  # :188-189
    # each axis uses its own bound: the longer one is really reached beyond what the shorter one would allow
    if W > H:
        assert R[..., 0].max() > H - 40 and B[..., 0].max() > H - 40
    else:
        assert R[..., 1].max() > W - 80 + 40 and B[..., 1].max() > W - 40


@pytest.mark.parametrize("preset", ["Dwide", "Ttall", "Gwide"])
def test_a_robot_placed_across_a_wall_is_clamped_to_that_walls_own_coordinate(preset):
    """Wall sliding is off in the reference (RR_Robot.py:66), so a move that hits a wall is taken back and the clamp behind it
    (RR_Robot.py:195-203) only acts on a robot that STARTS beyond a wall -- which the recorded trajectories never do.  Placed across
    each wall and driven into it, the robot ends with that edge half a pixel inside: W - .5 on the right, H - .5 at the bottom."""
    for wall, (robots, balls) in robots_across_the_walls(preset).items():
        e, o = el.EmuEnv(preset), ol.OracleEnv(preset)
        e.set_poses(robots, balls)
        o.set_clean_state(robots, balls)
        acts = [0] + [8] * (e.nr - 1)
        e.step(acts); o.step(acts)
        for st in (e.get_state(), o.get_state()):
            got, want = clamped_edge(preset, wall, st["robots"][0])
            assert abs(got - want) < TOL, (preset, wall, got, want)
        assert np.abs(e.get_state()["robots"][:, :7] - o.get_state()["robots"][:, :7]).max() < TOL


# ---------------------------------------------------------------------------------------------- hive view and goal scoring at Gwide
# (placements and layouts: tests/nonsquare_lib.py)
def test_the_swap_sensitive_placements_are_what_they_claim():
    for x, y in SWAP_IN:
        assert he.in_goal(np.float64(x), np.float64(y), W, H) and not he.in_goal(np.float64(x), np.float64(y), H, W)
    for x, y in SWAP_OUT:
        assert not he.in_goal(np.float64(x), np.float64(y), W, H) and he.in_goal(np.float64(x), np.float64(y), H, W)
    for x, y in NEAR_OUT:
        assert not he.in_goal(np.float64(x), np.float64(y), W, H)


@pytest.mark.parametrize("vw,mask", [(8, 0b1111), (16, 0b0011), (64, 0b1010)])
def test_hive_view_at_gwide_equals_the_restatement_and_the_oracles_observers(vw, mask):
    n = 600
    robots, balls = swap_sensitive_layouts(n)
    assign, obs = he.hive_observe("Gwide", robots, balls, mask, 0, vw)
    want, near = he.greedy_assign_batch(robots[:, :, :2], balls[:, :, :2], mask, W, H)
    assert not near.any() and np.array_equal(assign, want)
    swapped, _ = he.greedy_assign_batch(robots[:, :, :2], balls[:, :, :2], mask, H, W)
    assert (swapped != want).any(1).mean() > 0.1  # the layouts do tell (W, H) from (H, W), whichever robots the mask leaves in
    pos = balls[:, :, :2]
    for menu, free in ((SWAP_IN, False), (SWAP_OUT, True), (NEAR_OUT, True)):
        for xy in menu:
            at = np.all(pos == np.array(xy), axis=2)                       # [n, NB]: this placement
            taken = (assign[:, :, None] == np.arange(8)[None, None, :]).any(1)
            assert at.any() and (taken & at).any() == free, (xy, free)     # a free one is handed out somewhere, one in the goal never
    # the observation rows are the oracle's observer of the assigned pair (lidar walls and the goal corner at 1000 x 640)
    o = ol.OracleEnv("Gwide")
    for a in range(0, n, 7):
        o.set_clean_state(robots[a][:, [0, 1, 6]], balls[a][:, [0, 1, 6, 7]])
        for r in range(4):
            if assign[a, r] < 0:
                assert np.all(obs[a, r] == 0)
                continue
            ref = o.observe(1 if r < 2 else -1, r, int(assign[a, r]))
            assert np.abs(obs[a, r] - ref).max() <= TOL, (a, r)


def test_goal_scoring_at_gwide_emulation_equals_oracle_and_consumes_the_right_balls():
    """k_goal's source (rr_extras.hpp: goal_step) against the oracle's goal_step at 1000 x 640: balls at rest for 151 steps -- exactly
    the ones inside a triangle at (W, H) are consumed, scores and rewards agree, and the near-outside ones stay in play."""
    e, o = el.EmuEnv("Gwide"), ol.OracleEnv("Gwide")
    e.set_goal_scoring(True); o.set_goal_scoring(True)
    balls = [[x, y, 0.0, 0.0] for x, y in GOAL_BALLS]
    e.set_poses(GOAL_ROBOTS, balls)
    o.set_clean_state(GOAL_ROBOTS, balls)
    tot_e = tot_o = 0.0
    for s in range(151):
        re_, ro = e.step([8, 8, 8, 8]), o.step([8, 8, 8, 8])
        assert abs(re_["reward"] - ro["reward"]) < 1e-7 and abs(re_["reward_g"] - ro["reward_g"]) < 1e-7, (s, re_, ro)
        assert re_["done"] == ro["done"] and (re_["status"] & (2048 | 4096 | 8192)) == (ro["status"] & (2048 | 4096 | 8192))
        tot_e += re_["reward"]; tot_o += ro["reward"]
    se, so = e.get_state()["balls"], o.get_state()["balls"]
    assert np.array_equal(se, so)
    assert [b for b in range(8) if se[b, 0] < -900] == GOAL_WANT["consumed"]
    assert list(e.goal_scores()) == list(o.goal_scores()) == [GOAL_WANT["happy"], GOAL_WANT["grumpy"]]
    # the independent statement of which balls lie in a goal agrees (tests/hive_emu_lib.in_goal: the reference's contains_point)
    xy = np.array(GOAL_BALLS)
    assert np.nonzero(he.in_goal(xy[:, 0], xy[:, 1], W, H))[0].tolist() == GOAL_WANT["consumed"]


def test_random_rollouts_with_goal_scoring_at_gwide_match_the_oracle():
    """test_goal_scoring.py's rollout at 1000 x 640 with each axis' own extent: balls scattered into both corners, robots driven at
    random -- kernel source == oracle step by step, scores included."""
    rng = np.random.default_rng(6)
    scored = 0
    for trial in range(3):
        e, o = el.EmuEnv("Gwide"), ol.OracleEnv("Gwide")
        e.set_goal_scoring(True); o.set_goal_scoring(True)
        robots = [[W / 2 + 60 * (i - 2), H / 2, float(rng.integers(0, 360))] for i in range(4)]
        balls = []
        for b in range(8):
            if rng.integers(0, 2):
                balls.append([rng.uniform(W - 150, W - 20), rng.uniform(H - 60, H - 15), 0, 0])
            else:
                balls.append([rng.uniform(15, 60), rng.uniform(20, 150), 0, 0])
        e.set_poses(robots, balls)
        o.set_clean_state(robots, balls)
        done = False
        for s in range(200):
            if done:
                break
            acts = rng.integers(0, 8, size=4)
            re_, ro = e.step(acts), o.step(acts)
            se, so = e.get_state(), o.get_state()
            assert np.allclose(se["balls"], so["balls"], atol=TOL, rtol=0) and np.allclose(se["robots"][:, :7], so["robots"][:, :7], atol=TOL, rtol=0)
            assert abs(re_["reward"] - ro["reward"]) < 1e-7 and abs(re_["reward_g"] - ro["reward_g"]) < 1e-7, (trial, s)
            assert re_["done"] == ro["done"] and (re_["status"] & (2048 | 4096 | 8192)) == (ro["status"] & (2048 | 4096 | 8192))
            assert np.array_equal(e.goal_scores(), o.goal_scores())
            done = re_["done"]
        scored += int(e.goal_scores().any())
    assert scored  # (a condition on the input: in some trial a ball stayed in its corner for the 150 steps a goal takes)
