"""Non-square arenas on the MI355X, the parts that have no reference vector: k_hive and goal scoring at `Gwide` (G's counts at
1000 x 640) against the numpy restatement of the greedy rule (tests/hive_emu_lib.py) and the oracle, with balls placed where a
swapped width and height changes the answer (tests/nonsquare_lib.py has the placements, tests/test_nonsquare_arena.py the CPU half), and the Python
surface.  The reference-vector half at `Dwide` / `Ttall` is in test_gpu_parity.py, test_gpu_fp32.py and test_mixins_kernel.py."""
import numpy as np
import pytest

import hive_emu_lib as he
import oracle_lib as ol
from nonsquare_lib import (GOAL_BALLS, GOAL_ROBOTS, GOAL_WANT, H, NEAR_OUT, SWAP_IN, SWAP_OUT, W, clamped_edge, robots_across_the_walls,
                           swap_sensitive_layouts)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL64 = 1e-9


def _env(preset, n, **kw):
    import roborugby_amd as rr
    kw.setdefault("time_limit", False)
    kw.setdefault("auto_reset", False)
    return rr.BatchedRoboRugbyEnv(n, preset=ol.product_preset(preset), **kw)


@pytest.mark.parametrize("preset,high", [("Dwide", 1000.0), ("Ttall", 720.0), ("Gwide", 1000.0)])
def test_observation_space_high_is_the_longer_side(preset, high):
    """max(ARENA_WIDTH, ARENA_HEIGHT, 360) (RR_Observers.py:34)"""
    env = _env(preset, 4)
    env.reset()
    assert float(env.observation_space.high.max()) == float(env.observation_space.high.min()) == high
    assert float(env.observation_space.low.min()) == -high
    assert env.render("rgb_array", arena=1).shape == (int(ol.PRESETS[preset]["H"]), int(ol.PRESETS[preset]["W"]) + 300, 3)
    env.close()


@pytest.mark.parametrize("preset", ["Dwide", "Ttall", "Gwide"])
def test_a_robot_placed_across_a_wall_is_clamped_to_that_walls_own_coordinate(preset):
    """RR_Robot.py:195-203 on the device (tests/test_nonsquare_arena.py explains why only a hand-placed robot reaches that clamp): one
    arena per wall, edge half a pixel inside that wall afterwards, and the whole robot state equal to the oracle's."""
    layouts = robots_across_the_walls(preset)
    walls = list(layouts)
    env = _env(preset, len(walls))
    env.set_poses(np.array([layouts[w][0] for w in walls]), np.array([layouts[w][1] for w in walls]))
    acts = torch.full((len(walls), env.preset.nr), 8, dtype=torch.int32, device="cuda")
    acts[:, 0] = 0
    env.step_f64(acts)
    st = env.get_state()["robots"].cpu().numpy()
    for a, wall in enumerate(walls):
        got, want = clamped_edge(preset, wall, st[a, 0])
        assert abs(got - want) < TOL64, (preset, wall, got, want)
        o = ol.OracleEnv(preset)
        o.set_clean_state(*layouts[wall])
        o.step([0] + [8] * (env.preset.nr - 1))
        assert np.abs(st[a][:, :7] - o.get_state()["robots"][:, :7]).max() < TOL64, (preset, wall)
    env.close()


@pytest.mark.parametrize("n,mask,dtype", [(2048, 0b1111, "f64"), (513, 0b0011, "f64"), (2048, 0b1010, "f32")])
def test_hive_observe_at_gwide(n, mask, dtype):
    robots, balls = swap_sensitive_layouts(n)
    if dtype == "f32":  # the handle keeps fp32 records: compare on what it holds
        robots, balls = robots.astype(np.float32).astype(np.float64), balls.astype(np.float32).astype(np.float64)
    env = _env("Gwide", n, dtype=dtype)
    env.set_poses(robots[:, :, [0, 1, 6]], balls[:, :, [0, 1, 6, 7]])
    want, near = he.greedy_assign_batch(robots[:, :, :2], balls[:, :, :2], mask, W, H, dtype=np.float32 if dtype == "f32" else np.float64)
    assert near.mean() <= 0.001
    swapped, _ = he.greedy_assign_batch(robots[:, :, :2], balls[:, :, :2], mask, H, W)
    assert (swapped != want).any(1).mean() > 0.1  # the layouts tell (W, H) from (H, W)
    f64 = dtype == "f64"
    assign, obs = env.hive_observe(mask, observer="SingleBall_6wayLidar_v2", f64=f64)
    assign, obs = assign.cpu().numpy(), obs.cpu().numpy().astype(np.float64)
    assert np.array_equal(assign[~near], want[~near]), np.nonzero((assign != want).any(1) & ~near)[0][:5]
    taken = (assign[:, :, None] == np.arange(8)[None, None, :]).any(1)
    for menu, free in ((SWAP_IN, False), (SWAP_OUT, True), (NEAR_OUT, True)):
        for xy in menu:
            at = np.all(balls[:, :, :2] == np.array(xy, np.float32 if dtype == "f32" else np.float64).astype(np.float64), axis=2)
            assert at.any() and (taken & at).any() == free, (xy, free)
    if f64:  # the rows are the oracle's observer of the assigned pair: lidar walls and goal corner at 1000 x 640
        o = ol.OracleEnv("Gwide")
        for a in range(0, n, 16):
            o.set_clean_state(robots[a][:, [0, 1, 6]], balls[a][:, [0, 1, 6, 7]])
            for r in range(4):
                if assign[a, r] < 0:
                    assert np.all(obs[a, r] == 0)
                    continue
                ref = o.observe(1 if r < 2 else -1, r, int(assign[a, r]))
                assert np.abs(obs[a, r] - ref).max() <= TOL64, (a, r)
    env.close()


def test_goal_scoring_at_gwide_matches_the_oracle():
    """Eight balls at rest along the hypotenuse of the happy triangle at (W, H) = (1000, 640), each a few pixels inside or outside it
    (35 px apart: nothing touches), nobody moves, 151 steps: which balls are consumed, the scores, the summed rewards and done equal
    the oracle's, arena by arena.  Arena 0 is the hand-placed layout of tests/nonsquare_lib.py.  With W and H swapped in
    goal_step none of these balls would lie in a goal."""
    n, steps = 128, 151
    rng = np.random.default_rng(8)
    robots = np.tile(np.array([GOAL_ROBOTS]), (n, 1, 1))
    balls = np.zeros((n, 8, 4))
    off = rng.uniform(-10, 10, (n, 8)) / np.sqrt(2.0)
    balls[:, :, 0] = 790.0 + 25.0 * np.arange(8)[None, :] + off
    balls[:, :, 1] = 610.0 - 25.0 * np.arange(8)[None, :] + off
    balls[0, :, :2] = GOAL_BALLS
    inside = he.in_goal(balls[:, :, 0], balls[:, :, 1], W, H)
    assert 0.3 < inside[1:].mean() < 0.7 and not he.in_goal(balls[1:, :, 0], balls[1:, :, 1], H, W).any()
    assert np.nonzero(inside[0])[0].tolist() == GOAL_WANT["consumed"]
    env = _env("Gwide", n, goal_scoring=True)
    env.set_poses(robots, balls)
    acts = torch.full((n, 4), 8, dtype=torch.int32, device="cuda")
    total = torch.zeros(n, dtype=torch.float64, device="cuda")
    total_g = torch.zeros(n, dtype=torch.float64, device="cuda")
    for s in range(steps):
        o, r, d, info = env.step_f64(acts)
        total += r
        total_g += info.dblGrumpyScore
    scores = env.goal_scores().cpu().numpy()
    st = env.get_state()["balls"].cpu().numpy()
    d, total, total_g = d.cpu().numpy(), total.cpu().numpy(), total_g.cpu().numpy()
    assert np.array_equal(st[:, :, 0] < -900, inside)  # consumed == inside the triangle at (W, H), by the independent statement
    assert list(scores[0]) == [GOAL_WANT["happy"], GOAL_WANT["grumpy"]]
    for a in range(n):
        orc = ol.OracleEnv("Gwide")
        orc.set_goal_scoring(True)
        orc.set_clean_state(robots[a], balls[a])
        tot = tot_g = 0.0
        for s in range(steps):
            res = orc.step([8, 8, 8, 8])
            tot += res["reward"]; tot_g += res["reward_g"]
        assert abs(tot - total[a]) < 1e-6 and abs(tot_g - total_g[a]) < 1e-6, (a, tot, total[a])
        assert res["done"] == bool(d[a]) and np.array_equal(orc.goal_scores(), scores[a]), a
        assert np.array_equal(orc.get_state()["balls"], st[a]), a
    env.close()
