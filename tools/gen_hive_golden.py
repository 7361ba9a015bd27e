"""Records the reference's hive-mind player (DQN_pytorch_player.Stephen) into tests/golden/hive_{G,X}.npz.

    python tools/gen_hive_golden.py G      # one preset per process: the reference's constants are module globals
    python tools/gen_hive_golden.py X

The unmodified reference is imported under the stand-ins of oracle/refgen (pygame, gym) plus an in-memory `imageio` stand-in, so
that DQN_pytorch_player imports.  Stephen's class-level mind is a stub whose choose_action(obs, epsilon_override) records the
observation it is shown and returns a scripted action, so the hive never looks for its pickled checkpoint.  The env is the class
main.py builds (SingleBall_6wayLidar on top of the score keepers).  Cases: the happy team is the hive; every robot is; one robot
is -- the other robots get random thrusts.  Episodes are driven by the Stephens' own returned thrusts.  Per recorded step: the
state (canonical layout of include/roborugby_amd.h, as in traj_*.npz), the assignment read back from the hive, the observations the
mind was shown (kind 1) and SingleBall_6wayLidar_v2.get_game_state for the same pairs (kind 0).  Hand-placed states add what
episodes rarely visit: a ball inside each goal triangle, more hive robots than free balls, every ball in a goal.

A recorded episode step is dropped when two candidate pairs' distances (the reference's own `distance`) differ by less than 1e-9
relative: the order of ties is not defined by the reference.  `meta` counts the drops.  Test infrastructure only: nothing in the
product imports this file, and nothing of the reference's text is in it or in the fixture."""
import json
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.environ.get("RR_GOLDEN_OUT") or os.path.join(REPO, "tests", "golden")  # (the regeneration test writes to a scratch directory)
sys.path.insert(0, os.path.join(REPO, "oracle", "refgen"))

NAN = float("nan")
TIE_REL = 1e-9
EPISODE_STEPS, RECORD_EVERY = 240, 3  # per case; every third step is kept (contacts need the steps in between to be played)
SEEDS = {"G": 20260, "X": 20261}


def install_imageio_standin():
    if "imageio" not in sys.modules:
        m = types.ModuleType("imageio")
        m.get_writer = lambda *a, **k: None
        sys.modules["imageio"] = m


def robot_row(rb):
    r = rb.rectDbl
    st = rb._lstStates[(rb.lngMoveCount - 1) % 360]
    px, py, prot = (NAN, NAN, NAN) if st is None or st[3] != rb.lngMoveCount - 1 else (st[0], st[1], st[2])
    return ([r._dblCenterX, r._dblCenterY, r._dblLeft, r._dblRight, r._dblTop, r._dblBottom, float(r._dblRotation), px, py, float(prot)],
            [rb.lngMoveCount, rb.lngLThrust, rb.lngRThrust])


def ball_row(b):
    r = b.rectDbl
    return [r._dblCenterX, r._dblCenterY, r._dblLeft, r._dblRight, r._dblTop, r._dblBottom, float(b.dbl_velocity_x), float(b.dbl_velocity_y)]


class Mind:
    """stands in for the pickled DQNAgent: shows what the hive asks and answers with a scripted chase of the assigned ball"""

    def __init__(self, rng):
        self.rng = rng
        self.seen = []

    def choose_action(self, obs, epsilon_override=None):
        assert epsilon_override == 0.2
        self.seen.append(np.array(obs, dtype=np.float64))
        if self.rng.random() < 0.15:
            return self.rng.randint(0, 7)
        d = (obs[1] - obs[0] + 540.0) % 360.0 - 180.0
        return 0 if abs(d) < 8 else ((4 if d > 0 else 5) if abs(d) < 40 else (2 if d > 0 else 3))


class Recorder:
    def __init__(self, R, player_mod, nr, nb):
        self.R, self.S, self.nr, self.nb = R, player_mod.Stephen, nr, nb
        self.rows = dict(robots=[], robots_i=[], balls=[], step=[], mask=[], assign=[], obs_v1=[], obs_v2=[], hand=[], case=[])
        self.dropped_episode = self.dropped_hand = self.episode_steps = 0

    def new_hive(self, env, members, mind):
        S = self.S
        S._Stephen__hive, S._Stephen__assignments, S._Stephen__env, S._Stephen__mind = set(), {}, None, mind
        return {r: S(env, env.lstRobots[r]) for r in members}

    def near_tie(self, env, members):
        R = self.R
        d = sorted(R.MyUtils.distance(b.rectDbl.center, env.lstRobots[r].rectDbl.center) for b in env.lstBalls
                   if not (env.sprGrumpyGoal.ball_in_goal(b) or env.sprHappyGoal.ball_in_goal(b)) for r in members)
        return any(b - a < TIE_REL * max(b, 1e-300) for a, b in zip(d, d[1:]))

    def consult(self, env, hive, mind, keep, hand, case):
        """every Stephen's get_action for the current state; records the step when `keep`.  Returns {robot: (L, R)}."""
        rob = [robot_row(rb) for rb in env.lstRobots]
        balls = [ball_row(b) for b in env.lstBalls]
        thrust, assign = {}, np.full(self.nr, -1, np.int32)
        v1, v2 = np.zeros((self.nr, 11)), np.zeros((self.nr, 11))
        for r in sorted(hive):
            mind.seen.clear()
            thrust[r] = hive[r].get_action()
            ball = self.S._Stephen__assignments.get(hive[r])
            if ball is None:
                assert thrust[r] == (0, 0) and not mind.seen
                continue
            assign[r] = env.lstBalls.index(ball)
            assert len(mind.seen) == 1
            v1[r] = mind.seen[0]
            v2[r] = self.R.obs.SingleBall_6wayLidar_v2.get_game_state(env, obj_robot=env.lstRobots[r], obj_ball=ball)
        if not keep:
            return thrust
        if self.near_tie(env, sorted(hive)):
            if hand:
                self.dropped_hand += 1
            else:
                self.dropped_episode += 1
            return thrust
        w = self.rows
        w["robots"].append([x[0] for x in rob]); w["robots_i"].append([x[1] for x in rob]); w["balls"].append(balls)
        w["step"].append(env.lngStepCount); w["mask"].append(sum(1 << r for r in hive)); w["assign"].append(assign)
        w["obs_v1"].append(v1); w["obs_v2"].append(v2); w["hand"].append(int(hand)); w["case"].append(case)
        return thrust


def hand_layouts(nr, nb, nbp, W, H):
    """[(name, robots (x, y, rot), balls (x, y))]: goal triangles are the corners (W, H) [happy] and (0, 0) [grumpy], legs of 240"""
    rng = random.Random(99)
    rob = [(200.0 + 97.0 * r + 13.0 * (r % 2), 560.0 - 83.0 * r, (37.0 * r + 15.0) % 360.0) for r in range(nr)]
    free = [(330.0 + 41.0 * b + 7.0 * (b % 3), 300.0 + 29.0 * ((5 * b) % 7)) for b in range(nb)]
    in_h = [(W - 20.0 - 12.0 * b, H - 25.0 - 7.0 * (b % 4)) for b in range(nb)]   # well inside the happy triangle
    in_g = [(20.0 + 12.0 * b, 25.0 + 7.0 * (b % 4)) for b in range(nb)]            # ... the grumpy one
    out = [("all_free", rob, free)]
    b1 = list(free); b1[0] = in_h[0]
    out.append(("pos_ball_in_happy_goal", rob, b1))
    b2 = list(free); b2[nb - 1] = in_g[0]
    out.append(("last_ball_in_grumpy_goal", rob, b2))
    b3 = [in_h[b] if b % 2 else in_g[b] for b in range(nb)]; b3[nbp - 1] = free[0]
    out.append(("one_free_ball", rob, b3))                                        # more hive robots than free balls
    out.append(("all_in_goals", rob, [in_g[b] if b % 2 else in_h[b] for b in range(nb)]))
    # inside a goal's bounding box but beyond the hypotenuse (not in the goal), and just inside it
    b5 = list(free); b5[0] = (W - 200.0, H - 200.0); b5[1 % nb] = (100.0, 100.0)
    out.append(("box_not_triangle_and_inside", rob, b5))
    for k in range(6):  # a few random ones with balls thrown into both corners
        bb = [(rng.uniform(5, 235), rng.uniform(5, 235)) if rng.random() < .3 else (rng.uniform(W - 235, W - 5), rng.uniform(H - 235, H - 5))
              if rng.random() < .4 else (rng.uniform(250, W - 250), rng.uniform(250, H - 250)) for _ in range(nb)]
        rr_ = [(rng.uniform(260, W - 260), rng.uniform(60, H - 60), rng.uniform(0, 360)) for _ in range(nr)]
        out.append((f"random_corners_{k}", rr_, bb))
    return out


def main(preset):
    assert preset in ("G", "X")
    from load_reference import load_reference
    R = load_reference(preset)
    install_imageio_standin()
    # presets other than G are loaded into a synthetic package (load_reference): give it the names the package's own start-up
    # module would have bound, for `from robo_rugby.gym_env import ...` in the player modules
    pkg = sys.modules["robo_rugby.gym_env"]
    for name, val in (("GameEnv", R.base.GameEnv), ("GameEnv_Simple", R.base.GameEnv_Simple), ("Robot", R.robot.Robot),
                      ("Ball", R.ball.Ball), ("Goal", R.goal.Goal), ("RR_Observers", R.obs)):
        if not hasattr(pkg, name):
            setattr(pkg, name, val)
    import DQN_pytorch_player as player
    const = R.const
    nr, nb, nbp, nrh = const.NUM_ROBOTS_TOTAL, const.NUM_BALL_POS + const.NUM_BALL_NEG, const.NUM_BALL_POS, const.NUM_ROBOTS_HAPPY
    W, H = float(const.ARENA_WIDTH), float(const.ARENA_HEIGHT)

    class HiveGame(R.sk.PushPosBallsInYourGoal, R.sk.PushNegBallsInTheirGoal, R.sk.BaseDestruction, R.obs.SingleBall_6wayLidar,
                   R.base.GameEnv):  # the line-up of the reference's main.py
        pass

    seed = SEEDS[preset]
    random.seed(seed)
    np.random.seed(seed)
    rng = random.Random(seed + 1)
    rec = Recorder(R, player, nr, nb)
    faults = 0
    cases = [("happy_team", list(range(nrh))), ("all_robots", list(range(nr))), ("one_robot", [nr - 1])]
    for ci, (cname, members) in enumerate(cases):
        mind = Mind(rng)
        env = HiveGame()
        hive = rec.new_hive(env, members, mind)
        for step in range(EPISODE_STEPS):
            keep = step % RECORD_EVERY == 0
            rec.episode_steps += int(keep)
            thrust = rec.consult(env, hive, mind, keep, False, ci)
            acts = [thrust[r] if r in thrust else (rng.choice((-1, 0, 1)), rng.choice((-1, 0, 1))) for r in range(nr)]
            try:
                env.step(acts)
            except Exception:  # the reference raises from inside step when a contact cannot be resolved: a new game, like its main loop
                faults += 1
                env = HiveGame()
                hive = rec.new_hive(env, members, mind)
        for name, rob, balls in hand_layouts(nr, nb, nbp, W, H):
            env = HiveGame([rob, balls])
            hive = rec.new_hive(env, members, mind)
            rec.consult(env, hive, mind, True, True, ci)
    w = rec.rows
    meta = dict(generator="tools/gen_hive_golden.py", preset=preset, seed=seed,
                reference="harman097/RoboRugby (unmodified, imported under stand-ins): DQN_pytorch_player.Stephen with a stub mind",
                route="stub mind: assignments read back from the hive, observations as shown to choose_action",
                env_class="PushPosBallsInYourGoal, PushNegBallsInTheirGoal, BaseDestruction, SingleBall_6wayLidar, GameEnv",
                cases=[dict(name=c, robots=m) for c, m in cases], hand_layouts=[h[0] for h in hand_layouts(nr, nb, nbp, W, H)],
                subsampling=f"{EPISODE_STEPS} steps per case, every {RECORD_EVERY}rd recorded; every hand-placed state recorded",
                tie_rule=f"steps with two candidate pair distances closer than {TIE_REL} relative are dropped",
                episode_steps=rec.episode_steps, games_restarted_after_a_reference_exception=faults, dropped_episode_steps=rec.dropped_episode,
                hand_states=int(sum(w["hand"])) + rec.dropped_hand, dropped_hand_states=rec.dropped_hand,
                obs_v1="SingleBall_6wayLidar.get_game_state(obj_robot, obj_ball) as the mind saw it; rows of robots without a ball are 0",
                obs_v2="SingleBall_6wayLidar_v2.get_game_state, unbound call on the same env, same pairs")
    os.makedirs(GOLD, exist_ok=True)
    np.savez_compressed(os.path.join(GOLD, f"hive_{preset}.npz"),
                        robots=np.array(w["robots"], np.float64), robots_i=np.array(w["robots_i"], np.int32),
                        balls=np.array(w["balls"], np.float64), step=np.array(w["step"], np.int32), mask=np.array(w["mask"], np.uint32),
                        assign=np.array(w["assign"], np.int32), obs_v1=np.array(w["obs_v1"], np.float64),
                        obs_v2=np.array(w["obs_v2"], np.float64), hand=np.array(w["hand"], np.uint8), case=np.array(w["case"], np.int32),
                        meta=np.array(json.dumps(meta)))
    print(json.dumps(meta, indent=1))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "G")
