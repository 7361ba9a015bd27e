"""Writes tests/golden/robot_move_pin.npz: seeded arenas that take the robot move (Robot.move, csrc/rr_sim.hpp: robot_move_finish and its
lane-pair form in substep_phase1) through every arm, and the complete state the host emulation leaves after each step.

The fixture pins the move ACROSS a change of how it is spread over lanes, so it is generated from the sources BEFORE such a change:
run this tool on a checkout of the commit to compare with (it only needs tests/emu_lib.py and the emulation's sources there) and copy
the file.  The committed file is from the commit before the move's tail was split over the lane pair by component.

    python tools/gen_robot_move_pin.py [--out=FILE]

Per preset (T, D, G and the non-square Dwide) three groups of arenas: `act1` one step of rr_step's actions 0-7, `act3` three steps with a
new action each, `thr1` one step of (L, R) thrust pairs, which adds the ninth pattern (0, 0).  Balls stand still in the middle of the
arena, robots far from them and from each other: only the move runs.  A robot is one of
  free      anywhere, rot exactly 0 / 90 / 180 / 270 or random;
  lin_wall  an edge within 1 px of one of the four walls, heading into it (forwards or backwards): the linear move's revert;
  turn_wall an edge within 0.05 px of a wall, pivoting or spinning: the revert that also restores the rotation;
  turn_720  the same with a rotation that (rot + 720) % 360 perturbs (1e-13, 360 - 1e-13, a multiple of 90 one ulp off): the
            restore has to rebuild the corners;
  across    placed across one wall or two (l < 0, r > W, t <= 0, b >= H, the `<=` ones also exactly on the wall): the four clamp arms.
Arrays, per preset P and group G:  P_G_robots [n, NR, 10], P_G_robots_i [n, NR, 3], P_G_balls [n, NB, 8] (the canonical state to set),
P_G_actions [steps, n, NR] (int32) or P_G_thrust [steps, n, 2 NR] (float32), and for each build B (`default`, `exact`):
P_G_B_robots [steps, n, NR, 10], P_G_B_robots_i, P_G_B_balls, P_G_B_status [steps, n] (flags), P_G_B_naughty [steps, n] (robot set)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import emu_lib  # noqa: E402
import oracle_lib as ol  # noqa: E402

PRESETS = ("T", "D", "G", "Dwide")
GROUPS = (("act1", 130, 1, False), ("act3", 40, 3, False), ("thr1", 30, 1, True))  # name, arenas, steps, thrust entry
THRUST = {0: (1, 1), 1: (-1, -1), 2: (-1, 1), 3: (1, -1), 4: (0, 1), 5: (1, 0), 6: (-1, 0), 7: (0, -1)}  # RR_EnvBase.py:593-602
TURNS = (2, 3, 4, 5, 6, 7)
WALLS = "LRTB"
INTO = {"L": 180.0, "R": 0.0, "T": 90.0, "B": 270.0}  # the heading that drives forwards into the wall (dx = cos rot, dy = -sin rot)
KINDS = ("free", "lin_wall", "turn_wall", "turn_720", "across")
CX, CY, EL, ER, ET, EB, ROT = range(7)  # columns of a canonical robot row


def perturbed_rotations():
    """rotations that the rotation setter's (x + 720) % 360 does not give back"""
    out = [1e-13, 360.0 - 1e-13]
    for base in (90.0, 180.0, 270.0):
        for ulps in (-1, 1):
            x = base
            for _ in range(abs(ulps)):
                x = np.nextafter(x, np.inf if ulps > 0 else -np.inf)
            out.append(float(x))
    assert all((x + 720.0) % 360.0 != x for x in out)
    return out


PERTURBED = perturbed_rotations()


def plan_robot(rng, kind, j, W, H):
    """robot j of an arena: its clean pose, the edits of its row afterwards, its action"""
    along = (0.30, 0.43, 0.57, 0.70)[j]  # where it sits along a wall: robots of one arena stay > 70 px apart
    slot = ((0.3, 0.3), (0.7, 0.3), (0.3, 0.7), (0.7, 0.7))[j]
    p = dict(kind=kind, x=slot[0] * W + rng.uniform(-10, 10), y=slot[1] * H + rng.uniform(-10, 10), edits=[], rot_field=None)
    if kind == "free":
        p["rot"] = float(rng.choice([0.0, 90.0, 180.0, 270.0, rng.uniform(0, 360), rng.uniform(0, 360)]))
        p["action"] = int(rng.integers(0, 9))  # 8: the idle pattern (0, 0), thrust entry only
        return p
    walls = [WALLS[int(rng.integers(0, 4))]]
    if kind == "across" and rng.random() < 0.4:  # two walls at once: a corner of the arena
        walls = [str(rng.choice(["L", "R"])), str(rng.choice(["T", "B"]))]
    if "L" in walls or "R" in walls:
        p["y"] = along * H
    if "T" in walls or "B" in walls:
        p["x"] = along * W
    w = walls[0]
    if kind == "lin_wall":
        back = rng.random() < 0.3
        p["rot"] = (INTO[w] + (180.0 if back else 0.0) + float(rng.choice([0.0, rng.uniform(-40, 40)]))) % 360.0
        p["action"] = 1 if back else 0
        p["edits"] = [(w, rng.uniform(0, 1), False)]
    elif kind in ("turn_wall", "turn_720"):
        p["rot"] = float(rng.choice([0.0, 90.0, 180.0, 270.0])) + float(rng.choice([0.0, rng.uniform(-3, 3)]))
        p["rot"] %= 360.0
        p["action"] = int(rng.choice(TURNS))
        p["edits"] = [(w, rng.uniform(0, 0.05), False)]
        if kind == "turn_720":
            p["rot_field"] = PERTURBED[int(rng.integers(0, len(PERTURBED)))]
            p["rot"] = round(p["rot_field"]) % 360.0
    else:  # across: the edge beyond the wall by up to 3 px, or exactly on it (what `<` and `<=` tell apart)
        p["rot"] = float(rng.choice([0.0, 90.0, rng.uniform(0, 360)]))
        p["action"] = int(rng.integers(0, 9))
        p["edits"] = [(v, 0.0 if rng.random() < 0.25 else -rng.uniform(0, 3), True) for v in walls]
    return p


def apply_edit(row, wall, inside, exact, W, H):
    """shift the row so that the edge facing `wall` lies `inside` px inside the arena (negative: beyond the wall)"""
    col, target = {"L": (EL, inside), "R": (ER, W - inside), "T": (ET, inside), "B": (EB, H - inside)}[wall]
    d = target - row[col]
    for c in ((CX, EL, ER) if wall in "LR" else (CY, ET, EB)):
        row[c] += d
    if exact:
        row[col] = target


def ball_poses(nb, W, H):
    cols = (nb + 1) // 2 if nb > 1 else 1
    out = []
    for b in range(nb):
        out.append([W / 2 + 80.0 * (b % cols - (cols - 1) / 2), H / 2 + (80.0 * (b // cols) - 40.0 if nb > cols else 0.0), 0.0, 0.0])
    return np.array(out)


def build_group(preset, n, steps, thrust, rng):
    cfg = ol.PRESETS[preset]
    W, H = cfg["W"], cfg["H"]
    env = emu_lib.EmuEnv(preset, exact=False)
    nr, nb = env.nr, env.nb
    robots, robots_i, balls = np.zeros((n, nr, 10)), np.zeros((n, nr, 3), np.int32), np.zeros((n, nb, 8))
    acts = np.zeros((steps, n, nr), np.int32)
    for a in range(n):
        plans = [plan_robot(rng, KINDS[(a * nr + j) % len(KINDS)], j, W, H) for j in range(nr)]
        env.set_poses(np.array([[p["x"], p["y"], p["rot"]] for p in plans]), ball_poses(nb, W, H))
        st = env.get_state()
        for j, p in enumerate(plans):
            row = st["robots"][j]
            for wall, inside, exact in p["edits"]:
                apply_edit(row, wall, inside, exact, W, H)
            if p["rot_field"] is not None:
                row[ROT] = p["rot_field"]
            acts[0, a, j] = p["action"]
        robots[a], robots_i[a], balls[a] = st["robots"], st["robots_i"], st["balls"]
    acts[1:] = rng.integers(0, 9, acts[1:].shape)
    if not thrust:  # rr_step has no action for (0, 0): the other eight
        acts = np.where(acts == 8, rng.integers(0, 8, acts.shape), acts).astype(np.int32)
    out = dict(robots=robots, robots_i=robots_i, balls=balls)
    if thrust:
        table = np.array([THRUST[k] for k in range(8)] + [(0, 0)], np.float32)
        out["thrust"] = table[acts].reshape(steps, n, 2 * nr)
    else:
        out["actions"] = acts
    return out


def run_group(preset, g, exact, narrow=False):
    """the states after each step of the group's arenas, one emulated arena at a time"""
    n = g["robots"].shape[0]
    steps = (g["thrust"] if "thrust" in g else g["actions"]).shape[0]
    env = emu_lib.EmuEnv(preset, exact=exact, narrow=narrow)
    res = dict(robots=np.zeros((steps,) + g["robots"].shape), robots_i=np.zeros((steps,) + g["robots_i"].shape, np.int32),
               balls=np.zeros((steps,) + g["balls"].shape), status=np.zeros((steps, n), np.int32), naughty=np.zeros((steps, n), np.int32))
    for a in range(n):
        env.set_state(g["robots"][a], g["robots_i"][a], g["balls"][a], 0)
        for s in range(steps):
            r = env.step_thrust(g["thrust"][s, a]) if "thrust" in g else env.step(g["actions"][s, a])
            st = env.get_state()
            res["robots"][s, a], res["robots_i"][s, a], res["balls"][s, a] = st["robots"], st["robots_i"], st["balls"]
            res["status"][s, a], res["naughty"][s, a] = r["status"], r["naughty"]
    return res


def main():
    out_path = os.path.join(HERE, "..", "tests", "golden", "robot_move_pin.npz")
    for a in sys.argv[1:]:
        if a.startswith("--out="):
            out_path = a.split("=", 1)[1]
    rng = np.random.default_rng(20240607)
    arrays = {}
    for preset in PRESETS:
        for name, n, steps, thrust in GROUPS:
            g = build_group(preset, n, steps, thrust, rng)
            for k, v in g.items():
                arrays[f"{preset}_{name}_{k}"] = v
            for build, exact in (("default", False), ("exact", True)):
                res = run_group(preset, g, exact)
                for k, v in res.items():
                    arrays[f"{preset}_{name}_{build}_{k}"] = v
                moved = np.any(res["robots"][0][..., :7] != g["robots"][..., :7], axis=-1)
                print(f"{preset} {name} {build}: {n} arenas x {steps} steps, {int(moved.sum())} of {moved.size} robots changed in step 1, "
                      f"status {sorted(set(res['status'].ravel().tolist()))}")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    np.savez_compressed(out_path, **arrays)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
