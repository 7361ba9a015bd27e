"""Layouts the non-square-arena tests share between their CPU half (tests/test_nonsquare_arena.py: host emulation, oracle) and their GPU
half (tests/test_gpu_nonsquare.py) -- test harness only.  `Gwide` is G's counts at 1000 x 640 (tests/oracle_lib.py)."""
import numpy as np

import hive_emu_lib as he
import oracle_lib as ol

W, H = ol.PRESETS["Gwide"]["W"], ol.PRESETS["Gwide"]["H"]
# balls whose goal membership a swap of W and H changes.  The happy triangle at (W, H) = (1000, 640) has its corners at (1000, 640),
# (1000, 400), (760, 640): x + y >= 1400 inside the box; at (H, W) it would be x in [400, 640], y in [760, 1000], x + y >= 1400.
SWAP_IN = [(950.0, 620.0), (W - 130.0, H - 100.0), (W - 8.0, H - 230.0)]       # inside at (W, H), outside every triangle at (H, W)
SWAP_OUT = [(620.0, 950.0), (H - 100.0, W - 130.0)]                            # inside (H, W)'s triangle, a free ball at (W, H)
NEAR_OUT = [(W - 130.0, H - 115.0), (W - 245.0, H - 5.0)]                      # just outside the hypotenuse / the box at (W, H)

GOAL_ROBOTS = [[300.0, 100.0, 0.0], [300.0, 200.0, 0.0], [300.0, 300.0, 0.0], [300.0, 400.0, 0.0]]
# positive balls 0-3, negative 4-7; all at rest, nobody moves (action 8).  Inside the happy triangle: 0 (950, 620), 1, 4; free: the
# mirror-side and near-outside placements that fit the 640-px floor, and one ball in the grumpy triangle (which no swap moves)
GOAL_BALLS = [SWAP_IN[0], SWAP_IN[1], NEAR_OUT[0], (H - 100.0, 500.0), SWAP_IN[2], NEAR_OUT[1], (60.0, 70.0), (500.0, 300.0)]
GOAL_WANT = dict(consumed=[0, 1, 4, 6], happy=500 + 500 - 500, grumpy=-500)  # a goal's score: +500 per positive, -500 per negative ball


def swap_sensitive_layouts(n, seed=11):
    """Gwide layouts in canonical form (robots [n,4,10], balls [n,8,8]): hive_emu_lib.random_layouts over the 1000 x 640
    floor, and in every arena three balls overwritten with swap-sensitive placements: one of SWAP_IN, one of SWAP_OUT, one of NEAR_OUT."""
    rng = np.random.default_rng(seed)
    robots, balls = he.random_layouts(rng, n, 4, 8, W, H)
    for a in range(n):
        slots = rng.permutation(8)[:3]
        for slot, menu in zip(slots, (SWAP_IN, SWAP_OUT, NEAR_OUT)):
            balls[a, slot, :2] = menu[(a + slot) % len(menu)]
    return robots, balls


def robots_across_the_walls(preset):
    """One layout per wall: robot 0 placed across it, heading into it; everything else parked far away.  -> {wall: (robots_xyr, balls_xyv)}"""
    cfg = ol.PRESETS[preset]
    w, h, nr, nb = cfg["W"], cfg["H"], cfg["nr_h"] + cfg["nr_g"], cfg["nb_p"] + cfg["nb_n"]
    rest = [[120.0 + 70 * i, 120.0, 0.0] for i in range(nr - 1)]
    balls = [[150.0 + 40 * b, 300.0, 0.0, 0.0] for b in range(nb)]
    return {wall: ([[x, y, rot]] + rest, balls) for wall, (x, y, rot) in
            dict(left=(3.0, h / 2, 180.0), right=(w - 3.0, h / 2, 0.0), top=(w / 2, 3.0, 90.0), bottom=(w / 2, h - 3.0, 270.0)).items()}


def clamped_edge(preset, wall, robot_row):
    """(edge of the canonical robot row that the clamp sets, the value RR_Robot.py:195-203 gives it: buffer = .5 inside that wall)"""
    cfg = ol.PRESETS[preset]
    return {"left": (robot_row[2], 0.5), "right": (robot_row[3], cfg["W"] - 0.5), "top": (robot_row[4], 0.5), "bottom": (robot_row[5], cfg["H"] - 0.5)}[wall]
