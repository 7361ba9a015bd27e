"""Checks shared by tests/test_gpu_fp32_entries.py (the HIP library) and tests/test_fp32_entries_emulated.py (the kernel source on
the host): every entry a handle offers besides rr_step, on an RR_DTYPE_F32 / RR_DTYPE_F32_STATE handle, against a reference.

Every comparison is a single step (or none) from a state the test sets; the reference always gets the state as the handle holds it
(fp32-representable).  What is in here:
  keepers_ref   the seven reward keepers of RR_ScoreKeepers.py restated in numpy fp64 from the reference's own text;
  reward_bound  how far an fp32 / fp32-state reward may be from the fp64 one (derived, not measured);
  sensitivity   how far the fp64 oracle's OWN observation moves when the state moves by one fp32 ulp: the reference alone decides
                which values are ill-conditioned;
  angle_bound / DIST_ULPS / LIDAR_*   the per-value bars of the observers, and check_observers, which applies them.
Nothing here looks at what a kernel returns to set a bar."""
import math

import numpy as np

import fp32_checks as fc
import oracle_lib as ol
from hive_transition_lib import _dist  # MyUtils.distance with libm's pow, element by element

TOL64 = 1e-9
EDGE_CLEARANCE = 1e-3     # px: a robot corner / ball centre nearer than this to a goal-triangle edge is a knife edge for contains_point
MAX_LEFT_OUT = 0.01       # share of arenas the DontDriveInGoals knife edge may remove
LIDAR_P99 = 2e-3          # the project's bar for fp32 observations: test_gpu_fp32.py::test_f32_config2_rollout_vs_f64_oracle
LIDAR_GROSS, LIDAR_ILL = 1.0, 0.1   # px: no lidar value off by more than 1 px unless the reference's own value moves by more than 0.1 px
MAX_ILL = 0.005           # share of lidar values the reference may call ill-conditioned
DIST_ULPS = 4             # a point distance: within 4 ulp32(diag)
COUNT_KEEPERS = (1, 4, 5)  # NaughtyBots, DontDriveInGoals, KeepMovingGuys: -.005 per robot


def r32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def ulp32(x):
    return float(np.spacing(np.float32(x)))


def diag(cfg):
    return math.hypot(cfg["W"], cfg["H"])


def counts(preset):
    cfg = ol.PRESETS[preset]
    return cfg["nr_h"], cfg["nr_h"] + cfg["nr_g"], cfg["nb_p"], cfg["nb_p"] + cfg["nb_n"]


# ------------------------------------------------------------------------------------------------------------------ states
def golden_states(golden_dir, preset, cap=1500, files=("mix", "traj")):
    """Pre-step states of the reference's recorded steps (tests/golden/{mix,traj}_<preset>.npz), strided to at most `cap` arenas:
    dict robots [n,NR,10], robots_i [n,NR,3], balls [n,NB,8], step [n]."""
    parts = {k: [] for k in ("robots", "robots_i", "balls", "step")}
    for f in files:
        t = np.load(f"{golden_dir}/{f}_{preset}.npz")
        for ep in range(t["length"].shape[0]):
            L = int(t["length"][ep])
            for k in parts:
                parts[k].append(t["state_" + k][ep, :L])
    st = {k: np.concatenate(v) for k, v in parts.items()}
    n = len(st["step"])
    sel = np.arange(0, n, max(1, -(-n // cap)))
    return {k: np.ascontiguousarray(v[sel]) for k, v in st.items()}


def mix_steps(golden_dir, preset, which, cap=1500):
    """The recorded steps of one keeper stack (which: 0 = A, 1 = B) of mix_<preset>.npz in which every robot got an action:
    (state dict, actions int32 [n,NR], stack in class order, program in execution order)."""
    import json
    t = np.load(f"{golden_dir}/mix_{preset}.npz")
    meta = json.loads(str(t["meta"]))
    name = "AB"[which]
    nr = t["state_robots"].shape[2]
    idx = [(ep, s) for ep in np.nonzero(t["which"] == which)[0] for s in range(int(t["length"][ep])) if (t["actions"][ep, s] >= 0).sum() == nr]
    idx = idx[::max(1, -(-len(idx) // cap))]
    ep = np.array([i[0] for i in idx]); s = np.array([i[1] for i in idx])
    st = {k: np.ascontiguousarray(t["state_" + k][ep, s]) for k in ("robots", "robots_i", "balls", "step")}
    return st, t["actions"][ep, s].astype(np.int32), tuple(meta["programs_mro"][name]), list(meta["programs_exec"][name])


def clean_states(preset, robots_xyr, balls_xyv, step=0):
    """Full state rows of crafted arenas: the oracle builds the derived fields from centres, rotations and ball velocities."""
    out = {k: [] for k in ("robots", "robots_i", "balls")}
    for r, b in zip(robots_xyr, balls_xyv):
        o = ol.OracleEnv(preset)
        o.set_clean_state(r, b, step)
        st = o.get_state()
        for k in out:
            out[k].append(st[k])
    out = {k: np.array(v) for k, v in out.items()}
    out["step"] = np.full(len(robots_xyr), step, np.int32)
    return out


def blocked_arenas(preset):
    """Crafted arenas in which robot 0 PROVABLY does not move under FORWARD (action 0 for every robot): it faces a side wall with its
    front edge on the clamp line (0.5 px from the wall), at rotation 0 (cos = 1, sin = 0 exactly) or 180 (cos = -1 exactly; sin = 1.2e-16
    is absorbed by the top edge).  Each of its 12 moves shifts the rect by exactly 1 px, crosses the wall, and is taken back by the exact
    opposite shift (Robot._move_linear, RR_Robot.py:181-203) -- in fp64 and in fp32 alike, all values being small multiples of 0.5.  So
    KeepMovingGuys' `==` fires for it in either arithmetic.  Two of the six stand inside the happy goal (DontDriveInGoals fires too,
    every corner more than 1 px from an edge).  The other robots stand mid-field and drive; the balls lie out of everybody's way."""
    cfg = ol.PRESETS[preset]
    nrh, nr, nbp, nb = counts(preset)
    W, H = cfg["W"], cfg["H"]
    rob, bal = [], []
    for x, rot, y in ((W - 10.5, 0.0, H / 2 - 100), (W - 10.5, 0.0, H / 2 - 50), (10.5, 180.0, H / 2 + 30), (10.5, 180.0, H / 2 + 90),
                      (W - 10.5, 0.0, H - 100.0), (W - 10.5, 0.0, H - 60.0)):
        r = [[x, y, rot]] + [[200.0, 60.0 + 90.0 * k, 0.0] for k in range(1, nr)]
        b = [[400.0, 40.0 + 40.0 * j, 0.0, 0.0] for j in range(nb)]
        rob.append(r); bal.append(b)
    st = clean_states(preset, np.array(rob), np.array(bal))
    return st, np.zeros((len(rob), nr), np.int32)


def concat_states(a, b):
    return {k: np.concatenate([a[k], b[k]]) for k in a}


REWARD_CASES = ("A", "B", "DontDrive")


def reward_case(golden_dir, preset, case, cap=1500):
    """One step's inputs of a reward check: (state dict, actions, stack in class order, program in execution order, number of blocked
    arenas at the end).  "A" / "B": the two stacks of mix_<preset>.npz on their own recorded states.  "DontDrive": DontDriveInGoals
    alone on stack A's states -- in the reference stack B loses it to NaughtyBots' missing super(), and in stack A the distance keepers'
    bound (0.2 to 1) hides a -.005 that fired wrongly, so only a count-keeper-only program holds it to n x ulp32(.005).  Every case ends
    with blocked_arenas()."""
    st, acts, stack, prog = mix_steps(golden_dir, preset, 0 if case in ("A", "DontDrive") else 1, cap)
    if case == "DontDrive":
        stack, prog = ("DontDriveInGoals",), [4]
    bst, bacts = blocked_arenas(preset)
    return concat_states(st, bst), np.concatenate([acts, bacts]), stack, prog, len(bacts)


def oracle_at(preset, st, i):
    o = ol.OracleEnv(preset)
    o.set_state(st["robots"][i], st["robots_i"][i], st["balls"][i], None, int(st["step"][i]))
    return o


# ------------------------------------------------------------------------------------------------------------------ geometry
def robot_corners(cx, cy, rot):
    """FloatRect corners of a 20 x 40 robot (MyUtils.py:132-139, 277-316): the initial corners (+-10, +-20), unrotated when the rotation
    is 0, else turned by radians(360 - rot) and rescaled to the corner distance.  -> [..., 4, 2]"""
    cx, cy, rot = (np.asarray(v, np.float64) for v in (cx, cy, rot))
    rad = np.radians(360.0 - rot)
    c, s = np.cos(rad), np.sin(rad)
    cd = math.pow(10.0 ** 2 + 20.0 ** 2, .5)
    out = np.zeros(cx.shape + (4, 2))
    for k, (ix, iy) in enumerate(((-10.0, -20.0), (10.0, -20.0), (-10.0, 20.0), (10.0, 20.0))):
        qx, qy = ix * c - iy * s, ix * s + iy * c
        d = np.sqrt(qx * qx + qy * qy)
        out[..., k, 0] = cx + np.where(rot == 0, ix, qx * cd / d)
        out[..., k, 1] = cy + np.where(rot == 0, iy, qy * cd / d)
    return out


def tri_contains(happy, W, H, x, y):
    """RightTriangle.contains_point (MyUtils.py:438-445) of Goal.triShape (RR_Goal.py:14-28): inside the bounding box and
    Div0 slope from tplHyp0 >= the hypotenuse's slope (-1).  happy: (W,H),(W,H-240),(W-240,H), tplHyp0 = (W-240, H);
    grumpy: (240,0),(0,240),(0,0), tplHyp0 = (240, 0)."""
    l, r, t, b = (W - 240.0, W, H - 240.0, H) if happy else (0.0, 240.0, 0.0, 240.0)
    h0x, h0y = (l, b) if happy else (r, t)
    box = (l <= x) & (x <= r) & (t <= y) & (y <= b)
    num, den = y - h0y, x - h0x
    with np.errstate(divide="ignore", invalid="ignore"):
        sp = np.where(den != 0, num / np.where(den != 0, den, 1.0), np.where(num > 0, np.inf, -np.inf))
    return box & (sp >= -1.0) & ~((den == 0) & (num == 0))  # (0 / 0 raises in the reference: no golden state is there)


def tri_edge_distance(W, H, x, y):
    """distance of points to the nearest edge (segment) of either goal triangle"""
    def seg(ax, ay, bx, by):
        vx, vy = bx - ax, by - ay
        t = np.clip(((x - ax) * vx + (y - ay) * vy) / (vx * vx + vy * vy), 0.0, 1.0)
        return np.hypot(x - (ax + t * vx), y - (ay + t * vy))
    d = np.full(np.shape(x), np.inf)
    for tri in (((W, H), (W, H - 240.0), (W - 240.0, H)), ((240.0, 0.0), (0.0, 240.0), (0.0, 0.0))):
        for k in range(3):
            d = np.minimum(d, seg(*tri[k], *tri[(k + 1) % 3]))
    return d


def corner_clearance(preset, robots):
    """per arena: the smallest distance of any robot corner to a goal-triangle edge (robots [n,NR,>=7])"""
    cfg = ol.PRESETS[preset]
    c = robot_corners(robots[..., 0], robots[..., 1], robots[..., 6])
    return tri_edge_distance(cfg["W"], cfg["H"], c[..., 0], c[..., 1]).reshape(len(robots), -1).min(axis=1)


# ------------------------------------------------------------------------------------------------------------------ keepers
def keepers_ref(preset, program, pre, post, naughty):
    """RR_ScoreKeepers.py in numpy fp64.  pre / post: state dicts (robots [n,NR,>=7], balls [n,NB,>=2]) at on_step_begin / on_step_end;
    naughty [n]: NaughtyBots' set as a bit per robot (status bits 16+); program: keeper ids in on_step_end execution order (1 NaughtyBots,
    2 ChasePosBall, 3 PushPosBallsToGoal, 4 DontDriveInGoals, 5 KeepMovingGuys, 6 BaseDestruction, 7 PushNegBallsFromGoal).
    -> (reward_happy [n], reward_grumpy [n]).

    From the reference's text:
      * rectDblPriorStep is FloatRect.copy() at on_step_begin: a new rect (0,20,0,40) moved to the centre, 10 + (x - 10), 20 + (y - 20)
        (MyUtils.py:150-154, 264-275), rotation (rot + 720) % 360;
      * ChasePosBall (:53-66): for each robot of a team, each POSITIVE ball: (distance(prior centre, ball NOW) - distance(centre, ball
        NOW)) * POINTS_ROBOT_TRAVEL_MULT, accumulated term by term;
      * PushPosBallsToGoal (:138-157): (sum of distance((0,0), positive ball) now - the same sum at on_step_begin) * POINTS_BALL_TRAVEL_MULT,
        + for happy, - for grumpy; PushNegBallsFromGoal (:160-179) sums lstPosBalls as well (sic), signs swapped;
      * DontDriveInGoals (:69-81): -.005 per robot with a corner inside either goal triangle; KeepMovingGuys (:84-96): -.005 per robot
        whose centre and rotation EQUAL the prior-step copy's; NaughtyBots (:130-135): -.005 per robot of its set;
      * BaseDestruction (:99-109): pays only when a goal is destroyed, which the live path never does (goals are never fed)."""
    cfg = ol.PRESETS[preset]
    nrh, nr, nbp, nb = counts(preset)
    W, H = cfg["W"], cfg["H"]
    mb = 200000.0 / math.pow(W * W + H * H, .5)
    mr = mb / 100
    r0, b0, r1, b1 = (np.asarray(x, np.float64) for x in (pre["robots"], pre["balls"], post["robots"], post["balls"]))
    n = len(r0)
    px, py = 10.0 + (r0[..., 0] - 10.0), 20.0 + (r0[..., 1] - 20.0)
    prot = np.mod(r0[..., 6] + 720.0, 360.0)
    zero = np.zeros(n)

    def dist_sum(b):
        s = np.zeros(n)
        for j in range(nbp):
            s = s + _dist(zero, zero, b[:, j, 0], b[:, j, 1])
        return s
    sum0 = dist_sum(b0)
    rew = [np.zeros(n), np.zeros(n)]  # happy, grumpy

    def add(team, v):
        rew[team] = rew[team] + v
    naughty = np.asarray(naughty, np.int64)
    for k in program:
        if k == 1:
            for r in range(nr):
                add(int(r >= nrh), np.where((naughty >> r) & 1, -.005, 0.0))
        elif k == 2:
            for r in range(nr):
                for j in range(nbp):
                    now = _dist(r1[:, r, 0], r1[:, r, 1], b1[:, j, 0], b1[:, j, 1])
                    prior = _dist(px[:, r], py[:, r], b1[:, j, 0], b1[:, j, 1])
                    add(int(r >= nrh), (prior - now) * mr)
        elif k in (3, 7):
            delta = dist_sum(b1) - sum0
            sgn = 1.0 if k == 3 else -1.0
            add(0, sgn * (delta * mb)); add(1, -sgn * (delta * mb))
        elif k == 4:
            c = robot_corners(r1[..., 0], r1[..., 1], r1[..., 6])
            inside = (tri_contains(True, W, H, c[..., 0], c[..., 1]) | tri_contains(False, W, H, c[..., 0], c[..., 1])).any(axis=-1)
            for r in range(nr):
                add(int(r >= nrh), np.where(inside[:, r], -.005, 0.0))
        elif k == 5:
            still = (r1[..., 0] == px) & (r1[..., 1] == py) & (r1[..., 6] == prot)
            for r in range(nr):
                add(int(r >= nrh), np.where(still[:, r], -.005, 0.0))
        elif k != 6:
            raise KeyError(k)
    return rew[0], rew[1]


def reward_bound(preset, program, mode):
    """How far the reward of a keeper stack may be from keepers_ref / the fp64 oracle, per team: (bound_happy, bound_grumpy).
    It generalises hive_transition_lib.fp32_bound (16 x 2^-24 x diag x mult for its two distance terms: 8 roundings a term).

    mode "f32" (state and arithmetic in fp32; both sides read the SAME fp32 state, so only the arithmetic differs).  u = 2^-24.
      A distance of two fp32 points, d = sqrt(dx^2 + dy^2) <= diag: dx, dy are rounded differences (relative u each, hence u on d), the
      two squares and their sum add u/2 each ... at most u on d together, the root u/2, its own error doubling nothing: <= 3 u diag.
      * ChasePosBall, one term = two distances, their difference and its product and accumulation: 2 x 3 + 2 = 8 roundings of at most
        u x diag, times POINTS_ROBOT_TRAVEL_MULT.  Terms of a team: its robots x NBP.
      * PushPos / PushNeg: a term = one positive ball's distance in the sum at on_step_begin and in the sum at on_step_end (2 x 3), and the
        two running sums, whose k-th partial sum is <= k diag, rounded to u k diag: over NBP balls u diag NBP (NBP + 1) / 2 per sum, i.e.
        (NBP + 1) per ball for the two sums: 6 + NBP + 1 roundings a term (8 for one ball), times POINTS_BALL_TRAVEL_MULT.  NBP terms each,
        and both keepers reach both teams.
        The product and the accumulation round relative to their RESULT; counting each as u x diag x mult is safe because a term is a
        per-step travel (a robot moves at most 12 px a step, a ball a few tens) times mult, and the running sum of all terms of a step
        stays far below diag x mult, the scale the distance roundings are counted at.
      * the count keepers (-.005 per robot): .005 is not an fp32 number and every subtraction rounds: ulp32(.005) per possible decrement,
        n = robots of the team x count keepers in the program.  They add nothing else: a program of count keepers alone is held to
        n x ulp32(.005).
    mode "f32_state" (fp32 records, fp64 arithmetic): the arithmetic adds nothing (1e-9).  The keepers read the STORED post-state, which
      is the step's fp64 result rounded to fp32: each coordinate moves by at most half an fp32 ulp at the longer side, hs = ulp32(max(W,
      H)) / 2, and a distance moves by at most the sum of the moves of the coordinates it reads (|d dist| <= |d dx| + |d dy|).
      * ChasePosBall: `now` reads the robot's and the ball's post centre (4 coordinates), `prior` the ball's (2): 6 hs a term x mult_robot;
      * PushPos / PushNeg: the sum at on_step_end reads the ball's post centre: 2 hs a term x mult_ball (the sum at on_step_begin reads the
        state that was set: exact);
      * the count keepers: nothing (the same comparisons on the same stored numbers; .005 is the same double).
      Against keepers_ref on the handle's own stored pre / post state even this rounding is absent; the bound is the same one by the
      issue's wording and is then simply not tight."""
    cfg = ol.PRESETS[preset]
    nrh, nr, nbp, nb = counts(preset)
    d = diag(cfg)
    mb = 200000.0 / d
    mr = mb / 100
    u = 2.0 ** -24
    out = []
    for team_n in (nrh, nr - nrh):
        n_chase = team_n * nbp * sum(1 for k in program if k == 2)
        n_push = nbp * sum(1 for k in program if k in (3, 7))
        n_count = team_n * sum(1 for k in program if k in COUNT_KEEPERS)
        if mode == "f32":
            b = n_chase * 8 * u * d * mr + n_push * (6 + nbp + 1) * u * d * mb + n_count * ulp32(.005)
        elif mode == "f32_state":
            hs = ulp32(max(cfg["W"], cfg["H"])) / 2
            b = n_chase * 6 * hs * mr + n_push * 2 * hs * mb + TOL64
        else:
            raise KeyError(mode)
        out.append(b)
    return out[0], out[1]


def check_rewards(tag, preset, prog, mode, pre, post, naughty, rew, n_blocked):
    """rew [n,2] (happy, grumpy) of a handle / the emulation against keepers_ref on ITS OWN pre / post state and NaughtyBots bits, within
    reward_bound(mode).  fp32 arithmetic and DontDriveInGoals in the program: an arena with a robot corner within EDGE_CLEARANCE of a
    goal-triangle edge is left out (contains_point is a knife edge there; the reference's geometry decides), at most MAX_LEFT_OUT of them.
    The last n_blocked arenas are blocked_arenas(): their robot 0 must not have moved, so that KeepMovingGuys' `==` fired."""
    rh, rg = keepers_ref(preset, prog, pre, post, naughty)
    bh, bg = reward_bound(preset, prog, mode)
    keep = np.ones(len(rh), bool)
    if 4 in prog and mode == "f32":
        keep = corner_clearance(preset, post["robots"]) >= EDGE_CLEARANCE
        assert (~keep).mean() <= MAX_LEFT_OUT, (tag, float((~keep).mean()))
        assert keep[-n_blocked:].all()
    eh, eg = np.abs(rew[:, 0] - rh), np.abs(rew[:, 1] - rg)
    print(f"[{tag}] {int(keep.sum())} arenas ({int((~keep).sum())} left out): |reward - keepers_ref| max {eh[keep].max():.3e} (happy, bound "
          f"{bh:.3e}), {eg[keep].max():.3e} (grumpy, bound {bg:.3e})")
    assert (eh[keep] <= bh).all(), (tag, "happy", float(eh[keep].max()))
    assert (eg[keep] <= bg).all(), (tag, "grumpy", float(eg[keep].max()))
    tail = lambda d: {k: v[-n_blocked:] for k, v in d.items()}
    if 5 in prog:  # the blocked robots: KeepMovingGuys fires on equality, in fp32 as in fp64
        assert (keepers_ref(preset, [5], tail(pre), tail(post), np.zeros(n_blocked, int))[0] <= -.005).all(), tag
    if 4 in prog:  # DontDriveInGoals is really exercised both ways: it fires for the two blocked robots inside the happy goal and in some of
        # the recorded arenas, and stays silent in others
        fired = keepers_ref(preset, [4], pre, post, np.zeros(len(rh), int))
        fired = (fired[0] < 0) | (fired[1] < 0)
        assert fired[-2:].all() and not fired[-n_blocked:-2].any() and 0 < fired[:-n_blocked][keep[:-n_blocked]].sum() < keep[:-n_blocked].sum(), tag


# ------------------------------------------------------------------------------------------------------------------ observers
def observer_queries(preset):
    """(kind, team, robot, ball) for the observers V2 (0), V1 (1) and Basic (2): every robot, balls 0 and NB-1, both teams.  (Basic looks
    at lstPosBalls[0] whatever ball it is asked about, RR_Observers.py:133-144: asking it about ball NB-1 pins that.)"""
    nrh, nr, nbp, nb = counts(preset)
    q = [(kind, team, r, b) for kind in (0, 1, 2) for team in (1, -1) for r in range(nr) for b in sorted({0, nb - 1})]
    return q + [(kind, team, -1, -1) for kind in (0, 1, 2) for team in (1, -1)]  # the defaults: None where the team has no robot


def lidar_queries(preset):
    """one query per (kind, robot): the lidar values of an observation depend on neither the ball nor the team asking"""
    return [(kind, 1, r, 0) for kind in (0, 1, 2) for r in range(counts(preset)[1])]


def lidar_sensitivity(preset, st, n_pert=16, seed=0):
    """sensitivity() of lidar_queries, keyed (kind, robot)"""
    q = lidar_queries(preset)
    return {(k, r): v for (k, _, r, _), v in zip(q, sensitivity(preset, st, q, n_pert, seed))}


def oracle_observations(preset, st, queries, i):
    o = oracle_at(preset, st, i)
    return [o.observe_kind(k, t, r, b) for k, t, r, b in queries]


def nudge32(x, k):
    """x (fp32-representable) moved by k in {-1, 0, +1} fp32 ulps"""
    x32 = np.asarray(x, np.float32)
    up, dn = np.nextafter(x32, np.float32(np.inf)), np.nextafter(x32, np.float32(-np.inf))
    return np.where(k > 0, up, np.where(k < 0, dn, x32)).astype(np.float64)


def sensitivity(preset, st, queries, n_pert=16, seed=0):
    """The largest shift of each of the fp64 oracle's own observation values over `n_pert` seeded perturbations of the state, each moving
    every centre and every rotation by -1, 0 or +1 fp32 ulp (OracleEnv.set_clean_state).  -> list over queries of [n, dim] arrays."""
    rng = np.random.default_rng(seed)
    n = len(st["step"])
    rob = r32(st["robots"][..., [0, 1, 6]])
    bal = np.concatenate([r32(st["balls"][..., :2]), st["balls"][..., 6:8]], axis=-1)
    out = None
    for i in range(n):
        o = ol.OracleEnv(preset)
        o.set_clean_state(rob[i], bal[i], int(st["step"][i]))
        base = [o.observe_kind(k, t, r, b) for k, t, r, b in queries]
        if out is None:
            out = [np.zeros((n, len(v))) for v in base]
        for _ in range(n_pert):
            rp = nudge32(rob[i], rng.integers(-1, 2, rob[i].shape))
            bp = bal[i].copy()
            bp[:, :2] = nudge32(bal[i][:, :2], rng.integers(-1, 2, (bal.shape[1], 2)))
            o.set_clean_state(rp, bp, int(st["step"][i]))
            for q, (k, t, r, b) in enumerate(queries):
                v = o.observe_kind(k, t, r, b)
                d = np.abs(v - base[q])
                ang = angle_columns(k)
                d[ang] = np.abs((v[ang] - base[q][ang] + 180.0) % 360.0 - 180.0)  # angles: on the circle
                out[q][i] = np.maximum(out[q][i], d)
    return out


def angle_columns(kind):
    return [0, 1, 3] if kind in (0, 1) else [0, 1]


def dist_columns(kind):
    return [2, 4] if kind in (0, 1) else [2]


def lidar_columns(kind):
    return list(range(5, 11)) if kind in (0, 1) else [3, 4]


def angle_bound(cfg, d):
    """An fp32 angle (MyUtils.angle_degrees: atan of the quotient of two rounded differences, to degrees, + 360 and % 360, + 180 and % 360
    when the view is turned round) against the fp64 one, compared on the circle:
      * the two points are the same fp32 numbers on both sides; dx and dy are each rounded once, by at most ulp32(diag) / 2, which moves
        the direction by at most |(ddx, ddy)| / d <= ulp32(diag) / d radians; the quotient and the arc tangent's own error are relative
        to a result <= pi / 2 and stay below the same again: 2 ulp32(diag) / d radians in all, d the fp64 distance of the two points;
      * the result is a number of degrees < 360 rounded at each of up to four steps (degrees(), + 360, %, the turn): each at most
        ulp32(360) / 2 ... 4 ulp32(360) with the output's own rounding.
    A robot's own rotation (column 0) has no direction term: pass d = inf."""
    return 4 * ulp32(360.0) + np.degrees(2 * ulp32(diag(cfg)) / np.asarray(d, np.float64))


def check_observers(tag, preset, st, queries, got, ref, sens):
    """got / ref: lists over `queries` of [n, dim] arrays (fp32-mode result, fp64 oracle on the same state); sens: lidar_sensitivity().
    Asserts the per-value conditions of the fp32 observers and returns the measured figures (dict)."""
    cfg = ol.PRESETS[preset]
    dg = diag(cfg)
    rob, bal = st["robots"], st["balls"]
    lid_rel, lid_abs, lid_sens = [], [], []
    worst_ang = worst_dist = 0.0
    nrh = counts(preset)[0]
    for q, (kind, team, r, b) in enumerate(queries):
        assert (got[q] is None) == (ref[q] is None), (tag, queries[q], "None exactly where the reference returns None")
        if ref[q] is None:
            continue
        r, b = (r if r >= 0 else (0 if team == 1 else nrh)), (0 if kind == 2 else max(b, 0))
        g, f = np.asarray(got[q], np.float64), np.asarray(ref[q], np.float64)
        assert g.shape == f.shape and np.isfinite(g).all(), (tag, queries[q])
        d_ball = np.hypot(rob[:, r, 0] - bal[:, b, 0], rob[:, r, 1] - bal[:, b, 1])
        d_goal = np.hypot(rob[:, r, 0] - cfg["W"], rob[:, r, 1] - cfg["H"])
        for col, d in zip(angle_columns(kind), (np.inf, d_ball, d_goal)):
            err = np.abs((g[:, col] - f[:, col] + 180.0) % 360.0 - 180.0)
            bound = angle_bound(cfg, d) * np.ones(len(err))
            worst_ang = max(worst_ang, float((err / bound).max()))
            assert (err <= bound).all(), (tag, "angle", queries[q], col, float(err.max()), int(np.argmax(err / bound)))
        for col in dist_columns(kind):
            err = np.abs(g[:, col] - f[:, col])
            worst_dist = max(worst_dist, float(err.max()) / ulp32(dg))
            assert (err <= DIST_ULPS * ulp32(dg)).all(), (tag, "distance", queries[q], col, float(err.max()))
        lc = lidar_columns(kind)
        lid_rel.append(fc.rel_err(g[:, lc], f[:, lc]))
        lid_abs.append(np.abs(g[:, lc] - f[:, lc]).ravel())
        lid_sens.append(sens[(kind, r)][:, lc].ravel())
    lid_rel, lid_abs, lid_sens = np.concatenate(lid_rel), np.concatenate(lid_abs), np.concatenate(lid_sens)
    ill = lid_sens > LIDAR_ILL
    relative = lid_abs / np.maximum(lid_sens, ulp32(dg))
    fig = dict(lidar_p99_rel=float(np.percentile(lid_rel, 99)), lidar_max_abs=float(lid_abs.max()), ill_share=float(ill.mean()),
               sens_max=float(lid_sens.max()), ref_relative_p99=float(np.percentile(relative, 99)), ref_relative_max=float(relative.max()),
               angle_worst_of_bound=worst_ang, dist_worst_ulps=worst_dist, values=int(lid_abs.size))
    print(f"[{tag}] fp32 observers vs the fp64 oracle on the same state: angles at most {worst_ang:.2f} of their bound, point distances at most "
          f"{worst_dist:.2f} ulp32(diag); {lid_abs.size} lidar values: p99 rel err {fig['lidar_p99_rel']:.2e}, max abs {fig['lidar_max_abs']:.2e} px; "
          f"the reference's own largest shift {fig['sens_max']:.2e} px, {100 * fig['ill_share']:.3f} % ill-conditioned; error / max(sensitivity, "
          f"ulp32(diag)): p99 {fig['ref_relative_p99']:.2f}, max {fig['ref_relative_max']:.2f}")
    assert fig["ill_share"] <= MAX_ILL, (tag, fig["ill_share"])
    assert fig["lidar_p99_rel"] < LIDAR_P99, (tag, fig["lidar_p99_rel"])
    gross = (lid_abs > LIDAR_GROSS) & ~ill
    assert not gross.any(), (tag, "lidar off by more than 1 px where the reference is well conditioned", int(gross.sum()), float(lid_abs[gross].max()))
    return fig


# ------------------------------------------------------------------------------------------------------------------ goal scoring
def goal_batch(n=256, seed=3):
    """The crafted batch of tests/test_gpu_goal.py (preset T): one ball per arena in or around either goal triangle, the robot mid-field,
    nobody moves; rounded to fp32 as an fp32 handle holds it, every ball centre at least EDGE_CLEARANCE from every triangle edge."""
    rng = np.random.default_rng(seed)
    robots = np.tile(np.array([[[300.0, 300.0, 0.0]]]), (n, 1, 1))
    balls = np.zeros((n, 1, 4))
    for a in range(n):
        if a % 2:
            balls[a, 0, :2] = (rng.uniform(380, 590), rng.uniform(380, 590))
        else:
            balls[a, 0, :2] = (rng.uniform(10, 220), rng.uniform(10, 220))
    balls = r32(balls)
    assert tri_edge_distance(600.0, 600.0, balls[:, 0, 0], balls[:, 0, 1]).min() >= EDGE_CLEARANCE
    return robots, balls


def goal_oracle(st, steps):
    """The oracle's 150-step stay from the state a handle holds after set_poses: per arena the rewards, done, status words of every step
    it took (until STEP_AFTER_DONE), the goal scores and the final balls."""
    out = []
    for i in range(len(st["step"])):
        o = oracle_at("T", st, i)
        o.set_goal_scoring(True)
        rew, done, status = [], [], []
        for s in range(steps):
            res = o.step([8])
            status.append(res["status"])
            if res["status"] & 64:
                break
            rew.append(res["reward"]); done.append(res["done"])
        out.append(dict(reward=np.array(rew), done=np.array(done), status=np.array(status), scores=o.goal_scores(), balls=o.get_state()["balls"]))
    return out


def check_goal(tag, ora, reward, done, status, scores, balls):
    """reward / done / status [steps, n] of the handle (status: flag bits 0-15), scores [n,2], balls [n,1,8]: exact integer claims."""
    consumed = 0
    for a, o in enumerate(ora):
        k = len(o["reward"])
        assert np.array_equal(reward[:k, a], o["reward"]), (tag, a, "rewards")
        assert np.array_equal(done[:k, a].astype(bool), o["done"]), (tag, a, "done")
        assert np.array_equal(status[:len(o["status"]), a], o["status"]), (tag, a, "status", status[:len(o["status"]), a][-3:], o["status"][-3:])
        assert np.array_equal(o["scores"], scores[a]), (tag, a, "scores")
        assert np.array_equal(o["balls"], balls[a]), (tag, a, "parked ball")
        consumed += bool(o["done"].any())
    assert 40 < consumed < len(ora) - 40  # both outcomes are exercised
    assert set(np.unique(scores)) <= {0, 500}
    return consumed
