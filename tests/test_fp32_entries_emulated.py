"""CPU twin of tests/test_gpu_fp32_entries.py: whatever the host emulation EmuEnv(f32=True) -- the kernel source compiled with g++, every
Real a float -- can express of the fp32 handle's entries (observers, both reward stacks of the mix goldens, the thrust entry, goal
scoring) goes through the SAME helper functions and bars (tests/fp32_entry_checks.py), so the checks themselves are exercised without
a GPU; and the helpers are validated against golden files alone: keepers_ref against every recorded mix step, the exemption caps
(DontDriveInGoals knife edges, ill-conditioned lidar values) by the reference's own geometry and sensitivity.

The emulation has no fp32-STATE configuration (fp32 records with fp64 arithmetic): section 2 of the GPU file has no twin here."""
import json

import numpy as np
import pytest

import emu_lib as el
import fp32_checks as fc
import fp32_entry_checks as ec
import oracle_lib as ol

CAP = {"T": 500, "G": 160, "Dwide": 300, "D": 300}  # arenas per preset: one emulated wave and 17 oracle set-ups per arena, a few seconds


@pytest.mark.parametrize("preset", ["T", "G", "D", "X", "Dwide"])
def test_keepers_ref_equals_every_recorded_mix_step(golden_dir, preset):
    """keepers_ref (written from RR_ScoreKeepers.py) against the `reward` / `reward_g` of EVERY step of mix_<preset>.npz, both stacks,
    to 1e-7; the NaughtyBots set is the one OracleEnv.step reports for the step."""
    t = dict(np.load(f"{golden_dir}/mix_{preset}.npz"))  # (an NpzFile decompresses an array at every access)
    progs = json.loads(str(t["meta"]))["programs_exec"]
    seen = 0
    for which, name in ((0, "A"), (1, "B")):
        idx = [(ep, s) for ep in np.nonzero(t["which"] == which)[0] for s in range(int(t["length"][ep]))]
        ep = np.array([i[0] for i in idx]); s = np.array([i[1] for i in idx])
        naughty = np.zeros(len(idx), np.int64)
        for k, (e, q) in enumerate(idx):
            o = ol.OracleEnv(preset)
            o.set_state(t["state_robots"][e, q], t["state_robots_i"][e, q], t["state_balls"][e, q], t["state_inner"][e, q], t["state_step"][e, q])
            a = t["actions"][e, q]
            naughty[k] = o.step(a[a >= 0])["naughty"]
        pre = dict(robots=t["state_robots"][ep, s], balls=t["state_balls"][ep, s])
        post = dict(robots=t["state_robots"][ep, s + 1], balls=t["state_balls"][ep, s + 1])
        rh, rg = ec.keepers_ref(preset, progs[name], pre, post, naughty)
        assert np.abs(rh - t["reward"][ep, s]).max() < 1e-7, (preset, name, float(np.abs(rh - t["reward"][ep, s]).max()))
        assert np.abs(rg - t["reward_g"][ep, s]).max() < 1e-7, (preset, name)
        seen += len(idx)
        for k in (4, 5):  # DontDriveInGoals and KeepMovingGuys really fire in some recorded step of their stack, and not in every one
            if k in progs[name]:  # (NaughtyBots needs two robots to collide, and T has one)
                fh, fg = ec.keepers_ref(preset, [k], pre, post, naughty)
                fired = (fh < 0) | (fg < 0)
                print(f"[{preset} stack {name}] keeper {k} fires in {int(fired.sum())} of {len(fired)} recorded steps")
                assert 0 < fired.sum() < len(fired), (preset, name, k, int(fired.sum()))
    assert seen == int(t["length"].sum())


@pytest.mark.parametrize("preset", ["T", "G", "Dwide"])
def test_dont_drive_knife_edges_stay_under_the_cap(golden_dir, preset):
    """The condition of the DontDriveInGoals exemption, by the reference's geometry alone: of the recorded post-step states the reward
    checks use, at most 1 % have a robot corner within 1e-3 px of a goal-triangle edge."""
    for which in (0, 1):
        t = dict(np.load(f"{golden_dir}/mix_{preset}.npz"))
        post = np.concatenate([t["state_robots"][ep, 1:int(t["length"][ep]) + 1] for ep in np.nonzero(t["which"] == which)[0]])
        near = ec.corner_clearance(preset, ec.r32(post)) < ec.EDGE_CLEARANCE
        print(f"[{preset} stack {'AB'[which]}] {int(near.sum())} of {len(near)} recorded post-states within {ec.EDGE_CLEARANCE} px of a goal edge")
        assert near.mean() <= ec.MAX_LEFT_OUT
    st, _ = ec.blocked_arenas(preset)
    assert ec.corner_clearance(preset, st["robots"]).min() > 0.4  # the crafted ones: the leg on the wall is 0.5 px away, the rest further


def _emu_observations(preset, st, queries, i):
    e = el.EmuEnv(preset, f32=True)
    e.set_state(st["robots"][i], st["robots_i"][i], st["balls"][i], int(st["step"][i]))
    return e, [e.observe(t, r, b) if k == 0 else e.observe_kind(k, t, r, b) for k, t, r, b in queries]


@pytest.mark.parametrize("preset", ["T", "G", "Dwide"])
def test_emulated_f32_observers_vs_oracle_on_the_same_state(golden_dir, preset):
    """V2, V1 and Basic of the fp32 kernel source, every robot / ball 0 and NB-1 / both teams, no step, against the fp64 oracle on the
    state the fp32 build holds: fp32_entry_checks.check_observers.  AllCoords: bit-equal to that state.  The reference's own
    sensitivity is rechecked here: on the golden G and T states no lidar value is ill-conditioned (largest shift 1.9e-2 px)."""
    st = ec.golden_states(golden_dir, preset, CAP[preset])
    st = {k: (ec.r32(v) if v.dtype == np.float64 else v) for k, v in st.items()}
    queries = ec.observer_queries(preset)
    nrh, nr, nbp, nb = ec.counts(preset)
    n = len(st["step"])
    got, ref = None, None
    for i in range(n):
        e, g = _emu_observations(preset, st, queries, i)
        held = e.get_state()
        assert np.array_equal(held["robots"][:, [0, 1, 6]], st["robots"][i][:, [0, 1, 6]]) and np.array_equal(held["balls"][:, :2], st["balls"][i][:, :2])
        f = ec.oracle_observations(preset, st, queries, i)
        assert [x is None for x in g] == [x is None for x in f]
        if got is None:
            got, ref = ([None if x is None else np.zeros((n, len(x))) for x in f] for _ in range(2))
        for q in range(len(queries)):
            if f[q] is not None:
                got[q][i], ref[q][i] = g[q], f[q]
        for team in (1, -1):  # AllCoords: own team first
            own = list(range(nrh)) if team == 1 else list(range(nrh, nr))
            order = own + [r for r in range(nr) if r not in own]
            want = np.concatenate([st["robots"][i][order][:, [0, 1, 6]].ravel(), st["balls"][i][:, :2].ravel()])
            assert np.array_equal(e.observe_kind(3, team), want), (preset, i, team)
    sens = ec.lidar_sensitivity(preset, st)
    fig = ec.check_observers(f"{preset} emulated", preset, st, queries, got, ref, sens)
    if preset in ("T", "G"):
        assert fig["sens_max"] <= ec.LIDAR_ILL and fig["ill_share"] == 0.0, fig  # none is exempt on the golden states


@pytest.mark.parametrize("case", ec.REWARD_CASES)
@pytest.mark.parametrize("preset", ["T", "G", "Dwide"])
def test_emulated_f32_reward_stacks_vs_keepers_ref(golden_dir, preset, case):
    """Both keeper stacks of the mix goldens, and DontDriveInGoals alone, on the fp32 kernel source, one step from recorded states plus
    the blocked arenas: the reward against keepers_ref on the build's own pre / post state and NaughtyBots set, within reward_bound
    (stack B and DontDriveInGoals: n x ulp32(.005))."""
    st, acts, _, prog, n_blocked = ec.reward_case(golden_dir, preset, case, CAP[preset])
    n = len(acts)
    pre = {k: np.zeros_like(st[k]) for k in ("robots", "balls")}
    post = {k: np.zeros_like(st[k]) for k in ("robots", "balls")}
    rew, naughty = np.zeros((n, 2)), np.zeros(n, np.int64)
    for i in range(n):
        e = el.EmuEnv(preset, f32=True)
        e.set_program(prog)
        e.set_state(st["robots"][i], st["robots_i"][i], st["balls"][i], int(st["step"][i]))
        h = e.get_state()
        pre["robots"][i], pre["balls"][i] = h["robots"], h["balls"]
        r = e.step(acts[i])
        h = e.get_state()
        post["robots"][i], post["balls"][i] = h["robots"], h["balls"]
        rew[i], naughty[i] = (r["reward"], r["reward_g"]), r["naughty"]
    ec.check_rewards(f"{preset} stack {case} emulated", preset, prog, "f32", pre, post, naughty, rew, n_blocked)


@pytest.mark.parametrize("preset", ["T", "G", "D"])
def test_emulated_f32_thrust_entry_distribution(golden_dir, preset):
    """The thrust entry of the fp32 kernel source on the reference's GameEnv.step vectors (thrust_*.npz), scored by fp32_checks.score
    and held to the bars rr_step meets in this mode (fp32_checks.assert_distribution, as in test_gpu_fp32.py)."""
    pre, post, got, done_ok = _thrust_through(golden_dir, preset, lambda: el.EmuEnv(preset, f32=True))
    cfg = ol.PRESETS[preset]
    q, e, ints = fc.score(pre, post, got, cfg["W"], cfg["H"])
    fc.assert_distribution(f"{preset} thrust emulated", q, e, ints, done_ok)


def _thrust_through(golden_dir, preset, make):
    t = dict(np.load(f"{golden_dir}/thrust_{preset}.npz"))
    idx = [(ep, s) for ep in range(t["length"].shape[0]) for s in range(int(t["length"][ep]))]
    ep = np.array([i[0] for i in idx]); s = np.array([i[1] for i in idx])
    pre = {k: t["state_" + k][ep, s] for k in ("robots", "robots_i", "balls", "step")}
    post = {k: t["state_" + k][ep, s + 1] for k in ("robots", "robots_i", "balls", "step")}
    got = {k: np.zeros_like(post[k]) for k in ("robots", "robots_i", "balls")}
    done_ok = np.zeros(len(idx), bool)
    for i in range(len(idx)):
        e = make()
        e.set_state(pre["robots"][i], pre["robots_i"][i], pre["balls"][i], int(pre["step"][i]))
        th = t["thrust"][ep[i], s[i]]
        r = e.step_thrust(th[~np.isnan(th[:, 0])])
        h = e.get_state()
        for k in got:
            got[k][i] = h[k]
        done_ok[i] = r["done"] == bool(t["done"][ep[i], s[i]])
    return pre, post, got, done_ok


def test_emulated_f32_goal_scoring_equals_the_oracle():
    """Opt-in goal scoring on the fp32 kernel source: the crafted batch of test_gpu_goal.py (balls in and around both triangles, no centre
    within 1e-3 px of an edge), 150-step stay and ten more: rewards (+-500), done, status words, goal scores and the parked balls equal the
    oracle's from the same fp32 state, exactly."""
    steps = 160
    robots, balls = ec.goal_batch(128)
    n = len(robots)
    st = {k: [] for k in ("robots", "robots_i", "balls")}
    rew, done, status = np.zeros((steps, n)), np.zeros((steps, n), bool), np.zeros((steps, n), np.int64)
    scores, fin = np.zeros((n, 2), np.int32), np.zeros((n, 1, 8))
    for a in range(n):
        e = el.EmuEnv("T", f32=True)
        e.set_goal_scoring(True)
        e.set_poses(robots[a], balls[a])
        h = e.get_state()
        for k in st:
            st[k].append(h[k])
        for s in range(steps):
            r = e.step([8])
            rew[s, a], done[s, a], status[s, a] = r["reward"], r["done"], r["status"]
        scores[a], fin[a] = e.goal_scores(), e.get_state()["balls"]
    st = {k: np.array(v) for k, v in st.items()}
    st["step"] = np.zeros(n, np.int32)
    ec.check_goal("T emulated", ec.goal_oracle(st, steps), rew, done, status, scores, fin)
