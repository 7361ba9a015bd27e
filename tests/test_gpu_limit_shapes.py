"""The shapes at the limits of the one-shape library on the MI355X (roborugby_amd.build.shape_lanes; __graft_entry__.build() builds both):

  W = 1 + 1 robots, 4 + 7 balls: SIXTEEN lanes per arena (four arenas per wavefront), 55 ball pairs -- the upper half of the 64-bit
      ball-pair mask --, the one-pass two-team observation;
  R = 4 + 4 robots, 2 + 2 balls: eight robots (28 robot pairs, NaughtyBots bits 16..23, robot_mask 0xFF) and exactly 32 ball-robot
      pairs, so that bit 31 of that mask is a real pair.

Every entry the handle offers, against the oracle (1e-9, the bar of tests/test_gpu_parity.py), against the step it must equal bit for
bit (shortcuts off, rollout, budgets), or against the restated picture (tests/render_ref.py) -- each with the tolerance its sibling
for X or G has.  The golden step, the reset checks and the adversarial states of these shapes are in test_gpu_parity.py and
test_differential_adversarial.py; the CPU twins in test_limit_shapes_emulated.py and the parametrisations W and R joined."""
import functools
import json
import os

import numpy as np
import pytest

import adversarial as adv
import fp32_checks as fc
import fp32_entry_checks as ec
import oracle_lib as ol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
TOL64 = 1e-9
SHAPES = pytest.mark.parametrize("preset", ["W", "R"])
LANES = {"W": 16, "R": 8}


def _env(preset, n, **kw):
    import roborugby_amd as rr
    kw.setdefault("time_limit", False)
    kw.setdefault("auto_reset", False)
    return rr.BatchedRoboRugbyEnv(n, preset=ol.product_preset(preset), **kw)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _recorded_steps(preset, cap=400):
    """pre-step states and actions of the reference's recorded steps in which every robot got an action, strided to `cap` arenas"""
    t = np.load(f"{GOLDEN}/traj_{preset}.npz")
    nr = t["state_robots"].shape[2]
    idx = [(ep, s) for ep in range(t["length"].shape[0]) for s in range(int(t["length"][ep])) if (t["actions"][ep, s] >= 0).sum() == nr]
    idx = idx[::max(1, -(-len(idx) // cap))]
    ep = np.array([i[0] for i in idx]); s = np.array([i[1] for i in idx])
    st = {k: np.ascontiguousarray(t["state_" + k][ep, s]) for k in ("robots", "robots_i", "balls", "step")}
    return st, np.ascontiguousarray(t["actions"][ep, s].astype(np.int32))


@pytest.mark.parametrize("preset,n", [("W", 1), ("W", 3), ("W", 5), ("W", 65), ("R", 1), ("R", 7), ("R", 9)])
def test_lane_width_and_ragged_batch_sizes_match_oracle(preset, n):
    """batch sizes that leave the last wavefront partly empty (W: four arenas per wavefront, R: eight): every arena matches the oracle"""
    env = _env(preset, n, seed=21)
    assert env.lanes_per_env() == LANES[preset] and (env.preset.nr, env.preset.nb) == ((2, 11) if preset == "W" else (8, 4))
    env.reset()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n)
    checked = 0
    for _ in range(3):
        pre = _np(env.get_state())
        acts = torch.randint(0, 8, (n, env.preset.nr), generator=gen, device="cuda", dtype=torch.int32)
        o, r, d, info = env.step_f64(acts)
        post = _np(env.get_state())
        for a in range(n):
            orc = ol.OracleEnv(preset)
            orc.set_state(pre["robots"][a], pre["robots_i"][a], pre["balls"][a], None, pre["step"][a])
            res = orc.step(acts[a].cpu().numpy())
            assert (int(info.status[a]) & 0xFFFF & ~256) == (res["status"] & ~256), (preset, n, a)
            if res["status"] & 63:
                continue
            os_ = orc.get_state()
            assert np.allclose(os_["balls"], post["balls"][a], atol=TOL64, rtol=0)
            assert np.allclose(os_["robots"][:, :7], post["robots"][a][:, :7], atol=TOL64, rtol=0)
            assert np.array_equal(os_["robots_i"], post["robots_i"][a])
            assert np.allclose(res["obs"], o[a].cpu().numpy(), atol=TOL64, rtol=0)
            assert np.allclose(res["obs_g"], info.adblGrumpyState[a].cpu().numpy(), atol=TOL64, rtol=0)
            assert abs(res["reward"] - float(r[a])) < 1e-6 and abs(res["reward_g"] - float(info.dblGrumpyScore[a])) < 1e-6
            assert res["naughty"] == (int(info.status[a]) >> 16) & 0xFF
            checked += 1
    assert checked >= 2 * n
    env.close()


@SHAPES
def test_contact_dense_states_shortcuts_off_equals_on(preset):
    from test_gpu_shortcuts import _env as _switched, _run, _same
    n = 1024
    robots, balls, actions = adv.make_states(preset, n, seed=21)
    p = ol.product_preset(preset)
    e = _env(preset, n)
    e.set_poses(robots, balls)
    state = tuple(v.cpu().numpy() for v in (e.get_state()[k] for k in ("robots", "robots_i", "balls", "step")))
    e.close()
    a_t = torch.as_tensor(actions, device="cuda")
    on = _run(_switched(n, p), state, a_t, 4)  # the same action four times: robots keep pushing, islands form and freeze
    off = _run(_switched(n, p, RR_NO_MEMO=1, RR_NO_ORDER=1), state, a_t, 4)
    assert _same(on, off)
    moved = np.abs(on[0][8][:, :, 6:] - balls[:, :, 2:] * 0.995 ** 12).max(axis=(1, 2)) > 1e-6
    assert moved.mean() > 0.2  # the batch really is contact-dense


@SHAPES
def test_rollout_in_one_launch_equals_step_by_step(preset):
    """rr_rollout (S = 6 steps per launch, the record stays in LDS) against six rr_step calls across an episode boundary, and against
    four steps of one action with repeat=4: every per-step output and the final state bit-identical"""
    n, S = 513, 6
    nr = ol.product_preset(preset).nr
    gen = torch.Generator(device="cuda"); gen.manual_seed(4)
    acts = torch.randint(0, 8, (S, n, nr), generator=gen, device="cuda", dtype=torch.int32)
    envs = [_env(preset, n, seed=11, time_limit=True, auto_reset=True) for _ in range(2)]
    for e in envs:
        e.reset()
        st = e.get_state()
        st["step"][: n // 2] = e.preset.game_len_steps - 3  # half of the arenas finish (and are re-placed) inside the rollout
        e.set_state(st["robots"], st["robots_i"], st["balls"], st["step"])
    ref = [envs[0].step(acts[s]) for s in range(S)]
    o, r, d, info = envs[1].rollout(acts)
    for s in range(S):
        assert torch.equal(o[s], ref[s][0]) and torch.equal(r[s], ref[s][1]) and torch.equal(d[s], ref[s][2]), (preset, s)
        assert torch.equal(info.status[s], ref[s][3].status) and torch.equal(info.dblGrumpyScore[s], ref[s][3].dblGrumpyScore)
        assert torch.equal(info.adblGrumpyState[s], ref[s][3].adblGrumpyState)
    a, b = envs[0].get_state(), envs[1].get_state()
    assert all(torch.equal(a[k], b[k]) or (a[k].dtype.is_floating_point and torch.equal(a[k].nan_to_num(7e77), b[k].nan_to_num(7e77))) for k in a)
    assert int(d.sum()) >= n // 2  # the episode boundary really was inside
    rep = [envs[0].step(acts[0]) for _ in range(4)]
    o2, r2, d2, i2 = envs[1].rollout(acts[0], repeat=4)
    assert all(torch.equal(o2[s], rep[s][0]) and torch.equal(r2[s], rep[s][1]) and torch.equal(i2.status[s], rep[s][3].status) for s in range(4))
    for e in envs:
        e.close()


@SHAPES
def test_budgeted_equals_synchronous_on_contact_dense_arenas(preset):
    """per-arena streams of (observation, reward, done, status, the other team's) as a function of the accepted actions: the
    synchronous mode's bit for bit at a budget of 1 clock (every expensive sub-step parks) and of 50,000"""
    from budget_driver import equal, streams
    n, steps = 300, 5
    robots, balls, _ = adv.make_states(preset, n, seed=13)
    nr = ol.product_preset(preset).nr
    g = torch.Generator(device="cuda").manual_seed(5)
    table = torch.randint(0, 16, (steps, n, nr), generator=g, device="cuda", dtype=torch.int32)  # robot 0: half chase, half random
    ref = None
    for budget in (0, 1, 50_000):
        env = _env(preset, n, seed=3, time_limit=True, auto_reset=True, step_budget_clocks=budget)
        env.set_poses(robots, balls)
        got, calls, nr_rows = streams(env, table, steps, budget > 0, 4000)
        env.close()
        if ref is None:
            ref = got
            assert calls == steps and nr_rows == 0
        else:
            assert equal(got, ref), (preset, budget)
            if budget == 1:
                assert nr_rows > n  # contact-dense arenas: with a 1-clock budget they park over and over
        print(f"[{preset}] budget {budget}: {calls} calls for {steps} steps of {n} arenas, {nr_rows} NOT_READY rows")


@SHAPES
def test_f32_state_step_is_the_oracle_on_the_rounded_state(preset):
    """rr_step_f64 on an RR_DTYPE_F32_STATE handle over the reference's recorded steps, the two claims fp32_entry_checks.py's callers
    hold X and G to: the outputs are the fp64 oracle's from the SAME fp32-rounded state within 1e-9, and the stored post-state is the
    oracle's rounded to fp32, to one fp32 ulp, integer state equal -- on >= 99.9 % of the steps.  And the records are smaller."""
    st, acts = _recorded_steps(preset, cap=2000)  # every recorded step (a share of 99.9 % needs more than a thousand to allow a single miss)
    n = len(acts)
    env = _env(preset, n, dtype="f32_state")
    env.set_state(st["robots"], st["robots_i"], st["balls"], st["step"])
    held = _np(env.get_state())
    assert all(np.array_equal(ec.r32(held[k]), held[k], equal_nan=True) for k in ("robots", "balls"))
    o, r, d, info = env.step_f64(torch.as_tensor(acts))
    got = _np(env.get_state())
    o, r, og, rg = (x.cpu().numpy() for x in (o, r, info.adblGrumpyState, info.dblGrumpyScore))
    status = info.status.cpu().numpy()
    e_out, ref = np.zeros(n), {k: np.zeros_like(got[k]) for k in ("robots", "robots_i", "balls")}
    for i in range(n):
        orc = ec.oracle_at(preset, held, i)
        res = orc.step(acts[i])
        s = orc.get_state()
        ref["robots"][i], ref["balls"][i], ref["robots_i"][i] = ec.r32(s["robots"]), ec.r32(s["balls"]), s["robots_i"]
        e = max(np.abs(res["obs"] - o[i]).max(), np.abs(res["obs_g"] - og[i]).max(), abs(res["reward"] - r[i]), abs(res["reward_g"] - rg[i]))
        e_out[i] = e if res["done"] == bool(d[i]) and res["naughty"] == (status[i] >> 16) & 0xFF else np.inf
    e_k = np.maximum(fc.rel_err(got["robots"], ref["robots"]), fc.rel_err(got["balls"], ref["balls"]))
    same_i = np.all(got["robots_i"] == ref["robots_i"], axis=(1, 2))
    print(f"[{preset} fp32 state] {n} steps vs the oracle on the same rounded state: outputs within 1e-9 on {100 * (e_out <= TOL64).mean():.3f} %; "
          f"stored state max rel err {e_k.max():.2e}, within one fp32 ulp on {100 * (e_k <= 2.5e-7).mean():.3f} %, integers equal in {100 * same_i.mean():.3f} %")
    assert (e_out <= TOL64).mean() >= 0.999, preset
    assert (e_k <= 2.5e-7).mean() >= 0.999 and same_i.mean() >= 0.999, (preset, float(e_k.max()), float(same_i.mean()))
    e64 = _env(preset, 8)
    assert env.state_bytes_per_env() < e64.state_bytes_per_env()
    env.close(); e64.close()


@SHAPES
def test_allcoords_observers_and_a_seven_keeper_stack_match_the_oracle(preset):
    """AllCoords (3 NR + 2 NB values) and AllCoords_WithPrior (6 NR + 4 NB: 56 for W, 64 for R) of both teams, every row, and the rewards
    of all seven keepers -- stack A of tests/golden/mix_*.npz with NaughtyBots behind it -- after one step from recorded states"""
    meta = json.loads(str(np.load(f"{GOLDEN}/mix_G.npz")["meta"]))
    stack = tuple(meta["programs_mro"]["A"]) + ("NaughtyBots",)
    prog = [1] + list(meta["programs_exec"]["A"])
    from roborugby_amd.env import keeper_exec_order
    assert keeper_exec_order(stack) == prog and sorted(prog) == [1, 2, 3, 4, 5, 6, 7]
    st, acts = _recorded_steps(preset, cap=250)
    n = len(acts)
    p = ol.product_preset(preset)
    env = _env(preset, n, rewards=stack, observer="AllCoords_WithPrior")
    assert env.observation_space.shape == (6 * p.nr + 4 * p.nb,) == ((56,) if preset == "W" else (64,))
    env.set_state(st["robots"], st["robots_i"], st["balls"], st["step"])
    o, r, d, info = env.step_f64(torch.as_tensor(acts))
    r, rg = r.cpu().numpy(), info.dblGrumpyScore.cpu().numpy()
    got = {(kind, team): env.get_game_state(team, f64=True, observer=name).cpu().numpy()
           for kind, name in ((3, "AllCoords"), (4, "AllCoords_WithPrior")) for team in (1, -1)}
    assert got[(3, 1)].shape == (n, 3 * p.nr + 2 * p.nb) and got[(4, -1)].shape == (n, 6 * p.nr + 4 * p.nb)
    paid = 0
    for i in range(n):
        orc = ec.oracle_at(preset, st, i)
        orc.set_program(prog)
        res = orc.step(acts[i])
        assert not res["status"] & 63  # recorded steps: the reference did not raise
        assert abs(res["reward"] - r[i]) < 1e-7 and abs(res["reward_g"] - rg[i]) < 1e-7, (preset, i, res["reward"], r[i], res["reward_g"], rg[i])
        paid += int(res["reward"] != 0.0) + int(res["reward_g"] != 0.0)
        for (kind, team), g in got.items():
            want = orc.observe_kind(kind, team)
            assert want.shape == g[i].shape and np.array_equal(np.isnan(want), np.isnan(g[i])), (preset, i, kind, team)
            assert float(np.nan_to_num(np.abs(want - g[i])).max()) < TOL64, (preset, i, kind, team)
    assert paid > n  # the stack pays both teams
    env.close()


@pytest.mark.parametrize("preset,mask,n", [("R", 0xFF, 1), ("R", 0xFF, 65), ("W", 3, 1), ("W", 3, 65)])
def test_hive_observe_of_every_robot(preset, mask, n):
    """rr_hive_observe, kinds 0 and 1: the assignment is the numpy restatement's, the rows are the library's own single-pair observers'
    bit for bit (test_gpu_hive.py's check) and the oracle's observation of (robot, assigned ball) within 1e-9"""
    from test_gpu_hive import _check_against_own_observers_and_restatement
    env = _env(preset, n, seed=n)
    env.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(n)
    for _ in range(5):
        env.step(torch.randint(0, 8, (n, env.preset.nr), generator=g, device="cuda", dtype=torch.int32))
    p = env.preset
    st = env.get_state()
    rxy = st["robots"][:, :, [0, 1, 6]].clone()
    b = torch.cat([st["balls"][:, :, :2], torch.zeros_like(st["balls"][:, :, :2])], dim=2)
    u = torch.rand(n, p.nb, 2, generator=g, device="cuda", dtype=torch.float64) * 100 + 10
    far = torch.rand(n, p.nb, 1, generator=g, device="cuda") < .5
    corner = torch.rand(n, p.nb, generator=g, device="cuda") < 1 / 3  # a third of the balls into the goal corners
    wh = torch.tensor([p.arena_w, p.arena_h], device="cuda", dtype=torch.float64)
    b[:, :, :2] = torch.where(corner.unsqueeze(-1), torch.where(far, wh - u, u), b[:, :, :2])
    env.set_poses(rxy, b)
    want = _check_against_own_observers_and_restatement(env, mask, cap=0.01)
    assert (want >= 0).any()
    held = _np(env.get_state())
    for kind, name in ((0, "SingleBall_6wayLidar_v2"), (1, "SingleBall_6wayLidar")):
        assign, obs = env.hive_observe(mask, observer=name, f64=True)
        assign, obs = assign.cpu().numpy(), obs.cpu().numpy()
        for a in range(n):
            orc = ol.OracleEnv(preset)
            orc.set_state(held["robots"][a], held["robots_i"][a], held["balls"][a], None, int(held["step"][a]))
            for r in range(p.nr):
                if assign[a, r] < 0:
                    assert np.all(obs[a, r] == 0)
                    continue
                ref = orc.observe_kind(kind, 1 if r < p.nr_happy else -1, r, int(assign[a, r]))
                assert np.abs(obs[a, r] - ref[:11]).max() <= TOL64, (preset, kind, a, r)
    env.close()


@SHAPES
def test_field_frames_match_the_reference(preset):
    """render_batch with 8 robots / 11 balls in the draw list (it holds 16 of each kind), under tests/render_ref.py's rule"""
    import test_gpu_render as tr
    env = tr._env(preset)
    unique = tr._states(preset)[1]
    frames = env.render_batch(width=96, height=96)
    assert frames.shape == (tr.N, 96, 96, 3)
    tr._check_frames(preset, frames[:unique], range(unique), 96, 96, what="limit shape")
    tr._check_frames(preset, env.render_batch(arenas=[1], width=160, height=120), (1,), 160, 120, what="limit shape")
    env.close()


@SHAPES
def test_ego_frames_match_the_reference_from_every_robot(preset):
    import render_ego_ref as ego
    import test_gpu_render_ego as te
    env = te._env(preset)
    te._check_every_viewer(env, preset, ego.CONFIGS[1:3], "limit shape")
    env.close()
