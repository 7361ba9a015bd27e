"""Training the hive in the full game on the MI355X: rr_hive_transition through the C-ABI, players.Hive.transition / store and
dqn.train_hive.

The per-robot reward is this project's definition (include/roborugby_amd.h).  It is pinned to the reference where the reference has an
answer -- one robot per team and positive ball 0: the team's reward of the step itself and of the recorded trajectories -- and to the
numpy restatement of the definition (tests/hive_transition_lib.py) on the device's own states everywhere else.

Bars: fp64 rewards and observations 1e-9, the bar tests/test_gpu_parity.py holds fp64 state and observations to (a reward is three
differences of distances <= 1132 times <= 236: a few 1e-11 per ulp); next_obs bit-equal to rr_observe_kind_f64 on the same record
(same functions); fp32 arithmetic within 16 * 2^-24 * diag * mult_ball of the fp64 restatement (each term is a difference of two
distances <= diag rounded to fp32: derived, not measured)."""
import ctypes as C
import os

import numpy as np
import pytest

import hive_transition_lib as ht

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL64 = 1e-9
NAMES = {0: "SingleBall_6wayLidar_v2", 1: "SingleBall_6wayLidar"}


def _env(preset, n, **kw):
    import roborugby_amd as rr
    kw.setdefault("time_limit", False)
    kw.setdefault("auto_reset", False)
    return rr.BatchedRoboRugbyEnv(n, preset=preset, **kw)


def _np(t):
    return t.cpu().numpy()


def _golden_steps(golden_dir, preset, n, full_actions=True):
    """n recorded steps of traj_<preset>.npz, evenly spread over the episodes (only steps where every robot was given an action)"""
    t = np.load(os.path.join(golden_dir, f"traj_{preset}.npz"))
    idx = [(ep, s) for ep in range(len(t["length"])) for s in range(int(t["length"][ep]))
           if not full_actions or (t["actions"][ep, s] >= 0).all()]
    pick = np.linspace(0, len(idx) - 1, n).astype(int) if n <= len(idx) else np.arange(n) % len(idx)
    ep, s = np.array([idx[i][0] for i in pick]), np.array([idx[i][1] for i in pick])
    d = {k: t["state_" + k][ep, s] for k in ("robots", "robots_i", "balls", "step", "inner")}
    d.update({k: t[k][ep, s] for k in ("actions", "obs", "obs_g", "reward", "reward_g", "done")})
    return d


def _ulp_close32(o32, o64):
    want = o64.astype(np.float32)
    return np.all(np.abs(o32.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


def _centres(env):
    st = env.get_state()
    return _np(st["robots"])[:, :, :2], _np(st["balls"])[:, :, :2]


def _restate(env, c0, c1, mask, assign, status, done):
    p = env.preset
    name = {(1, 0, 1, 0): "T", (2, 2, 4, 4): "G", (1, 1, 1, 1): "D", (2, 1, 2, 3): "X"}[(p.nr_happy, p.nr_grumpy, p.nb_pos, p.nb_neg)]
    return ht.restate(name, c0[0], c0[1], c1[0], c1[1], mask, _np(assign), _np(status), _np(done).astype(np.uint8), W=p.arena_w, H=p.arena_h)


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact_trig"])
@pytest.mark.parametrize("preset,n,mask,robot", [("T", 65, 1, 0), ("D", 63, 2, 1)])
def test_one_robot_per_team_and_ball_0_is_the_steps_own_reward(golden_dir, preset, n, mask, robot, exact):
    d = _golden_steps(golden_dir, preset, n)
    env = _env(preset, n, exact_trig=exact)
    env.track_prior_step()
    env.set_state(d["robots"], d["robots_i"], d["balls"], d["step"])
    if exact:
        env.set_scratch_rect(d["inner"][:, :2])
    assign, _ = env.hive_observe(mask, f64=True)
    obs, rew, done, info = env.step_f64(torch.as_tensor(d["actions"].astype(np.int32)))
    next_obs, reward, terminal, valid = env.hive_transition(assign, info.status, done, mask, f64=True)
    sel = _np(assign)[:, robot] == 0  # the rows where the robot went for the positive ball 0
    assert sel.sum() >= 5, sel.sum()  # (not vacuous)
    assert np.array_equal(_np(valid)[:, robot].astype(bool), _np(assign)[:, robot] >= 0)
    own_r = _np(rew) if robot == 0 else _np(info.dblGrumpyScore)
    own_o = _np(obs) if robot == 0 else _np(info.adblGrumpyState)
    gold_r, gold_o = (d["reward"], d["obs"]) if robot == 0 else (d["reward_g"], d["obs_g"])
    got_r, got_o = _np(reward)[:, robot], _np(next_obs)[:, robot]
    errs = dict(own_reward=np.abs(got_r - own_r)[sel].max(), golden_reward=np.abs(got_r - gold_r)[sel].max(),
                own_obs=np.abs(got_o - own_o)[sel].max(), golden_obs=np.abs(got_o - gold_o)[sel].max())
    print(f"[{preset}{' exact' if exact else ''}] {int(sel.sum())} rows: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert all(v <= TOL64 for v in errs.values()), errs
    assert np.array_equal(_np(terminal)[:, robot][sel], _np(done).astype(np.uint8)[sel])
    env.close()


@pytest.mark.parametrize("preset,n,mask", [("G", 1, 15), ("G", 63, 3), ("G", 65, 12), ("G", 257, 4),
                                           ("X", 1, 7), ("X", 63, 3), ("X", 65, 4), ("X", 257, 6)])
def test_full_game_against_the_restatement_and_the_librarys_own_observers(golden_dir, preset, n, mask):
    d = _golden_steps(golden_dir, preset, n, full_actions=False)
    env = _env(preset, n)
    p = env.preset
    env.track_prior_step()
    env.set_state(d["robots"], d["robots_i"], d["balls"], d["step"])
    c0 = _centres(env)
    assign, _ = env.hive_observe(mask, f64=True)
    g = torch.Generator(device="cuda"); g.manual_seed(n + mask)
    _, _, done, info = env.step_f64(torch.randint(0, 8, (n, p.nr), generator=g, device="cuda", dtype=torch.int32))
    c1 = _centres(env)
    want, wterm, wvalid = _restate(env, c0, c1, mask, assign, info.status, done)
    assert np.array_equal(wvalid, (_np(assign) >= 0))  # (every arena stepped, no ball left play)
    for kind in (0, 1):
        next_obs, reward, terminal, valid = env.hive_transition(assign, info.status, done, mask, observer=NAMES[kind], f64=True)
        v = _np(valid).astype(bool)
        assert np.array_equal(v, wvalid)
        for r in range(p.nr):
            if not (mask >> r) & 1:
                assert not v[:, r].any()
        err = float(np.abs(_np(reward) - want).max())
        print(f"[{preset} n={n} mask={mask} kind={kind}] {int(v.sum())} valid rows, worst |reward - restatement| {err:.3e}")
        assert err <= TOL64, (kind, err)
        assert np.array_equal(_np(terminal), (_np(done).astype(np.uint8)[:, None] & v.astype(np.uint8)))
        assert np.array_equal(_np(terminal), wterm)
        assert bool(torch.all(next_obs[valid == 0] == 0)) and bool(torch.all(reward[valid == 0] == 0))
        for r in range(p.nr):
            for b in range(p.nb):
                s = (assign[:, r] == b) & (valid[:, r] != 0)
                if bool(s.any()):
                    own = env.get_game_state(1 if r < p.nr_happy else -1, r, b, f64=True, observer=NAMES[kind])
                    assert torch.equal(next_obs[s, r], own[s]), (kind, r, b)
        # the float entry: the fp64 values rounded, within 1 ulp (the bar tests/test_gpu_hive.py holds rr_hive_observe's float rows to)
        o32, r32, t32, v32 = env.hive_transition(assign, info.status, done, mask, observer=NAMES[kind])
        assert torch.equal(v32, valid) and torch.equal(t32, terminal)
        assert _ulp_close32(_np(r32), _np(reward)) and _ulp_close32(_np(o32), _np(next_obs))
    env.close()


def test_auto_reset_the_done_step_is_terminal_and_the_replacing_call_is_no_transition():
    n = 64
    env = _env("G", n, seed=5, auto_reset=True, time_limit=True)
    env.track_prior_step()
    env.reset()
    st = env.get_state()
    step = st["step"].clone()
    step[::2] = env.preset.game_len_steps - 1
    env.set_state(st["robots"], st["robots_i"], st["balls"], step)
    acts = torch.zeros(n, 4, dtype=torch.int32, device="cuda")
    assign, _ = env.hive_observe(15)
    _, _, done, info = env.step(acts)
    assert bool(done[::2].all()) and not bool(done[1::2].any())
    _, _, terminal, valid = env.hive_transition(assign, info.status, done, 15)
    assert torch.equal(valid != 0, assign >= 0) and bool((valid != 0).any(1).all())
    assert torch.equal(terminal[::2], valid[::2]) and not bool(terminal[1::2].any())
    assign, _ = env.hive_observe(15)
    _, _, done, info = env.step(acts)
    assert bool(((info.status[::2] & 1024) != 0).all()) and not bool((info.status[1::2] & 1024).any())
    next_obs, reward, terminal, valid = env.hive_transition(assign, info.status, done, 15)
    assert not bool(valid[::2].any()) and bool(torch.all(next_obs[::2] == 0)) and bool(torch.all(reward[::2] == 0))
    assert torch.equal(valid[1::2] != 0, assign[1::2] >= 0) and bool((valid[1::2] != 0).any(1).all())
    assert not bool(terminal.any())
    env.close()


def test_goal_scoring_a_ball_consumed_during_the_step_ends_the_pairing():
    n = 2
    env = _env("G", n, goal_scoring=True, action_mode="thrust")
    env.track_prior_step()
    robots = np.tile(np.array([[[400, 100, 0], [400, 200, 0], [400, 300, 0], [400, 400, 0]]], dtype=np.float64), (n, 1, 1))
    one = np.array([[760, 770, 0, 0], [100, 400, 0, 0], [100, 500, 0, 0], [100, 600, 0, 0],
                    [600, 100, 0, 0], [600, 200, 0, 0], [600, 300, 0, 0], [300, 700, 0, 0]], dtype=np.float64)
    balls = np.tile(one[None], (n, 1, 1))
    balls[1, 0, :2] = (400, 600)  # arena 1: ball 0 outside the goals
    env.set_poses(robots, balls)
    assign = torch.tensor([[0, 1, -1, -1]] * n, dtype=torch.int32, device="cuda")  # robot 0 holds ball 0 (no greedy pass would give it)
    still = torch.zeros(n, 8, device="cuda")
    consumed_at = None
    for s in range(160):
        _, _, done, info = env.step_thrust(still)
        _, _, _, valid = env.hive_transition(assign, info.status, done, 3)
        v = _np(valid)
        gone = float(env.get_state()["balls"][0, 0, 0]) < -900
        assert v[1].tolist() == [1, 1, 0, 0] and v[0, 1:].tolist() == [1, 0, 0], (s, v)
        assert v[0, 0] == (0 if gone else 1), (s, v)
        if gone:
            consumed_at = s
            break
    assert consumed_at == 150, consumed_at  # its 151st consecutive step inside the goal: 150 full steps there, consumed by this one
    env.close()


def test_precisions_fp32_state_exact_arithmetic_fp32_within_the_derived_bound(golden_dir):
    n = 65
    d = _golden_steps(golden_dir, "G", n, full_actions=False)
    acts = torch.as_tensor(np.random.default_rng(3).integers(0, 8, (n, 4)).astype(np.int32)).cuda()
    bound = ht.fp32_bound(800.0, 800.0)
    for dtype, tol in (("f32_state", TOL64), ("f32", bound)):
        env = _env("G", n, dtype=dtype)
        env.track_prior_step()
        env.set_state(np.nan_to_num(d["robots"]), d["robots_i"], d["balls"], d["step"])
        c0 = _centres(env)  # (the state as the handle holds it: rounded to fp32)
        assign, _ = env.hive_observe(15)
        _, _, done, info = env.step(acts)
        c1 = _centres(env)
        want, wterm, wvalid = _restate(env, c0, c1, 15, assign, info.status, done)
        if dtype == "f32":
            out = [torch.full((n, 4, 11), 7.0, dtype=torch.float64, device="cuda"), torch.full((n, 4), 7.0, dtype=torch.float64, device="cuda"),
                   torch.full((n, 4), 7, dtype=torch.uint8, device="cuda"), torch.full((n, 4), 7, dtype=torch.uint8, device="cuda")]
            rc = env._lib.rr_hive_transition_f64(env._h, 15, 0, C.c_void_p(assign.data_ptr()), C.c_void_p(info.status.data_ptr()),
                                                 C.c_void_p(done.view(torch.uint8).data_ptr()), *[C.c_void_p(t.data_ptr()) for t in out], None)
            assert rc == -1 and b"RR_DTYPE_F32" in env._lib.rr_last_error()
            torch.cuda.synchronize()
            assert all(bool((t == 7).all()) for t in out)
        for kind in (0, 1):
            _, reward, terminal, valid = env.hive_transition(assign, info.status, done, 15, observer=NAMES[kind], f64=dtype != "f32")
            assert np.array_equal(_np(valid).astype(bool), wvalid) and np.array_equal(_np(terminal), wterm)
            err = float(np.abs(_np(reward).astype(np.float64) - want).max())
            print(f"[{dtype} kind={kind}] worst |reward - fp64 restatement| {err:.3e} (bar {tol:.3e})")
            assert err <= tol, (dtype, kind, err, tol)
        env.close()


def test_the_entry_is_read_only_a_twin_that_never_calls_it_stays_bit_identical():
    n = 257
    envs = [_env("G", n, seed=21, auto_reset=True, time_limit=True) for _ in range(2)]
    for e in envs:
        e.track_prior_step()
        e.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(4)
    status = done = assign = None
    for s in range(12):
        acts = torch.randint(0, 8, (n, 4), generator=g, device="cuda", dtype=torch.int32)
        if assign is not None:
            envs[1].hive_transition(assign, status, done, 15, observer=NAMES[s % 2], f64=bool(s % 3 == 0))
        assign, _ = envs[1].hive_observe(15)
        (o0, r0, d0, i0), (o1, r1, d1, i1) = envs[0].step(acts), envs[1].step(acts)
        envs[1].hive_transition(assign, i1.status, d1, 15, observer=NAMES[s % 2])
        status, done = i1.status, d1
        assert torch.equal(o0, o1) and torch.equal(r0, r1) and torch.equal(d0, d1) and torch.equal(i0.status, i1.status), s
        assert torch.equal(i0.adblGrumpyState, i1.adblGrumpyState) and torch.equal(i0.dblGrumpyScore, i1.dblGrumpyScore), s
    prior = [e.get_game_state(observer="AllCoords_WithPrior", f64=True) for e in envs]  # the on_step_begin snapshot, through its observer
    assert torch.equal(prior[0], prior[1])
    a, b = envs[0].get_state(), envs[1].get_state()
    assert all(torch.equal(a[k].nan_to_num(7e77) if a[k].dtype.is_floating_point else a[k],
                           b[k].nan_to_num(7e77) if b[k].dtype.is_floating_point else b[k]) for k in a)
    for e in envs:
        e.close()


def test_refusals_return_minus_one_with_a_message_and_touch_nothing():
    n = 64
    env = _env("G", n)
    env.track_prior_step()
    env.reset()
    L = env._lib
    assign, _ = env.hive_observe(15)
    _, _, done, info = env.step(torch.zeros(n, 4, dtype=torch.int32, device="cuda"))
    ins = [C.c_void_p(assign.data_ptr()), C.c_void_p(info.status.data_ptr()), C.c_void_p(done.view(torch.uint8).data_ptr())]

    def outs(dt):
        ts = [torch.full((n, 4, 11), 7.0, dtype=dt, device="cuda"), torch.full((n, 4), 7.0, dtype=dt, device="cuda"),
              torch.full((n, 4), 7, dtype=torch.uint8, device="cuda"), torch.full((n, 4), 7, dtype=torch.uint8, device="cuda")]
        return ts, [C.c_void_p(t.data_ptr()) for t in ts]

    def refused(fn, h, mask, kind, ptrs, ts, word):
        assert fn(h, mask, kind, *ptrs, None) == -1, (mask, kind, word)
        msg = L.rr_last_error()
        assert msg and word in msg, (word, msg)
        torch.cuda.synchronize()
        assert all(bool((t == 7).all()) for t in ts), word

    for fn, dt in ((L.rr_hive_transition, torch.float32), (L.rr_hive_transition_f64, torch.float64)):
        ts, po = outs(dt)
        refused(fn, None, 15, 0, ins + po, ts, b"null")
        for k in range(7):
            ptrs = ins + po
            ptrs[k] = None
            refused(fn, env._h, 15, 0, ptrs, ts, b"null")
        refused(fn, env._h, 0, 0, ins + po, ts, b"empty")
        refused(fn, env._h, 16, 0, ins + po, ts, b"mask")
        refused(fn, env._h, 0x80000001, 0, ins + po, ts, b"mask")
        refused(fn, env._h, 15, 2, ins + po, ts, b"kind")
        refused(fn, env._h, 15, -1, ins + po, ts, b"kind")
        untracked = _env("G", n)
        refused(fn, untracked._h, 15, 0, ins + po, ts, b"rr_track_prior_step")
        untracked.track_prior_step()
        untracked.track_prior_step(False)
        refused(fn, untracked._h, 15, 0, ins + po, ts, b"rr_track_prior_step")
        untracked.close()
        budgeted = _env("G", n, step_budget_clocks=20000)
        budgeted.track_prior_step()
        refused(fn, budgeted._h, 15, 0, ins + po, ts, b"budget")
        budgeted.close()
        assert fn(env._h, 15, 0, *(ins + po), None) == 0  # ... and the well-formed call goes through
        torch.cuda.synchronize()
        assert not any(bool((t == 7).all()) for t in ts)
    from roborugby_amd import _lib
    fresh = _env("G", n)
    with pytest.raises(_lib.RRError):
        fresh.hive_transition(assign, info.status, done, 15)
    fresh.close()
    env.close()


def _agent(batch=64, mem=4096, seed=3):
    from roborugby_amd.dqn import BatchedDQNAgent
    return BatchedDQNAgent(device="cuda:0", seed=seed, batch_size=batch, max_mem_size=mem)


def test_hive_store_appends_the_valid_rows_in_arena_robot_order():
    from roborugby_amd.players import Hive, og_twitchy
    n = 65
    env = _env("G", n, seed=8, auto_reset=True, time_limit=True, action_mode="thrust")
    env.track_prior_step()
    env.reset()
    agent = _agent()
    assert agent.fused
    hive = Hive(env, agent, robots=(0, 1, 3), epsilon=0.3, seed=2)
    gen = torch.Generator(device="cuda"); gen.manual_seed(6)
    thrust = torch.zeros(n, 8, device="cuda")
    want = [[] for _ in range(5)]
    total = 0
    for s in range(3):
        thrust.copy_(og_twitchy(n, 4, generator=gen, device="cuda"))
        hive.act(out=thrust)
        _, _, done, info = env.step_thrust(thrust)
        next_obs, reward, terminal, valid = [t.clone() for t in hive.transition(done, info.status)]
        assert torch.equal(valid, (hive.assign >= 0)) and not bool(valid[:, 2].any())  # (nobody was re-placed in three steps)
        v = valid.reshape(-1)
        for k, t in enumerate((hive.obs.reshape(-1, 11), next_obs.reshape(-1, 11), hive.actions.reshape(-1).long(), reward.reshape(-1),
                               terminal.reshape(-1))):
            want[k].append(t[v].clone())
        hive.store(agent, done, info.status)
        total += int(v.sum())
        assert agent.mem_cntr == total, (s, agent.mem_cntr, total)
    assert total > 3 * n  # most arenas have a ball for each of the three hive robots
    for mem, rows in zip((agent.state_memory, agent.new_state_memory, agent.action_memory, agent.reward_memory, agent.terminal_memory), want):
        assert torch.equal(mem[:total], torch.cat(rows)), mem.dtype
    assert bool(torch.all(agent.state_memory[total:] == 0))
    hive.close()
    env.close()


def test_train_hive_smoke_and_its_checkpoint_plays(tmp_path):
    from roborugby_amd import dqn
    ck = str(tmp_path / "hive.pt")
    res = dqn.train_hive(num_envs=256, steps=6, batch_size=256, mem_size=16384, updates_per_step=1, checkpoint=ck, log_every=0)
    assert res["mode"] == "train_hive" and res["preset"] == "G" and res["hive_robots"] == [0, 1]
    assert res["transitions"] == res["valid_rows"] and 0 < res["transitions"] <= 6 * 256 * 2
    assert res["learn_calls"] == 6 and res["loss"] is not None and np.isfinite(res["loss"])
    assert 0 < res["valid_share"] <= 1 and np.isfinite(res["mean_robot_reward"]) and res["env_steps_per_sec"] > 0
    played = dqn.play_hive(ck, num_envs=256, steps=3, seed=2)
    assert played["mode"] == "play_hive" and np.isfinite(played["return_happy"])
    # fine-tuning: the agent of a checkpoint is taken over
    again = dqn.train_hive(num_envs=256, steps=2, batch_size=256, mem_size=16384, updates_per_step=1, resume=ck, log_every=0)
    assert again["resumed_from"] == ck and again["transitions"] == again["valid_rows"] > 0
