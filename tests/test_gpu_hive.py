"""The hive-mind player on the MI355X: rr_hive_observe through the C-ABI against what the reference's own player did
(tests/golden/hive_{G,X}.npz: DQN_pytorch_player.Stephen with a stub mind, tools/gen_hive_golden.py), against the library's own
single-pair observers on the same records (bitwise: same functions, same record), against the numpy restatement of the greedy
rule (tests/hive_emu_lib.py), and players.Hive end to end.

Bars: assignment exact; fp64 observations within 1e-9 of the reference (the bar of tests/test_gpu_parity.py); fp32 outputs = the
fp64 ones rounded, within 1 ulp.  The order of exactly tied distances is this project's rule: arenas where two candidate distances
differ by less than 1e-9 relative (fp32 arithmetic: 4 epsilon -- 1e-9 is below its resolution) are left out of the comparison with the
restatement (device sqrt vs numpy's may differ in the last bit there), and there may be at most 0.1 % of them."""
import ctypes as C
import os

import numpy as np
import pytest

import hive_emu_lib as he
import oracle_lib as ol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL64 = 1e-9
THRUST = torch.tensor(((1, 1), (-1, -1), (-1, 1), (1, -1), (0, 1), (1, 0), (-1, 0), (0, -1)), dtype=torch.float32)  # RR_EnvBase.py:593-602


def _env(preset, n, **kw):
    import roborugby_amd as rr
    kw.setdefault("time_limit", False)
    kw.setdefault("auto_reset", False)
    return rr.BatchedRoboRugbyEnv(n, preset=preset, **kw)


def _team(env, r):
    return 1 if r < env.preset.nr_happy else -1


def _ulp_close32(o32, o64):
    want = o64.astype(np.float32)
    return np.all(np.abs(o32.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


@pytest.mark.parametrize("preset,exact", [("G", False), ("G", True), ("X", False)],
                         ids=lambda v: {False: "default", True: "exact_trig"}.get(v, v) if isinstance(v, bool) else v)
def test_hive_observe_matches_the_reference_hive(golden_dir, preset, exact):
    d = np.load(os.path.join(golden_dir, f"hive_{preset}.npz"))
    worst = 0.0
    for mask in np.unique(d["mask"]):
        s = np.nonzero(d["mask"] == mask)[0]
        env = _env(preset, len(s), exact_trig=exact)
        env.set_state(d["robots"][s], d["robots_i"][s], d["balls"][s], d["step"][s])
        for name, key in (("SingleBall_6wayLidar", "obs_v1"), ("SingleBall_6wayLidar_v2", "obs_v2")):
            a64, o64 = env.hive_observe(int(mask), observer=name, f64=True)
            a32, o32 = env.hive_observe(int(mask), observer=name)
            assert np.array_equal(a64.cpu().numpy(), d["assign"][s]), (preset, int(mask), name)
            assert torch.equal(a32, a64)
            err = float(np.abs(o64.cpu().numpy() - d[key][s]).max())
            worst = max(worst, err)
            assert err <= TOL64, (preset, int(mask), name, err)
            assert _ulp_close32(o32.cpu().numpy(), o64.cpu().numpy()), (preset, int(mask), name)
        env.close()
    print(f"hive_observe[{preset}{' exact' if exact else ''}] vs reference: worst |obs error| {worst:.3e}")


def test_hive_observe_on_an_fp32_state_handle_sees_the_rounded_state(golden_dir):
    d = np.load(os.path.join(golden_dir, "hive_G.npz"))
    s = np.nonzero(d["mask"] == 15)[0][::2]
    env = _env("G", len(s), dtype="f32_state")
    env.set_state(d["robots"][s], d["robots_i"][s], d["balls"][s], d["step"][s])
    robots = np.nan_to_num(d["robots"][s]).astype(np.float32).astype(np.float64)
    balls = d["balls"][s].astype(np.float32).astype(np.float64)
    cfg = ol.PRESETS["G"]
    want, near = he.greedy_assign_batch(robots[:, :, :2], balls[:, :, :2], 15, cfg["W"], cfg["H"])
    for kind, name in ((0, "SingleBall_6wayLidar_v2"), (1, "SingleBall_6wayLidar")):
        assign, obs = env.hive_observe(15, observer=name, f64=True)
        assign, obs = assign.cpu().numpy(), obs.cpu().numpy()
        assert np.array_equal(assign[~near], want[~near])
        for a in range(len(s)):
            o = ol.OracleEnv("G")
            o.set_state(robots[a], d["robots_i"][s][a], balls[a], None, int(d["step"][s][a]))
            for r in range(4):
                if assign[a, r] < 0:
                    assert np.all(obs[a, r] == 0)
                    continue
                ref = o.observe_kind(kind, 1 if r < 2 else -1, r, int(assign[a, r])) if kind else o.observe(1 if r < 2 else -1, r, int(assign[a, r]))
                assert np.abs(obs[a, r] - ref[:11]).max() <= TOL64, (kind, a, r)
    env.close()


def _check_against_own_observers_and_restatement(env, mask, cap=0.001):
    """rows == get_game_state gathered per assigned pair (bitwise, both kinds); assignment == numpy restatement of get_state()"""
    p, n = env.preset, env.num_envs
    st = env.get_state()
    rxy, bxy = st["robots"][:, :, :2].cpu().numpy(), st["balls"][:, :, :2].cpu().numpy()
    want, near = he.greedy_assign_batch(rxy, bxy, mask, p.arena_w, p.arena_h, dtype=np.float32 if env.dtype == "f32" else np.float64)
    assert near.mean() <= cap, near.mean()
    for name in ("SingleBall_6wayLidar_v2", "SingleBall_6wayLidar"):
        assign, obs = env.hive_observe(mask, observer=name)
        a = assign.cpu().numpy()
        assert np.array_equal(a[~near], want[~near]), (name, np.nonzero((a != want).any(1) & ~near)[0][:5])
        assert torch.all(obs[assign < 0] == 0)
        for r in range(p.nr):
            for b in range(p.nb):
                sel = assign[:, r] == b
                if bool(sel.any()):
                    g = env.get_game_state(_team(env, r), r, b, observer=name)
                    assert torch.equal(obs[sel, r], g[sel]), (name, r, b)
    return want


def test_hive_observe_at_scale_after_chase_steps():
    from roborugby_amd.players import chase
    n = 65536
    env = _env("G", n, seed=3, auto_reset=True, time_limit=True)
    obs = env.reset()
    for s in range(50):
        obs, _, _, _ = env.step(chase(env, obs, step=s, seed=9))
    want = _check_against_own_observers_and_restatement(env, 0b1111)
    assert (want >= 0).all(1).mean() > 0.5  # (sanity: most arenas have a free ball for every robot)
    _check_against_own_observers_and_restatement(env, 0b0011)
    env.close()


@pytest.mark.parametrize("preset,n,mask,dtype", [("G", 1, 15, "f64"), ("G", 63, 3, "f64"), ("G", 65, 12, "f64"), ("G", 4097, 15, "f64"),
                                                 ("G", 4097, 15, "f32"), ("D", 4097, 3, "f64"), ("D", 65, 2, "f32_state"), ("X", 4097, 7, "f64"),
                                                 ("X", 63, 5, "f32_state")])
def test_hive_observe_ragged_sizes_and_shapes(preset, n, mask, dtype):
    env = _env(preset, n, seed=n, dtype=dtype)
    env.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(n)
    for _ in range(5):
        env.step(torch.randint(0, 8, (n, env.preset.nr), generator=g, device="cuda", dtype=torch.int32))
    # a third of the balls into the goal corners (random placement never puts one there on its own)
    st = env.get_state()
    rxy = st["robots"][:, :, [0, 1, 6]].clone()
    b = torch.cat([st["balls"][:, :, :2], torch.zeros_like(st["balls"][:, :, :2])], dim=2)
    u = torch.rand(n, env.preset.nb, 2, generator=g, device="cuda", dtype=torch.float64) * 100 + 10
    far = torch.rand(n, env.preset.nb, 1, generator=g, device="cuda") < .5
    corner = torch.rand(n, env.preset.nb, generator=g, device="cuda") < 1 / 3
    wh = torch.tensor([env.preset.arena_w, env.preset.arena_h], device="cuda", dtype=torch.float64)
    b[:, :, :2] = torch.where(corner.unsqueeze(-1), torch.where(far, wh - u, u), b[:, :, :2])
    env.set_poses(rxy, b)
    want = _check_against_own_observers_and_restatement(env, mask, cap=0.01 if n < 1000 else 0.001)
    if n > 1000:
        hive = bin(mask).count("1")
        assert ((want >= 0).sum(1) < min(hive, env.preset.nb)).any()  # someone went without a ball somewhere
    env.close()


def test_hive_observe_T_is_ball_0_unless_it_lies_in_a_goal():
    n = 4097
    env = _env("T", n, seed=4)
    env.reset()
    st = env.get_state()
    rxy = st["robots"][:, :, [0, 1, 6]].clone()
    b = torch.zeros(n, 1, 4, dtype=torch.float64, device="cuda")
    b[:, 0, :2] = st["balls"][:, 0, :2]
    b[::3, 0, 0], b[::3, 0, 1] = 30.0, 40.0                                              # grumpy goal
    b[1::6, 0, 0], b[1::6, 0, 1] = env.preset.arena_w - 50.0, env.preset.arena_h - 20.0  # happy goal
    env.set_poses(rxy, b)
    want = _check_against_own_observers_and_restatement(env, 1)
    idx = np.arange(n)
    assert np.all(want[(idx % 3 == 0) | (idx % 6 == 1), 0] == -1) and np.all(want[(idx % 3 != 0) & (idx % 6 != 1), 0] == 0)
    env.close()


def test_hive_observe_skips_balls_out_of_play_and_runs_on_a_budgeted_handle():
    n = 2048
    env = _env("G", n, seed=6, goal_scoring=True, step_budget_clocks=20000, auto_reset=True)
    env.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    for _ in range(6):
        _, _, _, info = env.step(torch.randint(0, 8, (n, 4), generator=g, device="cuda", dtype=torch.int32))
        assign, obs = env.hive_observe(15)  # parked arenas: a sub-step view, but always a valid assignment
        a = assign.cpu().numpy()
        assert a.min() >= -1 and a.max() < 8 and bool(torch.isfinite(obs).all())
        for row in a[:256]:
            got = row[row >= 0]
            assert len(set(got.tolist())) == len(got)
    env.set_step_budget(0)
    env.step(torch.zeros(n, 4, dtype=torch.int32, device="cuda"))
    env.step(torch.zeros(n, 4, dtype=torch.int32, device="cuda"))
    st = env.get_state()
    balls = st["balls"].clone()
    balls[:, 1, 0], balls[:, 1, 1] = -1040.0, -1000.0  # ball 1 as the goal bookkeeping parks a consumed ball
    env.set_state(st["robots"], st["robots_i"], balls, st["step"])
    assign, _ = env.hive_observe(15)
    assert not bool((assign == 1).any())
    p = env.preset
    want, near = he.greedy_assign_batch(st["robots"][:, :, :2].cpu().numpy(), balls[:, :, :2].cpu().numpy(), 15, p.arena_w, p.arena_h)
    assert np.array_equal(assign.cpu().numpy()[~near], want[~near])
    env.close()


def _agent(seed=3):
    from roborugby_amd.dqn import BatchedDQNAgent
    return BatchedDQNAgent(device="cuda:0", seed=seed, batch_size=64, max_mem_size=64)


def test_hive_act_greedy_thrusts_and_untouched_columns():
    from roborugby_amd.players import Hive
    n = 4097
    env = _env("G", n, seed=8)
    env.reset()
    agent = _agent()
    for robots, observer in (((0, 1), None), ((0, 1, 2, 3), "SingleBall_6wayLidar"), ((2,), None), (None, None)):
        hive = Hive(env, agent, robots=robots, epsilon=0.0, seed=1, observer=observer)
        members = (0, 1) if robots is None else robots
        out = torch.full((n, 8), 7.0, device="cuda")
        got = hive.act(out=out)
        assert got is out
        mask = sum(1 << r for r in members)
        assign, obs = env.hive_observe(mask, observer=observer or "SingleBall_6wayLidar_v2")
        assert torch.equal(hive.assign, assign) and torch.equal(hive.obs, obs)
        with torch.no_grad():
            w1, b1, w2, b2, w3, b3 = [p.double() for p in agent.Q_eval.parameters()]  # Linear 11 -> 256 -> 256 -> 8 + ReLU, in fp64
            h = torch.relu(obs.view(-1, 11).double() @ w1.T + b1)
            q = (torch.relu(h @ w2.T + b2) @ w3.T + b3).view(n, 4, 8)
        top = q.topk(2, dim=2).values
        clear = (top[..., 0] - top[..., 1]) > 1e-4 * top[..., 0].abs().clamp(min=1.0)  # fp32 sums of 256 terms: argmax is decided beyond this
        want = THRUST.cuda()[q.argmax(dim=2)] * (assign >= 0).unsqueeze(-1)
        o3 = out.view(n, 4, 2)
        for r in range(4):
            if r in members:
                ok = clear[:, r] | (assign[:, r] < 0)
                assert ok.float().mean() > 0.99
                assert torch.equal(o3[ok, r], want[ok, r]), (robots, r)
                assert torch.all(o3[assign[:, r] < 0, r] == 0)
            else:
                assert torch.all(o3[:, r] == 7.0), (robots, r)
        fresh = hive.act()
        assert torch.equal(fresh.view(n, 4, 2)[:, list(members)], o3[:, list(members)])
        rest = [r for r in range(4) if r not in members]
        assert torch.all(fresh.view(n, 4, 2)[:, rest] == 0)
        hive.close()
    # rows of arenas that are NOT_READY (budgeted step: parked mid-step) are left as the caller filled them
    hive = Hive(env, agent, epsilon=0.0)
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    status[::5] = 16384 | 1024
    out = torch.full((n, 8), 7.0, device="cuda")
    hive.act(out=out, status=status)
    ref = hive.act()
    assert torch.all(out[::5] == 7.0) and torch.all(out[:, 4:] == 7.0)
    keep = torch.ones(n, dtype=torch.bool, device="cuda"); keep[::5] = False
    assert torch.equal(out[keep][:, :4], ref[keep][:, :4])
    # the six parameter tensors instead of an agent
    hive = Hive(env, [p.detach() for p in agent.Q_eval.parameters()], epsilon=0.0)
    assert torch.equal(hive.act(), Hive(env, agent, epsilon=0.0).act())
    with pytest.raises(ValueError):
        Hive(env, agent, robots=(4,))
    env.close()


def test_hive_act_epsilon_share_of_non_greedy_actions():
    from roborugby_amd.players import Hive
    n = 65536
    env = _env("G", n, seed=12)
    env.reset()
    agent = _agent()
    greedy, eps = Hive(env, agent, robots=range(4), epsilon=0.0, seed=5), Hive(env, agent, robots=range(4), epsilon=0.2, seed=5)
    greedy.act(); eps.act()
    assert torch.equal(greedy.assign, eps.assign)
    differ = float((greedy.actions != eps.actions).double().mean())
    p = 0.2 * 7 / 8  # a draw replaces the action with probability epsilon; one uniform action in eight is the greedy one again
    sigma = (p * (1 - p) / (4 * n)) ** .5
    print(f"non-greedy share {differ:.5f} (expected {p:.5f}, sigma {sigma:.5f})")
    assert abs(differ - p) <= 4 * sigma, (differ, p, sigma)
    a1 = eps.actions.clone()
    eps.act()
    assert not torch.equal(a1, eps.actions)  # a fresh call counter: fresh draws
    env.close()


def test_hive_act_and_step_thrust_replay_from_a_hip_graph():
    from roborugby_amd.players import Hive
    n = 8192
    eager, graphed = _env("G", n, seed=5, auto_reset=True), _env("G", n, seed=5, auto_reset=True)
    eager.reset(); graphed.reset()
    agent = _agent()
    he_, hg = Hive(eager, agent, epsilon=0.0), Hive(graphed, agent, epsilon=0.0)
    buf_e, buf_g = torch.zeros(n, 8, device="cuda"), torch.zeros(n, 8, device="cuda")
    gen = torch.Generator(device="cuda"); gen.manual_seed(2)
    other = (torch.randint(-1, 2, (12, n, 4), generator=gen, device="cuda")).float()  # the grumpy team's thrusts
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch's capture protocol asks (single stream, no parallel branches)
        buf_g[:, 4:] = other[0]
        hg.act(out=buf_g)
        graphed.step_thrust(buf_g)
    torch.cuda.current_stream().wait_stream(side)
    buf_e[:, 4:] = other[0]
    he_.act(out=buf_e)
    eager.step_thrust(buf_e)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hg.act(out=buf_g)
        res = graphed.step_thrust(buf_g)
    for s in range(1, 12):
        buf_g[:, 4:] = other[s]
        g.replay()
        buf_e[:, 4:] = other[s]
        he_.act(out=buf_e)
        o, r, d, info = eager.step_thrust(buf_e)
        torch.cuda.synchronize()
        assert torch.equal(buf_g, buf_e), s
        assert torch.equal(res[0], o) and torch.equal(res[1], r) and torch.equal(res[2], d) and torch.equal(res[3].status, info.status), s
    a, b = eager.get_state(), graphed.get_state()
    assert all(torch.equal(a[k].nan_to_num(7e77) if a[k].dtype.is_floating_point else a[k],
                           b[k].nan_to_num(7e77) if b[k].dtype.is_floating_point else b[k]) for k in a)


def test_hive_observe_between_steps_changes_no_later_step():
    n = 4096
    envs = [_env("G", n, seed=21, auto_reset=True, time_limit=True) for _ in range(2)]
    for e in envs:
        e.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(4)
    for s in range(100):
        acts = torch.randint(0, 8, (n, 4), generator=g, device="cuda", dtype=torch.int32)
        envs[1].hive_observe(15, observer="SingleBall_6wayLidar_v2" if s % 2 else "SingleBall_6wayLidar", f64=bool(s % 3 == 0))
        (o0, r0, d0, i0), (o1, r1, d1, i1) = envs[0].step(acts), envs[1].step(acts)
        assert torch.equal(o0, o1) and torch.equal(r0, r1) and torch.equal(d0, d1) and torch.equal(i0.status, i1.status), s
        assert torch.equal(i0.adblGrumpyState, i1.adblGrumpyState) and torch.equal(i0.dblGrumpyScore, i1.dblGrumpyScore), s
    a, b = envs[0].get_state(), envs[1].get_state()
    assert all(torch.equal(a[k].nan_to_num(7e77) if a[k].dtype.is_floating_point else a[k],
                           b[k].nan_to_num(7e77) if b[k].dtype.is_floating_point else b[k]) for k in a)


def test_hive_observe_refuses_bad_arguments_with_a_message():
    from roborugby_amd import _lib
    env = _env("G", 64)
    L = env._lib
    assign = torch.empty(64, 4, dtype=torch.int32, device="cuda")
    obs = torch.empty(64, 4, 11, device="cuda")
    obs64 = torch.empty(64, 4, 11, dtype=torch.float64, device="cuda")
    ap, op, op64 = C.c_void_p(assign.data_ptr()), C.c_void_p(obs.data_ptr()), C.c_void_p(obs64.data_ptr())
    for fn, o in ((L.rr_hive_observe, op), (L.rr_hive_observe_f64, op64)):
        assert fn(env._h, 3, 0, ap, o, None) == 0 and fn(env._h, 15, 1, ap, o, None) == 0
        for args, word in (((None, 3, 0, ap, o, None), b"null"), ((env._h, 3, 0, None, o, None), b"null"), ((env._h, 3, 0, ap, None, None), b"null"),
                           ((env._h, 3, 2, ap, o, None), b"kind"), ((env._h, 3, -1, ap, o, None), b"kind"),
                           ((env._h, 16, 0, ap, o, None), b"mask"), ((env._h, 0x80000001, 0, ap, o, None), b"mask"),
                           ((env._h, 0, 0, ap, o, None), b"empty")):
            assert fn(*args) == -1, args
            assert word in L.rr_last_error(), (args, L.rr_last_error())
    with pytest.raises(_lib.RRError):
        env.hive_observe(0)
    f32 = _env("G", 64, dtype="f32")
    assert f32._lib.rr_hive_observe_f64(f32._h, 3, 0, ap, op64, None) == -1 and b"RR_DTYPE_F32" in f32._lib.rr_last_error()
    assert f32._lib.rr_hive_observe(f32._h, 3, 0, ap, op, None) == 0
    torch.cuda.synchronize()
    env.close(); f32.close()


def test_a_T_trained_checkpoint_plays_the_full_game(tmp_path):
    from roborugby_amd import dqn
    ck = str(tmp_path / "ck.pt")
    dqn.train(num_envs=1024, steps=6, preset="T", checkpoint=ck, log_every=0, batch_size=1024)
    res = dqn.play_hive(ck, num_envs=512, steps=8, seed=2)
    assert res["mode"] == "play_hive" and res["preset"] == "G" and res["hive_robots"] == [0, 1]
    assert np.isfinite(res["return_happy"]) and np.isfinite(res["return_grumpy"]) and res["env_steps_per_s"] > 0
    assert res["return_happy"] != 0.0  # somebody moved
