"""Every entry the C-ABI offers on a handle besides rr_step with the fused stack, on an RR_DTYPE_F32_STATE handle (fp32 records, fp64
arithmetic: each a `Store = float, Real = double` instantiation that widens on read and rounds on write) and on an RR_DTYPE_F32 handle
(each a `float` instantiation), against a reference: the fp64 oracle started from the state AS THE HANDLE HOLDS IT (get_state() after
set_state(): fp32-representable) and keepers_ref, the reward keepers restated from the reference's text.  Every comparison is one step,
or none, so the contact-step chaos fp32_checks.score has to handle never enters -- except in the thrust checks, which reuse the bars
test_gpu_fp32.py applies to rr_step.  Bars, bounds and helpers: tests/fp32_entry_checks.py; CPU twin: tests/test_fp32_entries_emulated.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import budget_driver as bd
import fp32_checks as fc
import fp32_entry_checks as ec
import oracle_lib as ol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
TOL64 = ec.TOL64
NAMES = {0: "SingleBall_6wayLidar_v2", 1: "SingleBall_6wayLidar", 2: "PosBall_BasicLidar", 3: "AllCoords", 4: "AllCoords_WithPrior"}
CAP = {"T": 1500, "G": 400, "Dwide": 800, "D": 800}  # arenas per handle (the oracle runs 17 set-ups per arena for the sensitivity)


def _env(preset, n, dtype, **kw):
    import roborugby_amd as rr
    kw.setdefault("time_limit", False)
    kw.setdefault("auto_reset", False)
    return rr.BatchedRoboRugbyEnv(n, preset=ol.product_preset(preset), dtype=dtype, **kw)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _hold(env, st):
    """set the state, return it as the handle holds it"""
    env.set_state(st["robots"], st["robots_i"], st["balls"], st["step"])
    return _np(env.get_state())


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _f32_representable(st):
    return all(_same(ec.r32(st[k]), st[k]) for k in ("robots", "balls"))


# ---------------------------------------------------------------------------------------------------- references, computed once
@functools.lru_cache(maxsize=None)
def _observer_reference(preset):
    """golden states rounded to fp32 (what either fp32 handle holds after set_state), the oracle's observations of them for every
    query, and the oracle's own lidar sensitivity -- shared by the fp32-state and the fp32 test, left unchanged"""
    st = ec.golden_states(GOLDEN, preset, CAP[preset])
    st = {k: (ec.r32(v) if v.dtype == np.float64 else v) for k, v in st.items()}
    queries = ec.observer_queries(preset)
    n = len(st["step"])
    ref = None
    for i in range(n):
        f = ec.oracle_observations(preset, st, queries, i)
        if ref is None:
            ref = [None if x is None else np.zeros((n, len(x))) for x in f]
        for q, x in enumerate(f):
            assert (x is None) == (ref[q] is None)
            if x is not None:
                ref[q][i] = x
    return st, queries, ref, ec.lidar_sensitivity(preset, st)


def _observe_all(env, queries, f64):
    out = []
    for k, t, r, b in queries:
        o = env.get_game_state(t, r, b, f64=f64, observer=NAMES[k])
        out.append(None if o is None else o.double().cpu().numpy())
    return out


def _allcoords_want(preset, st, team, prior=None):
    """AllCoords (RR_Observers.py:47-83) / AllCoords_WithPrior (:86-110) from a state dict: own team's robots first"""
    nrh, nr, nbp, nb = ec.counts(preset)
    own = list(range(nrh)) if team == 1 else list(range(nrh, nr))
    order = own + [r for r in range(nr) if r not in own]
    n = len(st["step"])
    if prior is None:
        return np.concatenate([st["robots"][:, order][:, :, [0, 1, 6]].reshape(n, -1), st["balls"][:, :, :2].reshape(n, -1)], axis=1)
    pr = prior["robots"][:, order][:, :, [0, 1, 6]].copy()
    # rectDblPriorStep is FloatRect.copy(): its rotation setter stores (rot + 720) % 360 (MyUtils.py:150-154, 277-279) -- the value itself for
    # every stored rotation in [2^-19, 360) (the sum is exact in fp64), and 0 where a rotation just below 360 was ROUNDED to the float 360
    in_range = (pr[..., 2] >= 2.0 ** -19) & (pr[..., 2] < 360.0)
    assert in_range.mean() > 0.95 and np.array_equal(np.mod(pr[..., 2] + 720.0, 360.0)[in_range], pr[..., 2][in_range])
    pr[..., 2] = np.mod(pr[..., 2] + 720.0, 360.0)
    rob = np.concatenate([st["robots"][:, order][:, :, [0, 1, 6]], pr], axis=2)
    bal = np.concatenate([st["balls"][:, :, :2], prior["balls"][:, :, :2]], axis=2)
    return np.concatenate([rob.reshape(n, -1), bal.reshape(n, -1)], axis=1)


def _thrust_steps(preset):
    t = dict(np.load(f"{GOLDEN}/thrust_{preset}.npz"))
    idx = [(ep, s) for ep in range(t["length"].shape[0]) for s in range(int(t["length"][ep]))]
    ep = np.array([i[0] for i in idx]); s = np.array([i[1] for i in idx])
    pre = {k: t["state_" + k][ep, s] for k in ("robots", "robots_i", "balls", "step")}
    post = {k: t["state_" + k][ep, s + 1] for k in ("robots", "robots_i", "balls", "step")}
    th = t["thrust"][ep, s].astype(np.float32)  # [n, NR, 2], NaN rows = robots that got no pair (the C-ABI takes float32)
    return pre, post, th, t["done"][ep, s]


def _run_thrust(preset, dtype, pre, th, f64):
    """every recorded thrust step through one handle per number of pairs: state after, outputs, held pre-state"""
    nk = (~np.isnan(th[:, :, 0])).sum(1)
    n = len(nk)
    got = {k: np.zeros_like(pre[k]) for k in ("robots", "robots_i", "balls")}
    held = {k: np.zeros_like(pre[k]) for k in ("robots", "robots_i", "balls", "step")}
    out = dict(obs=np.zeros((n, 11)), obs_g=np.zeros((n, 11)), reward=np.zeros(n), reward_g=np.zeros(n), done=np.zeros(n, bool), status=np.zeros(n, np.int64))
    for k in np.unique(nk):
        sel = np.nonzero(nk == k)[0]
        env = _env(preset, len(sel), dtype, action_mode="thrust")
        h = _hold(env, {kk: v[sel] for kk, v in pre.items()})
        for kk in held:
            held[kk][sel] = h[kk]
        o, r, d, info = env.step_thrust(torch.as_tensor(th[sel][:, :k].reshape(len(sel), 2 * k)), f64=f64)
        st = _np(env.get_state())
        for kk in got:
            got[kk][sel] = st[kk]
        out["obs"][sel], out["reward"][sel], out["done"][sel] = o.double().cpu().numpy(), r.double().cpu().numpy(), d.cpu().numpy()
        out["reward_g"][sel], out["status"][sel] = info.dblGrumpyScore.double().cpu().numpy(), info.status.cpu().numpy()
        if info.adblGrumpyState is not None:
            out["obs_g"][sel] = info.adblGrumpyState.double().cpu().numpy()
        env.close()
    return held, got, out


# ====================================================================================================== 2. the fp32-state handle
@pytest.mark.parametrize("preset", ["T", "G", "D"])
def test_f32_state_thrust_entry_is_the_oracle_on_the_rounded_state(preset):
    """rr_step_thrust_f64 on an RR_DTYPE_F32_STATE handle over the reference's GameEnv.step vectors (thrust_*.npz), the two claims of
    test_gpu_fp32._assert_state_mode with its accepted shares: the outputs are the fp64 oracle's from the SAME fp32-rounded state within
    1e-9 and the stored post-state is the oracle's rounded to fp32, to one fp32 ulp, integer state equal -- on >= 99.9 % of the steps (the
    library's sin / cos are not the oracle's to the last bit, so a knife-edge predicate may fall the other way on a few)."""
    pre, post, th, done = _thrust_steps(preset)
    held, got, out = _run_thrust(preset, "f32_state", pre, th, f64=True)
    assert _f32_representable(held) and _f32_representable(got)
    n = len(done)
    e_out, ref = np.zeros(n), {k: np.zeros_like(got[k]) for k in got}
    has_g = ol.PRESETS[preset]["nr_g"] > 0
    for i in range(n):
        o = ec.oracle_at(preset, held, i)
        r = o.step_thrust(th[i][~np.isnan(th[i][:, 0])].astype(np.float64))
        st = o.get_state()
        ref["robots"][i], ref["balls"][i], ref["robots_i"][i] = ec.r32(st["robots"]), ec.r32(st["balls"]), st["robots_i"]
        e = max(np.abs(r["obs"] - out["obs"][i]).max(), abs(r["reward"] - out["reward"][i]), abs(r["reward_g"] - out["reward_g"][i]))
        if has_g:
            e = max(e, np.abs(r["obs_g"] - out["obs_g"][i]).max())
        e_out[i] = e if r["done"] == out["done"][i] and r["naughty"] == (out["status"][i] >> 16) & 0xFF else np.inf
    e_k = np.maximum(fc.rel_err(got["robots"], ref["robots"]), fc.rel_err(got["balls"], ref["balls"]))
    same_i = np.all(got["robots_i"] == ref["robots_i"], axis=(1, 2))
    print(f"[{preset} thrust, fp32 state] {n} steps vs the oracle on the same rounded state: outputs within 1e-9 on {100 * (e_out <= TOL64).mean():.3f} % "
          f"(median {np.median(e_out):.1e}); stored state: max rel err {e_k.max():.2e} (one fp32 ulp = 1.2e-7), within it on "
          f"{100 * (e_k <= 2.5e-7).mean():.3f} %, integer state equal in {100 * same_i.mean():.3f} %")
    assert (e_out <= TOL64).mean() >= 0.999, preset
    assert (e_k <= 2.5e-7).mean() >= 0.999 and same_i.mean() >= 0.999, (preset, float(e_k.max()), float(same_i.mean()))
    assert np.array_equal(out["done"], done.astype(bool))


@pytest.mark.parametrize("preset", ["T", "G", "Dwide"])
def test_f32_state_observers_are_the_oracle_on_the_stored_state(preset):
    """rr_observe_f64 and rr_observe_kind_f64 (kinds 0..3) on an RR_DTYPE_F32_STATE handle, no step: every robot, balls 0 and NB-1, both
    teams and the defaults, within 1e-9 of the oracle on the same state (AllCoords: equal), None exactly where the reference returns None."""
    from roborugby_amd import _lib
    st, queries, ref, _ = _observer_reference(preset)
    env = _env(preset, len(st["step"]), "f32_state")
    held = _hold(env, st)
    assert _same(held["robots"][..., :7], st["robots"][..., :7]) and all(_same(held[k], st[k]) for k in ("robots_i", "balls", "step"))
    got = _observe_all(env, queries, f64=True)
    worst = 0.0
    for q, (g, f) in enumerate(zip(got, ref)):
        assert (g is None) == (f is None), (preset, queries[q])
        if f is not None:
            worst = max(worst, float(np.abs(g - f).max()))
            assert np.abs(g - f).max() < TOL64, (preset, queries[q], float(np.abs(g - f).max()))
    # rr_observe_f64 (the default observer's own entry) gives what rr_observe_kind_f64(kind 0) gives
    for q, (k, t, r, b) in enumerate(queries):
        if k == 0 and ref[q] is not None:
            o = torch.full((env.num_envs, 11), float("nan"), dtype=torch.float64, device="cuda")
            _lib.check(env._lib.rr_observe_f64(env._h, t, r, b, C.c_void_p(o.data_ptr()), env._stream()), "rr_observe_f64", env._lib)
            assert _same(o.cpu().numpy(), got[q]), (preset, queries[q])
    for team in (1, -1):
        g = env.get_game_state(team, f64=True, observer="AllCoords").cpu().numpy()
        assert _same(g, _allcoords_want(preset, held, team)), (preset, team)
    print(f"[{preset}] fp32-state observers, {len(queries)} queries x {env.num_envs} arenas: worst |delta| {worst:.2e}")
    env.close()


@pytest.mark.parametrize("dtype", ["f32_state", "f32"])
@pytest.mark.parametrize("preset", ["T", "G", "Dwide"])
def test_allcoords_and_prior_columns_are_the_stored_state_bit_for_bit(preset, dtype):
    """AllCoords equals get_state() (cast to fp32 for the float entry) in both team orders; after one step AllCoords_WithPrior's prior
    columns are the pre-step get_state() values and its current columns the post-step ones, bit for bit.  (One exception, the
    reference's own: 18 of the G states hold a rotation such as 359.99999999999727 that is the float 360 once stored; the prior-step copy
    normalises it to 0 as FloatRect.copy() does -- _allcoords_want.  Everywhere else the prior rotation is the stored one.)"""
    st, acts, stack, _ = ec.mix_steps(GOLDEN, preset, 0, CAP[preset])
    env = _env(preset, len(acts), dtype, observer="AllCoords_WithPrior")
    pre = _hold(env, st)
    assert _f32_representable(pre)
    for team in (1, -1):
        g = env.get_game_state(team, observer="AllCoords")
        assert g.dtype == torch.float32 and _same(g.cpu().numpy(), _allcoords_want(preset, pre, team).astype(np.float32)), (preset, dtype, team)
    a = torch.as_tensor(acts, device="cuda")
    (env.step_f64 if dtype == "f32_state" else env.step)(a)
    post = _np(env.get_state())
    assert not _same(post["robots"][:, :, :2], pre["robots"][:, :, :2])  # (the robots did move)
    for team in (1, -1):
        for f64 in ((True, False) if dtype == "f32_state" else (False,)):
            g = env.get_game_state(team, f64=f64).cpu().numpy()
            want = _allcoords_want(preset, post, team, prior=pre)
            assert _same(g, want if f64 else want.astype(np.float32)), (preset, dtype, team, f64)
    env.close()


def _reward_case(preset, case, dtype):
    st, acts, stack, prog, n_blocked = ec.reward_case(GOLDEN, preset, case, CAP[preset])
    env = _env(preset, len(acts), dtype, rewards=stack)
    pre = _hold(env, st)
    a = torch.as_tensor(acts, device="cuda")
    o, r, d, info = env.step_f64(a) if dtype == "f32_state" else env.step(a)
    post = _np(env.get_state())
    status = info.status.cpu().numpy()
    rew = np.stack([r.double().cpu().numpy(), info.dblGrumpyScore.double().cpu().numpy()], axis=1)
    env.close()
    return prog, pre, post, acts, (status >> 16) & 0xFF, status & 0xFFFF, rew, n_blocked


@pytest.mark.parametrize("case", ec.REWARD_CASES)
@pytest.mark.parametrize("preset", ["T", "G", "Dwide"])
def test_f32_state_reward_stacks(preset, case):
    """Both keeper stacks of mix_*.npz, and DontDriveInGoals alone (k_extras_begin / k_extras_end, Store = float, Real = double), through
    rewards= and step_f64, one step from recorded states plus the blocked arenas: against keepers_ref on the handle's own pre / post
    get_state() and against the oracle's step from the same rounded state, both within the fp32-state reward_bound (the rounding of the
    stored post-state)."""
    prog, pre, post, acts, naughty, flags, rew, nb_ = _reward_case(preset, case, "f32_state")
    tag = f"{preset} stack {case} fp32 state"
    ec.check_rewards(tag, preset, prog, "f32_state", pre, post, naughty, rew, nb_)
    # ... and sharper than the issue's bound, by reasoning: k_extras_end reads the STORED post-state, the very numbers keepers_ref is
    # given, and computes in fp64 -- so the two differ by fp64 round-off only; 1e-7 is what keepers_ref itself is validated to against
    # the goldens.  (A keeper accumulated in float would be off by ~1e-4: inside the bound above, outside this one.)
    rh, rg = ec.keepers_ref(preset, prog, pre, post, naughty)
    assert np.abs(rew[:, 0] - rh).max() < 1e-7 and np.abs(rew[:, 1] - rg).max() < 1e-7, tag
    bh, bg = ec.reward_bound(preset, prog, "f32_state")
    worst = 0.0
    for i in range(len(acts)):
        o = ec.oracle_at(preset, pre, i)
        o.set_program(prog)
        res = o.step(acts[i])
        assert res["naughty"] == naughty[i] and (res["status"] & 63) == (flags[i] & 63), (tag, i)
        eh, eg = abs(res["reward"] - rew[i, 0]), abs(res["reward_g"] - rew[i, 1])
        worst = max(worst, eh, eg)
        assert eh <= bh and eg <= bg, (tag, i, eh, eg, bh, bg)
    print(f"[{tag}] vs the oracle's step from the same rounded state: worst {worst:.3e} (bound {bh:.3e} / {bg:.3e})")


_GOAL_ORACLE = {}  # (state bytes, steps) -> ec.goal_oracle's result: both dtypes hold the same state, so the oracle runs once


@pytest.mark.parametrize("dtype", ["f32_state", "f32"])
def test_goal_scoring_equals_the_oracle_exactly(dtype):
    """k_goal on an fp32-state / fp32 handle: the crafted batch of test_gpu_goal.py (balls in and around both triangles, no centre within
    1e-3 px of an edge), the 150-step stay and ten more steps: rewards (+-500, else 0), done, the status words, goal_scores and the
    parked balls equal the oracle's from the state the handle holds, exactly."""
    steps = 160
    robots, balls = ec.goal_batch(256)
    n = len(robots)
    env = _env("T", n, dtype, goal_scoring=True)
    env.set_poses(robots, balls)
    st = _np(env.get_state())
    assert _same(st["balls"][:, :, :2], balls[:, :, :2]) and _f32_representable(st)
    acts = torch.full((n, 1), 8, dtype=torch.int32, device="cuda")  # nobody moves
    R, D, S = [], [], []
    for s in range(steps):
        o, r, d, info = env.step_f64(acts) if dtype == "f32_state" else env.step(acts)
        R.append(r.double()); D.append(d); S.append(info.status & 0xFFFF)
    R, D, S = torch.stack(R).cpu().numpy(), torch.stack(D).cpu().numpy(), torch.stack(S).cpu().numpy()
    key = (st["robots"].tobytes(), st["balls"].tobytes(), steps)
    if key not in _GOAL_ORACLE:
        _GOAL_ORACLE[key] = ec.goal_oracle(st, steps)
    consumed = ec.check_goal(f"T {dtype}", _GOAL_ORACLE[key], R, D, S, env.goal_scores().cpu().numpy(), _np(env.get_state())["balls"])
    print(f"[T goal scoring, {dtype}] {consumed} of {n} balls consumed, everything equal to the oracle")
    env.close()


@pytest.mark.parametrize("preset", ["T", "G", "Dwide"])
def test_f32_state_reset_and_poses_equal_the_oracle_draws(preset):
    """reset(), reset(bln_randomize_pos=False) (rr_reset_to_poses: back to the construction's placement) and set_poses on an fp32-state
    handle, n = 257: the centres and rotations are the oracle's draws, equal; the derived edges are the oracle's rounded to fp32 to one
    ulp; the first observation is the oracle's within 1e-9 (rr_observe_f64 on the stored state)."""
    n, seed = 257, 21
    env = _env(preset, n, "f32_state", seed=seed)
    draws = []
    for episode in (0, 1):
        d = {k: [] for k in ("robots", "balls")}
        for a in range(n):
            o = ol.OracleEnv(preset)
            for e in range(episode + 1):
                o.reset(seed, a, e)
            s = o.get_state()
            d["robots"].append(s["robots"]); d["balls"].append(s["balls"])
        draws.append({k: np.array(v) for k, v in d.items()})

    def check(what, want):
        st = _np(env.get_state())
        assert _f32_representable(st), what
        assert _same(st["robots"][:, :, [0, 1, 6]], want["robots"][:, :, [0, 1, 6]]) and _same(st["balls"][:, :, [0, 1, 6, 7]], want["balls"][:, :, [0, 1, 6, 7]]), (preset, what)
        assert fc.rel_err(st["robots"][:, :, :7], ec.r32(want["robots"][:, :, :7])).max() <= 2.5e-7, (preset, what)
        assert fc.rel_err(st["balls"], ec.r32(want["balls"])).max() <= 2.5e-7, (preset, what)
        return st

    check("construction", draws[0])
    env.reset()
    st1 = check("reset()", draws[1])
    obs = env.get_game_state(1, f64=True, observer="SingleBall_6wayLidar_v2").cpu().numpy()
    for a in range(0, n, 8):
        o = ol.OracleEnv(preset)
        o.set_state(st1["robots"][a], st1["robots_i"][a], st1["balls"][a], None, int(st1["step"][a]))
        assert np.abs(o.observe(1) - obs[a]).max() < TOL64, (preset, a)
    env.reset(bln_randomize_pos=False)
    check("reset(bln_randomize_pos=False)", draws[0])
    mask = np.arange(n) % 2 == 0
    env.reset(torch.as_tensor(mask))  # episode 2 for the even arenas; the odd ones keep the start placement
    st = _np(env.get_state())
    assert _same(st["robots"][~mask][:, :, [0, 1, 6]], draws[0]["robots"][~mask][:, :, [0, 1, 6]])
    assert not _same(st["robots"][mask][:, :, [0, 1, 6]], draws[0]["robots"][mask][:, :, [0, 1, 6]])
    bxyv = np.concatenate([draws[1]["balls"][:, :, :2], np.zeros_like(draws[1]["balls"][:, :, :2])], axis=2)
    env.set_poses(draws[1]["robots"][:, :, [0, 1, 6]], bxyv)
    check("set_poses", draws[1])
    env.close()


@pytest.mark.parametrize("preset", ["T", "G", "Dwide"])
def test_f32_state_rollout_of_one_step_equals_step(preset):
    """rr_rollout on an fp32-state handle: S = 1 is one rr_step bit for bit (outputs and stored state); S = 2 and repeat = 2 would keep
    unrounded state across steps and are still refused, leaving the handle as it was."""
    n, seed = 257, 6
    envs = [_env(preset, n, "f32_state", seed=seed, time_limit=True, auto_reset=True) for _ in range(2)]
    na = envs[0].preset.nr
    for e in envs:
        e.reset()
    gen = torch.Generator(device="cuda"); gen.manual_seed(8)
    acts = torch.randint(0, 8, (1, n, na), generator=gen, device="cuda", dtype=torch.int32)
    o, r, d, info = envs[0].step(acts[0])
    o2, r2, d2, info2 = envs[1].rollout(acts)
    assert torch.equal(o2[0], o) and torch.equal(r2[0], r) and torch.equal(d2[0], d) and torch.equal(info2.status[0], info.status)
    assert torch.equal(info2.dblGrumpyScore[0], info.dblGrumpyScore)
    if info.adblGrumpyState is not None:
        assert torch.equal(info2.adblGrumpyState[0], info.adblGrumpyState)
    a, b = _np(envs[0].get_state()), _np(envs[1].get_state())
    assert all(_same(a[k], b[k]) for k in a)
    with pytest.raises(RuntimeError, match="F32_STATE"):
        envs[1].rollout(torch.cat([acts, acts]))
    with pytest.raises(RuntimeError, match="F32_STATE"):
        envs[1].rollout(acts[0], repeat=2)
    torch.cuda.synchronize()
    b2 = _np(envs[1].get_state())
    assert all(_same(b[k], b2[k]) for k in b)
    for e in envs:
        e.close()


# ====================================================================================================== 3. the fp32 handle
@pytest.mark.parametrize("preset", ["T", "G"])
def test_f32_rollout_in_one_launch_equals_step_by_step(preset):
    """the fp32 twin of test_gpu_shortcuts.py::test_rollout_in_one_launch_equals_step_by_step at n = 513: rollout(acts) with S = 9 and
    repeat = 4 against S step() calls, every output and the final state bit for bit, an auto-reset inside the launch."""
    n, S = 513, 9
    gen = torch.Generator(device="cuda"); gen.manual_seed(4)
    envs = [_env(preset, n, "f32", seed=11, time_limit=True, auto_reset=True) for _ in range(2)]
    na = envs[0].preset.nr
    acts = torch.randint(0, 8, (S, n, na), generator=gen, device="cuda", dtype=torch.int32)
    for e in envs:
        e.reset()
        st = e.get_state()
        st["step"][: n // 2] = e.preset.game_len_steps - 4  # half of the arenas finish (and are re-placed) inside the rollout
        e.set_state(st["robots"], st["robots_i"], st["balls"], st["step"])
    ref = [envs[0].step(acts[s]) for s in range(S)]
    o, r, d, info = envs[1].rollout(acts)
    for s in range(S):
        assert torch.equal(o[s], ref[s][0]) and torch.equal(r[s], ref[s][1]) and torch.equal(d[s], ref[s][2]), (preset, s)
        assert torch.equal(info.status[s], ref[s][3].status) and torch.equal(info.dblGrumpyScore[s], ref[s][3].dblGrumpyScore)
        if info.adblGrumpyState is not None:
            assert torch.equal(info.adblGrumpyState[s], ref[s][3].adblGrumpyState)
    a, b = _np(envs[0].get_state()), _np(envs[1].get_state())
    assert all(_same(a[k], b[k]) for k in a)
    assert int(d.sum()) >= n // 2  # the episode boundary really was inside
    rep = [envs[0].step(acts[0]) for _ in range(4)]
    o2, r2, d2, i2 = envs[1].rollout(acts[0], repeat=4)
    for s in range(4):
        assert torch.equal(o2[s], rep[s][0]) and torch.equal(r2[s], rep[s][1]) and torch.equal(d2[s], rep[s][2]), (preset, "repeat", s)
        assert torch.equal(i2.status[s], rep[s][3].status) and torch.equal(i2.dblGrumpyScore[s], rep[s][3].dblGrumpyScore)
        if i2.adblGrumpyState is not None:
            assert torch.equal(i2.adblGrumpyState[s], rep[s][3].adblGrumpyState)
    a, b = _np(envs[0].get_state()), _np(envs[1].get_state())
    assert all(_same(a[k], b[k]) for k in a)
    for e in envs:
        e.close()


@pytest.mark.parametrize("preset", ["T", "G"])
def test_f32_budgeted_equals_synchronous_on_stuck_chase_arenas(preset):
    """the fp32 twin of test_gpu_budget.py::test_budgeted_equals_synchronous_on_stuck_chase_arenas: a budgeted fp32 handle driven by
    budget_driver.streams equals the synchronous fp32 handle, stream for stream, bit for bit."""
    import roborugby_amd as rr
    d = np.load(os.path.join(HERE, "data", f"stuck_chase_{preset}.npz"))
    n, na = len(d["step"]), d["actions"].shape[1]
    steps = 10
    g = torch.Generator(device="cuda").manual_seed(5)
    table = torch.randint(0, 8, (steps, n, na), generator=g, device="cuda", dtype=torch.int32)
    keep = torch.rand(steps, n, generator=g, device="cuda") < 0.7
    table = torch.where(keep.unsqueeze(-1), torch.as_tensor(d["actions"], device="cuda").to(torch.int32).expand(steps, n, na), table)
    ref = None
    for budget in (0, 1, 50_000, 400_000):
        env = rr.BatchedRoboRugbyEnv(n, preset=preset, seed=3, time_limit=True, auto_reset=True, step_budget_clocks=budget, dtype="f32")
        env.set_state(d["robots"], d["robots_i"], d["balls"], d["step"])
        got, calls, nr = bd.streams(env, table, steps, budget > 0, 2000, extras=(lambda e: e.get_state()["robots"], lambda e: e.get_state()["balls"]))
        env.close()
        if ref is None:
            ref = got
            assert calls == steps and nr == 0
        else:
            assert bd.equal(got, ref), (preset, budget)
            if budget == 1:
                assert nr > n  # these arenas are the stuck ones: with a 1-clock budget they park over and over
        print(f"[{preset} fp32] budget {budget}: {calls} calls for {steps} steps of {n} stuck arenas, {nr} NOT_READY rows")


def test_f32_handle_refuses_every_f64_entry_and_touches_nothing():
    """rr_step_f64, rr_step_thrust_f64, rr_observe_f64 and rr_observe_kind_f64 on an RR_DTYPE_F32 handle: -1 with the documented
    message, outputs and state as they were (the hive's _f64 entries: test_gpu_hive_budget.py, test_gpu_hive_transition.py)."""
    n = 64
    env = _env("G", n, "f32", seed=4)
    env.reset()
    before = _np(env.get_state())
    p = lambda t: C.c_void_p(t.data_ptr())
    f = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device="cuda")
    acts, thrust = torch.zeros(n, 4, dtype=torch.int32, device="cuda"), torch.ones(n, 8, dtype=torch.float32, device="cuda")
    obs, rew, obs_g, rew_g = f(n, 11), f(n), f(n, 11), f(n)
    done, status = torch.full((n,), 9, dtype=torch.uint8, device="cuda"), torch.full((n,), -3, dtype=torch.int32, device="cuda")
    wide = f(n, 28)
    L, s = env._lib, env._stream()
    needs_f64, is_f32 = b"fp64 outputs need a handle created with RR_DTYPE_F64", b"rr_observe_f64: handle was created with RR_DTYPE_F32"
    calls = [("rr_step_f64", lambda: L.rr_step_f64(env._h, p(acts), 4, p(obs), p(rew), p(done), p(obs_g), p(rew_g), p(status), s), needs_f64),
             ("rr_step_thrust_f64", lambda: L.rr_step_thrust_f64(env._h, p(thrust), 4, p(obs), p(rew), p(done), p(obs_g), p(rew_g), p(status), s), needs_f64),
             ("rr_observe_f64", lambda: L.rr_observe_f64(env._h, 1, -1, -1, p(obs), s), is_f32),
             ("rr_observe_kind_f64 v1", lambda: L.rr_observe_kind_f64(env._h, 1, 1, -1, -1, p(obs), 11, s), needs_f64),
             ("rr_observe_kind_f64 all", lambda: L.rr_observe_kind_f64(env._h, 3, 1, -1, -1, p(wide), 28, s), needs_f64)]
    for name, call, message in calls:
        # another refusal first, so that the message read below is the one THIS call set, not the previous call's
        assert L.rr_create(None, None) == -1 and L.rr_last_error() == b"rr_create: null argument"
        assert call() == -1, name
        assert L.rr_last_error() == message, (name, L.rr_last_error())
        torch.cuda.synchronize()
        assert all(bool((t == -7.0).all()) for t in (obs, rew, obs_g, rew_g, wide)) and bool((done == 9).all()) and bool((status == -3).all()), name
    after = _np(env.get_state())
    assert all(_same(before[k], after[k]) for k in before)
    with pytest.raises(RuntimeError, match="RR_DTYPE_F64"):
        env.get_game_state(1, f64=True, observer="PosBall_BasicLidar")
    env.close()


@pytest.mark.parametrize("case", ec.REWARD_CASES)
@pytest.mark.parametrize("preset", ["T", "G", "Dwide"])
def test_f32_reward_stacks_vs_keepers_ref(preset, case):
    """Both keeper stacks of mix_*.npz, and DontDriveInGoals alone, on an fp32 handle (the float instantiations of k_extras_begin /
    k_extras_end), one step from recorded states plus the blocked arenas, against keepers_ref on the handle's own pre / post get_state()
    and NaughtyBots bits.
    Stack B (NaughtyBots, KeepMovingGuys) and DontDriveInGoals alone (on stack A's states): within n x ulp32(.005), n = the team's
    robots x the program's count keepers; the blocked robots do not move and KeepMovingGuys' `==` fires in fp32 as in fp64; two of them
    stand inside a goal and DontDriveInGoals fires.  Stack A (the distance keepers with DontDriveInGoals and KeepMovingGuys): within
    reward_bound.  Wherever DontDriveInGoals runs, an arena with a robot corner within 1e-3 px of a goal-triangle edge is left out, at
    most 1 % of them (the reference's geometry decides)."""
    prog, pre, post, acts, naughty, flags, rew, nb_ = _reward_case(preset, case, "f32")
    assert _f32_representable(pre) and _f32_representable(post)
    ec.check_rewards(f"{preset} stack {case} fp32", preset, prog, "f32", pre, post, naughty, rew, nb_)


@pytest.mark.parametrize("preset", ["T", "G", "Dwide"])
def test_f32_observers_vs_oracle_on_the_same_state(preset):
    """rr_observe / rr_observe_kind (V2, V1, Basic) on an fp32 handle, no step, every robot / balls 0 and NB-1 / both teams / the defaults,
    against the fp64 oracle on the state the handle holds: angles on the circle within 4 ulp32(360) + degrees(2 ulp32(diag) / d), point
    distances within 4 ulp32(diag), lidar: p99 of rel_err < 2e-3 (the bar of test_f32_config2_rollout_vs_f64_oracle) and no value off by
    more than 1 px unless the oracle's own value moves by more than 0.1 px under one-ulp perturbations of the state (at most 0.5 % of the
    values; none on the golden states).  AllCoords in both team orders: get_state() cast to fp32, bit for bit.
    The error relative to max(sensitivity, ulp32(diag)) is printed, not asserted: DESIGN.md section 3 records it."""
    st, queries, ref, sens = _observer_reference(preset)
    env = _env(preset, len(st["step"]), "f32")
    held = _hold(env, st)
    assert _same(held["robots"][..., :7], st["robots"][..., :7]) and all(_same(held[k], st[k]) for k in ("robots_i", "balls", "step"))
    got = _observe_all(env, queries, f64=False)
    for team in (1, -1):
        g = env.get_game_state(team, observer="AllCoords").cpu().numpy()
        assert _same(g, _allcoords_want(preset, held, team).astype(np.float32)), (preset, team)
    env.close()
    ec.check_observers(f"{preset} fp32 device", preset, st, queries, got, ref, sens)


@pytest.mark.parametrize("preset", ["T", "G", "D"])
def test_f32_thrust_entry_distribution(preset):
    """rr_step_thrust on an fp32 handle over thrust_*.npz, scored by fp32_checks.score against the reference's fp64 vectors and held to
    the bars rr_step meets in this mode (fp32_checks.assert_distribution, as in test_gpu_fp32.py)."""
    pre, post, th, done = _thrust_steps(preset)
    held, got, out = _run_thrust(preset, "f32", pre, th, f64=False)
    cfg = ol.PRESETS[preset]
    q, e, ints = fc.score(pre, post, got, cfg["W"], cfg["H"])
    fc.assert_distribution(f"{preset} thrust fp32", q, e, ints, out["done"] == done.astype(bool))
