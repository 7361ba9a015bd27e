"""GPU parity tests proper: the HIP kernel, called through the C-ABI, against
  (1) the golden vectors captured from the reference (tests/golden/traj_*.npz) -- every recorded step is
      replayed as its own arena from the reference's dumped state, and
  (2) the CPU oracle on fresh seeded states.
Bar (fp64 mode): integer state / done / naughty-derived rewards exact; fp64 positions, observations and rewards
within 1e-9 absolute (the kernel repeats the reference's operation order; residual = libm vs ocml ulps).
fp32 mode: single step from synchronised state within 1e-5 * max(1, |x|)  (hard part 1)."""
import numpy as np
import pytest

import oracle_lib as ol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL64 = 1e-9


def _env(preset, n, **kw):
    import roborugby_amd as rr
    kw.setdefault("time_limit", False)
    kw.setdefault("auto_reset", False)
    return rr.BatchedRoboRugbyEnv(n, preset=ol.product_preset(preset), **kw)  # (Dwide, Ttall, Gwide: their shape's Preset at their W x H)


def _flatten_golden(t):
    """Every (episode, step) with a successor becomes one arena."""
    idx = [(ep, s) for ep in range(t["length"].shape[0]) for s in range(int(t["length"][ep]))]
    ep = np.array([i[0] for i in idx])
    s = np.array([i[1] for i in idx])
    pre = {k: t["state_" + k][ep, s] for k in ("robots", "robots_i", "balls", "step")}
    post = {k: t["state_" + k][ep, s + 1] for k in ("robots", "robots_i", "balls", "step")}
    out = {k: t[k][ep, s] for k in ("actions", "obs", "obs_g", "reward", "reward_g", "done", "naughty")}
    return pre, post, out


@pytest.mark.parametrize("preset,exact", [(p, e) for p in ("T", "G", "D") for e in (False, True)] + [("X", False)]
                         + [("Dwide", False), ("Dwide", True), ("Ttall", False)] + [("W", False), ("R", False)],
                         ids=lambda v: {False: "default", True: "exact_trig"}.get(v, v) if isinstance(v, bool) else v)
def test_step_matches_reference_golden_f64(golden_dir, preset, exact):
    """exact=True: the same bar for the exact-trig parity build (libroborugby_amd_exact.so).  Preset X (2 + 1 robots, 2 + 3 balls) is not
    one of the shapes inside the library: it runs through the one-shape library compiled on demand (build.build_shape_library).
    W (1 + 1 robots, 4 + 7 balls: 16 lanes per arena, 55 ball pairs) and R (4 + 4 robots, 2 + 2 balls: 8 robots, 32 ball-robot pairs) are the
    limits of such a library (build.shape_lanes), built by __graft_entry__.build().
    Dwide (1000 x 640) and Ttall (480 x 720) are the non-square arenas: every step that tells width from height -- walls, clamps, the
    ball / wall bounce with the reference's width-for-height line, lidar, goal corner, reward multiplier -- at W != H."""
    t = np.load(f"{golden_dir}/traj_{preset}.npz")
    pre, post, out = _flatten_golden(t)
    n = pre["step"].shape[0]
    env = _env(preset, n, exact_trig=exact)
    env.set_state(pre["robots"], pre["robots_i"], pre["balls"], pre["step"])
    acts = out["actions"].copy()
    na = env.preset.nr
    # episodes recorded with fewer actions than robots: the missing robots keep their thrust -> feed the action
    # that reproduces the thrust they already have is not possible in general, so group by NA instead
    na_used = (acts >= 0).sum(1)
    got_obs = torch.zeros(n, 11, dtype=torch.float64)
    results = {}
    for k in np.unique(na_used):
        sel = np.nonzero(na_used == k)[0]
        sub = _env(preset, len(sel), exact_trig=exact)
        sub.set_state(pre["robots"][sel], pre["robots_i"][sel], pre["balls"][sel], pre["step"][sel])
        o, r, d, info = sub.step_f64(torch.as_tensor(acts[sel][:, :k].astype(np.int32)))
        st = sub.get_state()
        results[k] = (sel, o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy(),
                      None if info.adblGrumpyState is None else info.adblGrumpyState.cpu().numpy(),
                      info.dblGrumpyScore.cpu().numpy(), info.status.cpu().numpy(),
                      {kk: v.cpu().numpy() for kk, v in st.items()})
    worst = 0.0
    for k, (sel, o, r, d, og, rg, status, st) in results.items():
        assert np.array_equal(st["robots_i"], post["robots_i"][sel])
        assert np.array_equal(st["step"], post["step"][sel])
        assert np.array_equal(np.isnan(st["robots"]), np.isnan(post["robots"][sel]))
        dr = np.nanmax(np.abs(st["robots"] - post["robots"][sel]))
        db = np.abs(st["balls"] - post["balls"][sel]).max()
        do = np.abs(o - out["obs"][sel]).max()
        drw = max(np.abs(r - out["reward"][sel]).max(), np.abs(rg - out["reward_g"][sel]).max())
        assert np.array_equal(d.astype(np.uint8), out["done"][sel])
        if og is not None:
            do = max(do, np.abs(og - out["obs_g"][sel]).max())
        assert (status & 0xFFFF & ~256).max() == 0
        if "naughty" in out:  # the robots NaughtyBots flagged travel in status bits 16+: exact
            assert np.array_equal((status >> 16) & 0xFF, out["naughty"][sel])
        worst = max(worst, dr, db, do, drw)
        print(f"[{preset}{' exact-trig build' if exact else ''}] {len(sel)} steps with {k} actions: robots {dr:.3e} balls {db:.3e} obs {do:.3e} rewards {drw:.3e}")
        assert dr < TOL64 and db < TOL64 and do < TOL64 and drw < 1e-7, (preset, k, dr, db, do, drw)
    print(f"[{preset}{' exact-trig build' if exact else ''}] {n} golden steps replayed on GPU, worst abs diff {worst:.3e}")


@pytest.mark.parametrize("preset", ["T", "G", "D", "X"])
def test_thrust_entry_matches_reference_golden(golden_dir, preset):
    """rr_step_thrust against the reference's own GameEnv.step vectors (RR_EnvBase.py:260-273, RR_Robot.py:100-102;
    tests/golden/thrust_*.npz, generated by driving the imported reference with Box thrust incl. +-0.5, +-1.5, +-2.5,
    0.49): every recorded step is one arena started from the reference's dumped state.  Integer state (thrust after
    round(), move counters), done and the NaughtyBots set exact; fp64 state AND observations within 1e-9, rewards within 1e-7
    (rr_step_thrust_f64)."""
    t = np.load(f"{golden_dir}/thrust_{preset}.npz")
    idx = [(ep, s) for ep in range(t["length"].shape[0]) for s in range(int(t["length"][ep]))]
    ep = np.array([i[0] for i in idx]); s = np.array([i[1] for i in idx])
    th = t["thrust"][ep, s]                       # [n, NR, 2], NaN rows = robots that got no pair
    nk = (~np.isnan(th[:, :, 0])).sum(1)
    assert np.array_equal(np.rint(th[~np.isnan(th)].astype(np.float32)), np.rint(th[~np.isnan(th)]))  # float32 ABI
    worst = 0.0
    for k in np.unique(nk):
        sel = np.nonzero(nk == k)[0]
        env = _env(preset, len(sel), action_mode="thrust")
        env.set_state(t["state_robots"][ep[sel], s[sel]], t["state_robots_i"][ep[sel], s[sel]], t["state_balls"][ep[sel], s[sel]],
                      t["state_step"][ep[sel], s[sel]])
        o, r, d, info = env.step_thrust(torch.as_tensor(th[sel][:, :k].reshape(len(sel), 2 * k).astype(np.float32)), f64=True)
        st = {kk: v.cpu().numpy() for kk, v in env.get_state().items()}
        post_r, post_b = t["state_robots"][ep[sel], s[sel] + 1], t["state_balls"][ep[sel], s[sel] + 1]
        assert np.array_equal(st["robots_i"], t["state_robots_i"][ep[sel], s[sel] + 1])
        assert np.array_equal(np.isnan(st["robots"]), np.isnan(post_r))
        dr = np.nanmax(np.abs(st["robots"] - post_r)); db = np.abs(st["balls"] - post_b).max()
        # rr_step_thrust_f64: observations and rewards of the thrust entry in fp64, both teams
        do = np.abs(o.cpu().numpy() - t["obs"][ep[sel], s[sel]]).max()
        drw = np.abs(r.cpu().numpy() - t["reward"][ep[sel], s[sel]]).max()
        if info.adblGrumpyState is not None and "obs_g" in t.files:
            do = max(do, np.abs(info.adblGrumpyState.cpu().numpy() - t["obs_g"][ep[sel], s[sel]]).max())
            drw = max(drw, np.abs(info.dblGrumpyScore.cpu().numpy() - t["reward_g"][ep[sel], s[sel]]).max())
        status = info.status.cpu().numpy()
        assert np.array_equal(d.cpu().numpy().astype(np.uint8), t["done"][ep[sel], s[sel]])
        assert np.array_equal((status >> 16) & 0xFF, t["naughty"][ep[sel], s[sel]])
        assert (status & 0xFFFF & ~256).max() == 0
        assert dr < TOL64 and db < TOL64 and do < TOL64 and drw < 1e-7, (preset, k, dr, db, do, drw)
        worst = max(worst, dr, db, do, drw)
        env.close()
    print(f"[{preset}] {len(idx)} golden thrust steps replayed on GPU, worst abs state diff {worst:.3e}")


@pytest.mark.parametrize("preset", ["T", "G", "D", "X", "Dwide", "Ttall", "Gwide", "W", "R"])
def test_reset_matches_oracle_bit_exact(preset):
    """Same Philox stream + same rejection rule -> identical placements and first observations."""
    n, seed = 257, 1234
    env = _env(preset, n, seed=seed, arena_offset=1000)
    obs = env.reset()
    st = {k: v.cpu().numpy() for k, v in env.get_state().items()}
    obs = obs.cpu().numpy()
    for a in (0, 1, 100, 256):
        o = ol.OracleEnv(preset)
        o.reset(seed, 1000 + a, 0)  # constructor placement
        o.reset(seed, 1000 + a, 1)  # env.reset()
        ost = o.get_state()
        assert np.array_equal(ost["robots"][:, [0, 1, 6]], st["robots"][a][:, [0, 1, 6]]), a
        assert np.allclose(ost["robots"][:, :7], st["robots"][a][:, :7], atol=1e-11, rtol=0), a
        assert np.array_equal(ost["balls"], st["balls"][a]), a
        assert np.allclose(o.observe(1), obs[a], rtol=0, atol=1e-3)
    assert (st["step"] == 0).all()


@pytest.mark.parametrize("preset", ["T", "G", "D", "X", "Dwide", "Ttall", "W", "R"])
def test_kernel_reset_distribution_matches_reference(golden_dir, preset):
    """The in-kernel reset (reset_arena, Philox) against the 1,000 layouts the imported reference's
    _set_random_positions produced (RR_EnvBase.py:155-200; tests/golden/reset_*.npz): 131,072 arenas constructed and
    reset once -- ranges with both end points, zero int-AABB overlaps (robots / goal boxes / balls), KS on every
    marginal, chi-square on the balls' occupancy; and the reference's own layouts, fed through rr_set_poses, give the
    first observations the reference's reset() returned."""
    import reset_checks as rc
    t = np.load(f"{golden_dir}/reset_{preset}.npz")
    cfg = ol.PRESETS[preset]
    n = 131072
    env = _env(preset, n, seed=77)
    env.reset()
    st = env.get_state()
    R, B = st["robots"].cpu().numpy(), st["balls"].cpu().numpy()
    assert (st["step"] == 0).all()
    rc.check_support(R, B, cfg["W"], cfg["H"])
    assert rc.overlaps(R, B, cfg["W"], cfg["H"]) == dict(robot_robot=0, ball_goal=0, ball_robot=0, ball_ball=0)
    assert (B[:, :, 6:] == 0).all() and np.isnan(R[:, :, 7:]).all()
    d = rc.ks_all(t["robots"], t["balls"], R, B, rot_col=6)
    p = rc.chi2_ball_occupancy(t["balls"], B, cfg["W"], cfg["H"])
    env.close()
    m = t["robots"].shape[0]
    env = _env(preset, m)
    env.set_poses(t["robots"], np.concatenate([t["balls"], np.zeros(t["balls"].shape[:2] + (2,))], axis=2))
    obs = env.get_game_state(1, f64=True).cpu().numpy()
    do = np.abs(obs - t["obs"]).max()
    assert do < TOL64, do
    print(f"[{preset}] {n} kernel layouts vs {m} reference layouts: max KS D = {d:.4f}, occupancy chi2 p = {p:.3f}; "
          f"first obs of the reference's layouts within {do:.2e}")


@pytest.mark.parametrize("preset", ["T", "G", "D"])
def test_free_running_episodes_vs_reference(golden_dir, preset):
    """Whole golden episodes replayed WITHOUT re-synchronisation (each episode = one arena started from the
    reference's step-0 state, driven by the recorded actions).  The dynamics are chaotic once contact responses
    fire: a 1-ulp libm/ocml difference is amplified by every bounce, so contact-rich episodes leave the reference
    trajectory after some tens of steps while contact-free ones stay within 1e-12 for all 301 steps
    (hard part 2 -- long-run parity is statistical).  Asserted here: every episode tracks
    the reference to 1e-9 for at least its first 20 steps, done flags are exact throughout, and a substantial share
    of the episodes tracks to the very end."""
    t = np.load(f"{golden_dir}/traj_{preset}.npz")
    na_used = (t["actions"][:, 0, :] >= 0).sum(1)
    full = np.nonzero(na_used == na_used.max())[0]  # episodes that drive every robot (one launch shape)
    env = _env(preset, len(full))
    env.set_state(t["state_robots"][full, 0], t["state_robots_i"][full, 0], t["state_balls"][full, 0], t["state_step"][full, 0])
    L = t["length"][full]
    first_bad = np.full(len(full), 10 ** 6)
    for s in range(int(L.max())):
        acts = np.clip(t["actions"][full, s, :na_used.max()], 0, 7).astype(np.int32)
        o, r, d, info = env.step_f64(torch.as_tensor(acts))
        o, d = o.cpu().numpy(), d.cpu().numpy()
        for i, ep in enumerate(full):
            if s < L[i]:
                assert bool(d[i]) == bool(t["done"][ep, s])
                if np.abs(o[i] - t["obs"][ep, s]).max() > 1e-9 and first_bad[i] > s:
                    first_bad[i] = s
    tracked = int((first_bad >= L).sum())
    print(f"[{preset}] {len(full)} free-running episodes: {tracked} track the reference to 1e-9 until their end; "
          f"first departure of the others at steps {sorted(int(x) for x in first_bad[first_bad < L])}")
    assert (np.minimum(first_bad, L) >= np.minimum(20, L)).all()
    # measured on the MI355X since round 2: 11 of 16 (T) and 11 of 15 (G) episodes stay within 1e-9 of the reference to their last
    # step; asserted exactly, so a change that loses tracked episodes fails here.  Which arithmetic difference makes the others
    # leave (the kernel's sin/cos in 21 episodes, the scratch-rect carry in 4) and where: profiles/r03/divergence_attribution.txt
    assert tracked == {"T": 11, "G": 11, "D": 6}[preset], tracked  # measured on the MI355X in rounds 2-3; exact, both directions


@pytest.mark.parametrize("preset,want", [("T", (4, 14)), ("G", (2, 12)), ("D", (1, 9))])
def test_exact_trig_build_follows_whole_episodes_bit_for_bit(golden_dir, preset, want):
    """The parity build (exact_trig=True -> libroborugby_amd_exact.so: sin / cos in double-double, ~correctly rounded, and the
    reference's scratch-rect carry, seeded from the golden `state_inner` through rr_set_scratch_rect)
    against the default build on the free-running golden episodes: counted is the number of episodes whose STATE (every robot and ball
    field the reference dumped after each step) equals the reference's BIT FOR BIT at every step to the last -- the state, not the
    observation: its atan2 is ocml's on the GPU and glibc's in the reference, a last-bit difference that never feeds back.  Host emulation of the same source (tests/test_parity_build.py): T 14 of 16,
    G 12 of 15, D 9 of 11 with the parity build against 4 / 2 / 1 with the default one; what is left is glibc's own rounding of
    sin / cos / pow (against the oracle with a correctly rounded libm: 42 of 42)."""
    t = np.load(f"{golden_dir}/traj_{preset}.npz")
    na_used = (t["actions"][:, 0, :] >= 0).sum(1)
    full = np.nonzero(na_used == na_used.max())[0]
    L = t["length"][full]
    counts = {}
    for exact in (False, True):
        env = _env(preset, len(full), exact_trig=exact)
        assert env.exact_trig == exact
        env.set_state(t["state_robots"][full, 0], t["state_robots_i"][full, 0], t["state_balls"][full, 0], t["state_step"][full, 0])
        if exact:
            env.set_scratch_rect(t["state_inner"][full, 0, :2])
            assert np.array_equal(env.get_scratch_rect().cpu().numpy(), t["state_inner"][full, 0, :2])
        else:
            with pytest.raises(RuntimeError):
                env.set_scratch_rect(t["state_inner"][full, 0, :2])
        first_bad = np.full(len(full), 10 ** 6)
        for s in range(int(L.max())):
            acts = np.clip(t["actions"][full, s, :na_used.max()], 0, 7).astype(np.int32)
            env.step_f64(torch.as_tensor(acts))
            st = env.get_state()
            R, B = st["robots"].cpu().numpy(), st["balls"].cpu().numpy()
            wr, wb = t["state_robots"][full, s + 1], t["state_balls"][full, s + 1]
            same = ((R == wr) | (np.isnan(R) & np.isnan(wr))).reshape(len(full), -1).all(1) & (B == wb).reshape(len(full), -1).all(1)
            bad = ~same & (s < L) & (first_bad > s)
            first_bad[bad] = s
        counts[exact] = int((first_bad >= L).sum())
        print(f"[{preset}] {'exact-trig' if exact else 'default'} build: {counts[exact]} of {len(full)} free-running episodes bit-identical to the "
              f"reference to their last step; first departures {sorted(int(x) for x in first_bad[first_bad < L])}")
        env.close()
    # (default build, parity build) as measured on the MI355X and on the host emulation of the same sources in round 3: exact
    assert (counts[False], counts[True]) == want, counts


@pytest.mark.parametrize("preset", ["T", "G", "D"])
def test_parity_build_equals_its_host_emulation_bit_for_bit_through_resets(preset):
    """The parity build on the MI355X against the same source run as a host-emulated wave (tests/emu_lib.py, which
    tests/test_parity_build.py pins to the reference arithmetic under a correctly rounded libm): 48 arenas from the constructor
    placement, 25 random steps, a reset (which moves the balls and leaves the scratch rect where it was), 25 more -- every state
    field and the rect's centre bit-identical after every step."""
    import emu_lib as el
    n, seed = 48, 5
    env = _env(preset, n, seed=seed, exact_trig=True)
    emus = [el.EmuEnv(preset, seed=seed, exact=True) for _ in range(n)]
    na = env.preset.nr
    rng = np.random.RandomState(3)
    for a, e in enumerate(emus):
        e.reset(a, 0)  # the constructor's placement
    episode = 0
    for phase in range(2):
        episode += 1
        env.reset()
        for a, e in enumerate(emus):
            e.reset(a, episode)
        for s in range(25):
            acts = rng.randint(0, 8, (n, na)).astype(np.int32)
            env.step_f64(torch.as_tensor(acts))
            st = {k: v.cpu().numpy() for k, v in env.get_state().items()}
            rect = env.get_scratch_rect().cpu().numpy()
            for a, e in enumerate(emus):
                e.step(acts[a])
                es = e.get_state()
                same = (np.array_equal(es["robots"], st["robots"][a], equal_nan=True) and np.array_equal(es["balls"], st["balls"][a])
                        and np.array_equal(es["robots_i"], st["robots_i"][a]))
                assert same, (preset, phase, s, a)
                assert np.array_equal(e.get_scratch_rect(), rect[a]), (preset, phase, s, a)
    env.close()
