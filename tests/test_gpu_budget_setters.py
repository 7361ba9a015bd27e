"""The budgeted step when the handle is changed while arenas are parked (a parked arena's step spans several calls).

Promise (include/roborugby_amd.h, the budgeted step): each arena's stream of obs, reward, done, status, obs_g, reward_g and episode
returns, as a function of the actions it ACCEPTED, is the synchronous step's bit for bit -- also across a setter or a masked reset
issued between two calls.  Per-arena differential test: the budgeted run applies the change between two calls and records c_i, the
steps arena i had completed by then; for every distinct c_i a synchronous run (budget 0, same seed, same state) applies the same
change just before accepted step c_i, and arena i's stream must equal that run's.  A setter on a budgeted handle either gives that
result or fails with -1 and changes nothing (refused while arenas are parked and their step-begin copies were not kept): then the
streams that follow are the synchronous ones without the change, and the same setter, retried after set_step_budget(0) and one
call, goes through -- the synchronous runs apply it where the retry did (case f).  The setters are called through the C-ABI
(env._lib / env._h) as a C caller would.  Fixtures: the stuck chase arenas (tests/data/stuck_chase_*.npz), which park from the
first call at these budgets."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

from budget_driver import streams  # noqa: E402

STACK = ("DontDriveInGoals", "KeepMovingGuys", "PushPosBallsToGoal", "ChasePosBall", "NaughtyBots")
OTHER = ("KeepMovingGuys", "PushPosBallsToGoal", "DontDriveInGoals")
STEPS = 8
EVENT_CALL = 2          # the change comes between call 2 and call 3 of the budgeted run
MAX_CALLS = 4000        # (a 1-clock budget: a squeezed G arena needs over a hundred calls per step)
NAMES = ("obs", "reward", "done", "status", "obs_g", "reward_g")


def _make(preset, budget, episodes=False, **kw):
    """the stuck arenas; episodes=True: time limit + auto-reset, every arena 2-5 steps before its time limit (episodes finish
    inside the window and the next ones start)"""
    import roborugby_amd as rr
    d = np.load(os.path.join(HERE, "data", f"stuck_chase_{preset}.npz"))
    n = len(d["step"])
    env = rr.BatchedRoboRugbyEnv(n, preset=preset, seed=3, time_limit=episodes, auto_reset=episodes, step_budget_clocks=budget, **kw)
    step = env.preset.game_len_steps - 2 - np.arange(n, dtype=np.int32) % 4 if episodes else d["step"]
    env.set_state(d["robots"], d["robots_i"], d["balls"], step)
    return env


def _table(env):
    na = env.preset.nr_happy + env.preset.nr_grumpy
    g = torch.Generator(device="cuda").manual_seed(11)
    t = torch.randint(0, 80, (STEPS, env.num_envs, na), generator=g, device="cuda", dtype=torch.int32)  # mostly "chase"
    t[:, :, 1:] %= 8
    return t


def _set_program(names):
    def setter(env):
        from roborugby_amd import _lib
        from roborugby_amd.env import keeper_exec_order
        prog = np.asarray(keeper_exec_order(names), np.int32)
        _lib.check(env._lib.rr_set_reward_program(env._h, prog.ctypes.data_as(C.c_void_p), len(prog)), "rr_set_reward_program", env._lib)
    return setter


def _track_prior(env):
    from roborugby_amd import _lib
    _lib.check(env._lib.rr_track_prior_step(env._h, 1, env._stream()), "rr_track_prior_step", env._lib)


def _goal_scoring(env):
    from roborugby_amd import _lib
    _lib.check(env._lib.rr_set_goal_scoring(env._h, 1, env._stream()), "rr_set_goal_scoring", env._lib)


def _returns(env):
    """episode bookkeeping after a step: running / last finished returns (fp64), episode index, length, count, last length, fault,
    and episode_stats()"""
    ep = env.get_episode_state()
    lr, lrg, ll, cnt = env.episode_stats()
    return torch.cat([ep["acc"], ep["ints"].double(), torch.stack([lr.double(), lrg.double(), ll.double(), cnt.double()], 1)], 1)


def _prior_coords(env):
    """observe_kind(4) (AllCoords_WithPrior): NaN rows while prior-step tracking is off"""
    from roborugby_amd import _lib
    try:
        return env.get_game_state(1, observer="AllCoords_WithPrior")
    except _lib.RRError:
        p = env.preset
        return torch.full((env.num_envs, 6 * p.nr + 4 * p.nb), float("nan"), device=env.device)


def _expected(refs, c):
    """arena i's expected streams: those of the synchronous run with j = c[i]"""
    js = sorted(refs)
    exp = []
    for k, x in enumerate(refs[js[0]]):
        if x is None:
            exp.append(None)
            continue
        e = x.clone()
        for j in js:
            m = c == j
            e[:, m] = refs[j][k][:, m]
        exp.append(e)
    return exp


def _assert_same(got, exp, names, what):
    bad = []
    for name, x, y in zip(names, got, exp):
        if x is None:
            continue
        a, b = torch.nan_to_num(x.double(), nan=-7.0), torch.nan_to_num(y.double(), nan=-7.0)
        diff = (a != b).reshape(a.shape[0], a.shape[1], -1).any(-1)  # [completed step, arena]
        if bool(diff.any()):
            arenas = torch.nonzero(diff.any(0)).flatten().tolist()
            bad.append(f"{name}: arenas {arenas} differ from the synchronous run (first at completed step "
                       f"{int(torch.nonzero(diff.any(1)).flatten()[0])})")
    assert not bad, f"{what}: " + "; ".join(bad)


def _setter_case(preset, budget, setter, extras, extra_names, episodes=False, **kw):
    """the budgeted run applies `setter` between call EVENT_CALL and the next, while arenas are parked; refused, it retries after
    set_step_budget(0) and one call.  Compares every arena's streams with the synchronous runs; returns the refusal message or None."""
    from roborugby_amd import _lib
    st = {}

    def hook(env, ctx):
        if ctx.call == EVENT_CALL:
            st["parked"] = int(ctx.parked.sum())
            st["c"] = ctx.cursor.clone()
            try:
                setter(env)
                st["refused"] = None
            except _lib.RRError as e:
                st["refused"] = str(e)
        elif st.get("refused") and ctx.call == EVENT_CALL + 2:   # the streams went on unchanged for two calls
            env.set_step_budget(0)                               # the parked arenas finish their step in the next call
        elif st.get("refused") and ctx.call == EVENT_CALL + 3:
            assert not bool(ctx.parked.any())
            st["c"] = ctx.cursor.clone()
            setter(env)                                          # nothing is parked: the change goes through
            env.set_step_budget(budget)

    env = _make(preset, budget, episodes, **kw)
    table = _table(env)
    got, calls, nr = streams(env, table, STEPS, True, MAX_CALLS, hook=hook, extras=extras)
    env.close()
    assert st["parked"] > 0, "no arena was parked at the change: the case is not exercised"
    c = st["c"]
    refs = {}
    for j in sorted(set(c.tolist())):
        def ref_hook(env, ctx, j=j):
            if ctx.call == j:
                setter(env)
        ref = _make(preset, 0, episodes, **kw)
        refs[j], _, _ = streams(ref, table, STEPS, False, STEPS, hook=ref_hook, extras=extras)
        ref.close()
    _assert_same(got, _expected(refs, c), NAMES + extra_names, f"{preset} budget {budget}")
    print(f"[{preset} budget {budget}] {st['parked']} arenas parked at the change, {'refused' if st['refused'] else 'applied'}; "
          f"{calls} calls, {nr} NOT_READY rows, synchronous runs for c in {sorted(refs)}")
    return got, st["refused"]


@pytest.mark.parametrize("episodes", [False, True], ids=["no_time_limit", "episodes"])
@pytest.mark.parametrize("change", ["default->stack", "custom->custom", "custom->default"])
@pytest.mark.parametrize("budget", [1, 30_000])
@pytest.mark.parametrize("preset", ["T", "G"])
def test_a_reward_program_switched_while_parked(preset, budget, change, episodes):
    """(a) rr_set_reward_program while arenas are parked: rewards and episode returns.  From the default program (no step-begin
    copies were kept) the switch is refused (f); between custom programs, and back to the default, the parked arenas' step-begin
    copies are there and the new program scores the step they complete."""
    before, after = {"default->stack": (None, STACK), "custom->custom": (STACK, OTHER), "custom->default": (STACK, None)}[change]
    from roborugby_amd.env import SIMPLE_DUEL3_REWARDS
    kw = {} if before is None else {"rewards": before}
    got, refused = _setter_case(preset, budget, _set_program(after or SIMPLE_DUEL3_REWARDS), (_returns,), ("returns",), episodes, **kw)
    if before is None:
        assert refused is not None and "parked" in refused, refused
    else:
        assert refused is None
    assert float(got[1].abs().sum()) > 0.0
    if episodes:  # finished episodes inside the window: their returns were compared (episode_stats' count is column 12 of _returns)
        assert float(got[6][-1, :, 12].min()) >= 1.0


@pytest.mark.parametrize("budget", [1, 30_000])
@pytest.mark.parametrize("preset", ["T", "G"])
def test_b_prior_step_tracking_switched_on_while_parked(preset, budget):
    """(b) rr_track_prior_step(1) on a default-program handle while arenas are parked: the observe_kind(4) rows of every completed
    step.  Nothing was kept at the parked arenas' step begin, so the call is refused (f) and goes through after the parks drain."""
    got, refused = _setter_case(preset, budget, _track_prior, (_prior_coords, _returns), ("observe_kind(4)", "returns"))
    assert refused is not None and "parked" in refused, refused
    assert not bool(torch.isnan(got[6][-1]).all(1).any())  # tracking was on for the last completed step of every arena


@pytest.mark.parametrize("budget", [1, 30_000])
def test_c_goal_scoring_switched_on_while_parked(budget):
    """(c) rr_set_goal_scoring(1) on G while arenas are parked: the goal frame of a parked arena comes with the call that completes
    its step, so the switch is synchronous-equivalent; goal_scores() after every completed step."""
    _, refused = _setter_case("G", budget, _goal_scoring, (lambda env: env.goal_scores(), _returns), ("goal_scores", "returns"))
    assert refused is None


@pytest.mark.parametrize("randomize", [True, False], ids=["rr_reset", "rr_reset_to_poses"])
@pytest.mark.parametrize("budget", [1, 30_000])
@pytest.mark.parametrize("preset", ["T", "G"])
def test_d_masked_reset_while_parked(preset, budget, randomize):
    """(d) env.reset(mask) in budgeted mode, the mask holding parked and ready arenas and leaving parked arenas out: reset rows equal
    the synchronous masked reset's (same Philox key), returned rows outside the mask are each arena's previous observation, a parked
    arena inside the mask loses its step in progress, and the NOT_READY rows of the calls that follow (step() without `out`) hold
    the previous observation of both teams."""
    st = {}

    def hook(env, ctx):
        if "mask" in st or ctx.call < 1:
            return
        p = ctx.parked
        if int(p.sum()) < 2 or not bool((~p).any()):
            return  # wait for a call after which some arenas are parked and some are not
        rank_p, rank_r = torch.cumsum(p.long(), 0) - 1, torch.cumsum((~p).long(), 0) - 1
        mask = (p & (rank_p % 2 == 0)) | (~p & (rank_r % 2 == 0))  # half of the parked arenas, half of the ready ones
        st.update(mask=mask, c=ctx.cursor.clone(), parked=p.clone(), prev=ctx.out[0].clone())
        st["ret"] = env.reset(mask, bln_randomize_pos=randomize).clone()
        ctx.out[0][mask] = st["ret"][mask]
        if ctx.out[3] is not None:
            ctx.out[3][mask] = env.get_game_state(-1)[mask]
        ctx.parked = p & ~mask

    env = _make(preset, budget)
    table = _table(env)
    got, calls, nr = streams(env, table, STEPS, True, MAX_CALLS, hook=hook, extras=(_returns,), default_outputs=True)
    env.close()
    assert "mask" in st, "no call left parked and ready arenas side by side"
    mask, c, p = st["mask"], st["c"], st["parked"]
    assert bool((mask & p).any()) and bool((mask & ~p).any()) and bool((~mask & p).any())
    out_rows = ~mask
    assert torch.equal(st["ret"][out_rows], st["prev"][out_rows]), \
        f"reset(mask) rows outside the mask are not the previous observation: arenas {torch.nonzero((st['ret'] != st['prev']).any(1) & out_rows).flatten().tolist()}"
    refs, ref_ret = {}, {}
    for j in sorted(set(c.tolist())):
        def ref_hook(env, ctx, j=j):
            if ctx.call == j:
                ref_ret[j] = env.reset(mask, bln_randomize_pos=randomize).clone()
                ctx.out[0][mask] = ref_ret[j][mask]
                if ctx.out[3] is not None:
                    ctx.out[3][mask] = env.get_game_state(-1)[mask]
        ref = _make(preset, 0)
        refs[j], _, _ = streams(ref, table, STEPS, False, STEPS, hook=ref_hook, extras=(_returns,))
        ref.close()
    for j in ref_ret:
        m = mask & (c == j)
        assert torch.equal(st["ret"][m], ref_ret[j][m]), f"reset rows differ from the synchronous masked reset (c = {j})"
    _assert_same(got, _expected(refs, c), NAMES + ("returns",), f"{preset} budget {budget}")
    print(f"[{preset} budget {budget} randomize={randomize}] reset {int(mask.sum())} arenas ({int((mask & p).sum())} parked), "
          f"{int((~mask & p).sum())} parked outside the mask; {calls} calls, {nr} NOT_READY rows")


@pytest.mark.parametrize("preset", ["T", "G"])
def test_e_step_budget_changed_while_parked(preset):
    """(e) set_step_budget(1 -> 30,000 -> 1) while arenas are parked: no change for the synchronous stream, and through step()'s
    own persistent outputs every NOT_READY row keeps the previous observation of both teams."""
    parked = []

    def hook(env, ctx):
        if ctx.call in (2, 4):
            parked.append(int(ctx.parked.sum()))
            env.set_step_budget(30_000 if ctx.call == 2 else 1)

    env = _make(preset, 1)
    table = _table(env)
    got, calls, nr = streams(env, table, STEPS, True, MAX_CALLS, hook=hook, extras=(_returns,), default_outputs=True)
    env.close()
    assert parked[0] > 0 and len(parked) == 2, parked
    ref = _make(preset, 0)
    want, _, _ = streams(ref, table, STEPS, False, STEPS, extras=(_returns,))
    ref.close()
    _assert_same(got, want, NAMES + ("returns",), preset)
    print(f"[{preset}] parked at the two switches: {parked}; {calls} calls, {nr} NOT_READY rows")
