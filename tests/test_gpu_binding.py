"""What the Python binding promises around the launches and no other test pins: `out=` tensors are written and handed back themselves,
the fp64 variants return float64 and report their own symbol, the tensor contracts refuse before any launch, and the setters' tails.
(render_batch / render_ego: `out=` identity and the refused `out` are pinned in test_gpu_render.py / test_gpu_render_ego.py.)"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N = 8
PRESETS = ["T", "G"]


def _env(preset, **kw):
    import roborugby_amd as rr
    env = rr.BatchedRoboRugbyEnv(N, preset=preset, seed=5, **kw)
    env.reset()
    return env


def _actions(env, lead=(), seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 8, lead + (N, env.preset.nr), generator=g, device="cuda", dtype=torch.int32)


def _step_out(env, lead=()):
    """the six step outputs, filled with values no step writes"""
    f = lambda *tail: torch.full(lead + (N,) + tail, -7.5, device="cuda")  # noqa: E731
    return (f(11), f(), torch.full(lead + (N,), 9, dtype=torch.uint8, device="cuda"), f(11) if env.has_grumpy else None, f(),
            torch.full(lead + (N,), -1, dtype=torch.int32, device="cuda"))


def _same_step(got, out, want):
    obs, rew, done, info = got
    assert obs is out[0] and rew is out[1] and done.data_ptr() == out[2].data_ptr() and done.dtype == torch.bool
    assert info.adblGrumpyState is out[3] and info.dblGrumpyScore is out[4] and info.status is out[5]
    w_obs, w_rew, w_done, w_info = want
    assert torch.equal(obs, w_obs) and torch.equal(rew, w_rew) and torch.equal(done, w_done)
    assert torch.equal(info.dblGrumpyScore, w_info.dblGrumpyScore) and torch.equal(info.status, w_info.status)
    assert (out[3] is None) == (w_info.adblGrumpyState is None) and (out[3] is None or torch.equal(out[3], w_info.adblGrumpyState))


@pytest.mark.parametrize("preset", PRESETS)
def test_step_and_rollout_write_into_out_and_return_those_tensors(preset):
    a, b = _env(preset), _env(preset)  # the same seed: the same arenas
    acts = _actions(a)
    out = _step_out(a)
    _same_step(a.step(acts, out=out), out, b.step(acts))
    table = _actions(a, (3,), seed=2)
    out = _step_out(a, (3,))
    _same_step(a.rollout(table, out=out), out, b.rollout(table))
    a.close(), b.close()


@pytest.mark.parametrize("preset", PRESETS)
def test_the_hive_entries_write_into_out_and_return_those_tensors(preset):
    env = _env(preset)
    nr = env.preset.nr
    env.track_prior_step()
    for held in (False, True):
        out = (torch.full((N, nr), -7, dtype=torch.int32, device="cuda"), torch.full((N, nr, 11), float("nan"), device="cuda"),
               torch.full((N,), 9, dtype=torch.uint8, device="cuda"))[:3 if held else 2]
        got = env.hive_observe(out=out, held=held)
        want = env.hive_observe(held=held)
        assert len(got) == len(out) == len(want) and all(x is y for x, y in zip(got, out))
        assert all(torch.equal(x, y) for x, y in zip(got, want))
    assign = got[0]
    assert bool((assign >= 0).any())
    _, _, done, info = env.step_thrust(torch.ones(N, 2 * nr, device="cuda"))
    out = (torch.full((N, nr, 11), 7.0, device="cuda"), torch.full((N, nr), 7.0, device="cuda"),
           torch.full((N, nr), 7, dtype=torch.uint8, device="cuda"), torch.full((N, nr), 7, dtype=torch.uint8, device="cuda"))
    got = env.hive_transition(assign, info.status, done, out=out)
    want = env.hive_transition(assign, info.status, done)
    assert all(x is y for x, y in zip(got, out)) and all(torch.equal(x, y) for x, y in zip(got, want))
    assert bool(got[3].any())
    env.close()


@pytest.mark.parametrize("preset", PRESETS)
def test_the_fp64_variants_return_float64_and_report_their_own_symbol(preset):
    from roborugby_amd._lib import RRError
    env = _env(preset)
    nr = env.preset.nr
    obs, rew, done, info = env.step_thrust(torch.ones(N, 2 * nr, device="cuda"), f64=True)
    assert obs.dtype == rew.dtype == info.dblGrumpyScore.dtype == torch.float64 and done.dtype == torch.bool
    assert info.adblGrumpyState is None or info.adblGrumpyState.dtype == torch.float64
    assert env.get_game_state(1, f64=True).dtype == torch.float64
    with pytest.raises(RRError, match="rr_observe_kind_f64 failed"):
        env.get_game_state(1, robot_idx=nr, f64=True)  # a robot the arena does not have
    with pytest.raises(RRError, match="rr_observe_kind failed"):
        env.get_game_state(1, robot_idx=nr)
    env.close()
    f32 = _env(preset, dtype="f32")  # no fp64 outputs from a handle that computes in fp32: refused before any launch
    with pytest.raises(RRError, match="rr_step_thrust_f64 failed"):
        f32.step_thrust(torch.ones(N, 2 * nr, device="cuda"), f64=True)
    assert f32.step_thrust(torch.ones(N, 2 * nr, device="cuda"))[0].dtype == torch.float32
    f32.close()


def test_hive_commit_refuses_tensors_that_break_its_contract():
    env = _env("G")
    nr = env.preset.nr
    i32 = lambda: torch.zeros(N, nr, dtype=torch.int32, device="cuda")  # noqa: E731
    held, thrust = torch.zeros(N, dtype=torch.uint8, device="cuda"), torch.full((N, 2 * nr), 5.0, device="cuda")
    with pytest.raises(AssertionError):
        env.hive_commit(i32().float(), i32(), held, i32(), thrust)  # a wrong dtype
    with pytest.raises(AssertionError):
        env.hive_commit(i32(), i32(), held.cpu(), i32(), thrust)  # a tensor that is not on the device
    assert bool((thrust == 5.0).all())  # nothing was launched
    env.hive_commit(i32(), i32(), held, i32(), thrust, robot_mask=(1 << nr) - 1)  # ... and the well-formed call goes through
    assert bool((thrust != 5.0).all())
    env.close()


@pytest.mark.parametrize("preset", PRESETS)
def test_set_state_on_a_handle_that_has_had_a_budget_and_set_episode_state(preset):
    """set_state seeds the persistent step outputs again: after it a row of step() whose arena is parked reads as the observation of the
    state that was set, and the row of the call that completes an arena's step is a fresh env's.  The state: the first arenas of the
    stuck chase fixture, which park at this budget."""
    from roborugby_amd.env import STATUS_NOT_READY
    d = np.load(os.path.join(HERE, "data", f"stuck_chase_{preset}.npz"))
    state = [d[k][:N] for k in ("robots", "robots_i", "balls", "step")]
    acts = torch.as_tensor(d["actions"][:N], device="cuda").to(torch.int32)
    kw = dict(time_limit=False, auto_reset=False)
    env, fresh = _env(preset, step_budget_clocks=30_000, **kw), _env(preset, **kw)
    env.step(_actions(env))  # the persistent outputs now hold another state's rows
    env.set_state(*state)
    fresh.set_state(*state)
    before = fresh.get_game_state(1), (fresh.get_game_state(-1) if fresh.has_grumpy else None)
    w_obs, w_rew, w_done, w_info = fresh.step(acts)
    want = (w_obs, w_rew, w_done, w_info.status, w_info.dblGrumpyScore, w_info.adblGrumpyState)
    rows = [None if x is None else torch.zeros_like(x) for x in want]  # every arena's row of the call that completed its step
    pending = torch.ones(N, dtype=torch.bool, device="cuda")
    for call in range(400):
        obs, rew, done, info = env.step(acts)  # (a parked arena goes on with its step, whatever the action)
        parked = (info.status & STATUS_NOT_READY) != 0
        if call == 0:
            print(f"[{preset}] {int(parked.sum())} of {N} arenas parked in the call after set_state")
            assert torch.equal(obs[parked], before[0][parked])
            assert before[1] is None or torch.equal(info.adblGrumpyState[parked], before[1][parked])
        take = pending & ~parked
        for r, x in zip(rows, (obs, rew, done, info.status, info.dblGrumpyScore, info.adblGrumpyState)):
            if r is not None:
                r[take] = x[take]
        pending &= parked
        if not bool(pending.any()):
            break
    assert not bool(pending.any()), "arenas still parked after 400 calls"
    assert all(r is None and w is None or torch.equal(r, w) for r, w in zip(rows, want))
    g = torch.Generator().manual_seed(3)
    ints, acc = torch.randint(0, 50, (N, 5), generator=g, dtype=torch.int32), torch.rand(N, 4, generator=g, dtype=torch.float64)
    fresh.set_episode_state(ints, acc)
    got = fresh.get_episode_state()
    assert torch.equal(got["ints"].cpu(), ints) and torch.equal(got["acc"].cpu(), acc)
    env.close(), fresh.close()
