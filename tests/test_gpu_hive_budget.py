"""The hive under the budgeted step on the MI355X: rr_hive_observe_held / rr_hive_commit / rr_hive_transition_held through the C-ABI,
players.Hive's held pipeline, dqn.train_hive / play_hive with a budget.

Promise: with the call order of include/roborugby_amd.h and the same assign / obs / accepted buffers in every call, each arena's stream of
(assign, obs, accepted, reward, next_obs, terminal, valid), as a function of the answers it ACCEPTED, is the synchronous mode's bit for
bit -- whatever the budget, down to 1 clock.  tests/test_hive_held_emulated.py is the CPU twin of the three kernels' write sets."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

import hive_budget_driver as hb  # noqa: E402
from hive_budget_driver import NOT_READY  # noqa: E402


def _env(preset, n, **kw):
    import roborugby_amd as rr
    kw.setdefault("time_limit", True)
    kw.setdefault("auto_reset", True)
    return rr.BatchedRoboRugbyEnv(n, preset=preset, **kw)


def _stuck_env(budget):
    d = np.load(os.path.join(HERE, "data", "stuck_chase_G.npz"))
    env = _env("G", len(d["step"]), seed=3, step_budget_clocks=budget)
    env.set_state(d["robots"], d["robots_i"], d["balls"], d["step"])
    env.track_prior_step()  # (after set_state: the copies start from the fixture's poses)
    return env, d


@pytest.mark.parametrize("kind,mask,budgets", [(0, 15, (0, 1, 50_000)), (1, 3, (0, 1))])
def test_budgeted_hive_transitions_equal_the_synchronous_ones_on_stuck_chase_arenas(kind, mask, budgets):
    steps = 8
    ref = None
    for budget in budgets:
        env, d = _stuck_env(budget)
        n, nr = env.num_envs, env.preset.nr
        g = torch.Generator(device="cuda").manual_seed(5)
        table = torch.randint(0, 16, (steps, n, nr), generator=g, device="cuda", dtype=torch.int32)  # >= 8: chase on the hive's own view
        keep = torch.rand(steps, n, generator=g, device="cuda") < 0.7                                  # mostly the fixture's action
        table = torch.where(keep.unsqueeze(-1), torch.as_tensor(d["actions"], device="cuda").to(torch.int32).expand(steps, n, nr), table)
        got, calls, nrdy = hb.streams(env, table, steps, mask, kind, budget > 0, 2000)
        env.close()
        members = [r for r in range(nr) if (mask >> r) & 1]
        share = float(got["valid"][:, :, members].float().mean())
        print(f"[kind {kind} mask {mask}] budget {budget}: {calls} calls for {steps} steps of {n} stuck arenas, {nrdy} NOT_READY rows, "
              f"valid share of the hive's rows {share:.3f}")
        if ref is None:
            ref = got
            assert calls == steps and nrdy == 0
            assert bool(got["valid"][0][:, members].all())       # every hive robot has a ball at the first step
            assert share >= 0.5                                   # (against a vacuous comparison)
            assert not bool(got["valid"][:, :, [r for r in range(nr) if r not in members]].any())
        else:
            assert hb.equal(got, ref) == [], (kind, mask, budget)
            if budget == 1:
                assert nrdy > n  # these arenas are the stuck ones: with a 1-clock budget they park over and over


def test_held_rows_keep_what_the_buffers_hold_and_a_reset_arena_is_observed_afresh():
    env, d = _stuck_env(1)
    n = env.num_envs
    thrust = torch.ones(n, 8, device="cuda")
    _, _, _, info = env.step_thrust(thrust)
    parked = (info.status & NOT_READY) != 0
    assert int(parked.sum()) >= 8, "the 1-clock budget parked (almost) nobody: nothing to hold"
    # a reset clears the parked mark in the record: the status still says NOT_READY, the arena is observed afresh
    again = torch.zeros(n, dtype=torch.bool, device="cuda")
    again[torch.nonzero(parked).view(-1)[::4]] = True
    env.reset(again)
    for kind, mask in ((0, 15), (1, 5)):
        assign = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
        obs = torch.full((n, 4, 11), float("nan"), device="cuda")
        held = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        env.hive_observe(mask, hb.NAMES[kind], out=(assign, obs, held), held=True)
        h = held.bool()
        assert torch.equal(h, parked & ~again) and bool(h.any()) and bool((~h).any())
        assert bool((assign[h] == -7).all()) and bool(torch.isnan(obs[h]).all())
        want_a, want_o = env.hive_observe(mask, hb.NAMES[kind])
        assert torch.equal(assign[~h], want_a[~h]) and torch.equal(obs[~h], want_o[~h])
        assert bool((want_a[~h] >= 0).any())
    env.close()


@pytest.mark.parametrize("preset,mask", [("G", 15), ("G", 6), ("T", 1)])
def test_without_a_budget_the_held_entries_are_the_plain_ones(preset, mask):
    n = 257  # (the last block is ragged)
    env = _env(preset, n, seed=4)
    nr = env.preset.nr
    env.track_prior_step()
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(n + mask)
    for s in range(3):
        pre = {(kind, f64): env.hive_observe(mask, hb.NAMES[kind], f64=f64) for kind in (0, 1) for f64 in (False, True)}
        for (kind, f64), (want_a, want_o) in pre.items():
            a, o, held = env.hive_observe(mask, hb.NAMES[kind], f64=f64, held=True)
            assert not bool(held.any()) and torch.equal(a, want_a) and torch.equal(o, want_o), (s, kind, f64)
        _, _, done, info = env.step_thrust(torch.rand(n, 2 * nr, generator=g, device="cuda") * 2 - 1)
        for (kind, f64), (assign, _) in pre.items():
            want = env.hive_transition(assign, info.status, done, mask, hb.NAMES[kind], f64=f64)
            got = env.hive_transition_held(assign, info.status, done, mask, hb.NAMES[kind], f64=f64)
            assert all(torch.equal(x, y) for x, y in zip(got, want)), (s, kind, f64)
            assert bool(want[3].any())
        # an arena whose status says it did not step: the early return writes hive_transition's rows
        status = info.status.clone()
        status[::3] |= NOT_READY
        status[1::7] |= 1024
        assign = pre[(0, False)][0]
        want = env.hive_transition(assign, status, done, mask)
        outs = (torch.full((n, nr, 11), 7.0, device="cuda"), torch.full((n, nr), 7.0, device="cuda"),
                torch.full((n, nr), 7, dtype=torch.uint8, device="cuda"), torch.full((n, nr), 7, dtype=torch.uint8, device="cuda"))
        got = env.hive_transition_held(assign, status, done, mask, out=outs)
        assert all(torch.equal(x, y) for x, y in zip(got, want)) and not bool(got[3][::3].any())
    env.close()


def test_commit_on_the_device_equals_the_table_lookup_and_leaves_held_cells_alone():
    from roborugby_amd.players import _THRUST_FROM_DIRECTION
    n = 257
    env = _env("G", n, seed=2)
    g = torch.Generator(device="cuda").manual_seed(7)
    table = torch.tensor(_THRUST_FROM_DIRECTION, device="cuda")
    for mask in (3, 15, 4):
        fresh = torch.randint(-2, 10, (n, 4), generator=g, device="cuda", dtype=torch.int32)
        assign = torch.where(torch.rand(n, 4, generator=g, device="cuda") < .4, -1,
                             torch.randint(0, 8, (n, 4), generator=g, device="cuda")).to(torch.int32)
        held = (torch.arange(n, device="cuda") % 4 == 0).to(torch.uint8)
        accepted = torch.full((n, 4), -99, dtype=torch.int32, device="cuda")
        thrust = torch.full((n, 8), 7.5, device="cuda")
        env.hive_commit(fresh, assign, held, accepted, thrust, mask)
        may = (held == 0).view(n, 1) & (((mask >> torch.arange(4, device="cuda")) & 1) == 1).view(1, 4)
        moves = (assign >= 0) & (fresh >= 0) & (fresh < 8)
        want_t = torch.where(moves.unsqueeze(-1), table[fresh.clamp(0, 7).long()], torch.zeros(n, 4, 2, device="cuda"))
        assert torch.equal(accepted, torch.where(may, fresh, torch.full_like(fresh, -99)))
        assert torch.equal(thrust.view(n, 4, 2), torch.where(may.unsqueeze(-1), want_t, torch.full((n, 4, 2), 7.5, device="cuda")))
    env.close()


def test_refusals_return_minus_one_with_a_message_and_touch_nothing():
    n = 64
    env = _env("G", n)
    env.track_prior_step()
    env.reset()
    L = env._lib
    assign, _ = env.hive_observe(15)
    _, _, done, info = env.step(torch.zeros(n, 4, dtype=torch.int32, device="cuda"))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def refused(fn, args, ts, word, name):
        assert fn(*args, None) == -1, (name, word)
        msg = L.rr_last_error()
        assert msg and word in msg and name in msg, (name, word, msg)  # (name: the entry's, without _f64 -- the impl's messages share it)
        torch.cuda.synchronize()
        assert all(bool((t == 7).all()) for t in ts), (name, word)

    def variants(h, head, ptrs, kinded):
        """(args, word) of every malformed call: head = (mask, kind) or (mask,)"""
        yield [None, *head, *ptrs], b"null"
        for k in range(len(ptrs)):
            yield [h, *head, *ptrs[:k], None, *ptrs[k + 1:]], b"null"
        yield [h, 0, *head[1:], *ptrs], b"empty"
        yield [h, 16, *head[1:], *ptrs], b"mask"
        yield [h, 0x80000001, *head[1:], *ptrs], b"mask"
        if kinded:
            yield [h, head[0], 2, *ptrs], b"kind"
            yield [h, head[0], -1, *ptrs], b"kind"

    f32 = _env("G", n, dtype="f32")
    f32.track_prior_step()
    for sfx, dt in (("", torch.float32), ("_f64", torch.float64)):
        # rr_hive_observe_held
        name, base = "rr_hive_observe_held" + sfx, b"rr_hive_observe_held"
        fn = getattr(L, name)
        ts = [torch.full((n, 4), 7, dtype=torch.int32, device="cuda"), torch.full((n, 4, 11), 7.0, dtype=dt, device="cuda"),
              torch.full((n,), 7, dtype=torch.uint8, device="cuda")]
        for args, word in variants(env._h, (15, 0), [p(t) for t in ts], True):
            refused(fn, args, ts, word, base)
        if sfx:
            refused(getattr(f32._lib, name), [f32._h, 15, 0, *[p(t) for t in ts]], ts, b"RR_DTYPE_F32", name.encode())
        assert fn(env._h, 15, 0, *[p(t) for t in ts], None) == 0  # ... and the well-formed call goes through
        torch.cuda.synchronize()
        assert not any(bool((t == 7).all()) for t in ts)
        # rr_hive_transition_held
        name, base = "rr_hive_transition_held" + sfx, b"rr_hive_transition_held"
        fn = getattr(L, name)
        ins = [p(assign), p(info.status), p(done.view(torch.uint8))]
        ts = [torch.full((n, 4, 11), 7.0, dtype=dt, device="cuda"), torch.full((n, 4), 7.0, dtype=dt, device="cuda"),
              torch.full((n, 4), 7, dtype=torch.uint8, device="cuda"), torch.full((n, 4), 7, dtype=torch.uint8, device="cuda")]
        for args, word in variants(env._h, (15, 0), ins + [p(t) for t in ts], True):
            refused(fn, args, ts, word, base)
        untracked = _env("G", n)
        refused(fn, [untracked._h, 15, 0, *ins, *[p(t) for t in ts]], ts, b"rr_track_prior_step", base)
        untracked.close()
        if sfx:
            refused(getattr(f32._lib, name), [f32._h, 15, 0, *ins, *[p(t) for t in ts]], ts, b"RR_DTYPE_F32", name.encode())
        budgeted = _env("G", n, step_budget_clocks=20000)
        budgeted.track_prior_step()
        refused(getattr(L, "rr_hive_transition" + sfx), [budgeted._h, 15, 0, *ins, *[p(t) for t in ts]], ts, b"budget", b"rr_hive_transition")
        assert fn(budgeted._h, 15, 0, *ins, *[p(t) for t in ts], None) == 0  # the held entry is accepted on a budgeted handle
        torch.cuda.synchronize()
        assert not any(bool((t == 7).all()) for t in ts)
        budgeted.close()
    # rr_hive_commit
    fresh = torch.zeros(n, 4, dtype=torch.int32, device="cuda")
    held = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ts = [torch.full((n, 4), 7, dtype=torch.int32, device="cuda"), torch.full((n, 8), 7.0, device="cuda")]
    for args, word in variants(env._h, (15,), [p(fresh), p(assign), p(held)] + [p(t) for t in ts], False):
        refused(L.rr_hive_commit, args, ts, word, b"rr_hive_commit")
    assert L.rr_hive_commit(env._h, 15, p(fresh), p(assign), p(held), *[p(t) for t in ts], None) == 0
    torch.cuda.synchronize()
    assert not any(bool((t == 7).all()) for t in ts)
    f32.close()
    env.close()


def test_hive_end_to_end_under_a_budget(tmp_path):
    from roborugby_amd import dqn
    from roborugby_amd.players import Hive, og_twitchy
    n = 2048
    env = _env("G", n, seed=6, action_mode="thrust", step_budget_clocks=20000)
    env.track_prior_step()
    env.reset()
    assert env.has_had_budget
    agent = dqn.BatchedDQNAgent(device="cuda:0", seed=3, batch_size=64, max_mem_size=65536)
    hive = Hive(env, agent, epsilon=0.0, seed=2)
    gen = torch.Generator(device="cuda").manual_seed(6)
    thrust = torch.zeros(n, 8, device="cuda")
    prev, ever_held, total, status = None, 0, 0, torch.zeros(n, dtype=torch.int32, device="cuda")
    for call in range(12):
        thrust[:, 4:] = og_twitchy(n, 2, generator=gen, device="cuda")
        before = thrust.clone()
        hive.act(out=thrust)
        h = hive.held
        assert torch.equal(h, (status & NOT_READY) != 0), call
        now = (hive.obs.clone(), hive.assign.clone(), hive.actions.clone())
        if prev is not None:
            assert all(torch.equal(x[h], y[h]) for x, y in zip(now, prev)), call  # held rows are the call before's
        assert torch.equal(thrust[h], before[h]) and torch.equal(thrust[:, 4:], before[:, 4:])
        ever_held += int(h.sum())
        prev = now
        _, _, done, info = env.step_thrust(thrust)
        status = info.status
        hive.store(agent, done, status)
        assert not bool(hive._valid.view(n, 4)[(status & NOT_READY) != 0].any())
        total += int(hive._valid.sum())
        assert agent.mem_cntr == total, (call, agent.mem_cntr, total)
    assert ever_held > 0 and total > 0
    print(f"Hive under a 20,000-clock budget: {ever_held} held arena-calls of {12 * n}, {total} transitions stored")
    hive.close()
    env.close()
    ck = str(tmp_path / "hive_budget.pt")
    res = dqn.train_hive(num_envs=2048, steps=6, step_budget_clocks=20000, learn=True, log_every=0, checkpoint=ck)
    assert res["step_budget_clocks"] == 20000 and res["transitions"] == res["valid_rows"] > 0
    assert res["loss"] is not None and np.isfinite(res["loss"])
    assert 0 <= res["not_ready_share"] < 1 and 0 < res["stepped_rows"] <= 6 * 2048
    played = dqn.play_hive(ck, num_envs=2048, steps=6, seed=2, step_budget_clocks=20000)
    assert played["step_budget_clocks"] == 20000 and np.isfinite(played["return_happy"]) and np.isfinite(played["return_grumpy"])
    assert 0 < played["stepped_rows"] <= 6 * 2048
    with pytest.raises(ValueError, match="f32_state"):
        dqn.train_hive(num_envs=64, steps=1, dtype="f32_state", step_budget_clocks=20000, log_every=0)
