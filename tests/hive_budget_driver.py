"""Driver of the hive's budgeted-step GPU tests (tests/test_gpu_hive_budget.py), modelled on tests/budget_driver.py.

It steps an env through the held pipeline -- hive_observe(held=True) -> policy -> hive_commit -> step_thrust -> hive_transition_held,
the same assign / obs / accepted buffers in every call -- until every arena has accepted a given number of steps, and records, per
arena and at the arena's own cursor, what the call that COMPLETED each of its steps saw: so a budgeted run (arenas park, calls and steps
no longer line up) and a synchronous run compare row for row."""
import torch

NOT_READY = 16384
NAMES = {0: "SingleBall_6wayLidar_v2", 1: "SingleBall_6wayLidar"}


def policy(row, obs):
    """row [n, NR] int32: a value < 8 is the direction itself; >= 8 means "chase on the robot's own hive observation": turn toward
    obs[1] - obs[0], forward within 8 degrees (hive_commit makes a robot without a ball stand still).  -> fresh int32 [n, NR]"""
    d = (obs[:, :, 1] - obs[:, :, 0] + 540.0) % 360.0 - 180.0
    chase = torch.where(d.abs() < 8, 0, torch.where(d > 0, 2, 3)).to(torch.int32)
    return torch.where(row < 8, row, chase).contiguous()


def streams(env, table, steps, mask, kind, budget_mode, max_calls):
    """-> (dict of per-arena streams [steps, n, ...], calls, NOT_READY rows).  table [steps, n, NR] int32: the draw of an arena's k-th
    accepted step is table[k, arena] -- the thrust is a function of it and of the hive's obs / assign of that arena, the same in both
    modes.  In budget mode a parked arena is handed a different answer on purpose: hive_commit must not accept it."""
    n, dev, nr = env.num_envs, env.device, env.preset.nr
    assign = torch.full((n, nr), -7, dtype=torch.int32, device=dev)
    obs = torch.full((n, nr, 11), float("nan"), device=dev)
    held = torch.zeros(n, dtype=torch.uint8, device=dev)
    accepted = torch.full((n, nr), -7, dtype=torch.int32, device=dev)
    thrust = torch.zeros(n, 2 * nr, device=dev)
    rec = None
    cursor = torch.zeros(n, dtype=torch.long, device=dev)  # steps accepted AND completed
    parked = torch.zeros(n, dtype=torch.bool, device=dev)
    ar = torch.arange(n, device=dev)
    calls = not_ready_rows = 0
    while int(cursor.min()) < steps:
        env.hive_observe(mask, NAMES[kind], out=(assign, obs, held), held=True)
        assert torch.equal(held.bool(), parked), f"call {calls + 1}: held is not the previous call's NOT_READY"
        assert budget_mode or not bool(held.any())
        fresh = policy(table[cursor.clamp(max=steps - 1), ar], obs)
        if budget_mode:
            fresh = torch.where(parked.view(n, 1), (fresh + 3) % 8, fresh).contiguous()
        env.hive_commit(fresh, assign, held, accepted, thrust, mask)
        _, reward, done, info = env.step_thrust(thrust)
        next_obs, hreward, terminal, valid = env.hive_transition_held(assign, info.status, done, mask, NAMES[kind])
        calls += 1
        assert calls <= max_calls, "arenas do not make progress"
        ready = (info.status & NOT_READY) == 0
        assert budget_mode or bool(ready.all())
        assert not bool(valid[~ready].any())
        not_ready_rows += int((~ready).sum())
        now = dict(assign=assign, obs=obs, accepted=accepted, next_obs=next_obs, hive_reward=hreward, terminal=terminal, valid=valid,
                   reward=reward, done=done.to(torch.uint8), status=info.status)
        if rec is None:
            rec = {k: torch.zeros((steps,) + tuple(v.shape), dtype=v.dtype, device=dev) for k, v in now.items()}
        idx = ar[ready & (cursor < steps)]
        c = cursor[idx]
        for k, v in now.items():
            rec[k][c, idx] = v[idx]
        cursor += ready.long()
        parked = ~ready
    return rec, calls, not_ready_rows


def equal(a, b):
    """every recorded tensor torch.equal (NaN rows -- an unassigned robot's sentinel never survives a non-held observe -- compared as bits)"""
    return [k for k in a if not torch.equal(torch.nan_to_num(a[k].double(), nan=-7.0), torch.nan_to_num(b[k].double(), nan=-7.0))]
