"""Chase-policy driver of the budgeted-step GPU tests (tests/test_gpu_budget.py, tests/test_gpu_budget_setters.py).

It steps an env until every arena has accepted a given number of steps and records, per arena, the stream of what each of its
completed steps returned -- so a budgeted run (arenas park, calls and steps no longer line up) and a synchronous run compare row
for row."""
import types

import torch

NOT_READY = 16384


def chase(obs, cursor, table):
    """turn toward the ball, else forward; the noise of an arena's k-th accepted step comes from table[k, arena]: the action is a
    function of the arena's own observation and of how many steps it has accepted -- the same in both modes."""
    n = obs.shape[0]
    d = (obs[:, 1] - obs[:, 0] + 540.0) % 360.0 - 180.0
    a = torch.where(d.abs() < 8, 0, torch.where(d > 0, 2, 3)).to(torch.int32)
    row = table[cursor.clamp(max=table.shape[0] - 1), torch.arange(n, device=obs.device)]  # [n, na]: >= 8 keeps the chase action
    a1 = torch.where(row[:, 0] < 8, row[:, 0], a)
    return torch.cat([a1.view(n, 1), row[:, 1:] % 8], 1).contiguous()


def streams(env, table, steps, budget_mode, max_calls, hook=None, extras=(), default_outputs=False):
    """runs until every arena has accepted `steps` steps; returns per-arena streams [steps, n, ...] of obs / reward / done / status /
    obs_g / reward_g, then one per callable of `extras` (env -> tensor [n, ...], read after every call: the rows of the arenas
    whose step completed in it are kept), with the number of calls and of NOT_READY rows.

    hook(env, ctx) runs before every call: ctx.call = calls made so far, ctx.cursor = steps each arena has completed, ctx.parked =
    arenas whose step is in progress, ctx.out = the output buffers, whose rows 0 / 3 are the observations the policy reads next
    (a hook that rewrites arenas updates those rows and ctx.parked).  default_outputs=True steps through env.step(actions) without
    `out` -- the persistent buffers of the budgeted mode -- and checks that every NOT_READY row of both teams holds the arena's
    previous observation."""
    n, dev = env.num_envs, env.device
    na = table.shape[2]
    rec_o = torch.zeros(steps, n, 11, device=dev); rec_r = torch.zeros(steps, n, device=dev)
    rec_d = torch.zeros(steps, n, dtype=torch.uint8, device=dev); rec_s = torch.zeros(steps, n, dtype=torch.int32, device=dev)
    rec_og = torch.zeros(steps, n, 11, device=dev) if env.has_grumpy else None
    rec_rg = torch.zeros(steps, n, device=dev)
    rec_x = [None] * len(extras)
    out = (torch.zeros(n, 11, device=dev), torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev),
           torch.zeros(n, 11, device=dev) if env.has_grumpy else None, torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
    out[0].copy_(env.get_game_state(1))
    if out[3] is not None:
        out[3].copy_(env.get_game_state(-1))
    cursor = torch.zeros(n, dtype=torch.long, device=dev)   # steps accepted AND completed
    parked = torch.zeros(n, dtype=torch.bool, device=dev)
    ar = torch.arange(n, device=dev)
    calls = not_ready_rows = 0
    ctx = types.SimpleNamespace(call=0, cursor=cursor, parked=parked, out=out)
    while int(cursor.min()) < steps:
        if hook is not None:
            ctx.call, ctx.parked = calls, parked
            hook(env, ctx)
            parked = ctx.parked
        a = chase(out[0], cursor, table)
        if budget_mode:  # a parked arena must ignore what it is given: hand it something else
            a = torch.where(parked.view(n, 1), (a + 3) % 8, a)
        if default_outputs:
            o, r, d, info = env.step(a[:, :na])
            nr = (info.status & NOT_READY) != 0
            assert torch.equal(o[nr], out[0][nr]), f"call {calls + 1}: a NOT_READY row does not hold the previous observation"
            if out[3] is not None:
                assert torch.equal(info.adblGrumpyState[nr], out[3][nr]), f"call {calls + 1}: a NOT_READY grumpy row is not the previous one"
            for dst, src in zip(out, (o, r, d.to(torch.uint8), info.adblGrumpyState, info.dblGrumpyScore, info.status)):
                if dst is not None:
                    dst.copy_(src)
        else:
            env.step(a[:, :na], out=out)
        calls += 1
        assert calls <= max_calls, "arenas do not make progress"
        ready = (out[5] & NOT_READY) == 0
        assert budget_mode or bool(ready.all())
        not_ready_rows += int((~ready).sum())
        idx = ar[ready & (cursor < steps)]
        c = cursor[idx]
        rec_o[c, idx] = out[0][idx]; rec_r[c, idx] = out[1][idx]; rec_d[c, idx] = out[2][idx]; rec_s[c, idx] = out[5][idx]
        rec_rg[c, idx] = out[4][idx]
        if rec_og is not None:
            rec_og[c, idx] = out[3][idx]
        for k, f in enumerate(extras):
            x = f(env)
            if rec_x[k] is None:
                rec_x[k] = torch.zeros((steps,) + tuple(x.shape), dtype=x.dtype, device=dev)
            rec_x[k][c, idx] = x[idx]
        cursor += ready.long()
        parked = ~ready
    return (rec_o, rec_r, rec_d, rec_s, rec_og, rec_rg, *rec_x), calls, not_ready_rows


def equal(a, b):
    return all(x is None or torch.equal(torch.nan_to_num(x.double(), nan=-7.0), torch.nan_to_num(y.double(), nan=-7.0)) for x, y in zip(a, b))
