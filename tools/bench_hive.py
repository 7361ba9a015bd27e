"""Times the hive-mind player's path (rr_hive_observe, players.Hive) on the MI355X -- profiles/hive/README.md holds the results.

    python tools/bench_hive.py [--num-envs 65536] [--reps 30] [--steps 200] [--out profiles/hive/bench_hive.json]

At 65,536 arenas of preset G, fp64, HIP events, median (and min / max) of `--reps` repetitions after warm-up; every repetition times
a block of launches long enough to be more than clock resolution (INNER launches between two events, time / INNER reported):
  (a) rr_hive_observe, 4-robot mask, both observer kinds;
  (b) what a caller has to write WITHOUT the entry: NR x NB rr_observe_kind launches + the distance sort and the greedy pass in
      torch + a gather -- carried here as plain Python on the public API of the parent commit (get_state, get_game_state);
  (c) four plain rr_observe launches with a fixed ball: less work than (a) (no assignment), a floor for its observation part;
  (d) a full step of the game: Hive.act + step_thrust, next to the scripted chase + step on the same batch (200 steps each after
      200 steps of warm-up: the contact mix has to settle, the step's cost depends on it).
States: 50 chase steps from reset, so that robots are near balls.  No GPU, no numbers: the script raises without a device."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

INNER = 10


def timed(fn, reps, inner=INNER, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(inner):
            fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) / inner)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), reps=reps, launches_per_rep=inner)


def in_goal(x, y, W, H):
    """goal triangles (legs of 240 at the corners (W, H) and (0, 0)) as the library's goal_contains evaluates them"""
    inf = torch.tensor(float("inf"), device=x.device, dtype=x.dtype)

    def slope(dy, dx):
        return torch.where(dx != 0, dy / torch.where(dx != 0, dx, torch.ones_like(dx)), torch.where(dy > 0, inf, torch.where(dy < 0, -inf, torch.zeros_like(dy))))
    happy = (W - 240 <= x) & (x <= W) & (H - 240 <= y) & (y <= H) & (slope(y - H, x - (W - 240)) >= -1)
    grumpy = (0 <= x) & (x <= 240) & (0 <= y) & (y <= 240) & (slope(y, x - 240) >= -1)
    return happy | grumpy


def composed_hive_observe(env, mask):
    """(b): the same (assign, obs) from the entries the library had before rr_hive_observe"""
    p, n = env.preset, env.num_envs
    st = env.get_state()
    rxy, bxy = st["robots"][:, :, :2], st["balls"][:, :, :2]
    cand = ~in_goal(bxy[:, :, 0], bxy[:, :, 1], p.arena_w, p.arena_h) & (bxy[:, :, 0] > -900)
    d = ((bxy[:, :, None, :] - rxy[:, None, :, :]) ** 2).sum(-1).sqrt()  # [n, NB, NR]
    hive = torch.tensor([(mask >> r) & 1 for r in range(p.nr)], device=env.device, dtype=torch.bool)
    d = torch.where(cand[:, :, None] & hive[None, None, :], d, torch.full_like(d, float("inf"))).reshape(n, -1)
    order = torch.sort(d, dim=1, stable=True).indices  # ball-major pair index: ties go to the lower ball, then the lower robot
    ds = torch.gather(d, 1, order)
    assign = torch.full((n, p.nr), -1, dtype=torch.int32, device=env.device)
    taken = torch.zeros(n, p.nb, dtype=torch.bool, device=env.device)
    rows = torch.arange(n, device=env.device)
    for k in range(order.shape[1]):  # the walk over the sorted list
        b, r = order[:, k] // p.nr, order[:, k] % p.nr
        ok = torch.isfinite(ds[:, k]) & ~taken[rows, b] & (assign[rows, r] < 0)
        assign[rows, r] = torch.where(ok, b.to(torch.int32), assign[rows, r])
        taken[rows, b] |= ok
    obs = torch.zeros(n, p.nr, 11, dtype=torch.float32, device=env.device)
    for r in range(p.nr):
        if not (mask >> r) & 1:
            continue
        for b in range(p.nb):
            g = env.get_game_state(1 if r < p.nr_happy else -1, r, b)
            obs[:, r] = torch.where((assign[:, r] == b).unsqueeze(-1), g, obs[:, r])
    return assign, obs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_hive needs the MI355X: a timing taken elsewhere says nothing")
    import roborugby_amd as rr
    from roborugby_amd.dqn import BatchedDQNAgent
    from roborugby_amd.players import Hive, chase, og_twitchy
    n = a.num_envs
    env = rr.BatchedRoboRugbyEnv(n, preset="G", seed=3)
    p = env.preset
    obs = env.reset()
    for s in range(50):
        obs, _, _, _ = env.step(chase(env, obs, step=s, seed=9))
    res = dict(num_envs=n, preset="G", dtype="f64", lanes_per_env=env.lanes_per_env())
    full = (1 << p.nr) - 1
    out_a = (torch.empty(n, p.nr, dtype=torch.int32, device=env.device), torch.empty(n, p.nr, 11, device=env.device))
    res["a_hive_observe_v2"] = timed(lambda: env.hive_observe(full, observer="SingleBall_6wayLidar_v2", out=out_a), a.reps)
    res["a_hive_observe_v1"] = timed(lambda: env.hive_observe(full, observer="SingleBall_6wayLidar", out=out_a), a.reps)
    ref_assign, ref_obs = env.hive_observe(full, observer="SingleBall_6wayLidar_v2")
    got_assign, got_obs = composed_hive_observe(env, full)
    res["b_agrees_with_a"] = dict(assign_rows_equal=float((got_assign == ref_assign).all(1).double().mean()),
                                  obs_rows_equal_where_assign_equal=bool(torch.equal(got_obs[got_assign == ref_assign], ref_obs[got_assign == ref_assign])))
    res["b_composed_on_parent_api"] = timed(lambda: composed_hive_observe(env, full), max(5, a.reps // 3), inner=1, warmup=2)
    row = torch.empty(n, 11, device=env.device)
    import ctypes as C
    stream = lambda: C.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)  # noqa: E731

    def four_observes():
        for r in range(p.nr):
            env._lib.rr_observe(env._h, 1 if r < p.nr_happy else -1, r, r, C.c_void_p(row.data_ptr()), stream())
    res["c_four_rr_observe"] = timed(four_observes, a.reps)
    # (d) full steps
    agent = BatchedDQNAgent(device=str(env.device), seed=0, batch_size=64, max_mem_size=64)  # fixed random weights: the cost does not depend on them
    hive = Hive(env, agent, epsilon=0.2, seed=1)
    gen = torch.Generator(device=env.device)
    gen.manual_seed(5)
    thrust = torch.zeros(n, 2 * p.nr, device=env.device)

    def hive_step():
        thrust[:, 2 * p.nr_happy:] = og_twitchy(n, p.nr_grumpy, generator=gen, device=env.device)
        hive.act(out=thrust)
        env.step_thrust(thrust)
    state = {"obs": obs, "s": 50}

    def chase_step():
        state["obs"], _, _, _ = env.step(chase(env, state["obs"], step=state["s"], seed=9))
        state["s"] += 1
    for name, fn in (("d_hive_act_plus_step_thrust", hive_step), ("d_chase_plus_step", chase_step)):
        env.reset()
        state["obs"] = env.get_game_state()
        for _ in range(a.steps):
            fn()
        r = timed(fn, 5, inner=a.steps // 5, warmup=0)
        r["env_steps_per_s"] = n / (r["median_ms"] / 1e3)
        res[name] = r
    res["d_hive_act_alone"] = timed(lambda: hive.act(out=thrust), a.reps)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
