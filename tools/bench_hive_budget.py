"""Measures the hive under the budgeted step on the MI355X -- profiles/hive_budget/README.md holds the results.

    python tools/bench_hive_budget.py [--checkpoint ckpt.pt] [--num-envs 65536] [--steps 300] [--budgets 0,50000,150000,400000]
                                      [--launches 200] [--out profiles/hive_budget/bench_hive_budget.json]

Preset G, fp64.  Without --checkpoint a short dqn.train run (preset T) writes one first: the hive needs a policy that chases.
  (a) dqn.play_hive and dqn.train_hive (the agent resumed from the checkpoint) at every budget, identical arguments otherwise: ready
      env-steps/s and the NOT_READY share;
  (b) kernel times, HIP events around `--launches` back-to-back launches after warm-up: rr_hive_observe_held against rr_hive_observe and
      rr_hive_transition_held against rr_hive_transition on a handle that never had a budget (nobody parked), and the held entries on a
      budgeted handle at the parked share a hive run leaves behind (rr_hive_transition refuses that handle);
  (c) Hive.act: the plain path against the held path on the same state.
No GPU, no numbers: the script raises without a device."""
import argparse
import json
import os
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, launches, warmup=20, reps=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(launches):
            fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) / launches)
    out.sort()
    return dict(median_ms=out[len(out) // 2], min_ms=out[0], max_ms=out[-1], reps=reps, launches_per_rep=launches)


def hive_state(n, budget, agent, steps):
    """an env after `steps` steps in which the hive drives all four robots, with what the last step returned"""
    import roborugby_amd as rr
    from roborugby_amd.players import Hive
    env = rr.BatchedRoboRugbyEnv(n, preset="G", seed=3, action_mode="thrust", step_budget_clocks=budget)
    env.track_prior_step()
    env.reset()
    hive = Hive(env, agent, robots=range(4), epsilon=0.2, seed=1)
    thrust = torch.zeros(n, 8, device=env.device)
    for _ in range(steps):
        hive.act(out=thrust)
        _, _, done, info = env.step_thrust(thrust)
    return env, hive, thrust, done, info.status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--budgets", default="0,50000,150000,400000")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_hive_budget needs the MI355X: a timing taken elsewhere says nothing")
    from roborugby_amd import dqn
    n = a.num_envs
    budgets = [int(b) for b in a.budgets.split(",")]
    ck = a.checkpoint
    tmp = None
    if ck is None:
        tmp = tempfile.TemporaryDirectory()
        ck = os.path.join(tmp.name, "ckpt.pt")
        dqn.train(num_envs=n, steps=150, preset="T", checkpoint=ck, log_every=0)
    res = dict(num_envs=n, steps=a.steps, preset="G", dtype="f64", budgets=budgets, play_hive={}, train_hive={})
    keys = ("env_steps_per_s", "env_steps_per_sec", "not_ready_share", "stepped_rows", "ms_per_vector_step", "valid_rows", "transitions")
    for b in budgets:
        r = dqn.play_hive(ck, num_envs=n, steps=a.steps, step_budget_clocks=b)
        res["play_hive"][str(b)] = {k: r[k] for k in keys if k in r}
        print("play_hive", b, json.dumps(res["play_hive"][str(b)]), flush=True)
    for b in budgets:
        r = dqn.train_hive(num_envs=n, steps=a.steps, resume=ck, log_every=0, step_budget_clocks=b)
        res["train_hive"][str(b)] = {k: r[k] for k in keys if k in r}
        print("train_hive", b, json.dumps(res["train_hive"][str(b)]), flush=True)
    # (b), (c): the agent of the checkpoint drives all four robots, so that the state is the contact-rich one
    agent = dqn.BatchedDQNAgent(batch_size=64, max_mem_size=64, device="cuda:0", seed=0)
    agent.load_state_dict(torch.load(ck, map_location="cuda:0")["agent"])
    kt = res["kernels_ms"] = {}
    for label, budget in (("never_budgeted", 0), ("budget_150000", 150000)):
        env, hive, thrust, done, status = hive_state(n, budget, agent, 60)
        parked = float(((status & 16384) != 0).float().mean())
        kt[label] = dict(parked_share=parked)
        for kind, name in ((0, "SingleBall_6wayLidar_v2"), (1, "SingleBall_6wayLidar")):
            buf = (torch.zeros(n, 4, dtype=torch.int32, device=env.device), torch.zeros(n, 4, 11, device=env.device),
                   torch.zeros(n, dtype=torch.uint8, device=env.device))
            outs = (torch.zeros(n, 4, 11, device=env.device), torch.zeros(n, 4, device=env.device),
                    torch.zeros(n, 4, dtype=torch.uint8, device=env.device), torch.zeros(n, 4, dtype=torch.uint8, device=env.device))
            assign = hive.assign
            kt[label][f"observe_kind{kind}"] = timed(lambda: env.hive_observe(15, name, out=buf[:2]), a.launches)
            kt[label][f"observe_held_kind{kind}"] = timed(lambda: env.hive_observe(15, name, out=buf, held=True), a.launches)
            if not budget:
                kt[label][f"transition_kind{kind}"] = timed(lambda: env.hive_transition(assign, status, done, 15, name, out=outs), a.launches)
            kt[label][f"transition_held_kind{kind}"] = timed(lambda: env.hive_transition_held(assign, status, done, 15, name, out=outs),
                                                              a.launches)
        fresh = torch.zeros(n, 4, dtype=torch.int32, device=env.device)
        acc = torch.zeros(n, 4, dtype=torch.int32, device=env.device)
        held = torch.zeros(n, dtype=torch.uint8, device=env.device)
        kt[label]["commit"] = timed(lambda: env.hive_commit(fresh, hive.assign, held, acc, thrust, 15), a.launches)
        if not budget:  # (c) both paths of Hive.act on the same state (the held entries run on any handle)
            import ctypes as C
            stream = C.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
            res["hive_act_ms"] = dict(plain=timed(lambda: hive.act(out=thrust), a.launches),
                                      held=timed(lambda: hive._act_held(thrust, stream), a.launches))
        print(label, json.dumps(kt[label]), flush=True)
        hive.close()
        env.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
