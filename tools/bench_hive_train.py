"""Times hive training in the full game (rr_hive_transition, players.Hive.store, dqn.train_hive's vector step) on the MI355X --
profiles/hive_train/README.md holds the results.

    python tools/bench_hive_train.py [--num-envs 65536] [--reps 30] [--steps 200] [--out profiles/hive_train/bench_hive_train.json]

tools/bench_hive.py's protocol: 65,536 arenas of preset G, fp64, HIP events, median (and min / max) of `--reps` repetitions of
10 back-to-back launches after warm-up:
  (a) rr_hive_transition, 4-robot mask, both observer kinds, next to rr_hive_observe on the same records (the same loads and
      observations, plus the reward arithmetic);
  (b) one full vector step of dqn.train_hive with learning on -- og_twitchy + Hive.act + step_thrust + Hive.store + 4 x learn() --
      and the same step without the learn() calls and without the store: `--steps` steps each after `--steps` of warm-up (the contact
      mix has to settle, the step's cost depends on it).
States for (a): 50 chase steps from reset, the last one with prior-step tracking on.  No GPU, no numbers: the script raises without a
device."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_hive import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--updates-per-step", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_hive_train needs the MI355X: a timing taken elsewhere says nothing")
    import roborugby_amd as rr
    from roborugby_amd.dqn import BatchedDQNAgent
    from roborugby_amd.players import Hive, chase, og_twitchy
    n = a.num_envs
    # (a) the entry alone
    env = rr.BatchedRoboRugbyEnv(n, preset="G", seed=3)
    p = env.preset
    env.track_prior_step()
    obs = env.reset()
    full = (1 << p.nr) - 1
    for s in range(50):
        if s == 49:
            assign, _ = env.hive_observe(full)
        obs, _, done, info = env.step(chase(env, obs, step=s, seed=9))
    res = dict(num_envs=n, preset="G", dtype="f64", lanes_per_env=env.lanes_per_env())
    out_o = (torch.empty(n, p.nr, dtype=torch.int32, device=env.device), torch.empty(n, p.nr, 11, device=env.device))
    out_t = (torch.empty(n, p.nr, 11, device=env.device), torch.empty(n, p.nr, device=env.device),
             torch.empty(n, p.nr, dtype=torch.uint8, device=env.device), torch.empty(n, p.nr, dtype=torch.uint8, device=env.device))
    for kind, name in ((0, "SingleBall_6wayLidar_v2"), (1, "SingleBall_6wayLidar")):
        res[f"a_hive_transition_v{2 - kind}"] = timed(lambda: env.hive_transition(assign, info.status, done, full, observer=name, out=out_t), a.reps)
        res[f"a_hive_observe_v{2 - kind}"] = timed(lambda: env.hive_observe(full, observer=name, out=out_o), a.reps)
    res["a_valid_share"] = float((out_t[3] != 0).double().mean())
    env.close()
    # (b) the trainer's vector step
    for name, learn in (("b_train_hive_step", True), ("b_act_step_transition_no_learning", False)):
        env = rr.BatchedRoboRugbyEnv(n, preset="G", seed=3, action_mode="thrust")
        env.track_prior_step()
        rows = n * p.nr_happy
        agent = BatchedDQNAgent(device=str(env.device), seed=0, batch_size=min(32768, max(64, rows // 2 // 64 * 64)), max_mem_size=max(500000, 32 * rows))
        hive = Hive(env, agent, epsilon=0.2, seed=1)
        gen = torch.Generator(device=env.device)
        gen.manual_seed(5)
        thrust = torch.zeros(n, 2 * p.nr, device=env.device)
        env.reset()

        def step():
            hive.epsilon = agent.epsilon
            thrust.copy_(og_twitchy(n, p.nr, generator=gen, device=env.device))
            hive.act(out=thrust)
            _, _, done, info = env.step_thrust(thrust)
            if learn:
                hive.store(agent, done, info.status)
                for _ in range(a.updates_per_step):
                    agent.learn()
            else:
                hive.transition(done, info.status)
        for _ in range(a.steps):
            step()
        r = timed(step, 5, inner=max(1, a.steps // 5), warmup=0)
        r["env_steps_per_s"] = n / (r["median_ms"] / 1e3)
        if learn:
            r.update(updates_per_step=a.updates_per_step, batch_size=agent.batch_size, transitions_stored=int(agent.mem_cntr), learn_calls=agent.updates,
                     valid_share=agent.mem_cntr / (rows * 2 * a.steps), epsilon=agent.epsilon)
        res[name] = r
        hive.close()
        agent.close()
        env.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
