"""A seeded trace of both DQN agents (roborugby_amd/dqn.py) through their public surface, to show that a change of the host-side code
moved nothing: run it against two trees (PYTHONPATH) and compare the files byte for byte.

    python tools/agent_trace.py [--device cpu | cuda:0] [--out trace.json] [--params-out params.pt]

Both agents go through one script on the torch path (device "cpu", one thread): construct -> choose_action at epsilon 1, 0.5 and 0 ->
store_transition with a `valid` mask that drops rows -> stores until the ring has wrapped -> learn() / store / learn() / learn() with one
target sync on the way -> state_dict() into a fresh agent built with another seed -> choose_action again.
The JSON has two sections:
  exact   what depends on integer arithmetic and the CPU generator alone: the actions drawn at epsilon 1, the rows _sample would draw
          (from a copy of the agent's generator), ring positions and contents (the inputs are integer-valued), every counter after
          every call, the key set and value types of state_dict().  tests/golden/agent_trace.json holds this section (and the epsilons,
          compared to 1e-12) and tests/test_agent_trace.py holds every tree to it;
  floats  what goes through floating-point kernels: parameter hashes, losses, greedy actions, epsilon.  Equal between two trees on one
          machine with one torch; another CPU may round a convolution differently.
--device cuda:0 adds the fused paths on the GPU: the fused vector agent (128 rows, batch 64, ring 256: rr_dqn_act, rr_dqn_store with
`valid`, rr_dqn_update, checkpoint round trip), the fused pixel agent (40 rows: one whole and one partial 32-row tile) and a players.Hive
over 64 arenas of preset G, once on the agent's rr_dqn handle and once on its own."""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (after PYTHONPATH: another tree's package, where one is given, wins)

COUNTERS = ("mem_cntr", "_eps_cntr", "_next_target_sync", "updates", "target_syncs", "_act_calls")


def _hash(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def _ints(t):
    return t.detach().cpu().to(torch.int64).reshape(-1).tolist()


def _counters(agent):
    return [int(getattr(agent, k)) for k in COUNTERS]


def _params(agent):
    return {k: _hash(v) for k, v in agent.Q_eval.state_dict().items()}


def _rows(kind, n, g, device):
    """observations of either agent with integer-valued entries: a copy into the ring is exact in every format"""
    if kind == "vector":
        return (torch.randint(0, 2048, (n, 11), generator=g).float() / 8).to(device)
    return torch.randint(0, 256, (n, 6, 64, 64), generator=g, dtype=torch.uint8).to(device)


def _make(kind, device, seed, fused, ring, batch, sync):
    from roborugby_amd import dqn
    if kind == "vector":
        return dqn.BatchedDQNAgent(batch_size=batch, max_mem_size=ring, target_update_freq=sync, device=device, seed=seed, fused=fused)
    return dqn.PixelDQNAgent(channels=6, batch_size=batch, max_mem_size=ring, target_update_freq=sync, device=device, seed=seed, fused=fused)


def trace_agent(kind, device="cpu", fused=False, n=None, ring=None, batch=None, sync=None):
    """-> (exact, floats, agent after its three updates).  Defaults: vector agent n = 100, ring 256, batch 64; pixel agent n = 8, ring 32, batch 8."""
    n = n or (100 if kind == "vector" else 8)
    ring = ring or (256 if kind == "vector" else 32)
    batch = batch or (64 if kind == "vector" else 8)
    sync = sync or ring * 3 // 4
    g = torch.Generator().manual_seed(1234)
    exact, floats = dict(counters=[], ring_positions=[], sample_rows=[]), dict(losses=[], epsilon=[])
    agent = _make(kind, device, 3, fused, ring, batch, sync)
    floats["initial_parameters"] = _params(agent)
    floats["target_equals_eval"] = all(torch.equal(a, b) for a, b in zip(agent.Q_eval.parameters(), agent.Q_target.parameters()))

    def mark():
        exact["counters"].append(_counters(agent))

    def store(mask_every):
        s, s2 = _rows(kind, n, g, device), _rows(kind, n, g, device)
        a = torch.randint(0, 8, (n,), generator=g, dtype=torch.int32).to(device)
        r = torch.randint(-3, 4, (n,), generator=g).float().to(device)
        d = (torch.randint(0, 4, (n,), generator=g) == 0).to(device)
        valid = None
        if mask_every:
            valid = torch.ones(n, dtype=torch.bool)
            valid[::mask_every] = False
            valid = valid.to(device)
        agent.store_transition(s, a, r, s2, d, valid=valid)
        exact["ring_positions"].append(int(agent.mem_cntr % agent.mem_size))
        mark()

    def learn():
        copy = torch.Generator(device=agent.gen.device)
        copy.set_state(agent.gen.get_state())
        max_mem = min(agent.mem_size, agent.mem_cntr)
        exact["sample_rows"].append(_ints(torch.randperm(max_mem, generator=copy, device=agent.gen.device)[:agent.batch_size]))
        loss = agent.learn()
        floats["losses"].append(None if loss is None else repr(float(loss)))
        floats["epsilon"].append(agent.epsilon)
        mark()

    mark()
    obs = _rows(kind, n, g, device)
    drawn = agent.choose_action(obs, epsilon_override=1.0)
    exact["actions_epsilon_1"] = _ints(drawn)
    exact["action_dtype"] = str(drawn.dtype)
    mark()
    floats["actions_epsilon_half"] = _ints(agent.choose_action(obs, epsilon_override=0.5))
    mark()
    floats["actions_greedy"] = _ints(agent.choose_action(obs, epsilon_override=0.0))
    mark()
    store(4)  # drops every fourth row
    while agent.mem_cntr <= agent.mem_size:  # ... until the ring has wrapped
        store(0)
    learn()   # the sync: more than `sync` transitions are stored
    store(7)
    learn()
    learn()
    exact["ring"] = dict(state=_hash(agent.state_memory), new_state=_hash(agent.new_state_memory), action=_ints(agent.action_memory),
                         reward=_ints(agent.reward_memory), terminal=_ints(agent.terminal_memory),
                         dtypes=[str(t.dtype) for t in (agent.state_memory, agent.new_state_memory, agent.action_memory,
                                                        agent.reward_memory, agent.terminal_memory)])
    floats["parameters_after_3_updates"] = _params(agent)
    floats["target_after_3_updates"] = {k: _hash(v) for k, v in agent.Q_target.state_dict().items()}
    sd = agent.state_dict()
    exact["state_dict"] = {k: type(v).__name__ for k, v in sorted(sd.items())}
    exact["state_dict_ints"] = {k: sd[k] for k in ("mem_cntr", "updates", "target_syncs", "act_calls", "fused")}
    fresh = _make(kind, device, 11, fused, ring, batch, sync)
    fresh.load_state_dict(sd)
    exact["fresh_counters"] = _counters(fresh)
    floats["fresh_epsilon"] = fresh.epsilon
    floats["fresh_parameters"] = _params(fresh)
    floats["fresh_actions_greedy"] = _ints(fresh.choose_action(obs, epsilon_override=0.0))
    fresh_drawn = _ints(fresh.choose_action(obs, epsilon_override=1.0))
    exact["fresh_actions_epsilon_1"] = fresh_drawn  # (its own seed's draws: the generator's, or the kernel's keyed by seed and call counter)
    floats["next_actions_epsilon_half"] = _ints(agent.choose_action(obs, epsilon_override=0.5))
    exact["fresh_counters_after_acting"] = _counters(fresh)
    fresh.close()
    return exact, floats, agent


def trace_hive(device, agent):
    """three act() / step_thrust rounds of a Hive over 64 arenas of preset G, on the agent's rr_dqn handle and on one of its own"""
    import roborugby_amd as rr
    from roborugby_amd.players import Hive
    exact = {}
    for label, mind in (("borrowed", agent), ("owned", [p.detach() for p in agent.Q_eval.parameters()])):
        env = rr.BatchedRoboRugbyEnv(64, preset="G", device=device, seed=5, action_mode="thrust")
        env.reset()
        hive = Hive(env, mind, epsilon=0.3, seed=2)
        rounds = []
        for _ in range(3):
            env.step_thrust(hive.act())
            rounds.append(dict(actions=_ints(hive.actions), assign=_ints(hive.assign), calls=int(hive.calls)))
        exact[label] = rounds
        hive.close()
        env.close()
    return exact


def trace(device="cpu", params_out=None):
    torch.set_num_threads(1)
    out = dict(exact={}, floats={})
    for kind in ("vector", "pixel"):
        out["exact"][kind], out["floats"][kind], agent = trace_agent(kind)
        agent.close()
    if torch.device(device).type == "cuda":
        kept = {}
        for kind, kw in (("vector", dict(n=128, ring=256, batch=64)), ("pixel", dict(n=40, ring=96, batch=8))):
            out["exact"][f"fused_{kind}"], out["floats"][f"fused_{kind}"], agent = trace_agent(kind, device, fused=True, **kw)
            kept[kind] = {k: v.detach().cpu() for k, v in agent.Q_eval.state_dict().items()}
            if kind == "vector":
                out["exact"]["hive"] = trace_hive(device, agent)
            agent.close()
        if params_out:
            torch.save(kept, params_out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--out", default=None)
    ap.add_argument("--params-out", default=None, help="--device cuda:0: the fused agents' parameters after their updates (torch.save)")
    a = ap.parse_args()
    text = json.dumps(trace(a.device, a.params_out), indent=1, sort_keys=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    import roborugby_amd
    print(hashlib.sha256((text + "\n").encode()).hexdigest(), a.out or "", f"(package: {os.path.dirname(roborugby_amd.__file__)})")


if __name__ == "__main__":
    main()
