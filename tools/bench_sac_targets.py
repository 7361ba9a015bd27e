"""rr_sac_targets against the torch no-grad half of the SAC learn step it replaces, and a whole learn() with fused_targets on and off, on
the GPU: B = 4,096 and 65,536 rows, A = 2 and 4 actions.

    python tools/bench_sac_targets.py [--out profiles/sac_targets/bench_sac_targets.json] [--launches 50] [--rounds 5] [--step-limit 240]

Per shape, in one child process under its own time limit (a child that fails or runs out of time ends the run: nothing else is started
on the GPU after it), on one agent whose replay holds 2 B transitions:
  (a) targets_kernel_ms   one rr_sac_targets call on the rings (gathers, its own draws, value_target, q_hat, the gathered state / action)
      targets_torch_ms    what it replaces: the five replay gathers, torch.randn, BatchedSACAgent.targets (actor sample, both critics,
                          the target value net, the closing arithmetic) -- the same index vector for both
  (b) learn_fused_ms / learn_torch_ms   a whole learn() -- torch.randint, the targets, the autograd half, three Adam steps, the soft
                          update -- on two agents that differ in fused_targets alone
The paths are ALTERNATED -- every round times each of them over `launches` back-to-back calls between HIP events, after a warm-up -- and
the median round is reported, so that clocks and whatever else drifts during the run weigh on all of them alike."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
SHAPES = [(4096, 2), (4096, 4), (65536, 2), (65536, 4)]


def _timed(fn, launches):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / launches  # ms per call


def step_shape(B, n_actions, launches, rounds, warmup=5):
    import torch
    from roborugby_amd.sac import BatchedSACAgent
    dev = "cuda:0"
    rows = 2 * B
    g = torch.Generator(device=dev).manual_seed(B + n_actions)

    def agent(fused_targets):
        ag = BatchedSACAgent(n_actions=n_actions, batch_size=B, max_mem_size=rows, device=dev, seed=1, fused_targets=fused_targets)
        ag.remember(torch.rand(rows, 11, generator=g, device=dev) * 2 - 1, torch.rand(rows, n_actions, generator=g, device=dev) * 2 - 1,
                    torch.randn(rows, generator=g, device=dev), torch.rand(rows, 11, generator=g, device=dev) * 2 - 1,
                    torch.rand(rows, generator=g, device=dev) < 0.2)
        return ag

    on, off = agent(True), agent(False)
    idx = torch.randint(0, rows, (B,), generator=g, device=dev)

    def targets_torch():
        batch = (on.state_memory[idx], on.action_memory[idx], on.reward_memory[idx], on.new_state_memory[idx], on.terminal_memory[idx])
        return on.targets(batch, torch.randn((B, n_actions), generator=on.gen, device=dev))

    def targets_kernel():
        on._learn_calls += 1
        return on.targets_fused(idx)

    paths = dict(targets_kernel_ms=targets_kernel, targets_torch_ms=targets_torch, learn_fused_ms=on.learn, learn_torch_ms=off.learn)
    for fn in paths.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(_timed(fn, launches))
    res = dict(batch=B, n_actions=n_actions, replay_rows=rows, launches=launches, rounds=rounds)
    for k, v in times.items():
        res[k] = statistics.median(v)
        res[k.replace("_ms", "_ms_min_max")] = [min(v), max(v)]
    # same parameters, same rows, the kernel's draws fed to the torch path: the two target vectors next to each other (fp32 both)
    noise = torch.empty(B, n_actions, device=dev)
    vt, qh, state, action = on.targets_fused(idx, noise_out=noise)
    vt_t, qh_t = on.targets((state, action, on.reward_memory[idx], on.new_state_memory[idx], on.terminal_memory[idx]), noise)
    res["q_hat_max_abs_diff_to_torch"] = float((qh - qh_t).abs().max())
    res["value_target_median_abs_diff_to_torch"] = float((vt - vt_t).abs().median())
    res["targets_torch_over_kernel"] = res["targets_torch_ms"] / res["targets_kernel_ms"]
    res["learn_torch_over_fused"] = res["learn_torch_ms"] / res["learn_fused_ms"]
    on.close()
    off.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sac_targets", "bench_sac_targets.json"))
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=240, help="seconds per step (a child process)")
    ap.add_argument("--step", default=None, help="(internal) run one shape in this process and print its JSON: 'B,A'")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step_shape(*[int(v) for v in a.step.split(",")], a.launches, a.rounds)), flush=True)
        return 0
    out = dict(tool="tools/bench_sac_targets.py", launches=a.launches, rounds=a.rounds, shapes=[])
    for step in [f"{B},{A}" for B, A in SHAPES]:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--launches", str(a.launches), "--rounds", str(a.rounds)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_limit)
        except subprocess.TimeoutExpired:
            print(f"step {step}: no result within {a.step_limit} s; stopping here", flush=True)
            return 1
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"step {step}: exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", flush=True)
            return 1
        res = json.loads(line[-1][7:])
        print(f"step {step}: {json.dumps(res)}", flush=True)
        out["shapes"].append(res)
    out["kernel_faster_at_every_shape"] = all(s["targets_torch_over_kernel"] > 1.0 for s in out["shapes"])
    out["learn_faster_at_every_shape"] = all(s["learn_torch_over_fused"] > 1.0 for s in out["shapes"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
