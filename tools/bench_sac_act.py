"""rr_sac_act against the torch path of the same agent, on the GPU: n = 4,096 and 65,536 rows, A = 2 and 4 actions.

    python tools/bench_sac_act.py [--out profiles/sac_act/bench_sac_act.json] [--launches 50] [--rounds 5] [--step-limit 240]

Per shape, in one child process under its own time limit (a child that fails or runs out of time ends the run: nothing else is started
on the GPU after it): BatchedSACAgent.choose_action through rr_sac_act, with and without its optional outputs, and the agent's torch path
(the modules' forward, clamp, torch.randn, mul / add, tanh) on the same parameters and observations.  The paths are ALTERNATED -- every
round times each of them over `launches` back-to-back calls between HIP events, after a warm-up -- and the median round is reported, so
that clocks and whatever else drifts during the run weigh on all of them alike."""
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


def step_shape(n, n_actions, launches, rounds, warmup=5):
    import torch
    from roborugby_amd.sac import BatchedSACAgent
    dev = "cuda:0"
    ag = BatchedSACAgent(n_actions=n_actions, batch_size=64, max_mem_size=64, device=dev, seed=1, fused=True)
    g = torch.Generator(device=dev).manual_seed(n + n_actions)
    obs = torch.rand(n, 11, generator=g, device=dev) * 2.0 - 1.0
    lp = torch.empty(n, device=dev)
    head = torch.empty(n, 2 * n_actions, device=dev)
    noise = torch.empty(n, n_actions, device=dev)
    paths = dict(kernel_ms=lambda: ag.choose_action(obs),
                 kernel_all_outputs_ms=lambda: ag._act_fused(obs, False, lp, head, noise),
                 torch_ms=lambda: ag._act_torch(obs))
    for fn in paths.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(_timed(fn, launches))
    res = dict(n=n, n_actions=n_actions, launches=launches, rounds=rounds)
    for k, v in times.items():
        res[k] = statistics.median(v)
        res[k.replace("_ms", "_ms_min_max")] = [min(v), max(v)]
    # same parameters, same observations: the kernel's head next to the modules' (fp32 both, another summation order)
    ag._act_fused(obs, True, None, head, None)
    mu, raw = ag.actor.head(obs)
    res["head_max_abs_diff_to_torch"] = float((head - torch.cat([mu, raw], 1)).abs().max())
    res["torch_over_kernel"] = res["torch_ms"] / res["kernel_ms"]
    ag.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sac_act", "bench_sac_act.json"))
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=240, help="seconds per step (a child process)")
    ap.add_argument("--step", default=None, help="(internal) run one shape in this process and print its JSON: 'N,A'")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step_shape(*[int(v) for v in a.step.split(",")], a.launches, a.rounds)), flush=True)
        return 0
    out = dict(tool="tools/bench_sac_act.py", launches=a.launches, rounds=a.rounds, shapes=[])
    for step in [f"{n},{A}" for n, A in SHAPES]:
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
    out["kernel_faster_at_every_shape"] = all(s["torch_over_kernel"] > 1.0 for s in out["shapes"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
