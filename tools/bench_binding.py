"""Host time per call of the Python binding, this tree against another checkout of the project (--parent DIR: the commit before, its
roborugby_amd/ holding a copy of the same built library), both loaded into ONE process under different names and timed alternately.

Two launch-bound loops at 64 arenas, where the Python around a launch is what shows: env.step(a, out=out) at preset T, and
Hive.act(out=thrust) + env.step_thrust(thrust) at preset G.  Per repeat: perf_counter around CALLS calls, closed by one synchronise.
The bar: this tree's median per-call time <= the parent's median + the parent's own spread (max - min over its repeats).

    python tools/bench_binding.py --parent ../parent-checkout [--out binding_ab.json]"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEATS, CALLS, WARM, N = 5, 2000, 300, 64


def load_pkg(name, root):
    d = os.path.join(root, "roborugby_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def step_loop(pkg):
    env = pkg.BatchedRoboRugbyEnv(N, preset="T", dtype="f64", seed=1)
    env.reset()
    a = torch.randint(0, 8, (N, 1), device="cuda", dtype=torch.int32)
    f = lambda *t, d=torch.float32: torch.empty((N,) + t, dtype=d, device="cuda")  # noqa: E731
    out = (f(11), f(), f(d=torch.uint8), f(11) if env.has_grumpy else None, f(), f(d=torch.int32))

    def run(k):
        for _ in range(k):
            env.step(a, out=out)
    return run


def hive_loop(pkg):
    players = importlib.import_module(pkg.__name__ + ".players")
    env = pkg.BatchedRoboRugbyEnv(N, preset="G", dtype="f64", seed=1)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(2)
    shapes = [(256, 11), (256,), (256, 256), (256,), (8, 256), (8,)]
    params = [(torch.rand(s, generator=g, device="cuda") - 0.5) * 0.2 for s in shapes]
    hive = players.Hive(env, params, epsilon=0.2, seed=1)
    thr = torch.zeros(N, 2 * env.preset.nr, device="cuda")

    def run(k):
        for _ in range(k):
            hive.act(out=thr)
            env.step_thrust(thr)
    return run


def timed(run):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(CALLS)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t2 - t0) / CALLS * 1e6, (t1 - t0) / CALLS * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="root of the checkout to compare against")
    ap.add_argument("--out", help="write the result here as JSON as well")
    args = ap.parse_args()
    pkgs = {"parent": load_pkg("rr_parent", os.path.abspath(args.parent)), "new": load_pkg("rr_new", ROOT)}
    for name, p in pkgs.items():
        print(name, os.path.dirname(p.__file__), flush=True)
    res = {}
    for wl, make in (("step_T_f64_64", step_loop), ("hive_act+step_thrust_G_64", hive_loop)):
        runs = {k: make(p) for k, p in pkgs.items()}
        for r in runs.values():
            r(WARM)
        torch.cuda.synchronize()
        t = {k: [] for k in runs}
        for rep in range(REPEATS):
            for k in (("parent", "new") if rep % 2 == 0 else ("new", "parent")):
                t[k].append(timed(runs[k]))
        row = {}
        for k, v in t.items():
            total = [x[0] for x in v]
            row[k] = dict(us_per_call=total, enqueue_us_per_call=[x[1] for x in v], median=statistics.median(total),
                          spread=max(total) - min(total))
        row["bar"] = row["parent"]["median"] + row["parent"]["spread"]
        row["met"] = row["new"]["median"] <= row["bar"]
        res[wl] = row
        print(wl, json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
