"""Times rr_render_ego (BatchedRoboRugbyEnv.render_ego) on the MI355X next to rr_render -- profiles/render_ego/README.md holds the results.

    python tools/bench_render_ego.py [--num-envs 65536] [--reps 30] [--out profiles/render_ego/bench_render_ego.json]

tools/bench_render.py's protocol: preset G, fp64, 50 chase steps from reset, HIP events, median (and min / max) of `--reps` repetitions of
10 back-to-back launches after warm-up, in a fresh child process under its own time limit.  Two modes, each with rr_render at the same
frame count and size timed in the same process (rr_render's frames show the whole field, the ego frames 400 arena units around a robot:
the same number of samples, each through the same layers):
  observation  65,536 frames of 64x64, S = 1 -- every arena seen from one robot (robot k % NR of arena k) -- interleaved and planar;
  clip         1,024 frames of 96x96, S = 1 and S = 4.
No GPU, no numbers: the script raises without a device."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_render import _env, timed  # noqa: E402

LIMIT = 300  # seconds


def section_kernel(a):
    import torch
    env = _env(a.num_envs)
    nr = env.preset.nr
    res = {}
    g = torch.Generator(device=env.device).manual_seed(1)
    modes = (("frames_65536_64x64_s1", 65536, 64, 1, (False, True)), ("frames_1024_96x96_s1", 1024, 96, 1, (False,)),
             ("frames_1024_96x96_s4", 1024, 96, 4, (False,)))
    for name, m, w, S, layouts in modes:
        idx = (torch.randperm(a.num_envs, generator=g, device=env.device)[:m] if m <= a.num_envs else
               torch.arange(m, device=env.device) % a.num_envs).to(torch.int32)
        robots = (torch.arange(m, device=env.device) % nr).to(torch.int32)
        out = torch.empty((m, w, w, 3), dtype=torch.uint8, device=env.device)
        nsamples = m * w * w * S * S

        def stats(r):
            r.update(frames=m, width=w, height=w, samples=S, bytes_written=out.numel(),
                     written_TB_per_s=out.numel() / (r["median_ms"] * 1e-3) / 1e12, samples_per_s=nsamples / (r["median_ms"] * 1e-3))
            return r
        field = stats(timed(lambda: env.render_batch(idx, w, w, S, out=out), a.reps))
        res[name] = dict(field=field)
        for planar in layouts:
            ego = stats(timed(lambda: env.render_ego(idx, robots, w, w, 400.0, 0.0, S, True, planar, out=out), a.reps))
            ego["ego_over_field_time"] = ego["median_ms"] / field["median_ms"]
            res[name]["ego_planar" if planar else "ego_interleaved"] = ego
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--section", default=None, choices=["kernel"], help="run the section in this process and print its JSON")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("bench_render_ego needs the MI355X: a timing taken elsewhere says nothing")
    if a.section:
        print("RESULT " + json.dumps(section_kernel(a)))
        return
    res = dict(num_envs=a.num_envs, preset="G", dtype="f64", span=400.0, ahead=0.0, relative=True)
    cmd = [sys.executable, os.path.abspath(__file__), "--section", "kernel", "--num-envs", str(a.num_envs), "--reps", str(a.reps)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT)
    if done.returncode != 0:
        raise RuntimeError(f"section kernel ended with status {done.returncode}")
    res["kernel"] = json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
