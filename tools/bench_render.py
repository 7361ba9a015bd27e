"""Times rr_render (BatchedRoboRugbyEnv.render_batch) on the MI355X -- profiles/render/README.md holds the results.

    python tools/bench_render.py [--num-envs 65536] [--reps 30] [--out profiles/render/bench_render.json]

tools/bench_hive.py's protocol: preset G, fp64, HIP events, median (and min / max) of `--reps` repetitions of 10 back-to-back launches
after warm-up.  Three sections, each run in a fresh child process under its own time limit (the first one that fails ends the run):
  kernel  1,024 frames of 96x96 at S = 1 and S = 4, 64 frames of 800x800 at S = 1: time per launch and bytes written over time, next to
          the copy probe (rr_probe_hbm_copy) timed in the same process;
  host    16 native frames on the host: render("rgb_array", arena=k) sixteen times -- the only route before rr_render: a whole-batch
          get_state, one arena copied, PIL -- against render_batch(arenas=those 16).cpu(); host clock around a synchronise, both in
          the same process;
  play    dqn.play_hive at --num-envs arenas for 300 steps with and without record (16 arenas, 96x96), same process.
States: 50 chase steps from reset.  No GPU, no numbers: the script raises without a device."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

INNER = 10
LIMITS = {"kernel": 240, "host": 240, "play": 400}  # seconds per section


def timed(fn, reps, inner=INNER, warmup=3):
    import torch
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


def _env(n):
    import roborugby_amd as rr
    from roborugby_amd.players import chase
    env = rr.BatchedRoboRugbyEnv(n, preset="G", seed=3)
    obs = env.reset()
    for s in range(50):
        obs, _, _, _ = env.step(chase(env, obs, step=s, seed=9))
    return env


def section_kernel(a):
    import ctypes as C
    import torch
    from roborugby_amd import _lib
    env = _env(a.num_envs)
    res = {}
    g = torch.Generator(device=env.device).manual_seed(1)
    for name, m, w, h, S in (("frames_1024_96x96_s1", 1024, 96, 96, 1), ("frames_1024_96x96_s4", 1024, 96, 96, 4),
                             ("frames_64_800x800_s1", 64, 800, 800, 1)):
        idx = torch.randperm(a.num_envs, generator=g, device=env.device)[:m].to(torch.int32)
        out = torch.empty((m, h, w, 3), dtype=torch.uint8, device=env.device)
        r = timed(lambda: env.render_batch(idx, w, h, S, out=out), a.reps)
        r.update(frames=m, width=w, height=h, samples=S, bytes_written=out.numel(),
                 written_TB_per_s=out.numel() / (r["median_ms"] * 1e-3) / 1e12,
                 samples_per_s=m * w * h * S * S / (r["median_ms"] * 1e-3))
        res[name] = r
    nbytes = 1 << 30
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=env.device), torch.empty(nbytes, dtype=torch.uint8, device=env.device)
    lib = _lib.load()

    def probe():
        lib.rr_probe_hbm_copy(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), C.c_size_t(nbytes),
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    r = timed(probe, a.reps)
    r.update(bytes_read_plus_written=2 * nbytes, TB_per_s=2 * nbytes / (r["median_ms"] * 1e-3) / 1e12)
    res["copy_probe_1GiB"] = r
    env.close()
    return res


def section_host(a):
    import torch
    env = _env(a.num_envs)
    arenas = list(range(0, 16 * 37, 37))

    def old():
        return [env.render("rgb_array", arena=k) for k in arenas]

    def new():
        return env.render_batch(arenas=arenas).cpu()
    res = {}
    for name, fn in (("parent_route_16x_render_rgb_array", old), ("render_batch_16_native_to_host", new)):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name] = dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), reps=5, frames=16)
    res["speedup"] = res["parent_route_16x_render_rgb_array"]["median_ms"] / res["render_batch_16_native_to_host"]["median_ms"]
    env.close()
    return res


def section_play(a):
    from roborugby_amd import dqn
    with tempfile.TemporaryDirectory() as d:
        ck, gif = os.path.join(d, "ck.pt"), os.path.join(d, "hive.gif")
        dqn.train(num_envs=1024, steps=4, preset="T", checkpoint=ck, log_every=0, batch_size=1024)  # (the cost does not depend on the weights)
        dqn.play_hive(ck, num_envs=a.num_envs, steps=20, seed=1)  # warm-up
        plain = dqn.play_hive(ck, num_envs=a.num_envs, steps=300, seed=2)
        t0 = time.perf_counter()
        taped = dqn.play_hive(ck, num_envs=a.num_envs, steps=300, seed=2, record=gif)
        wall = time.perf_counter() - t0
        size = os.path.getsize(gif)
    return dict(steps=300, record_arenas=16, record_size=96, env_steps_per_s_plain=plain["env_steps_per_s"],
                env_steps_per_s_recording=taped["env_steps_per_s"], ratio=taped["env_steps_per_s"] / plain["env_steps_per_s"],
                recording_call_wall_s=wall, gif_bytes=size, same_returns=plain["return_happy"] == taped["return_happy"])


SECTIONS = {"kernel": section_kernel, "host": section_host, "play": section_play}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--section", default=None, choices=sorted(SECTIONS), help="run ONE section in this process and print its JSON")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("bench_render needs the MI355X: a timing taken elsewhere says nothing")
    if a.section:
        print("RESULT " + json.dumps(SECTIONS[a.section](a)))
        return
    res = dict(num_envs=a.num_envs, preset="G", dtype="f64")
    for name in ("kernel", "host", "play"):
        cmd = [sys.executable, os.path.abspath(__file__), "--section", name, "--num-envs", str(a.num_envs), "--reps", str(a.reps)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMITS[name])
        if done.returncode != 0:  # nothing more is started on the device after a failure
            raise RuntimeError(f"section {name} ended with status {done.returncode}")
        res[name] = json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
