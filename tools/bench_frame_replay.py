"""The frame-sharing replay (FrameReplay: rr_frames_push / rr_frames_sample) next to the dense replay of PixelDQNAgent, on the GPU, in one
run: 4,096 rows, stacks 1 and 4, batch 256.

    python tools/bench_frame_replay.py [--out profiles/frame_replay/bench_frame_replay.json] [--launches 20] [--rounds 5] [--step-limit 300]

Each step is a child process under its own time limit (a child that fails or runs out of time ends the run: nothing else is started on the
GPU after it).
  copy        the HBM copy probe (rr_probe_hbm_copy, 1 GiB): what a plain 16-byte-per-thread copy reaches on this card
  replay,S    per vector step, the store of both replays (dense: the copy of the observation before the step + store_transition, as
              train_pixels does it; frames: one rr_frames_push) and, per learn(), what brings a batch to the network (dense: the index draw
              + the five gathers of _learn_core; frames: one rr_frames_sample).  HIP events over `launches` calls after a warm-up, `rounds`
              rounds that alternate the two replays; the median round is quoted, all rounds are kept.  Also rr_frames_sample at a batch of
              32,768, where the launch is long enough to be a bandwidth measurement, with its bytes (2 * stack frames written and
              the distinct frames read per sample, counted from the ages on the device) over its time.
  train,S,M   train_pixels(4096 arenas, stack S, replay M), env-steps/s, two runs per mode, alternating."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
ROWS, BATCH, MEM, FB = 4096, 256, 65536, 12288


def _timed(fn, launches, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / launches  # ms per call


def step_copy_probe(launches):
    import torch
    from roborugby_amd import _lib
    lib = _lib.load()
    nbytes = 1 << 30
    src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)

    def copy():
        assert lib.rr_probe_hbm_copy(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    ms = _timed(copy, launches)
    return dict(copy_bytes=nbytes, copy_ms=ms, copy_TB_per_s_read_plus_write=2 * nbytes / (ms * 1e-3) / 1e12)


def step_replay(stack, launches, rounds):
    import torch
    from roborugby_amd.dqn import PixelDQNAgent
    from roborugby_amd.frame_replay import FrameReplay
    dev = "cuda:0"
    slots = MEM // ROWS + stack
    dense = PixelDQNAgent(channels=3 * stack, batch_size=BATCH, max_mem_size=MEM, device=dev, seed=1)
    rep = FrameReplay(ROWS, slots, stack, device=dev, seed=1)
    g = torch.Generator(device=dev).manual_seed(stack)
    pixels = torch.randint(0, 256, (ROWS, 3 * stack, 64, 64), dtype=torch.uint8, generator=g, device=dev)
    before = torch.empty_like(pixels)
    action = torch.randint(0, 8, (ROWS,), dtype=torch.int32, generator=g, device=dev)
    reward = torch.randn(ROWS, generator=g, device=dev)
    first = torch.rand(ROWS, generator=g, device=dev) < 1 / 300  # an episode of preset T is 300 steps
    done, valid = first.roll(1), ~first

    def dense_store():
        before.copy_(pixels)
        dense.store_transition(before, action, reward, pixels, done, valid=valid)

    def frames_store():
        rep.push(pixels, first, action, reward, done, valid)

    def dense_sample():
        b = dense._sample(min(dense.mem_size, dense.mem_cntr))
        return dense.state_memory[b], dense.new_state_memory[b], dense.action_memory[b], dense.reward_memory[b], dense.terminal_memory[b]

    out = rep._outputs(BATCH)

    def frames_sample():
        rep.sample(BATCH, out=out)

    for _ in range(2 * slots):  # both rings full and wrapped before anything is timed
        dense_store()
        frames_store()
    res = dict(stack=stack, rows=ROWS, batch=BATCH, slots=slots, launches=launches, rounds=rounds, dense_transitions=dense.mem_size,
               frames_capacity=rep.capacity, dense_bytes_per_transition=2 * 3 * stack * 4096 + 13, frames_bytes_per_transition=rep.bytes_per_transition,
               dense_ring_bytes=2 * dense.state_memory.numel(), frames_ring_bytes=rep.frames.numel())
    per_round = dict(dense_store_ms=[], frames_store_ms=[], dense_sample_ms=[], frames_sample_ms=[])
    for _ in range(rounds):
        per_round["dense_store_ms"].append(_timed(dense_store, launches))
        per_round["frames_store_ms"].append(_timed(frames_store, launches))
        per_round["dense_sample_ms"].append(_timed(dense_sample, launches))
        per_round["frames_sample_ms"].append(_timed(frames_sample, launches))
    for k, v in per_round.items():
        res[k], res[k + "_rounds"] = statistics.median(v), v
    res["dense_store_plus_sample_ms"] = res["dense_store_ms"] + res["dense_sample_ms"]
    res["frames_store_plus_sample_ms"] = res["frames_store_ms"] + res["frames_sample_ms"]
    res["frames_push_bytes"] = 2 * ROWS * FB
    res["frames_push_TB_per_s"] = res["frames_push_bytes"] / (res["frames_store_ms"] * 1e-3) / 1e12
    # the sampler as a bandwidth measurement: a batch long enough to fill the card
    big = 32768
    big_out = rep._outputs(big)
    picked = torch.empty((big, 2), dtype=torch.int64, device=dev)
    ms = statistics.median(_timed(lambda: rep.sample(big, out=big_out), launches) for _ in range(rounds))
    # bytes of that launch: what the last call drew (the same call again, with `picked`), the ages behind it
    rep._dqn.call("rr_frames_sample", *[C.c_void_p(x.data_ptr()) for x in (rep.frames, rep.age, rep.action, rep.reward, rep.flags)], ROWS, FB, slots,
                  rep.head, stack, big, None, rep.seed, rep.calls, *[C.c_void_p(x.data_ptr()) for x in (*big_out, picked)], rep._dqn.stream())
    k, row = picked[:, 0], picked[:, 1]
    okk = k >= 0
    k, row = k.clamp(min=1), row.clamp(min=0)
    a1 = rep.age[k % slots, row].long().clamp(max=stack - 1)
    a0 = rep.age[(k - 1) % slots, row].long().clamp(max=stack - 1)
    distinct = torch.maximum(a1, a0 + 1) + 1  # pushes k - max(a1, a0 + 1) .. k
    read = int((distinct * okk).sum()) * FB
    written = big * 2 * stack * FB
    res.update(sample_large_batch=big, sample_large_ms=ms, sample_large_ok_share=float(okk.float().mean()), sample_large_bytes_read=read,
               sample_large_bytes_written=written, sample_large_TB_per_s_read_plus_write=(read + written) / (ms * 1e-3) / 1e12)
    res["sample_bytes_per_batch_of_256"] = dict(written=BATCH * 2 * stack * FB, read_at_most=BATCH * (stack + 1) * FB)
    rep.close()
    dense.close()
    return res


def step_train(stack, mode, steps):
    from roborugby_amd.dqn import train_pixels
    res = train_pixels(num_envs=ROWS, steps=steps, stack=stack, mem_size=MEM, batch_size=BATCH, log_every=0, replay=mode)
    return {k: res[k] for k in ("env_steps_per_sec", "seconds", "steps", "num_envs", "stack", "replay", "replay_bytes_per_transition", "replay_capacity",
                                "learn_calls", "transitions", "loss")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "frame_replay", "bench_frame_replay.json"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--train-steps", type=int, default=150)
    ap.add_argument("--step-limit", type=int, default=300, help="seconds per step (a child process)")
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and print its JSON: 'copy', 'replay,S' or 'train,S,MODE'")
    a = ap.parse_args()
    if a.step:
        kind, *rest = a.step.split(",")
        res = (step_copy_probe(a.launches) if kind == "copy" else step_replay(int(rest[0]), a.launches, a.rounds) if kind == "replay"
               else step_train(int(rest[0]), rest[1], a.train_steps))
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    out = dict(tool="tools/bench_frame_replay.py", launches=a.launches, rounds=a.rounds, replay=[], train=[])
    steps = ["copy", "replay,1", "replay,4"] + [f"train,{s},{m}" for s in (1, 4) for _ in range(2) for m in ("dense", "frames")]
    for step in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--launches", str(a.launches), "--rounds", str(a.rounds),
               "--train-steps", str(a.train_steps)]
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
        if step == "copy":
            out["copy_probe"] = res
        elif step.startswith("replay"):
            res["sample_large_share_of_copy_probe"] = res["sample_large_TB_per_s_read_plus_write"] / out["copy_probe"]["copy_TB_per_s_read_plus_write"]
            out["replay"].append(res)
        else:
            out["train"].append(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
