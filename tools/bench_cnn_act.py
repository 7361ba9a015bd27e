"""rr_cnn_act against the torch module it replaces, on the GPU: n = 4,096 and 65,536 rows, C = 3 and 12 channels.

    python tools/bench_cnn_act.py [--out profiles/cnn_act/bench_cnn_act.json] [--launches 20] [--step-limit 240]

Per shape, in one child process under its own time limit (a child that fails or runs out of time ends the run: nothing else is
started on the GPU after it): rr_cnn_act with qvalues = NULL and with qvalues, and PixelQNetwork forward + argmax in torch (fp32, the
agent's fallback path), each timed by HIP events over `launches` launches after a warm-up.  One more child times the HBM copy probe
(rr_probe_hbm_copy, 1 GiB), so that the pixel bytes per second of the kernel stand next to what a plain copy reaches on the same card."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
SHAPES = [(4096, 3), (4096, 12), (65536, 3), (65536, 12)]


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
    return t0.elapsed_time(t1) / launches  # ms per launch


def step_shape(n, channels, launches):
    import torch
    from roborugby_amd.dqn import PixelDQNAgent
    dev = "cuda:0"
    ag = PixelDQNAgent(channels=channels, batch_size=64, max_mem_size=64, device=dev, seed=1, fused=True)
    g = torch.Generator(device=dev).manual_seed(n + channels)
    pixels = torch.randint(0, 256, (n, channels, 64, 64), dtype=torch.uint8, generator=g, device=dev)
    q = torch.empty((n, 8), dtype=torch.float32, device=dev)
    res = dict(n=n, channels=channels, launches=launches, pixel_bytes=pixels.numel())
    res["kernel_ms"] = _timed(lambda: ag.choose_action(pixels, epsilon_override=0.0), launches)
    res["kernel_qvalues_ms"] = _timed(lambda: ag.choose_action(pixels, epsilon_override=0.0, qvalues=q), launches)
    with torch.no_grad():
        res["torch_ms"] = _timed(lambda: ag.Q_eval(pixels).argmax(dim=1).to(torch.int32), launches)
        same = ag.choose_action(pixels, epsilon_override=0.0) == ag.Q_eval(pixels).argmax(dim=1).to(torch.int32)
    res["actions_equal_to_torch_fp32_share"] = float(same.float().mean())  # (bf16 against fp32: near-ties may differ)
    res["kernel_pixel_TB_per_s"] = res["pixel_bytes"] / (res["kernel_ms"] * 1e-3) / 1e12
    res["torch_over_kernel"] = res["torch_ms"] / res["kernel_ms"]
    ag.close()
    return res


def step_copy_probe(launches):
    import torch
    from roborugby_amd import _lib
    lib = _lib.load()
    nbytes = 1 << 30
    src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)

    def copy():
        rc = lib.rr_probe_hbm_copy(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
    ms = _timed(copy, launches)
    return dict(copy_bytes=nbytes, copy_ms=ms, copy_TB_per_s_read_plus_write=2 * nbytes / (ms * 1e-3) / 1e12,
                copy_TB_per_s_read_only=nbytes / (ms * 1e-3) / 1e12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cnn_act", "bench_cnn_act.json"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--step-limit", type=int, default=240, help="seconds per step (a child process)")
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and print its JSON: 'copy' or 'N,C'")
    a = ap.parse_args()
    if a.step:
        res = step_copy_probe(a.launches) if a.step == "copy" else step_shape(*[int(v) for v in a.step.split(",")], a.launches)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    out = dict(tool="tools/bench_cnn_act.py", launches=a.launches, shapes=[])
    for step in ["copy"] + [f"{n},{c}" for n, c in SHAPES]:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--launches", str(a.launches)]
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
        else:
            res["kernel_share_of_copy_probe_read_rate"] = res["kernel_pixel_TB_per_s"] / out["copy_probe"]["copy_TB_per_s_read_plus_write"]
            out["shapes"].append(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
