"""Differential test on synthetic contact-dense states: the kernel's phase source (host-emulated wave) and, on the
GPU, the HIP kernel through the C-ABI, against the CPU oracle."""
import numpy as np
import pytest

import adversarial as adv
import emu_lib as el

TOL = 1e-9
FATAL = 63
# the shapes at the limits of shape_lanes (oracle_lib.PRESETS), at 64 lanes and at their own lane width
LIMIT_SHAPE_CASES = [(p, 120, narrow) for p in "WRQP" for narrow in (False, True)]
# make_corner_states(min_gap=) per preset: R's eight robots, dropped anywhere, overlap in a quarter of the arenas and the reference
# raises there (only the fault flag is defined: 88 of 120 states left, below the 0.8 bar); its robot centres are kept 60 px apart
CORNER_MIN_GAP = {"R": 60.0}


def _oracle_is_unstable_here(preset, robots_xyr, balls_xyv, actions, st):
    """True when the ORACLE's own result moves macroscopically under a 1e-12 perturbation of the ball state: the
    reference's branch structure sits on a knife edge there (typically `bounce_ball_off_bot` deciding whether a
    velocity that is exactly tangent to the contact opposes it, RR_TrashyPhysics.py:201-204)."""
    rng = np.random.RandomState(0)
    for _ in range(12):
        b = balls_xyv * (1.0 + rng.uniform(-1e-12, 1e-12, balls_xyv.shape))
        _, st2 = adv.oracle_step(preset, robots_xyr, b, actions)
        if np.abs(st2["balls"] - st["balls"]).max() > 1e-6 or not np.array_equal(st2["robots_i"], st["robots_i"]):
            return True
    return False


def _compare(preset, res, st, r_res, r_st, ctx, inputs=None):
    """'ok' | 'fault' (the reference would have raised: only the flag is defined) | 'knife' (mismatch on a state where
    the oracle itself is unstable at 1e-12).  Anything else fails."""
    def bad(msg):
        if inputs is not None and _oracle_is_unstable_here(preset, *inputs, st):
            return "knife"
        raise AssertionError((ctx, msg))
    if (r_res["status"] & ~256) != (res["status"] & ~256):
        return bad(("status", r_res["status"], res["status"]))
    if res["status"] & FATAL:
        return "fault"
    if not np.array_equal(r_st["robots_i"], st["robots_i"]) or not np.array_equal(np.isnan(r_st["robots"]), np.isnan(st["robots"])):
        return bad("integer state")
    d = max(float(np.nanmax(np.abs(r_st["robots"] - st["robots"]))), float(np.abs(r_st["balls"] - st["balls"]).max()),
            float(np.abs(r_res["obs"] - res["obs"]).max()))
    if not (d < TOL and abs(r_res["reward"] - res["reward"]) < 1e-6 and r_res["done"] == res["done"]):
        return bad(d)
    return "ok"


@pytest.mark.parametrize("preset,n,narrow", [("T", 360, False), ("T", 240, True), ("G", 150, False), ("G", 150, True), ("D", 240, False), ("D", 180, True),
                                                  ("X", 200, False), ("X", 200, True), ("Y", 240, False), ("Y", 240, True)] + LIMIT_SHAPE_CASES)
def test_emulated_kernel_vs_oracle_on_adversarial_states(preset, n, narrow):
    robots, balls, actions = adv.make_states(preset, n, seed=11 + int(narrow))
    env = el.EmuEnv(preset, narrow=narrow)
    ok = faults = knife = contacts = 0
    for a in range(n):
        res, st = adv.oracle_step(preset, robots[a], balls[a], actions[a])
        env.set_poses(robots[a], balls[a])
        r_res = env.step(actions[a])
        r_st = env.get_state()
        v = _compare(preset, res, st, r_res, r_st, (preset, a), (robots[a], balls[a], actions[a]))
        ok += v == "ok"
        faults += v == "fault"
        knife += v == "knife"
        if v == "ok":
            contacts += int(np.abs(st["balls"][:, 6:] - balls[a][:, 2:] * 0.995 ** 12).max() > 1e-6)
    assert ok > 0.5 * n and contacts > 0.2 * n and knife <= 0.05 * n, (ok, faults, knife, contacts)
    print(f"[{preset} narrow={narrow}] {ok} match ({contacts} with contact responses), {faults} faulted identically, "
          f"{knife} on a knife edge of the reference itself")


@pytest.mark.parametrize("preset,n,narrow", [("T", 900, False), ("T", 600, True), ("G", 160, False), ("G", 120, True), ("D", 400, False), ("D", 300, True),
                                                  ("X", 240, False), ("X", 200, True), ("Y", 300, True)] + LIMIT_SHAPE_CASES)
def test_emulated_kernel_vs_oracle_on_balls_around_robot_corners(preset, n, narrow):
    """the broad phase's corner-zone bound (ball_near_robot) must not drop a hit: balls at 6.4-7.7 px from robot corners"""
    robots, balls, actions = adv.make_corner_states(preset, n, seed=3 + int(narrow), min_gap=CORNER_MIN_GAP.get(preset, 0.0))
    env = el.EmuEnv(preset, narrow=narrow)
    ok = knife = contacts = 0
    for a in range(n):
        res, st = adv.oracle_step(preset, robots[a], balls[a], actions[a])
        env.set_poses(robots[a], balls[a])
        r_res = env.step(actions[a])
        v = _compare(preset, res, st, r_res, env.get_state(), (preset, a), (robots[a], balls[a], actions[a]))
        ok += v == "ok"
        knife += v == "knife"
        if v == "ok":
            contacts += int(np.abs(st["balls"][:, 6:] - balls[a][:, 2:] * 0.995 ** 12).max() > 1e-6)
    assert ok > 0.8 * n and contacts > 0.15 * n and knife <= 0.03 * n, (ok, knife, contacts)


@pytest.mark.gpu
@pytest.mark.parametrize("preset,n,gen", [("T", 6000, "mixed"), ("G", 3000, "mixed"), ("T", 5000, "corners"), ("G", 1500, "corners"), ("D", 4000, "mixed"), ("D", 2500, "corners"),
                                          ("X", 3000, "mixed"), ("X", 1500, "corners"),
                                          ("W", 1500, "mixed"), ("W", 1500, "corners"), ("R", 1500, "mixed"), ("R", 1500, "corners")])
def test_gpu_kernel_vs_oracle_on_adversarial_states(preset, n, gen):
    import torch
    import oracle_lib as ol
    import roborugby_amd as rr
    # (W, R: the seeds of the emulated tests above, at which the oracle alone is known to stay inside the caps below)
    seed = 5 if preset not in "WR" else 11 if gen == "mixed" else 3
    if gen == "mixed":
        robots, balls, actions = adv.make_states(preset, n, seed=seed)
    else:
        robots, balls, actions = adv.make_corner_states(preset, n, seed=seed, min_gap=CORNER_MIN_GAP.get(preset, 0.0))
    env = rr.BatchedRoboRugbyEnv(n, preset=ol.product_preset(preset), time_limit=False, auto_reset=False)
    env.set_poses(robots, balls)
    o, r, d, info = env.step_f64(torch.as_tensor(actions))
    st = {k: v.cpu().numpy() for k, v in env.get_state().items()}
    o, r, d, status = o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy(), info.status.cpu().numpy()
    ok = faults = knife = 0
    for a in range(0, n, 5):
        res, ost = adv.oracle_step(preset, robots[a], balls[a], actions[a])
        g_res = dict(status=int(status[a]) & 0xFFFF, obs=o[a], reward=float(r[a]), done=bool(d[a]))
        g_st = {k: st[k][a] for k in ("robots", "robots_i", "balls")}
        v = _compare(preset, res, ost, g_res, g_st, (preset, a), (robots[a], balls[a], actions[a]))
        ok += v == "ok"
        faults += v == "fault"
        knife += v == "knife"
    assert ok > 0.5 * (n // 5) and knife <= 0.05 * (n // 5)
    print(f"[{preset}] GPU: {ok} adversarial states match the oracle, {faults} faulted identically, {knife} knife-edge")
