"""The robot move on the device, its tail spread over the robot's lane pair by component (csrc/rr_sim.hpp: robot_move_comp_begin), against
the fixture of tests/test_robot_move_pair.py (tests/golden/robot_move_pin.npz: the host emulation of the sources with the move's tail on
one lane; what its arenas are made of: tools/gen_robot_move_pin.py).  One arena per fixture row through set_state / step_f64 / step_thrust:
  * fp64, the parity library and the default library: every array of the state after every step, the status flags and NaughtyBots' set
    bit for bit (the parity library is held to its host emulation this way by test_gpu_parity.py; the default library's sin / cos is
    made of exactly specified operations, so it is held to the same -- the libraries before the split met it too);
  * an fp32-state and an fp32 handle on the one-step arenas, against the bars those handles are held to elsewhere
    (test_gpu_fp32_entries.py: the fp64 oracle on the rounded state to one fp32 ulp on 99.9 % of the arenas; fp32_checks.BAR)."""
import os

import numpy as np
import pytest

import fp32_checks as fc
import fp32_entry_checks as ec
import oracle_lib as ol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robot_move_pin.npz")
PRESETS = ("T", "D", "G", "Dwide")
GROUPS = ("act1", "act3", "thr1")


@pytest.fixture(scope="module")
def pin():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _env(preset, n, **kw):
    import roborugby_amd as rr
    kw.setdefault("time_limit", False)
    kw.setdefault("auto_reset", False)
    return rr.BatchedRoboRugbyEnv(n, preset=ol.product_preset(preset), **kw)


def _same_bits(got, want):
    """equal bit for bit (-0.0 is not +0.0); a NaN matches a NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != np.float64:
        return got == want
    return (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))


def _run(pin, preset, group, **kw):
    """the group's arenas through one handle: the state after every step, the flags and NaughtyBots' set"""
    key = f"{preset}_{group}_"
    thrust = pin.get(key + "thrust")
    acts = thrust if thrust is not None else pin[key + "actions"]
    steps, n = acts.shape[:2]
    env = _env(preset, n, **({"action_mode": "thrust"} if thrust is not None else {}), **kw)
    env.set_state(pin[key + "robots"], pin[key + "robots_i"], pin[key + "balls"], np.zeros(n, np.int32))
    held = {k: v.cpu().numpy() for k, v in env.get_state().items()}
    out = {k: [] for k in ("robots", "robots_i", "balls", "status", "naughty")}
    f64 = kw.get("dtype", "f64") != "f32"
    for s in range(steps):
        if thrust is not None:
            _, _, _, info = env.step_thrust(torch.as_tensor(acts[s]), f64=f64)
        else:
            _, _, _, info = env.step_f64(torch.as_tensor(acts[s])) if f64 else env.step(torch.as_tensor(acts[s]))
        st = env.get_state()
        for k in ("robots", "robots_i", "balls"):
            out[k].append(st[k].cpu().numpy())
        status = info.status.cpu().numpy().astype(np.int64)
        out["status"].append(status & 0xFFFF)
        out["naughty"].append((status >> 16) & 0xFF)
    env.close()
    return held, {k: np.array(v) for k, v in out.items()}


@pytest.mark.parametrize("exact", [True, False], ids=["parity", "default"])
@pytest.mark.parametrize("preset", PRESETS)
def test_device_move_equals_the_fixture_bit_for_bit(pin, preset, exact):
    build = "exact" if exact else "default"
    bad = []
    for group in GROUPS:
        _, got = _run(pin, preset, group, exact_trig=exact)
        for k, g in got.items():
            want = pin[f"{preset}_{group}_{build}_{k}"]
            same = _same_bits(g, want)
            print(f"[{preset} {build} {group}] {k}: {int((~same).sum())} of {same.size} words differ")
            if not same.all():
                at = np.argwhere(~same)[0]
                bad.append((group, k, int((~same).sum()), at.tolist(), g[tuple(at)], want[tuple(at)]))
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["f32_state", "f32"])
@pytest.mark.parametrize("preset", PRESETS)
def test_fp32_handles_on_the_one_step_arenas(pin, preset, dtype):
    key = f"{preset}_act1_"
    acts = pin[key + "actions"][0]
    held, got = _run(pin, preset, "act1", dtype=dtype)
    got = {k: v[0] for k, v in got.items()}
    assert all(np.array_equal(ec.r32(held[k]), held[k], equal_nan=True) for k in ("robots", "balls"))
    if dtype == "f32_state":  # fp64 arithmetic on fp32 records: the oracle's step from the same rounded state, rounded
        ref = fc.oracle_on_rounded_state(preset, held, acts)
        e = np.maximum(fc.rel_err(got["robots"], ref["robots"]), fc.rel_err(got["balls"], ref["balls"]))
        ints = np.all(got["robots_i"] == ref["robots_i"], axis=(1, 2))
        print(f"[{preset} fp32 state] {len(e)} arenas vs the oracle on the rounded state: max rel err {e.max():.2e}, within one fp32 ulp on "
              f"{100 * (e <= 2.5e-7).mean():.2f} %, integer state equal in {100 * ints.mean():.2f} %")
        assert (e <= 2.5e-7).mean() >= 0.999 and ints.mean() >= 0.999, (preset, float(e.max()), float(ints.mean()))
    else:  # all fp32: no contact in these arenas, so the quiet bar
        cfg = ol.PRESETS[preset]
        pre = {k: pin[key + k] for k in ("robots", "robots_i", "balls")}
        post = {k: pin[f"{key}default_{k}"][0] for k in ("robots", "robots_i", "balls")}
        _, e, ints = fc.score(pre, post, got, cfg["W"], cfg["H"])
        # A robot the fixture puts with an edge EXACTLY on its wall is left out, by its input alone: a move into the wall is taken back
        # by adding and subtracting differences, and whether the edge then lies a rounding residue before or behind the wall -- that is,
        # whether the clamp's 0.5 px follows -- is decided by the last bit of the arithmetic at hand.  That is what the bit-for-bit test
        # above pins for fp64; fp32 arithmetic has its own residue (the fp32 host emulation flips 0.5 px in the same arenas).
        r0 = pre["robots"]
        on_wall = ((r0[..., 2] == 0) | (r0[..., 3] == cfg["W"]) | (r0[..., 4] == 0) | (r0[..., 5] == cfg["H"])).any(axis=1)
        assert 0 < on_wall.sum() < 0.5 * len(e)  # (G: 31 of 130 arenas, four robots each)
        print(f"[{preset} fp32] {int((~on_wall).sum())} arenas ({int(on_wall.sum())} with an edge exactly on a wall left out) vs the fp64 fixture: "
              f"max rel err {e[~on_wall].max():.2e} (bar {fc.BAR:g}; left out: {e[on_wall].max():.2e}), integer state equal in {100 * ints.mean():.2f} %")
        assert e[~on_wall].max() <= fc.BAR and ints.all(), (preset, float(e[~on_wall].max()), float(ints.mean()))
