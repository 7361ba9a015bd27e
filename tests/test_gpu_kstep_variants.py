"""Every k_step instantiation the C-ABI can reach, through every entry that launches it, with and without the optional outputs and with
the slowest-first dispatch order on and off -- the place where a wrong kernel argument or a wrong constant in the step kernel's
register plumbing (rr_kstep.hpp: which arguments live where, per instantiation) shows up.

Shapes T, G, D; the batch is one arena more than a wavefront holds (T 33, G 9, D 17: a ragged last wavefront); 3 steps from
contact-rich states of the reference's recorded trajectories (tests/golden/traj_*.npz: a ball in motion).

  * The reference run of a shape is rr_step_f64 on an fp64 handle with every output.  Each of its steps is checked against the oracle
    started from the handle's own pre-step state, the comparison and the tolerances of tests/test_gpu_env.py (integer state equal,
    fp64 state / observation within 1e-9, rewards within 1e-6, an arena in which the reference would have raised: flag only).
  * Every other way to take the same three steps must give the same bits: rr_step, rr_step_thrust, rr_step_thrust_f64 (the thrust pairs
    are the Direction table's entries of the same actions), rr_rollout with 2 steps followed by one rr_step, a handle with a step budget
    nothing reaches -- each with all outputs and with obs_g / reward_g / status left out, each with RR_NO_ORDER unset and set.  The state
    after every step equals the reference run's bit for bit; fp64 outputs equal it bit for bit; fp32 outputs equal each other bit for
    bit, their rewards are the fp64 ones rounded, their observations lie within 1e-3 of them (test_gpu_env.py's bar for fp32 rows).
  * The fp32-state handle (rr_step, rr_step_f64, rr_step_thrust, rr_step_thrust_f64) and the fp32 handle (rr_step, rr_step_thrust,
    rr_rollout, the budgeted step) take the same steps from the state as they hold it: all their variants agree bit for bit, and the
    fp32-state handle's fp64 outputs are the oracle's from the same rounded state within 1e-9 / 1e-6.
  * rr_create only builds a dispatch order above 2,048 workgroups, so at the batches above RR_NO_ORDER changes nothing.  The order is
    therefore exercised at the smallest batch that has one (plus the same ragged tail): on and off bit for bit, and a sample of arenas
    against the oracle.
No tolerance here is new."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle_lib as ol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BATCH = {"T": 33, "G": 9, "D": 17}                              # arenas per wavefront (64 / lanes per arena) + 1
ORDERED = {"T": 2048 * 32 + 33, "G": 2048 * 8 + 9, "D": 2048 * 16 + 17}  # more than 2,048 workgroups (rr_create) and the same tail
STEPS = 3
NEVER = 2_000_000_000                                           # a step budget in shader clocks that no wavefront reaches
DIR_L = np.array([1, -1, -1, 1, 0, 1, -1, 0], np.float32)       # Direction table, RR_EnvBase.py:593-602: (left, right) per action
DIR_R = np.array([1, -1, 1, -1, 1, 0, 0, -1], np.float32)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@functools.lru_cache(maxsize=None)
def _inputs(preset, n):
    """n pre-step states with a ball in motion, strided over the recorded episodes (repeated when n is larger than their number),
    and seeded actions for every robot: (state dict, actions int32 [STEPS, n, NR])"""
    t = np.load(f"{GOLDEN}/traj_{preset}.npz")
    room = ol.PRESETS[preset]["game_len"] - STEPS - 1
    idx = [(ep, s) for ep in range(t["length"].shape[0]) for s in range(int(t["length"][ep]) - STEPS)
           if np.abs(t["state_balls"][ep, s][:, 6:8]).sum() > 0 and t["state_step"][ep, s] < room]
    assert len(idx) >= min(n, 64)
    take = np.arange(n) % len(idx) if n > len(idx) else np.arange(n) * (len(idx) // n)
    ep = np.array([idx[i][0] for i in take]); s = np.array([idx[i][1] for i in take])
    st = {k: np.ascontiguousarray(t["state_" + k][ep, s]) for k in ("robots", "robots_i", "balls", "step")}
    nr = st["robots"].shape[1]
    acts = np.random.default_rng(n).integers(0, 8, (STEPS, n, nr)).astype(np.int32)
    return st, acts


def _env(preset, n, dtype="f64", budget=0):
    import roborugby_amd as rr
    return rr.BatchedRoboRugbyEnv(n, preset=preset, dtype=dtype, seed=1, time_limit=False, auto_reset=False, step_budget_clocks=budget)


def _call(env, entry, acts, full, steps=1):
    """one launch through the C-ABI itself (the Python wrapper always asks for every output).  acts: int32 [n, NR], or [steps, n, NR]
    for rr_rollout.  -> dict of numpy outputs ([steps, ...] for rr_rollout); obs_g / reward_g / status only when `full`"""
    from roborugby_amd import _lib
    n, dev = env.num_envs, env.device
    f64 = entry.endswith("_f64")
    od = torch.float64 if f64 else torch.float32
    lead = (steps,) if entry == "rr_rollout" else ()
    new = lambda shape, dt: torch.full(lead + shape, 7, dtype=dt, device=dev)
    out = dict(obs=new((n, 11), od), reward=new((n,), od), done=new((n,), torch.uint8))
    if full:
        out.update(obs_g=new((n, 11), od) if env.has_grumpy else None, reward_g=new((n,), od), status=new((n,), torch.int32))
    p = lambda k: C.c_void_p(out[k].data_ptr()) if out.get(k) is not None else None
    a = torch.as_tensor(acts, device=dev).contiguous()
    na = a.shape[-1]
    if "thrust" in entry:  # the same commands as (left, right) pairs
        an = np.asarray(acts)
        a = torch.as_tensor(np.stack([DIR_L[an], DIR_R[an]], axis=-1).reshape(n, 2 * na), device=dev).contiguous()
    args = [env._h, C.c_void_p(a.data_ptr()), na]
    if entry == "rr_rollout":
        args += [steps, 0]
    args += [p("obs"), p("reward"), p("done"), p("obs_g"), p("reward_g"), p("status"), env._stream()]
    _lib.check(getattr(env._lib, entry)(*args), entry, env._lib)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def _run(preset, n, dtype, entry, full, budget=0):
    """STEPS steps through `entry` on a fresh handle: (held pre-state, per-step outputs or None, per-step post-states or None).
    rr_rollout takes 2 steps in one launch and the rest through rr_step: the state after its first step is not observable."""
    st, acts = _inputs(preset, n)
    env = _env(preset, n, dtype, budget)
    env.set_state(st["robots"], st["robots_i"], st["balls"], st["step"])
    held = _np(env.get_state())
    outs, posts = [], []
    if entry == "rr_rollout":
        o = _call(env, entry, acts[:2], full, steps=2)
        outs += [{k: v[0] for k, v in o.items()}, {k: v[1] for k, v in o.items()}]
        posts += [None, _np(env.get_state())]
        for s in range(2, STEPS):
            outs.append(_call(env, "rr_step", acts[s], full)); posts.append(_np(env.get_state()))
    else:
        for s in range(STEPS):
            outs.append(_call(env, entry, acts[s], full)); posts.append(_np(env.get_state()))
    env.close()
    return held, outs, posts


def _check_vs_oracle(tag, preset, pre, post, acts, out, arenas):
    """test_gpu_env.py's comparison of one step: the oracle from the handle's pre-step state (out: fp64 outputs with every member)"""
    has_g = ol.PRESETS[preset]["nr_g"] > 0
    checked = 0
    for a in arenas:
        o = ol.OracleEnv(preset)
        o.set_state(pre["robots"][a], pre["robots_i"][a], pre["balls"][a], None, int(pre["step"][a]))
        r = o.step(acts[a])
        os_ = o.get_state()
        if r["status"] & ~256:  # the reference would have raised: only the flag is comparable
            assert out["status"][a] & r["status"] & ~256, (tag, a)
            continue
        if post is not None:
            assert np.array_equal(os_["robots_i"], post["robots_i"][a]), (tag, a)
            assert np.allclose(os_["balls"], post["balls"][a], atol=1e-9, rtol=0), (tag, a)
            assert np.allclose(os_["robots"][:, :7], post["robots"][a][:, :7], atol=1e-9, rtol=0), (tag, a)
        assert np.allclose(r["obs"], out["obs"][a], atol=1e-9, rtol=0), (tag, a)
        if has_g:
            assert np.allclose(r["obs_g"], out["obs_g"][a], atol=1e-9, rtol=0), (tag, a)
        assert abs(r["reward"] - out["reward"][a]) < 1e-6 and abs(r["reward_g"] - out["reward_g"][a]) < 1e-6, (tag, a)
        assert bool(out["done"][a]) == r["done"] and r["naughty"] == (out["status"][a] >> 16) & 0xFF, (tag, a)
        checked += 1
    return checked


@functools.lru_cache(maxsize=None)
def _reference(preset):
    """the fp64 handle's rr_step_f64 run with every output, each step held to the oracle; shared by the tests, left unchanged"""
    n = BATCH[preset]
    st, acts = _inputs(preset, n)
    held, outs, posts = _run(preset, n, "f64", "rr_step_f64", True)
    assert all(_same(held[k], st[k]) for k in ("robots_i", "balls", "step")) and _same(held["robots"][..., :7], st["robots"][..., :7])
    checked, pre = 0, held
    for s in range(STEPS):
        checked += _check_vs_oracle(f"{preset} step {s}", preset, pre, posts[s], acts[s], outs[s], range(n))
        pre = posts[s]
    assert checked >= STEPS * n // 2  # (most of the steps are comparable: no fault flags)
    return outs, posts


def _assert_same_outputs(tag, got, want):
    """two runs' outputs, member by member over the members both have"""
    for s, (g, w) in enumerate(zip(got, want)):
        for k in g:
            if k in w:
                assert _same(g[k], w[k]), (tag, s, k)


def _assert_same_states(tag, got, want):
    for s, (g, w) in enumerate(zip(got, want)):
        if g is not None and w is not None:
            assert all(_same(g[k], w[k]) for k in w), (tag, s)


def _order_settings(monkeypatch):
    def off(): monkeypatch.delenv("RR_NO_ORDER", raising=False)
    def on(): monkeypatch.setenv("RR_NO_ORDER", "1")
    return (("order default", off), ("RR_NO_ORDER=1", on))


@pytest.mark.parametrize("preset", ["T", "G", "D"])
def test_f64_handle_every_entry_is_the_reference_run(preset, monkeypatch):
    ref_out, ref_post = _reference(preset)
    n = BATCH[preset]
    f32_first = None
    runs = 0
    for oname, setenv in _order_settings(monkeypatch):
        setenv()
        for entry, budget in (("rr_step_f64", 0), ("rr_step", 0), ("rr_step_thrust", 0), ("rr_step_thrust_f64", 0), ("rr_rollout", 0),
                              ("rr_step", NEVER), ("rr_step_f64", NEVER)):
            for full in (True, False):
                tag = f"{preset} f64 handle {entry} budget={budget} full={full} {oname}"
                _, outs, posts = _run(preset, n, "f64", entry, full, budget)
                _assert_same_states(tag, posts, ref_post)
                assert all(("status" in o) == full and ("reward_g" in o) == full for o in outs), tag
                if entry.endswith("_f64"):
                    _assert_same_outputs(tag, outs, ref_out)
                else:
                    if f32_first is None:
                        f32_first = outs
                    _assert_same_outputs(tag, outs, f32_first)
                    for s in range(STEPS):
                        assert _same(outs[s]["reward"], ref_out[s]["reward"].astype(np.float32)), (tag, s)
                        assert np.allclose(outs[s]["obs"], ref_out[s]["obs"], atol=1e-3, rtol=0), (tag, s)
                        assert _same(outs[s]["done"], ref_out[s]["done"]), (tag, s)
                        if full:
                            assert _same(outs[s]["status"], ref_out[s]["status"]), (tag, s)
                            assert _same(outs[s]["reward_g"], ref_out[s]["reward_g"].astype(np.float32)), (tag, s)
                runs += 1
    print(f"[{preset}] {runs} runs of {STEPS} steps x {n} arenas equal the oracle-checked reference run")


@pytest.mark.parametrize("preset", ["T", "G", "D"])
def test_f32_state_handle_every_entry(preset, monkeypatch):
    n = BATCH[preset]
    _, acts = _inputs(preset, n)
    first = {}
    for oname, setenv in _order_settings(monkeypatch):
        setenv()
        for entry in ("rr_step_f64", "rr_step", "rr_step_thrust", "rr_step_thrust_f64"):
            for full in (True, False):
                tag = f"{preset} f32_state handle {entry} full={full} {oname}"
                held, outs, posts = _run(preset, n, "f32_state", entry, full)
                kind = entry.endswith("_f64")
                if "post" not in first:  # the first run: rr_step_f64 with every output, held to the oracle on the same rounded state
                    first["post"] = posts
                    checked, pre = 0, held
                    for s in range(STEPS):
                        checked += _check_vs_oracle(tag, preset, pre, None, acts[s], outs[s], range(n))
                        pre = posts[s]
                    assert checked >= STEPS * n // 2, tag  # (the comparison is not empty: most steps carry no fault flag)
                _assert_same_states(tag, posts, first["post"])
                _assert_same_outputs(tag, outs, first.setdefault(kind, outs))
    for s in range(STEPS):
        assert _same(first[False][s]["reward"], first[True][s]["reward"].astype(np.float32)), (preset, s)
        assert np.allclose(first[False][s]["obs"], first[True][s]["obs"], atol=1e-3, rtol=0), (preset, s)


@pytest.mark.parametrize("preset", ["T", "G", "D"])
def test_f32_handle_every_entry(preset, monkeypatch):
    n = BATCH[preset]
    first = None
    for oname, setenv in _order_settings(monkeypatch):
        setenv()
        for entry, budget in (("rr_step", 0), ("rr_step_thrust", 0), ("rr_rollout", 0), ("rr_step", NEVER)):
            for full in (True, False):
                tag = f"{preset} f32 handle {entry} budget={budget} full={full} {oname}"
                _, outs, posts = _run(preset, n, "f32", entry, full, budget)
                if first is None:
                    first = (outs, posts)
                    assert all(np.isfinite(o["obs"]).all() and np.isfinite(o["reward"]).all() for o in outs), tag
                    assert not _same(posts[-1]["robots"], posts[0]["robots"])  # (the robots do move)
                _assert_same_states(tag, posts, first[1])
                _assert_same_outputs(tag, outs, first[0])


@pytest.mark.parametrize("preset", ["T", "G", "D"])
def test_dispatch_order_on_equals_off(preset, monkeypatch):
    """the smallest batch for which rr_create builds the slowest-first order (it is rebuilt from the launch's own costs after every
    step, so steps 2 and 3 run in an order that is not the identity)"""
    n = ORDERED[preset]
    _, acts = _inputs(preset, n)
    ref = {}
    for oname, setenv in _order_settings(monkeypatch):
        setenv()
        for entry, budget in (("rr_step_f64", 0), ("rr_step", 0), ("rr_rollout", 0), ("rr_step", NEVER)):
            tag = f"{preset} n={n} {entry} budget={budget} {oname}"
            held, outs, posts = _run(preset, n, "f64", entry, True, budget)
            if not ref:
                ref["post"] = posts
                sample = sorted(set(range(0, n, n // 12)) | {n - 1, n - 2})
                checked, pre = 0, held
                for s in range(STEPS):
                    checked += _check_vs_oracle(tag, preset, pre, posts[s], acts[s], outs[s], sample)
                    pre = posts[s]
                assert checked >= STEPS * len(sample) // 2, tag  # (the comparison is not empty)
            _assert_same_states(tag, posts, ref["post"])
            _assert_same_outputs(tag, outs, ref.setdefault(entry.endswith("_f64"), outs))
