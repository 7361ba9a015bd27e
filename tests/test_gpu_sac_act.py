"""rr_sac_act (roborugby_amd/csrc/rr_sac.hip) against tests/sac_ref.py, through the C ABI as a C caller would use it.  Every output is
pre-filled with NaN (and padded with rows the kernel must not touch), so an unwritten element shows.  The bars:
  head      err <= max(1e-5 * scale, 1.25 * err32) against the float64 forward, err32 = the torch float32 forward's error on the same rows
            (tests/test_gpu_dqn_kernels.py's rule for the same hidden layers);
  noise     max err <= 4 E against the float64 draw, E = the float32 numpy restatement's largest error on the same rows;
  actions   against the float64 squash of the kernel's OWN head and noise: <= max(4 E, 2^-22 * max_action), E the restatement's on them;
  log_prob  the same 4 E rule on the rows where every component has 1 - (a / max_action)^2 >= 2^-10 (beyond, the reference's
            log(1 - a^2 + 1e-6) cancels catastrophically); finite on the others.
tests/test_sac_ref.py holds the reference and the inputs to their own conditions without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sac_ref  # noqa: E402

DEV = "cuda:0"
PAD = 8
DET = 1  # RR_SAC_DETERMINISTIC
BIG_SEED = 0x1234ABCD00000002


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Handle:
    def __init__(self):
        from roborugby_amd import _lib
        self.lib = _lib.load()
        self.h = C.c_void_p()
        assert self.lib.rr_dqn_create(0, C.byref(self.h)) == 0, self.lib.rr_dqn_last_error()

    def close(self):
        self.lib.rr_dqn_destroy(self.h)

    def act(self, params, obs, n, A, max_action=1.0, flags=0, seed=0, call=1, want=(True, True, True)):
        """-> dict of numpy arrays actions [n + PAD, A], log_prob [n + PAD], head [n + PAD, 2A], noise [n + PAD, A] (None where not
        wanted): NaN wherever the kernel did not write"""
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
        out = dict(actions=nan(n + PAD, A), log_prob=nan(n + PAD) if want[0] else None, head=nan(n + PAD, 2 * A) if want[1] else None,
                   noise=nan(n + PAD, A) if want[2] else None)
        ptrs = (C.c_void_p * 8)(*[p.data_ptr() for p in params])
        rc = self.lib.rr_sac_act(self.h, C.byref(ptrs), _ptr(obs), n, A, max_action, flags, seed, call, _ptr(out["actions"]), _ptr(out["log_prob"]),
                                 _ptr(out["head"]), _ptr(out["noise"]), _stream())
        assert rc == 0, self.lib.rr_dqn_last_error()
        torch.cuda.synchronize()
        return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


@pytest.fixture(scope="module")
def handle():
    h = Handle()
    yield h
    h.close()


@pytest.fixture(scope="module")
def two_workgroups():
    old = os.environ.get("RR_DQN_WGS")
    os.environ["RR_DQN_WGS"] = "2"  # read at rr_dqn_create
    try:
        h = Handle()
    finally:
        if old is None:
            del os.environ["RR_DQN_WGS"]
        else:
            os.environ["RR_DQN_WGS"] = old
    yield h
    h.close()


_device_cache = {}


def _on_device(A):
    if A not in _device_cache:
        params, obs = sac_ref.case(A)
        _device_cache[A] = ([torch.as_tensor(p).to(DEV).contiguous() for p in params], torch.as_tensor(obs).to(DEV).contiguous())
    return _device_cache[A]


def _torch_head32(params, obs):
    w1, b1, w2, b2, wm, bm, ws, bs = params
    with torch.no_grad():
        h = torch.relu(torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(obs, w1, b1)), w2, b2))
        return torch.cat([torch.nn.functional.linear(h, wm, bm), torch.nn.functional.linear(h, ws, bs)], 1).cpu().numpy()


def _written_exactly(label, out, n):
    for k, v in out.items():
        if v is not None:
            assert np.all(np.isfinite(v[:n])), f"{label}: {k} has unwritten or non-finite elements in rows < n"
            assert np.all(np.isnan(v[n:])), f"{label}: {k} was written beyond row n"


def _check_squash(label, out, n, max_action):
    """actions and log_prob against the float64 squash of the kernel's own head and noise"""
    head, z = out["head"][:n], out["noise"][:n]
    a64, lp64, _ = sac_ref.squash64(head, z, max_action)
    E_a, E_lp = sac_ref.squash_E(head, z, max_action)
    rows = sac_ref.well_conditioned_rows(a64, max_action)
    err_a = float(np.abs(out["actions"][:n] - a64).max())
    err_lp = float(np.abs(out["log_prob"][:n] - lp64)[rows].max())
    print(f"  {label}: actions max err {err_a:.3g} (E {E_a:.3g}, bar {max(4 * E_a, 2.0 ** -22 * max_action):.3g}); log_prob max err {err_lp:.3g} "
          f"(E {E_lp:.3g}, bar {4 * E_lp:.3g}) on {int(rows.sum())}/{n} well-conditioned rows")
    assert err_a <= max(4 * E_a, 2.0 ** -22 * max_action), (label, err_a, E_a)
    assert err_lp <= 4 * E_lp, (label, err_lp, E_lp)
    assert np.all(np.isfinite(out["log_prob"][:n])), label
    assert np.all(np.abs(out["actions"][:n]) <= max_action), label


def _check_all(label, out, params, obs, n, A, seed, call, max_action=1.0):
    _written_exactly(label, out, n)
    h64 = sac_ref.case_head64(A)[:n]
    err32 = float(np.abs(_torch_head32(params, obs[:n]).astype(np.float64) - h64).max())
    err, scale = float(np.abs(out["head"][:n] - h64).max()), float(np.abs(h64).max())
    z64 = sac_ref.draw64(seed, n, call)[:, :A]
    E = float(np.abs(sac_ref.draw32(seed, n, call)[:, :A] - z64).max())
    err_z = float(np.abs(out["noise"][:n] - z64).max())
    print(f"  {label}: head {err / scale:.2e}, torch fp32 forward {err32 / scale:.2e} of max |head| = {scale:.3g} (vs fp64 forward); "
          f"noise max err {err_z:.3g} (E {E:.3g}, bar {4 * E:.3g})")
    assert err <= max(1e-5 * scale, 1.25 * err32), (label, err, err32, scale)
    assert err_z <= 4 * E, (label, err_z, E)
    _check_squash(label, out, n, max_action)


def _tiles_cus_plus_one():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return min(cus + 1, sac_ref.CASE_ROWS // 64)


@pytest.mark.parametrize("A", [2, 4])
@pytest.mark.parametrize("shape", ["one tile", "CUs + 1 tiles", "9 tiles on 2 workgroups"])
def test_outputs_match_the_reference(handle, two_workgroups, shape, A):
    params, obs = _on_device(A)
    h, n, seed, call = {"one tile": (handle, 64, 2, 7), "CUs + 1 tiles": (handle, 64 * _tiles_cus_plus_one(), BIG_SEED, 0xFFFFFFFF),
                        "9 tiles on 2 workgroups": (two_workgroups, 64 * 9, BIG_SEED, 1)}[shape]
    out = h.act(params, obs, n, A, seed=seed, call=call)
    _check_all(f"A = {A}, {shape} (n = {n})", out, params, obs, n, A, seed, call)
    again = h.act(params, obs, n, A, seed=seed, call=call)
    for k in out:
        assert np.array_equal(out[k][:n].view(np.uint32), again[k][:n].view(np.uint32)), (shape, k)  # two calls: bit-identical


def test_grid_size_does_not_change_a_bit(handle, two_workgroups):
    params, obs = _on_device(4)
    a, b = handle.act(params, obs, 64 * 9, 4, seed=2, call=7), two_workgroups.act(params, obs, 64 * 9, 4, seed=2, call=7)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_max_action_scales_the_action_and_enters_the_log_prob(handle):
    params, obs = _on_device(2)
    n = 256
    out = handle.act(params, obs, n, 2, max_action=0.5, seed=2, call=7)
    _written_exactly("max_action 0.5", out, n)
    _check_squash("A = 2, max_action 0.5", out, n, 0.5)
    assert np.abs(out["actions"][:n]).max() <= 0.5


def test_seed_high_word_and_call_change_the_draws(handle):
    params, obs = _on_device(4)
    n = 128
    base = handle.act(params, obs, n, 4, seed=2, call=7)["noise"][:n]
    high = handle.act(params, obs, n, 4, seed=2 + (1 << 32), call=7)["noise"][:n]
    call = handle.act(params, obs, n, 4, seed=2, call=8)["noise"][:n]
    assert not np.array_equal(base, high) and not np.array_equal(base, call)
    for seed, c, got in ((2 + (1 << 32), 7, high), (2, 8, call)):
        z64 = sac_ref.draw64(seed, n, c)
        E = float(np.abs(sac_ref.draw32(seed, n, c) - z64).max())
        assert float(np.abs(got - z64).max()) <= 4 * E
    # A = 2 takes z0 and z1 of the same rows
    two = handle.act(_on_device(2)[0], obs, n, 2, seed=2, call=7)["noise"][:n]
    assert np.array_equal(two, base[:, :2])


@pytest.mark.parametrize("A", [2, 4])
def test_deterministic_flag(handle, A):
    params, obs = _on_device(A)
    n = 192
    out = handle.act(params, obs, n, A, flags=DET, seed=2, call=7)
    _written_exactly(f"deterministic A = {A}", out, n)
    assert np.all(out["noise"][:n] == 0.0)
    mu = out["head"][:n, :A].astype(np.float64)
    ref = np.tanh(mu)
    E_a, _ = sac_ref.squash_E(out["head"][:n], np.zeros((n, A), np.float32))
    err = float(np.abs(out["actions"][:n] - ref).max())
    print(f"  deterministic A = {A}: actions max err {err:.3g} against tanh(mu) (E {E_a:.3g})")
    assert err <= max(4 * E_a, 2.0 ** -22)
    _check_squash(f"deterministic A = {A}", out, n, 1.0)  # log_prob: the formula at z = 0
    other = handle.act(params, obs, n, A, flags=DET, seed=99, call=1)
    assert np.array_equal(out["actions"][:n], other["actions"][:n])  # no draw enters


@pytest.mark.parametrize("A", [2, 4])
def test_null_outputs_leave_the_actions_alone(handle, A):
    params, obs = _on_device(A)
    n = 128
    full = handle.act(params, obs, n, A, seed=BIG_SEED, call=3)
    for mask in range(8):
        want = (bool(mask & 1), bool(mask & 2), bool(mask & 4))
        out = handle.act(params, obs, n, A, seed=BIG_SEED, call=3, want=want)
        _written_exactly(f"outputs {want}", out, n)
        assert np.array_equal(out["actions"][:n].view(np.uint32), full["actions"][:n].view(np.uint32)), want
        for k, w in zip(("log_prob", "head", "noise"), want):
            assert (out[k] is not None) == w
            if w:
                assert np.array_equal(out[k][:n].view(np.uint32), full[k][:n].view(np.uint32)), (want, k)


def test_clamp_arms(handle):
    """sigma.weight = 0 with sigma.bias = -1: sigma = 1e-6, so x = mu + 1e-6 z and tanh's slope <= 1 keep the action within 1e-6 |z| of
    the deterministic one -- in exact arithmetic.  In float32 both actions are rounded (and x is, before tanh): a difference that small
    is 0 or one step of the float32 grid, so the bar is 1e-6 |z| plus the actions' own rounding floor 2^-22 (the floor of the actions
    bar above).  sigma.bias = 7: sigma is exactly 1 and the action is tanh(mu + z)."""
    A, n = 4, 256
    params, obs = _on_device(A)
    low = list(params)
    low[6], low[7] = torch.zeros_like(params[6]), torch.full_like(params[7], -1.0)
    det = handle.act(low, obs, n, A, flags=DET)
    out = handle.act(low, obs, n, A, seed=2, call=7)
    _written_exactly("sigma bias -1", out, n)
    assert np.all(out["head"][:n, A:] == -1.0)
    z = out["noise"][:n].astype(np.float64)
    diff = np.abs(out["actions"][:n].astype(np.float64) - det["actions"][:n])
    print(f"  sigma = 1e-6: max |a - a_det| {diff.max():.3g}, max excess over 1e-6 |z| {(diff - 1e-6 * np.abs(z)).max():.3g}")
    assert np.all(diff <= 1e-6 * np.abs(z) + 2.0 ** -22)
    _check_squash("sigma = 1e-6", out, n, 1.0)  # (log_prob carries -log(1e-6) per component)
    high = list(params)
    high[6], high[7] = torch.zeros_like(params[6]), torch.full_like(params[7], 7.0)
    out = handle.act(high, obs, n, A, seed=2, call=7)
    assert np.all(out["head"][:n, A:] == 7.0)
    ref = np.tanh(out["head"][:n, :A].astype(np.float64) + 1.0 * out["noise"][:n].astype(np.float64))
    E_a, _ = sac_ref.squash_E(out["head"][:n], out["noise"][:n])
    assert float(np.abs(out["actions"][:n] - ref).max()) <= max(4 * E_a, 2.0 ** -22)
    _check_squash("sigma = 1", out, n, 1.0)


def test_misuse_is_refused_before_any_launch(handle):
    A, n = 2, 64
    params, obs = _on_device(A)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    actions, lp, head, noise = nan(n, A), nan(n), nan(n, 2 * A), nan(n, A)
    good = (C.c_void_p * 8)(*[p.data_ptr() for p in params])
    holed = (C.c_void_p * 8)(*[p.data_ptr() for p in params])
    holed[6] = None
    lib, h = handle.lib, handle.h
    ob, outs = _ptr(obs), (_ptr(actions), _ptr(lp), _ptr(head), _ptr(noise))
    g = C.byref(good)
    bad = {
        "null handle": (None, g, ob, n, A, 1.0, 0, 0, 1, *outs),
        "null params": (h, None, ob, n, A, 1.0, 0, 0, 1, *outs),
        "null params entry": (h, C.byref(holed), ob, n, A, 1.0, 0, 0, 1, *outs),
        "null obs": (h, g, None, n, A, 1.0, 0, 0, 1, *outs),
        "null actions": (h, g, ob, n, A, 1.0, 0, 0, 1, None, *outs[1:]),
        "n 0": (h, g, ob, 0, A, 1.0, 0, 0, 1, *outs),
        "n negative": (h, g, ob, -64, A, 1.0, 0, 0, 1, *outs),
        "n 100": (h, g, ob, 100, A, 1.0, 0, 0, 1, *outs),
        "n 63": (h, g, ob, 63, A, 1.0, 0, 0, 1, *outs),
        "n_actions 0": (h, g, ob, n, 0, 1.0, 0, 0, 1, *outs),
        "n_actions 3": (h, g, ob, n, 3, 1.0, 0, 0, 1, *outs),
        "n_actions 8": (h, g, ob, n, 8, 1.0, 0, 0, 1, *outs),
        "max_action 0": (h, g, ob, n, A, 0.0, 0, 0, 1, *outs),
        "max_action negative": (h, g, ob, n, A, -1.0, 0, 0, 1, *outs),
        "max_action inf": (h, g, ob, n, A, float("inf"), 0, 0, 1, *outs),
        "max_action NaN": (h, g, ob, n, A, float("nan"), 0, 0, 1, *outs),
        "flags 2": (h, g, ob, n, A, 1.0, 2, 0, 1, *outs),
        "flags 3": (h, g, ob, n, A, 1.0, 3, 0, 1, *outs),
        "flags negative": (h, g, ob, n, A, 1.0, -2, 0, 1, *outs),
    }
    for label, args in bad.items():
        rc = lib.rr_sac_act(*args, _stream())
        assert rc == -1, label
        assert (lib.rr_dqn_last_error() or b"").startswith(b"rr_sac_act: "), label
    torch.cuda.synchronize()
    for t in (actions, lp, head, noise):
        assert bool(torch.isnan(t).all())
    rc = lib.rr_sac_act(h, g, ob, n, A, 1.0, 0, 0, 1, *outs, _stream())  # ... and the same buffers are accepted when nothing is wrong
    assert rc == 0
    torch.cuda.synchronize()
    for t in (actions, lp, head, noise):
        assert bool(torch.isfinite(t).all())
