"""rr_cnn_act (roborugby_amd/csrc/rr_cnn.hip) against tests/cnn_ref.py, through the C ABI as a C caller would use it.  The bars come from
the reference alone (cnn_ref.Reference: E, E99 = what three fp32 summation orders on the CPU differ from the fp64-accumulated forward A;
the floor = the classical bound of the last layer): max |Q - Q_A| <= max(4 E, floor), 99th percentile <= max(4 E99, floor), the action =
the first argmax of the returned Q-values on every row and the reference's on every row whose top-two gap exceeds 8 E.
tests/test_cnn_ref.py holds the reference and these input sets to their own conditions without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cnn_ref  # noqa: E402
import dqn_ref  # noqa: E402

DEV = "cuda:0"
POISON_A, POISON_Q = -77, -12345.5


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

    def act(self, params, pixels, n, channels, epsilon=0.0, seed=0, call=1, want_q=True, pad=8):
        """-> (actions [n + pad], qvalues [n + pad, 8] or None) as numpy: rows >= n hold the poison unless the kernel wrote there"""
        actions = torch.full((n + pad,), POISON_A, dtype=torch.int32, device=DEV)
        q = torch.full((n + pad, 8), POISON_Q, dtype=torch.float32, device=DEV) if want_q else None
        ptrs = (C.c_void_p * 8)(*[p.data_ptr() for p in params])
        rc = self.lib.rr_cnn_act(self.h, C.byref(ptrs), _ptr(pixels), n, channels, epsilon, seed, call, _ptr(actions), _ptr(q), _stream())
        assert rc == 0, self.lib.rr_dqn_last_error()
        torch.cuda.synchronize()
        return actions.cpu().numpy(), (q.cpu().numpy() if want_q else None)


@pytest.fixture(scope="module")
def handle():
    h = Handle()
    yield h
    h.close()


_device_cache = {}


def _on_device(name):
    if name not in _device_cache:
        ref = cnn_ref.case(name)
        _device_cache[name] = ([torch.as_tensor(p).to(DEV).contiguous() for p in ref.params], torch.as_tensor(ref.pixels).to(DEV).contiguous())
    return _device_cache[name]


def _assert_within_bars(label, ref, actions, q, n):
    assert np.all(actions[n:] == POISON_A) and np.all(q[n:] == POISON_Q), f"{label}: rows beyond n were written"
    a, q = actions[:n], q[:n]
    assert np.all(np.isfinite(q))
    err = np.abs(q.astype(np.float64) - ref.q[:n])
    bar, bar99 = ref.bars(n)
    decided = ref.decided(n)
    print(f"{label}: max err {err.max():.3g} (E {ref.E:.3g}, 4E {4 * ref.E:.3g}, floor max {ref.floor[:n].max():.3g}), p99 {np.percentile(err, 99):.3g} "
          f"(bar {bar99:.3g}), spread {ref.spread:.3g}, decided rows {int(decided.sum())}/{n}")
    assert np.all(err <= bar), (label, float(err.max()), float((err - bar).max()))
    assert np.percentile(err, 99) <= bar99, (label, float(np.percentile(err, 99)), bar99)
    assert np.array_equal(a, dqn_ref.first_argmax(q)), label
    assert np.array_equal(a[decided], ref.actions[:n][decided]), label


RANDOM_AND_BLOCK = sorted(k for k in cnn_ref.CASES if not k.endswith("onepixel"))


@pytest.mark.parametrize("n", [1, 63, 65, 200])
@pytest.mark.parametrize("name", RANDOM_AND_BLOCK)
def test_qvalues_and_actions_match_the_reference(handle, name, n):
    ref = cnn_ref.case(name)
    params, pixels = _on_device(name)
    actions, q = handle.act(params, pixels, n, cnn_ref.CASES[name][0])
    _assert_within_bars(f"{name} n={n}", ref, actions, q, n)


@pytest.mark.parametrize("channels", [3, 6, 9, 12])
def test_one_pixel_rows_index_every_corner_residue_and_channel(handle, channels):
    name = f"c{channels}-onepixel"
    ref = cnn_ref.case(name)
    params, pixels = _on_device(name)
    n = ref.pixels.shape[0]
    actions, q = handle.act(params, pixels, n, channels)
    _assert_within_bars(name, ref, actions, q, n)


def test_tiles_grid_override_repeat_and_null_qvalues(handle):
    name, n = "c6-random-x3", 200
    params, pixels = _on_device(name)
    a0, q0 = handle.act(params, pixels, n, 6)
    a1, q1 = handle.act(params, pixels, n, 6)
    assert np.array_equal(a0, a1) and np.array_equal(q0.view(np.uint32), q1.view(np.uint32))  # two calls: bit-identical
    a2, none = handle.act(params, pixels, n, 6, want_q=False)
    assert none is None and np.array_equal(a0, a2)
    old = os.environ.get("RR_DQN_WGS")
    os.environ["RR_DQN_WGS"] = "2"  # 7 tiles on 2 workgroups: 4 and 3 tiles each
    try:
        two = Handle()
    finally:
        if old is None:
            del os.environ["RR_DQN_WGS"]
        else:
            os.environ["RR_DQN_WGS"] = old
    try:
        a3, q3 = two.act(params, pixels, n, 6)
    finally:
        two.close()
    assert np.array_equal(a0, a3) and np.array_equal(q0.view(np.uint32), q3.view(np.uint32))
    assert np.all(a3[n:] == POISON_A) and np.all(q3[n:] == POISON_Q)


def test_ties_take_the_lower_index(handle):
    c, n = 9, 40
    params = [torch.zeros(s, device=DEV) for s in ((16, c, 8, 8), (16,), (32, 16, 4, 4), (32,), (256, 1152), (256,), (8, 256), (8,))]
    params[7].copy_(torch.tensor([0.0, 5.0, 1.0, 5.0, 0.0, -2.0, 5.0, 0.0]))
    pixels = torch.as_tensor(cnn_ref.random_images(n, c, 3)).to(DEV)
    actions, q = handle.act(params, pixels, n, c)
    assert np.all(actions[:n] == 1)
    assert np.array_equal(q[:n], np.tile(params[7].cpu().numpy(), (n, 1)))


@pytest.mark.parametrize("seed,call", [(2, 1), (2 ** 64 - 1, 7)])
def test_epsilon_draw_is_rr_dqn_acts(handle, seed, call):
    name, n = "c3-block-x3", 200
    params, pixels = _on_device(name)
    greedy, _ = handle.act(params, pixels, n, 3)
    actions, q = handle.act(params, pixels, n, 3, epsilon=0.3, seed=seed, call=call)
    u, drawn = dqn_ref.act_draw_rows(seed, n, call)
    explored = u <= np.float32(0.3)
    assert 30 <= int(explored.sum()) <= 90
    assert np.array_equal(actions[:n][explored], drawn[explored])
    assert np.array_equal(actions[:n][~explored], greedy[:n][~explored])
    assert np.array_equal(greedy[:n], dqn_ref.first_argmax(q[:n]))  # the Q-values are the greedy ones either way
    every, _ = handle.act(params, pixels, n, 3, epsilon=1.0, seed=seed, call=call)
    assert np.array_equal(every[:n], drawn)


def test_guards_refuse_before_launching(handle):
    c, n = 6, 40
    params, pixels = _on_device("c6-random-x1")
    actions = torch.full((n,), POISON_A, dtype=torch.int32, device=DEV)
    q = torch.full((n, 8), POISON_Q, dtype=torch.float32, device=DEV)
    good = (C.c_void_p * 8)(*[p.data_ptr() for p in params])
    holed = (C.c_void_p * 8)(*[p.data_ptr() for p in params])
    holed[5] = None
    lib, h = handle.lib, handle.h
    px, ac, qv = _ptr(pixels), _ptr(actions), _ptr(q)
    off = C.c_void_p(pixels.data_ptr() + 4)
    bad = {
        "null handle": (None, C.byref(good), px, n, c, 0.0, 0, 1, ac, qv),
        "null params": (h, None, px, n, c, 0.0, 0, 1, ac, qv),
        "null params entry": (h, C.byref(holed), px, n, c, 0.0, 0, 1, ac, qv),
        "null pixels": (h, C.byref(good), None, n, c, 0.0, 0, 1, ac, qv),
        "null actions": (h, C.byref(good), px, n, c, 0.0, 0, 1, None, qv),
        "channels 4": (h, C.byref(good), px, n, 4, 0.0, 0, 1, ac, qv),
        "channels 0": (h, C.byref(good), px, n, 0, 0.0, 0, 1, ac, qv),
        "channels 15": (h, C.byref(good), px, n, 15, 0.0, 0, 1, ac, qv),
        "n 0": (h, C.byref(good), px, 0, c, 0.0, 0, 1, ac, qv),
        "n negative": (h, C.byref(good), px, -5, c, 0.0, 0, 1, ac, qv),
        "n too large": (h, C.byref(good), px, (1 << 22) + 1, c, 0.0, 0, 1, ac, qv),
        "epsilon NaN": (h, C.byref(good), px, n, c, float("nan"), 0, 1, ac, qv),
        "epsilon negative": (h, C.byref(good), px, n, c, -0.01, 0, 1, ac, qv),
        "epsilon above one": (h, C.byref(good), px, n, c, 1.5, 0, 1, ac, qv),
        "misaligned pixels": (h, C.byref(good), off, n, c, 0.0, 0, 1, ac, qv),
    }
    for label, args in bad.items():
        rc = lib.rr_cnn_act(*args, _stream())
        assert rc == -1, label
        assert b"rr_cnn_act" in (lib.rr_dqn_last_error() or b""), label
    torch.cuda.synchronize()
    assert bool((actions == POISON_A).all()) and bool((q == POISON_Q).all())
    rc = lib.rr_cnn_act(h, C.byref(good), px, n, c, 0.0, 0, 1, ac, qv, _stream())  # ... and the same buffers are accepted when nothing is wrong
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((actions != POISON_A).all()) and bool((q != POISON_Q).all())
