"""rr_sac_grads (roborugby_amd/csrc/rr_sac.hip k_sac_grads, k_sac_grads_reduce) against tests/sac_grads_ref.py, through the C ABI as a C
caller would use it.  Every gradient buffer (and loss) is 64 floats longer than its tensor and pre-filled with NaN, so an unwritten
element and a write beyond the tensor both show.

The bar, per gradient tensor and per loss (the project's yardstick, tests/test_agent_reference.py): err <= max(1e-5 * scale, 1.25 * E)
against the float64 restatement, scale = max |float64 value| of the tensor, E = the error of torch float32 autograd of the same loss on the
same rows and device against the same float64.  Printed before it is asserted; profiles/sac_grads/gpu_tests_errors.txt keeps a printout.

The shapes are the smallest at which the item / chunk / reduce logic can go wrong (G = workgroups of the handle, C = max(1, G / 3)
chunks per net): one tile on the default handle (almost every chunk empty); 7 tiles on G = 3 (one workgroup per net, seven tiles deep in
the register accumulators), on G = 2 and G = 1 (a workgroup takes several nets in turn); 5 tiles on G = 7 (C = 2, uneven chunks; the
seventh workgroup would have no item and is not launched); CUs + 1 tiles on the default handle (tiles wrap onto chunk 0)."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sac_grads_ref as gr  # noqa: E402
import sac_ref  # noqa: E402

DEV = "cuda:0"
PAD = 64
GRADS = ("grad_value", "grad_critic_1", "grad_critic_2")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Handle:
    """an rr_dqn handle made under RR_DQN_WGS = wgs (None: the default, one workgroup per CU)"""

    def __init__(self, wgs=None):
        from roborugby_amd import _lib
        self._lib = _lib
        self.lib = _lib.load()
        self.h = C.c_void_p()
        old = os.environ.get("RR_DQN_WGS")
        if wgs is not None:
            os.environ["RR_DQN_WGS"] = str(wgs)  # read at rr_dqn_create
        elif old is not None:
            del os.environ["RR_DQN_WGS"]
        try:
            assert self.lib.rr_dqn_create(0, C.byref(self.h)) == 0, self.lib.rr_dqn_last_error()
        finally:
            if old is None:
                os.environ.pop("RR_DQN_WGS", None)
            else:
                os.environ["RR_DQN_WGS"] = old

    def close(self):
        self.lib.rr_dqn_destroy(self.h)

    def buffers(self, A):
        """NaN-filled outputs: per net six tensors, each PAD floats longer than the parameter, and loss [3 + PAD]"""
        nets = _on_device(A)[0]
        out = {g: [torch.full((p.numel() + PAD,), float("nan"), dtype=torch.float32, device=DEV) for p in nets[n]] for g, n in zip(GRADS, gr.NETS)}
        out["loss"] = torch.full((3 + PAD,), float("nan"), dtype=torch.float32, device=DEV)
        return out

    def args(self, A, B, out):
        nets, state, action, value_target, q_hat = _on_device(A)
        a = self._lib.RRSacGradsArgs()
        a.struct_size, a.batch, a.n_actions, a.flags = C.sizeof(a), B, A, 0
        for name in gr.NETS:
            arr = getattr(a, name)
            for k, p in enumerate(nets[name]):
                arr[k] = p.data_ptr()
        a.state, a.action, a.value_target, a.q_hat = state.data_ptr(), action.data_ptr(), value_target.data_ptr(), q_hat.data_ptr()
        for g in GRADS:
            arr = getattr(a, g)
            for k, t in enumerate(out[g]):
                arr[k] = t.data_ptr()
        a.loss = out["loss"].data_ptr()
        return a

    def run(self, A, B):
        """-> dict: per net the six padded gradient buffers and the padded loss, as numpy arrays"""
        out = self.buffers(A)
        a = self.args(A, B, out)
        rc = self.lib.rr_sac_grads(self.h, C.byref(a), _stream())
        assert rc == 0, self.lib.rr_dqn_last_error()
        torch.cuda.synchronize()
        res = {g: [t.cpu().numpy() for t in out[g]] for g in GRADS}
        res["loss"] = out["loss"].cpu().numpy()
        return res


_handles = {}


def _handle(wgs=None):
    if wgs not in _handles:
        _handles[wgs] = Handle(wgs)
    return _handles[wgs]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _handles.values():
        h.close()
    _handles.clear()


_device_cache = {}


def _on_device(A):
    """(nets on the device, state, action, value_target, q_hat on the device: all CASE_ROWS rows; a call reads its first B)"""
    if A not in _device_cache:
        nets, state, action, value_target, q_hat = gr.case(A)
        dev = lambda x: torch.as_tensor(np.array(x)).to(DEV).contiguous()
        _device_cache[A] = ({k: [dev(p) for p in v] for k, v in nets.items()}, dev(state), dev(action), dev(value_target), dev(q_hat))
    return _device_cache[A]


_e32_cache = {}


def _torch32(A, B):
    """torch float32 autograd of the same two losses on the same rows and device: ({net: six gradients}, loss [3]) as numpy"""
    if (A, B) not in _e32_cache:
        nets, state, action, value_target, q_hat = _on_device(A)
        lin = torch.nn.functional.linear
        grads, losses = {}, []
        for name in gr.NETS:
            params = [p.clone().requires_grad_(True) for p in nets[name]]
            x = state[:B] if name == "value" else torch.cat([state[:B], action[:B]], 1)
            y = value_target[:B] if name == "value" else q_hat[:B]
            f = lin(torch.relu(lin(torch.relu(lin(x, params[0], params[1])), params[2], params[3])), params[4], params[5]).view(-1)
            loss = 0.5 * torch.nn.functional.mse_loss(f, y)
            grads[name] = [g.cpu().numpy() for g in torch.autograd.grad(loss, params)]
            losses.append(float(loss.detach()))
        _e32_cache[(A, B)] = (grads, np.array(losses))
    return _e32_cache[(A, B)]


def _written_exactly(label, res, A):
    nets = gr.case(A)[0]
    for g, n in zip(GRADS, gr.NETS):
        for k, (buf, p) in enumerate(zip(res[g], nets[n])):
            assert np.all(np.isfinite(buf[:p.size])), f"{label}: {g}[{k}] has unwritten or non-finite elements"
            assert np.all(np.isnan(buf[p.size:])), f"{label}: {g}[{k}] was written beyond its tensor"
    assert np.all(np.isfinite(res["loss"][:3])) and np.all(np.isnan(res["loss"][3:])), label


def _bar(label, got, ref64, got32):
    ref64 = np.asarray(ref64, np.float64)
    scale = float(np.abs(ref64).max())
    err = float(np.abs(np.asarray(got, np.float64) - ref64).max())
    E = float(np.abs(np.asarray(got32, np.float64) - ref64).max())
    print(f"  {label}: err {err / scale:.2e}, E {E / scale:.2e} of scale {scale:.3g}")
    assert scale > 0 and err <= max(1e-5 * scale, 1.25 * E), (label, err, E, scale)


def _check(label, res, A, B):
    _written_exactly(label, res, A)
    ref = gr.case_grads64(A, B)
    g32, l32 = _torch32(A, B)
    for j, (g, n) in enumerate(zip(GRADS, gr.NETS)):
        for k, key in enumerate(gr.KEYS):
            want = ref[n]["grads"][k]
            _bar(f"{label} {n}.{key}", res[g][k][:want.size].reshape(want.shape), want, g32[n][k])
        _bar(f"{label} loss[{j}] ({n})", res["loss"][j], ref[n]["loss"], l32[j])


def _same_bits(a, b):
    for g in GRADS:
        for x, y in zip(a[g], b[g]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), g
    assert np.array_equal(a["loss"].view(np.uint32), b["loss"].view(np.uint32))


def _tiles_cus_plus_one():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return min(cus + 1, sac_ref.CASE_ROWS // 64)


SHAPES = {"one tile": (None, 1), "7 tiles on 3 workgroups": (3, 7), "7 tiles on 2 workgroups": (2, 7), "7 tiles on 1 workgroup": (1, 7),
          "5 tiles on 7 workgroups": (7, 5), "CUs + 1 tiles": (None, None)}


@pytest.mark.parametrize("A", [2, 4])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gradients_match_the_reference(shape, A):
    wgs, tiles = SHAPES[shape]
    B = 64 * (_tiles_cus_plus_one() if tiles is None else tiles)
    h = _handle(wgs)
    res = h.run(A, B)
    _check(f"A = {A}, {shape} (B = {B})", res, A, B)
    _same_bits(res, h.run(A, B))  # two identical calls: bit-identical


@pytest.mark.parametrize("A", [2, 4])
def test_inputs_and_parameters_are_left_alone(A):
    nets, state, action, value_target, q_hat = _on_device(A)
    B = 64 * 5
    before = [t.clone() for n in gr.NETS for t in nets[n]] + [state.clone(), action.clone(), value_target.clone(), q_hat.clone()]
    _handle(7).run(A, B)
    after = [t for n in gr.NETS for t in nets[n]] + [state, action, value_target, q_hat]
    for x, y in zip(before, after):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("A", [2, 4])
def test_the_scratch_grows_with_the_batch(A):
    """a fresh handle: one tile (three slots), then 9 tiles (27 slots), then one tile again -- each as a handle that only ever saw that
    shape computes it"""
    h = Handle()
    try:
        small, large, small_again = h.run(A, 64), h.run(A, 64 * 9), h.run(A, 64)
    finally:
        h.close()
    _check(f"A = {A}, 9 tiles after one", large, A, 64 * 9)
    _same_bits(small, _handle().run(A, 64))
    _same_bits(large, _fresh_run(A, 64 * 9))
    _same_bits(small, small_again)


def _fresh_run(A, B):
    h = Handle()
    try:
        return h.run(A, B)
    finally:
        h.close()


def test_misuse_is_refused_before_any_launch():
    A, B = 2, 64
    handle = _handle()
    lib, h = handle.lib, handle.h
    out = handle.buffers(A)
    good = lambda: handle.args(A, B, out)

    def edited(**fields):
        a = good()
        for k, v in fields.items():
            setattr(a, k, v)
        return a

    def holed(name, k):
        a = good()
        getattr(a, name)[k] = None
        return a

    bad = {"wrong struct_size": edited(struct_size=C.sizeof(good()) - 8), "struct_size 0": edited(struct_size=0),
           "batch 0": edited(batch=0), "batch negative": edited(batch=-64), "batch 100": edited(batch=100), "batch 63": edited(batch=63),
           "n_actions 0": edited(n_actions=0), "n_actions 3": edited(n_actions=3), "n_actions 8": edited(n_actions=8),
           "flags 1": edited(flags=1), "flags negative": edited(flags=-1)}
    for name in ("state", "action", "value_target", "q_hat", "loss"):
        bad[f"null {name}"] = edited(**{name: None})
    for name in gr.NETS + GRADS:
        for k in range(6):
            bad[f"null {name}[{k}]"] = holed(name, k)
    for label, a in bad.items():
        rc = lib.rr_sac_grads(h, C.byref(a), _stream())
        assert rc == -1, label
        assert (lib.rr_dqn_last_error() or b"").startswith(b"rr_sac_grads: "), label
    assert lib.rr_sac_grads(None, C.byref(good()), _stream()) == -1 and lib.rr_dqn_last_error().startswith(b"rr_sac_grads: ")
    assert lib.rr_sac_grads(h, None, _stream()) == -1 and lib.rr_dqn_last_error().startswith(b"rr_sac_grads: ")
    torch.cuda.synchronize()
    tensors = [t for g in GRADS for t in out[g]] + [out["loss"]]
    for t in tensors:
        assert bool(torch.isnan(t).all())
    assert lib.rr_sac_grads(h, C.byref(good()), _stream()) == 0  # ... and the same buffers are accepted when nothing is wrong
    torch.cuda.synchronize()
    res = {g: [t.cpu().numpy() for t in out[g]] for g in GRADS}
    res["loss"] = out["loss"].cpu().numpy()
    _written_exactly("after the refusals", res, A)
