"""rr_frames_push / rr_frames_sample (roborugby_amd/csrc/rr_frames.hip) against tests/frames_ref.py, through the C ABI as a C caller would
use it: every ring and every output starts as poison, the outputs carry 8 pad rows, everything is compared bit for bit.  Then FrameReplay
against the dense replay of PixelDQNAgent on the real pipeline, and the agent and trainer on it.
tests/test_frames_ref.py holds the reference to a naive model without a GPU; tests/test_frames_emulated.py runs the same grid on the
g++ build of the kernel source."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import frames_ref as fr  # noqa: E402

DEV = "cuda:0"


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


class Handle:
    def __init__(self):
        from roborugby_amd import _lib
        self.lib = _lib.load()
        self.h = C.c_void_p()
        assert self.lib.rr_dqn_create(0, C.byref(self.h)) == 0, self.lib.rr_dqn_last_error()

    def close(self):
        self.lib.rr_dqn_destroy(self.h)


@pytest.fixture(scope="module")
def handle():
    h = Handle()
    yield h
    h.close()


class DeviceRing:
    """frames_ref.Ring's five arrays on the device, poison and all"""

    def __init__(self, rows, slots, frame_bytes, head=0):
        host = fr.Ring(rows, slots, frame_bytes)
        self.rows, self.slots, self.frame_bytes, self.head = rows, slots, frame_bytes, head
        self.t = {f: _dev(a) for f, a in host.arrays().items()}

    def ptrs(self):
        return [_ptr(self.t[f]) for f in fr.RING_FIELDS]

    def push(self, handle, src, stride=None, first=None, action=None, reward=None, done=None, valid=None, offset=0):
        """src: a device tensor; the frames start `offset` bytes in, `stride` bytes apart; the rest: numpy [rows] or None"""
        self.keep = [_dev(x) for x in (first, action, reward, done, valid)]
        f, a, r, d, v = self.keep
        rc = handle.lib.rr_frames_push(handle.h, C.c_void_p(src.data_ptr() + offset), self.frame_bytes if stride is None else stride, _ptr(f),
                                       _ptr(a), _ptr(r), _ptr(d), _ptr(v), self.rows, self.frame_bytes, self.slots, self.head, *self.ptrs(), _stream())
        assert rc == 0, handle.lib.rr_dqn_last_error()
        self.head += 1

    def same_as(self, ref, label):
        torch.cuda.synchronize()
        assert self.head == ref.head
        for f in fr.RING_FIELDS:
            assert self.t[f].cpu().numpy().tobytes() == getattr(ref, f).tobytes(), (label, f)

    def sample(self, handle, stack, batch, index=None, seed=0, call=0, pad=8):
        out = {f: _dev(a) for f, a in fr.poisoned_outputs(batch, stack, self.frame_bytes, pad).items()}
        idx = _dev(None if index is None else np.asarray(index, np.int64))
        rc = handle.lib.rr_frames_sample(handle.h, *self.ptrs(), self.rows, self.frame_bytes, self.slots, self.head, stack, batch, _ptr(idx), seed, call,
                                         *[_ptr(out[f]) for f in fr.OUT_FIELDS], _stream())
        assert rc == 0, handle.lib.rr_dqn_last_error()
        torch.cuda.synchronize()
        return {f: out[f].cpu().numpy() for f in fr.OUT_FIELDS}


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("extra", [1, 3])
@pytest.mark.parametrize("stack", [1, 2, 4])
@pytest.mark.parametrize("fb", [16, 48, 12288])
def test_every_explicit_index_equals_the_reference(handle, fb, stack, extra, rows):
    slots = stack + extra
    rng = np.random.default_rng(fb + 10 * stack + extra + 100 * rows)
    ref, ring = fr.Ring(rows, slots, fb), DeviceRing(rows, slots, fb)
    pushes = 3 * slots + 1
    for n, args in enumerate(fr.random_stream(rng, rows, fb, pushes)):
        fr.push(ref, *args)
        ring.push(handle, _dev(args[0]), None, *args[1:])
        if n + 1 in (1, slots, slots + 1, pushes):
            ring.same_as(ref, n)
            index = fr.every_index(n + 1, rows)
            got = ring.sample(handle, stack, len(index), index=index)
            fr.assert_outputs(got, fr.sample(ref, stack, len(index), index=index), len(index), (n, "explicit"))


@pytest.mark.parametrize("batch", [1, 64, 257])
@pytest.mark.parametrize("density", [1.0, 0.5, 0.02, 0.0])
def test_draw_mode_equals_the_reference(handle, density, batch):
    rows, slots, stack, fb = 37, 9, 4, 48
    rng = np.random.default_rng(int(density * 100) + batch)
    ref, ring = fr.Ring(rows, slots, fb), DeviceRing(rows, slots, fb)
    for args in fr.random_stream(rng, rows, fb, 2 * slots + 3, p_valid=density):
        fr.push(ref, *args)
        ring.push(handle, _dev(args[0]), None, *args[1:])
    seed = 2 ** 64 - 3
    got = ring.sample(handle, stack, batch, seed=seed, call=11)
    want = fr.sample(ref, stack, batch, seed=seed, call=11)
    fr.assert_outputs(got, want, batch, (density, batch))
    if density == 1.0:
        assert got["ok"][:batch].all()
    if density == 0.0:
        assert not got["ok"][:batch].any()
    again = ring.sample(handle, stack, batch, seed=seed, call=11)
    assert all(again[f].tobytes() == got[f].tobytes() for f in fr.OUT_FIELDS)  # the same (seed, call) repeats
    other = ring.sample(handle, stack, batch, seed=seed, call=12)
    fr.assert_outputs(other, fr.sample(ref, stack, batch, seed=seed, call=12), batch, (density, batch, "call 12"))
    if density == 1.0 and batch > 1:
        assert other["picked"].tobytes() != got["picked"].tobytes()  # another call draws differently


def test_strided_source_takes_the_last_three_planes(handle):
    rows, stack, fb = 5, 4, 12288
    rng = np.random.default_rng(8)
    ref, ring = fr.Ring(rows, 6, fb), DeviceRing(rows, 6, fb)
    for n in range(8):
        obs = rng.integers(0, 256, (rows, 3 * stack, 64, 64), dtype=np.uint8)
        meta = fr.random_stream(rng, rows, 16, 1)[0][1:]
        first, rest = (None, (None,) * 4) if n % 3 == 2 else (meta[0], meta[1:])
        fr.push(ref, obs[:, -3:].reshape(rows, fb), first, *rest)
        ring.push(handle, _dev(obs), stack * fb, first, *rest, offset=(stack - 1) * fb)
        ring.same_as(ref, n)
    index = fr.every_index(8, rows)
    fr.assert_outputs(ring.sample(handle, stack, len(index), index=index), fr.sample(ref, stack, len(index), index=index), len(index), "strided")


def test_offsets_beyond_four_gib(handle):
    """a ring just over 4 GiB, allocated and not filled; stack + 1 pushes into its highest slots; the reference follows four of the rows"""
    rows, slots, fb, stack = 4096, 86, 12288, 4
    assert rows * slots * fb > 1 << 32
    ring = DeviceRing.__new__(DeviceRing)
    ring.rows, ring.slots, ring.frame_bytes, ring.head = rows, slots, fb, slots - (stack + 1)
    ring.t = dict(frames=torch.empty((slots, rows, fb), dtype=torch.uint8, device=DEV), age=torch.empty((slots, rows), dtype=torch.uint8, device=DEV),
                  action=torch.empty((slots, rows), dtype=torch.int32, device=DEV), reward=torch.empty((slots, rows), dtype=torch.float32, device=DEV),
                  flags=torch.empty((slots, rows), dtype=torch.uint8, device=DEV))
    watch = [0, 1, 2047, 4095]
    ref = fr.Ring(len(watch), slots, fb)
    ref.head = ring.head
    g = torch.Generator(device=DEV).manual_seed(4)
    rng = np.random.default_rng(4)
    for n in range(stack + 1):
        frames = torch.randint(0, 256, (rows, fb), generator=g, device=DEV, dtype=torch.uint8)
        action, reward = rng.integers(0, 8, rows, dtype=np.int32), rng.standard_normal(rows).astype(np.float32)
        done, valid = (rng.random(rows) < 0.2).astype(np.uint8), np.ones(rows, np.uint8)
        first = None if n == 0 else np.zeros(rows, np.uint8)  # (the first of them restarts every row: nothing is read from the unfilled ring)
        meta = (None,) * 4 if n == 0 else (action, reward, done, valid)
        ring.push(handle, frames, None, first, *meta)
        fr.push(ref, frames[watch].cpu().numpy(), None if first is None else first[watch], *[None if m is None else m[watch] for m in meta])
    assert ring.head == slots
    torch.cuda.synchronize()
    for s in range(slots - (stack + 1), slots):  # the pushed slots, read back where they lie: byte offsets up to 4.3e9
        assert np.array_equal(ring.t["frames"][s, watch].cpu().numpy(), ref.frames[s])
    ks = list(range(slots - (stack + 1), slots))
    index = np.array([(k, r) for k in ks for r in watch], np.int64)
    local = np.array([(k, j) for k in ks for j in range(len(watch))], np.int64)
    got = ring.sample(handle, stack, len(index), index=index)
    want = fr.sample(ref, stack, len(index), index=local)
    assert want["ok"].sum() == stack * len(watch)  # every transition but the bare first push
    want["picked"][want["ok"] == 1, 1] = index[want["ok"] == 1, 1]
    fr.assert_outputs(got, want, len(index), "4 GiB")


def test_guards_refuse_before_launching(handle):
    rows, slots, stack, fb, batch = 5, 6, 4, 48, 4
    rng = np.random.default_rng(1)
    ring = DeviceRing(rows, slots, fb)
    stream = fr.random_stream(rng, rows, fb, 8)
    for args in stream:
        ring.push(handle, _dev(args[0]), None, *args[1:])
    torch.cuda.synchronize()
    before = {f: ring.t[f].clone() for f in fr.RING_FIELDS}
    lib, h = handle.lib, handle.h
    src = torch.zeros((rows, fb + 16), dtype=torch.uint8, device=DEV)
    keep = [_dev(x) for x in stream[0][1:]]
    f, a, r, d, v = [_ptr(x) for x in keep]
    fp, ag, ac, rw, fl = ring.ptrs()
    s = _ptr(src)
    good = dict(h=h, src=s, stride=fb, first=f, action=a, reward=r, done=d, valid=v, rows=rows, fb=fb, slots=slots, head=8, frames=fp, age=ag,
                action_ring=ac, reward_ring=rw, flags=fl)
    bad_push = {
        "null handle": dict(h=None), "null src": dict(src=None), "null frames": dict(frames=None), "null age": dict(age=None),
        "null action ring": dict(action_ring=None), "null reward ring": dict(reward_ring=None), "null flags": dict(flags=None),
        "partly null: action": dict(action=None), "partly null: valid": dict(valid=None), "partly null: three": dict(action=None, reward=None, done=None),
        "rows 0": dict(rows=0), "rows negative": dict(rows=-1), "rows too large": dict(rows=(1 << 22) + 1),
        "frame_bytes 0": dict(fb=0), "frame_bytes 40": dict(fb=40, stride=48), "frame_bytes too large": dict(fb=(1 << 20) + 16, stride=(1 << 20) + 16),
        "stride below frame_bytes": dict(stride=fb - 16), "stride 56": dict(stride=56),
        "misaligned src": dict(src=C.c_void_p(src.data_ptr() + 4)), "misaligned frames": dict(frames=C.c_void_p(ring.t["frames"].data_ptr() + 8)),
        "slots 1": dict(slots=1), "slots 0": dict(slots=0), "head negative": dict(head=-1),
    }
    for label, change in bad_push.items():
        k = dict(good, **change)
        rc = lib.rr_frames_push(k["h"], k["src"], k["stride"], k["first"], k["action"], k["reward"], k["done"], k["valid"], k["rows"], k["fb"], k["slots"],
                                k["head"], k["frames"], k["age"], k["action_ring"], k["reward_ring"], k["flags"], _stream())
        assert rc == -1, label
        assert b"rr_frames_push" in (lib.rr_dqn_last_error() or b""), label
    torch.cuda.synchronize()
    for name in fr.RING_FIELDS:
        assert torch.equal(ring.t[name], before[name]), name

    out = {name: _dev(x) for name, x in fr.poisoned_outputs(batch, stack, fb, 0).items()}
    o = {name: _ptr(out[name]) for name in fr.OUT_FIELDS}
    index = _dev(np.array([[7, 0], [6, 1], [5, 2], [4, 3]], np.int64))
    good = dict(h=h, frames=fp, age=ag, action_ring=ac, reward_ring=rw, flags=fl, rows=rows, fb=fb, slots=slots, head=8, stack=stack, batch=batch,
                index=None, **o)
    bad_sample = {
        "null handle": dict(h=None), "null frames": dict(frames=None), "null age": dict(age=None), "null action ring": dict(action_ring=None),
        "null reward ring": dict(reward_ring=None), "null flags": dict(flags=None), "null state": dict(state=None),
        "null next_state": dict(next_state=None), "null action": dict(action=None), "null reward": dict(reward=None),
        "null terminal": dict(terminal=None), "null ok": dict(ok=None),
        "rows 0": dict(rows=0), "rows too large": dict(rows=(1 << 22) + 1), "frame_bytes 40": dict(fb=40), "frame_bytes 0": dict(fb=0),
        "frame_bytes too large": dict(fb=(1 << 20) + 16), "misaligned frames": dict(frames=C.c_void_p(ring.t["frames"].data_ptr() + 8)),
        "misaligned state": dict(state=C.c_void_p(out["state"].data_ptr() + 4)),
        "misaligned next_state": dict(next_state=C.c_void_p(out["next_state"].data_ptr() + 4)),
        "slots 1": dict(slots=1, stack=1), "head negative": dict(head=-1), "stack 0": dict(stack=0), "stack 9": dict(stack=9, slots=16),
        "slots below stack + 1": dict(slots=4), "batch 0": dict(batch=0), "batch negative": dict(batch=-3), "batch too large": dict(batch=(1 << 20) + 1),
        "empty window, head 0": dict(head=0), "empty window, head 1": dict(head=1),
    }
    for label, change in bad_sample.items():
        k = dict(good, **change)
        rc = lib.rr_frames_sample(k["h"], k["frames"], k["age"], k["action_ring"], k["reward_ring"], k["flags"], k["rows"], k["fb"], k["slots"], k["head"],
                                  k["stack"], k["batch"], _ptr(k["index"]), 5, 1, *[k[name] for name in fr.OUT_FIELDS], _stream())
        assert rc == -1, label
        assert b"rr_frames_sample" in (lib.rr_dqn_last_error() or b""), label
    torch.cuda.synchronize()
    fresh = fr.poisoned_outputs(batch, stack, fb, 0)
    for name in fr.OUT_FIELDS:
        assert out[name].cpu().numpy().tobytes() == fresh[name].tobytes(), name
    # ... an empty window is no refusal with an index (every row ok = 0), and the same buffers are accepted when nothing is wrong
    for change in (dict(head=1, index=index), dict(), dict(picked=None)):
        k = dict(good, **change)
        rc = lib.rr_frames_sample(k["h"], k["frames"], k["age"], k["action_ring"], k["reward_ring"], k["flags"], k["rows"], k["fb"], k["slots"], k["head"],
                                  k["stack"], k["batch"], _ptr(k["index"]), 5, 1, *[k[name] for name in fr.OUT_FIELDS], _stream())
        assert rc == 0, lib.rr_dqn_last_error()
        torch.cuda.synchronize()
        assert bool((out["ok"] <= 1).all()) and (change.get("head") != 1 or not bool(out["ok"].any()))


@pytest.mark.parametrize("stack", [1, 4])
def test_frame_replay_equals_the_dense_replay_on_the_real_pipeline(stack):
    """Preset T with episodes of 12 steps, 64 arenas, 40 steps: one stream feeds the dense ring of PixelDQNAgent and a FrameReplay of 45
    slots; every real transition, fetched by explicit index, equals the dense ring's row bit for bit.
    The masked view.reset comes right after the call that re-placed every arena.  A push is one frame for EVERY row, so a row the masked
    reset leaves alone gets its newest frame a second time -- which no observation can tell from PixelObservation keeping that row's stack
    exactly where the stack is uniform, as it is after a re-placement; anywhere else the loop would call restart() instead."""
    import roborugby_amd as rr
    from roborugby_amd.dqn import PixelDQNAgent
    from roborugby_amd.env import STATUS_NOT_READY, STATUS_WAS_RESET
    from roborugby_amd.frame_replay import FrameReplay
    N, steps = 64, 40
    env = rr.BatchedRoboRugbyEnv(N, preset=dataclasses.replace(rr.PRESETS["T"], game_len_steps=12), device=DEV, seed=3)
    view = rr.PixelObservation(env, robots=0, size=64, stack=stack)
    dense = PixelDQNAgent(channels=3 * stack, batch_size=32, max_mem_size=N * (steps + 1), device=DEV, seed=0)
    rep = FrameReplay(N, 45, stack, device=DEV, seed=0)
    g = torch.Generator(device=DEV).manual_seed(9)
    pixels = view.reset()
    rep.push(pixels)
    where, resets, masked = [], torch.zeros(N, dtype=torch.int64, device=DEV), False
    for i in range(steps):
        before = pixels.clone()
        action = torch.randint(0, 8, (N,), generator=g, device=DEV, dtype=torch.int32)
        pixels, reward, done, info = view.step(action.view(-1, 1))
        first = (info.status & STATUS_WAS_RESET) != 0
        real = (info.status & (STATUS_WAS_RESET | STATUS_NOT_READY)) == 0
        resets += first
        at = dense.mem_cntr
        dense.store_transition(before, action, reward, pixels, done, valid=real)
        rep.push(pixels, first, action, reward, done, real)
        rows = real.nonzero(as_tuple=True)[0]
        where.append((torch.full_like(rows, rep.head - 1), rows, at + torch.arange(len(rows), device=DEV)))
        if not masked and bool(first.all()):
            mask = torch.arange(N, device=DEV) % 3 == 0
            pixels = view.reset(mask)
            rep.push(pixels, first=mask)
            resets += mask
            masked = True
    assert masked and int(resets.min()) >= 2 and rep.head == steps + 2
    k, row, pos = (torch.cat(x) for x in zip(*where))
    assert len(k) == dense.mem_cntr == int((rep.flags.view(-1)[: rep.head * N] & 1).sum()) and len(k) > N * steps // 2
    lo, hi = rep.window()
    assert lo == 1 and hi == rep.head - 1  # nothing has left the ring
    s, s2, a, r, t, ok = rep.sample(len(k), index=torch.stack([k, row], dim=1))
    torch.cuda.synchronize()
    assert bool(ok.all())
    assert torch.equal(s, dense.state_memory[pos]) and torch.equal(s2, dense.new_state_memory[pos])
    assert torch.equal(a.long(), dense.action_memory[pos]) and torch.equal(t, dense.terminal_memory[pos])
    assert torch.equal(r.view(torch.int32), dense.reward_memory[pos].view(torch.int32))
    assert bool(t.any()) and not bool(t.all())
    rep.close()
    dense.close()
    env.close()


TRAIN_KEYS = {"env_steps_per_sec", "seconds", "num_envs", "steps", "transitions", "step_budget_clocks", "learn_calls", "updates_per_step",
              "batch_size", "samples_per_transition", "overlap_learn", "replay_transitions", "target_update_freq", "target_syncs", "epsilon",
              "eps_dec", "eps_end", "finished_episodes", "fused_learn_step", "mean_step_reward", "preset", "dtype", "curve", "stack", "span",
              "fused_act", "loss"}  # what train_pixels reported before the frames replay
NEW_KEYS = {"replay", "replay_bytes_per_transition", "replay_capacity"}


def test_agent_on_frames_learns_without_a_dense_memory():
    """The loss bar: with every row ok the agent's sum(ok * err^2) / sum(ok) and F.mse_loss are the same mean of the same 32 fp32 squares,
    summed in another order -- at most 32 roundings of 2^-24 relative apart; the forward the test repeats may pick another convolution
    algorithm, whose fp32 sums over up to 1152 products differ by some 1e-6 relative in Q.  rtol 1e-4 covers both with a decade to spare."""
    import copy

    import roborugby_amd as rr
    import torch.nn.functional as F
    from roborugby_amd.dqn import PixelDQNAgent
    from roborugby_amd.env import STATUS_WAS_RESET
    N, stack = 64, 2
    env = rr.BatchedRoboRugbyEnv(N, preset="T", device=DEV, seed=5)
    view = rr.PixelObservation(env, robots=0, size=64, stack=stack)
    ag = PixelDQNAgent(channels=3 * stack, batch_size=32, device=DEV, seed=2, replay="frames", replay_rows=N, replay_slots=8)
    assert ag.state_memory is None and ag.new_state_memory is None and ag.action_memory is None and ag.mem_size == ag.replay.capacity == 6 * N
    with pytest.raises(RuntimeError, match="store_step"):
        ag.store_transition(None, None, None, None, None)
    pixels = view.reset()
    ag.store_step(pixels)
    assert ag.mem_cntr == 0 and ag.learn() is None
    for _ in range(4):
        action = ag.choose_action(pixels)
        pixels, reward, done, info = view.step(action.view(-1, 1))
        ag.store_step(pixels, action, reward, done, (info.status & STATUS_WAS_RESET) == 0, first=(info.status & STATUS_WAS_RESET) != 0)
    assert ag.mem_cntr == 4 * N and ag.replay.head == 5
    q_eval, q_target = copy.deepcopy(ag.Q_eval), copy.deepcopy(ag.Q_target)
    before = [p.detach().clone() for p in ag.Q_eval.parameters()]
    loss = ag.learn()
    torch.cuda.synchronize()
    assert loss is not None and bool(torch.isfinite(loss)) and ag.updates == 1
    assert any(not torch.equal(p, q) for p, q in zip(ag.Q_eval.parameters(), before))
    s, s2, a, r, t, ok = ag._sampled
    assert bool(ok.all())  # no arena has finished an episode yet: every row of the ring is a transition
    with torch.no_grad():
        qe = q_eval(s).gather(1, a.long().view(-1, 1)).squeeze(1)
        qt = r + ag.gamma * q_target(s2).masked_fill(t.view(-1, 1), 0.0).max(dim=1)[0]
        want = F.mse_loss(qe, qt)
    print(f"loss {float(loss):.9g}, F.mse_loss on the sampled tensors {float(want):.9g}")
    assert torch.allclose(loss, want, rtol=1e-4, atol=0.0)
    ag.close()
    env.close()


def test_train_pixels_on_frames_and_the_default_call():
    from roborugby_amd import dqn
    res = dqn.train_pixels(replay="frames", num_envs=64, steps=24, batch_size=32, mem_size=1024, log_every=0)
    assert TRAIN_KEYS | NEW_KEYS == set(res)
    assert res["replay"] == "frames" and res["replay_bytes_per_transition"] == 12298 and res["replay_capacity"] == 1024 == res["replay_transitions"]
    assert res["learn_calls"] == 24 and res["loss"] is not None and np.isfinite(res["loss"]) and 0 < res["transitions"] <= 64 * 24
    base = dqn.train_pixels(num_envs=64, steps=6, stack=2, batch_size=32, mem_size=512, log_every=0)
    assert TRAIN_KEYS | NEW_KEYS == set(base)
    assert base["replay"] == "dense" and base["replay_bytes_per_transition"] == 2 * 6 * 4096 + 13 and base["replay_capacity"] == 512 == base["replay_transitions"]
    assert base["learn_calls"] == 6 and base["stack"] == 2 and base["transitions"] == 64 * 6 and np.isfinite(base["loss"])
    with pytest.raises(ValueError, match="replay"):
        dqn.train_pixels(num_envs=64, steps=1, replay="sparse")
