"""Host-only reference of the frame-sharing pixel replay (include/roborugby_amd.h: rr_frames_push / rr_frames_sample): the header
comment's data layout and rules restated in numpy, none of the project's kernel code (the Philox is tests/dqn_ref.py's).
tests/test_frames_ref.py holds it to a naive model that stores every stack whole; tests/test_frames_emulated.py and
tests/test_gpu_frames.py hold the kernel source and the kernels to it, byte for byte."""
import numpy as np

import dqn_ref

DRAW_STREAM, ATTEMPTS = 0x5A3E, 16
POISON_U8, POISON_I32, POISON_F32 = 0xAB, -77, -12345.5
RING_FIELDS = ("frames", "age", "action", "reward", "flags")
OUT_FIELDS = ("state", "next_state", "action", "reward", "terminal", "ok", "picked")


class Ring:
    """the five arrays + head; every byte starts as poison, so what a push leaves alone shows"""

    def __init__(self, rows, slots, frame_bytes):
        self.rows, self.slots, self.frame_bytes, self.head = int(rows), int(slots), int(frame_bytes), 0
        self.frames = np.full((slots, rows, frame_bytes), POISON_U8, np.uint8)
        self.age = np.full((slots, rows), POISON_U8, np.uint8)
        self.action = np.full((slots, rows), POISON_I32, np.int32)
        self.reward = np.full((slots, rows), POISON_F32, np.float32)
        self.flags = np.full((slots, rows), POISON_U8, np.uint8)

    def arrays(self):
        return {f: getattr(self, f) for f in RING_FIELDS}


def push(ring, frame, first=None, action=None, reward=None, done=None, valid=None):
    """push number ring.head: frame [rows, frame_bytes] u8; first [rows] or None (all); the four metadata arrays [rows] or all None"""
    k, rows = ring.head, ring.rows
    s = k % ring.slots
    frame = np.asarray(frame, np.uint8).reshape(rows, ring.frame_bytes)
    group = [action, reward, done, valid]
    assert all(g is None for g in group) or all(g is not None for g in group)
    for i in range(rows):
        ring.frames[s, i] = frame[i]
        restarted = k == 0 or first is None or bool(first[i])
        ring.age[s, i] = 0 if restarted else min(int(ring.age[(k - 1) % ring.slots, i]) + 1, 255)
        ring.action[s, i] = 0 if action is None else action[i]
        ring.reward[s, i] = 0.0 if reward is None else reward[i]
        ring.flags[s, i] = 0 if (k == 0 or valid is None) else (1 if valid[i] else 0) | (2 if done[i] else 0)
    ring.head = k + 1


def window(head, slots, stack):
    """(lo, hi): the transitions lo <= k <= hi are whole in the ring (empty when hi < lo)"""
    return max(1, head - slots + stack), head - 1


def observation(ring, k, row, stack):
    """[stack, frame_bytes]: row `row` as seen at push k, oldest frame first"""
    age = int(ring.age[k % ring.slots, row])
    return np.stack([ring.frames[(k - min(stack - 1 - j, age)) % ring.slots, row] for j in range(stack)])


def sampleable(ring, stack, k, row):
    lo, hi = window(ring.head, ring.slots, stack)
    return lo <= k <= hi and 0 <= row < ring.rows and bool(ring.flags[k % ring.slots, row] & 1)


def draw(ring, stack, batch, seed, call):
    """the (k, row) of every sample in draw mode, or None: the first of the 16 attempts that lands on a real transition"""
    lo, hi = window(ring.head, ring.slots, stack)
    assert hi >= lo
    b = np.repeat(np.arange(batch, dtype=np.uint64), ATTEMPTS)
    a = np.tile(np.arange(ATTEMPTS, dtype=np.uint64), batch)
    w = dqn_ref.philox4x32_10_rows(b, int(call) & dqn_ref.MASK32, DRAW_STREAM, a, int(seed) & dqn_ref.MASK32, (int(seed) >> 32) & dqn_ref.MASK32)
    picks = []
    for i in range(batch):
        found = None
        for t in range(ATTEMPTS):
            k = lo + ((int(w[0][i * ATTEMPTS + t]) * (ring.head - lo)) >> 32)
            row = (int(w[1][i * ATTEMPTS + t]) * ring.rows) >> 32
            if sampleable(ring, stack, k, row):
                found = (k, row)
                break
        picks.append(found)
    return picks


def sample(ring, stack, batch, index=None, seed=0, call=0):
    """dict of OUT_FIELDS as rr_frames_sample fills rows 0 .. batch-1"""
    if index is None:
        picks = draw(ring, stack, batch, seed, call)
    else:
        picks = [(int(k), int(r)) if sampleable(ring, stack, int(k), int(r)) else None for k, r in np.asarray(index).reshape(batch, 2)]
    fb = ring.frame_bytes
    out = dict(state=np.zeros((batch, stack, fb), np.uint8), next_state=np.zeros((batch, stack, fb), np.uint8), action=np.zeros(batch, np.int32),
               reward=np.zeros(batch, np.float32), terminal=np.zeros(batch, np.uint8), ok=np.zeros(batch, np.uint8),
               picked=np.full((batch, 2), -1, np.int64))
    for b, p in enumerate(picks):
        if p is None:
            continue
        k, row = p
        s = k % ring.slots
        out["state"][b] = observation(ring, k - 1, row, stack)
        out["next_state"][b] = observation(ring, k, row, stack)
        out["action"][b], out["reward"][b] = ring.action[s, row], ring.reward[s, row]
        out["terminal"][b], out["ok"][b], out["picked"][b] = (int(ring.flags[s, row]) >> 1) & 1, 1, (k, row)
    return out


def poisoned_outputs(batch, stack, frame_bytes, pad=8):
    """output arrays of batch + pad rows, all poison: what a sampler under test writes into"""
    n = batch + pad
    return dict(state=np.full((n, stack, frame_bytes), POISON_U8, np.uint8), next_state=np.full((n, stack, frame_bytes), POISON_U8, np.uint8),
                action=np.full(n, POISON_I32, np.int32), reward=np.full(n, POISON_F32, np.float32), terminal=np.full(n, POISON_U8, np.uint8),
                ok=np.full(n, POISON_U8, np.uint8), picked=np.full((n, 2), POISON_I32, np.int64))


def assert_outputs(got, want, batch, label=""):
    """got: poisoned_outputs after the sampler ran (numpy); want: sample()'s dict.  Rows < batch equal bit for bit, the pad holds the poison"""
    fresh = poisoned_outputs(0, got["state"].shape[1], got["state"].shape[2], pad=got["ok"].shape[0] - batch)
    for f in OUT_FIELDS:
        g, w = np.asarray(got[f]), want[f]
        assert g[:batch].tobytes() == w.tobytes(), (label, f, np.argwhere(g[:batch] != w)[:4].tolist())
        assert g[batch:].tobytes() == fresh[f].tobytes(), (label, f, "a row at or beyond batch was written")


def every_index(head, rows):
    """every (k, row) with k in -1 .. head and row in -1 .. rows: the window, what lies around it and rows out of range"""
    return np.array([(k, r) for k in range(-1, head + 1) for r in range(-1, rows + 1)], np.int64)


def random_stream(rng, rows, frame_bytes, pushes, p_first=0.3, p_valid=0.7, p_done=0.2):
    """`pushes` argument tuples for push(): random frames, first with probability p_first, random valid / done, actions and rewards"""
    out = []
    for _ in range(pushes):
        out.append((rng.integers(0, 256, (rows, frame_bytes), dtype=np.uint8), (rng.random(rows) < p_first).astype(np.uint8),
                    rng.integers(0, 8, rows, dtype=np.int32), rng.standard_normal(rows).astype(np.float32),
                    (rng.random(rows) < p_done).astype(np.uint8), (rng.random(rows) < p_valid).astype(np.uint8)))
    return out
