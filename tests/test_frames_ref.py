"""tests/frames_ref.py held to a naive model that keeps every pushed stack whole, per row, and rebuilds nothing (no GPU): the ring's
age / slot arithmetic against PixelObservation's stacking rule written out, and the window rule before, at and after the wrap."""
import numpy as np
import pytest

import frames_ref as fr


class Naive:
    """every observation of every push, whole: stacks[k][row] = [stack, frame_bytes]; nothing is ever overwritten"""

    def __init__(self, rows, stack):
        self.rows, self.stack, self.stacks, self.meta = rows, stack, [], []

    def push(self, frame, first, action, reward, done, valid):
        k = len(self.stacks)
        now = []
        for i in range(self.rows):
            if k == 0 or first is None or first[i]:
                now.append(np.stack([frame[i]] * self.stack))
            else:
                now.append(np.concatenate([self.stacks[-1][i][1:], frame[i][None]]))
        self.stacks.append(now)
        self.meta.append((action, reward, done, valid))

    def transition(self, k, row):
        action, reward, done, valid = self.meta[k]
        return self.stacks[k - 1][row], self.stacks[k][row], action[row], reward[row], bool(done[row]), bool(valid[row])


@pytest.mark.parametrize("stack", [1, 2, 4])
@pytest.mark.parametrize("extra", [1, 3])
def test_reference_rebuilds_what_a_naive_model_keeps(stack, extra):
    rows, fb, slots = 5, 16, stack + extra
    rng = np.random.default_rng(100 * stack + extra)
    ring, naive = fr.Ring(rows, slots, fb), Naive(rows, stack)
    for n, args in enumerate(fr.random_stream(rng, rows, fb, 3 * slots + 1)):
        first = None if n % 6 == 5 else args[1]
        fr.push(ring, args[0], first, *args[2:])
        naive.push(args[0], first, *args[2:])
        head = n + 1
        index = fr.every_index(head, rows)
        out = fr.sample(ring, stack, len(index), index=index)
        lo, hi = fr.window(head, slots, stack)
        for b, (k, row) in enumerate(index):
            inside = lo <= k <= hi and 0 <= row < rows
            if inside and naive.transition(k, row)[5]:
                s, s2, a, r, d, _ = naive.transition(k, row)
                assert out["ok"][b] == 1 and tuple(out["picked"][b]) == (k, row)
                assert np.array_equal(out["state"][b], s) and np.array_equal(out["next_state"][b], s2)
                assert out["action"][b] == a and out["reward"][b] == r and out["terminal"][b] == int(d)
            else:
                assert out["ok"][b] == 0 and tuple(out["picked"][b]) == (-1, -1)
                assert not out["state"][b].any() and not out["next_state"][b].any()
                assert out["action"][b] == 0 and out["reward"][b] == 0 and out["terminal"][b] == 0


def test_push_zero_is_all_first_and_carries_no_transition():
    ring = fr.Ring(3, 4, 16)
    frame = np.arange(48, dtype=np.uint8).reshape(3, 16)
    ones = np.ones(3, np.uint8)
    fr.push(ring, frame, np.zeros(3, np.uint8), np.full(3, 5, np.int32), np.ones(3, np.float32), ones, ones)
    assert not ring.age[0].any() and not ring.flags[0].any() and np.array_equal(ring.frames[0], frame)
    assert (ring.age[1:] == fr.POISON_U8).all() and (ring.frames[1:] == fr.POISON_U8).all()  # nothing outside the slot
    fr.push(ring, frame)  # a push that only records frames
    assert not ring.age[1].any() and not ring.flags[1].any() and not ring.action[1].any() and not ring.reward[1].any()


def test_age_saturates_at_255():
    ring = fr.Ring(1, 2, 16)
    frame, zero = np.zeros((1, 16), np.uint8), np.zeros(1, np.uint8)
    for _ in range(300):
        fr.push(ring, frame, zero)
    assert int(ring.age[299 % 2, 0]) == 255 and int(ring.age[298 % 2, 0]) == 255


@pytest.mark.parametrize("stack", [1, 4])
def test_window_before_at_and_after_the_wrap(stack):
    T = stack + 3
    assert fr.window(0, T, stack) == (1, -1) and fr.window(1, T, stack) == (1, 0)  # empty: one push is no transition
    assert fr.window(2, T, stack) == (1, 1)
    assert fr.window(T - 1, T, stack) == (max(1, stack - 1), T - 2)  # head < T: the same rule as after the wrap
    assert fr.window(T, T, stack) == (max(1, stack), T - 1)          # head == T: push 0 is still there, the state at stack - 1 reaches it
    assert fr.window(4 * T, T, stack) == (3 * T + stack, 4 * T - 1)  # three wraps: T - stack transitions
    # the oldest frame the oldest transition reads has not been overwritten, one older would have been
    for head in (T - 1, T, T + 1, 4 * T):
        lo, _ = fr.window(head, T, stack)
        assert lo - stack >= head - T or lo == 1
        assert lo - 1 - stack < max(head - T, 0) or lo == 1


def test_draw_takes_the_lowest_accepted_attempt_and_repeats():
    rng = np.random.default_rng(3)
    ring = fr.Ring(7, 6, 16)
    for args in fr.random_stream(rng, 7, 16, 9, p_valid=0.3):
        fr.push(ring, *args)
    a = fr.draw(ring, 2, 64, seed=5, call=1)
    assert a == fr.draw(ring, 2, 64, seed=5, call=1) and a != fr.draw(ring, 2, 64, seed=5, call=2)
    assert all(p is None or fr.sampleable(ring, 2, *p) for p in a) and any(p is not None for p in a)
    import dqn_ref
    lo, hi = fr.window(ring.head, ring.slots, 2)
    for b in range(64):  # the header's formula on the scalar Philox, attempt by attempt
        want = None
        for t in range(16):
            w = dqn_ref.philox4x32_10((b, 1, 0x5A3E, t), (5, 0))
            k, row = lo + ((w[0] * (ring.head - lo)) >> 32), (w[1] * 7) >> 32
            assert lo <= k <= hi and 0 <= row < 7
            if ring.flags[k % 6, row] & 1:
                want = (k, row)
                break
        assert a[b] == want
