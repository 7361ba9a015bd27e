"""A pixel replay that stores every frame once: a ring of `slots` time slots x `rows` rows (include/roborugby_amd.h: rr_frames_push /
rr_frames_sample; csrc/rr_frames.hpp).  A dense replay of stacked observations holds a 12 KB frame up to 2 * stack times per transition;
here a vector step adds ONE frame per row, and sampling rebuilds the two stacks of a transition from the at most stack + 1 distinct frames
behind them.  Rows are arenas -- or (arena, robot) pairs of a PixelObservation with several robots --, slots are vector steps, so storing
needs no compaction of the valid rows and nothing here synchronises with the host."""
import torch

from . import _lib
from ._lib import ptr


class FrameReplay:
    """The ring: five device tensors (frames u8 [slots, rows, frame_bytes]; age u8, action i32, reward f32, flags u8: each [slots, rows]),
    `head` = the pushes so far, and the counter that keys the sampler's draws.

    bytes_per_transition: frame_bytes + 10 (one frame, one age byte, action, reward, one flag byte) -- 12,298 for a 3 x 64 x 64 frame where
    the dense ring of PixelDQNAgent holds 2 * stack * 12,288 + 13.
    capacity: (slots - stack) * rows, the transitions the ring holds once it has wrapped: of its `slots` pushes the oldest `stack` only
    serve as the past of the ones after them.  Rows that were no transition (re-placements, flags bit 0 clear) take their place in the ring
    all the same and are skipped by the sampler.
    dqn: a _lib.DqnHandle to share (None: the replay opens, and closes, its own)."""

    def __init__(self, rows, slots, stack, frame_bytes=12288, device="cuda:0", seed=0, dqn=None):
        self.rows, self.slots, self.stack, self.frame_bytes = int(rows), int(slots), int(stack), int(frame_bytes)
        if self.rows < 1 or not 1 <= self.stack <= 8 or self.slots < self.stack + 1 or self.frame_bytes % 16 or self.frame_bytes < 16:
            raise ValueError("FrameReplay: rows >= 1, stack in 1..8, slots >= stack + 1, frame_bytes a multiple of 16")
        self.device = torch.device(device)
        self.seed, self.head, self.calls = int(seed), 0, 0
        self._own = dqn is None
        self._dqn = _lib.DqnHandle(self.device) if dqn is None else dqn
        T, N, d = self.slots, self.rows, self.device
        self.frames = torch.zeros((T, N, self.frame_bytes), dtype=torch.uint8, device=d)
        self.age = torch.zeros((T, N), dtype=torch.uint8, device=d)
        self.action = torch.zeros((T, N), dtype=torch.int32, device=d)
        self.reward = torch.zeros((T, N), dtype=torch.float32, device=d)
        self.flags = torch.zeros((T, N), dtype=torch.uint8, device=d)
        self._restart = True

    bytes_per_transition = property(lambda self: self.frame_bytes + 10)
    capacity = property(lambda self: (self.slots - self.stack) * self.rows)

    def window(self):
        """(lo, hi): the pushes whose transitions can be sampled now (empty while hi < lo)"""
        return max(1, self.head - self.slots + self.stack), self.head - 1

    def close(self):
        if self._own and self._dqn is not None:
            self._dqn.close()
        self._dqn = None

    def restart(self):
        """the next push starts every row's stack over, whatever its `first` says (PixelObservation.restart: the frames before it are of
        another state)"""
        self._restart = True

    def _row_bytes(self, t, name, dtype):
        if t is None:
            return None
        t = t.reshape(-1)
        if t.dtype != dtype:
            t = t.to(dtype)
        if t.shape[0] != self.rows or t.device != self.device:
            raise ValueError(f"FrameReplay.push({name}=...): {self.rows} values on {self.device}")
        return t.contiguous()

    @torch.no_grad()
    def push(self, pixels, first=None, action=None, reward=None, done=None, valid=None):
        """One vector step: the newest frame of every row + the row's transition from the push before.  pixels: a stacked observation
        [rows, 3 * stack', 64, 64] (any stack'; [N, R, ...] for several robots) -- its last three planes are read in place, through the row
        stride -- or a single frame [rows, frame_bytes] / [rows, 3, 64, 64]; uint8, contiguous.  first: bool [rows], rows whose stack
        starts over with this frame (None: all).  action, reward, done, valid [rows]: all None (a push that only records frames: after
        reset / restart) or all given; valid marks the rows whose step was a real transition."""
        if pixels.dtype != torch.uint8 or not pixels.is_contiguous() or pixels.device != self.device:
            raise ValueError("FrameReplay.push: contiguous uint8 pixels on the replay's device")
        if pixels.numel() % self.rows or (pixels.numel() // self.rows) % self.frame_bytes:
            raise ValueError(f"FrameReplay.push: {self.rows} rows of whole {self.frame_bytes}-byte frames, not {tuple(pixels.shape)}")
        stride = pixels.numel() // self.rows
        group = [action, reward, done, valid]
        if any(g is None for g in group) and not all(g is None for g in group):
            raise ValueError("FrameReplay.push: action, reward, done and valid are all None or all given")
        f = None if (first is None or self._restart) else self._row_bytes(first, "first", torch.bool)
        a, r = self._row_bytes(action, "action", torch.int32), self._row_bytes(reward, "reward", torch.float32)
        d, v = self._row_bytes(done, "done", torch.bool), self._row_bytes(valid, "valid", torch.bool)
        self._dqn.launch("rr_frames_push", ptr(pixels, stride - self.frame_bytes), stride, ptr(f), ptr(a), ptr(r), ptr(d), ptr(v),
                         self.rows, self.frame_bytes, self.slots, self.head, ptr(self.frames), ptr(self.age), ptr(self.action), ptr(self.reward),
                         ptr(self.flags))
        self._keep = (pixels, f, a, r, d, v)  # read asynchronously
        self.head += 1
        self._restart = False

    def _outputs(self, batch):
        d, fb = self.device, self.frame_bytes
        shape = (batch, 3 * self.stack, 64, 64) if fb == 12288 else (batch, self.stack, fb)
        return (torch.empty(shape, dtype=torch.uint8, device=d), torch.empty(shape, dtype=torch.uint8, device=d),
                torch.empty(batch, dtype=torch.int32, device=d), torch.empty(batch, dtype=torch.float32, device=d),
                torch.empty(batch, dtype=torch.bool, device=d), torch.empty(batch, dtype=torch.bool, device=d))

    @torch.no_grad()
    def sample(self, batch, index=None, out=None):
        """`batch` transitions: (state, next_state, action, reward, terminal, ok).  state / next_state: uint8 [batch, 3 * stack, 64, 64]
        ([batch, stack, frame_bytes] for another frame size), action int32, reward float32, terminal and ok bool.  index: int64
        [batch, 2] of (push, row) to fetch; None: uniform draws over the window, up to 16 per sample until one lands on a real transition
        (ok = False where none did, and wherever an index names none: that row is all zero).  out: the six tensors of an earlier call to
        write into.  The draws are a function of (seed, the number of sample calls so far)."""
        batch = int(batch)
        out = self._outputs(batch) if out is None else out
        s, s2, a, r, t, ok = out
        if index is not None:
            index = index.to(device=self.device, dtype=torch.int64).contiguous()
            if tuple(index.shape) != (batch, 2):
                raise ValueError("FrameReplay.sample(index=...): int64 [batch, 2] of (push, row)")
        self.calls += 1
        self._dqn.launch("rr_frames_sample", ptr(self.frames), ptr(self.age), ptr(self.action), ptr(self.reward), ptr(self.flags), self.rows,
                         self.frame_bytes, self.slots, self.head, self.stack, batch, ptr(index), self.seed & 0xFFFFFFFFFFFFFFFF,
                         self.calls & 0xFFFFFFFF, ptr(s), ptr(s2), ptr(a), ptr(r), ptr(t), ptr(ok), None)
        self._keep_index = index
        return out
