"""Pixel observations: every arena seen from one or several of its robots (BatchedRoboRugbyEnv.render_ego: centred on the robot, its front
up, colours from its own side), rendered on the device after every step, with frame stacking.  The observation a convolutional policy that
drives ONE robot can look at; the 11-float lidar observation stays available next to it."""
import numbers

import numpy as np
import torch

from .env import STATUS_NOT_READY, STATUS_WAS_RESET
from .spaces import Box


class PixelObservation:
    """Wraps a BatchedRoboRugbyEnv: reset / step / step_thrust return pixels instead of the lidar observation.

    robots: the viewing robot (happy robots first) -- an int: pixels [N, 3*stack, size, size]; a sequence of R robots: pixels
    [N, R, 3*stack, size, size].  size, span, ahead, samples, relative: the frames (render_ego), planar, `size` x `size`.
    stack: the last `stack` frames of a row, the oldest first.  A row that was reset -- reset(), a masked reset, a step whose status has
    WAS_RESET -- has every slot equal to its first frame; a row whose status has NOT_READY (budgeted step: the arena is parked mid-step)
    keeps its stack; every other row drops its oldest frame and appends the frame of the new state.
    Before the first reset the stack holds the picture of the state the wrapper found.  The pixels live in ONE persistent device buffer that the next call overwrites (clone what has to last); nothing synchronises with
    the host.  step / step_thrust return (pixels, reward, done, info) with the env's own observation as info.lidar."""

    def __init__(self, env, robots=0, size=64, span=400.0, ahead=0.0, samples=1, relative=True, stack=1):
        self.env = env
        self.single = isinstance(robots, numbers.Integral)
        rob = [int(robots)] if self.single else [int(r) for r in robots]
        if not rob or any(r < 0 or r >= env.preset.nr for r in rob):
            raise ValueError(f"PixelObservation(robots=...): robot indices in 0 .. {env.preset.nr - 1}")
        if int(stack) < 1:
            raise ValueError("PixelObservation(stack=...): at least one frame")
        self.robots, self.size, self.stack = tuple(rob), int(size), int(stack)
        self.span, self.ahead, self.samples, self.relative = float(span), float(ahead), int(samples), bool(relative)
        N, R, dev = env.num_envs, len(rob), env.device
        self._arenas = torch.arange(N, dtype=torch.int32, device=dev).repeat_interleave(R)
        self._robots = torch.tensor(rob, dtype=torch.int32, device=dev).repeat(N)
        self._frame = torch.zeros((N, R, 1, 3, self.size, self.size), dtype=torch.uint8, device=dev)
        self._buf = torch.zeros((N, R, self.stack, 3, self.size, self.size), dtype=torch.uint8, device=dev)
        self.observation_space = Box(0, 255, (3 * self.stack, self.size, self.size), np.uint8)
        self.num_envs, self.device = N, dev
        self._update(None, None)  # the stack starts as the picture of the state it finds (and a bad size / span / samples is refused here)

    def _render(self):
        self.env.render_ego(self._arenas, self._robots, self.size, self.size, self.span, self.ahead, self.samples, self.relative, True,
                            out=self._frame)
        return self._frame

    def _pixels(self):
        N, R = self.num_envs, len(self.robots)
        return self._buf.view(N, 3 * self.stack, self.size, self.size) if self.single else self._buf.view(N, R, 3 * self.stack, self.size, self.size)

    def _update(self, first, keep):
        """first / keep: bool [N] or None -- rows whose stack restarts with the new frame / rows whose stack stays as it is"""
        new = self._render()
        if first is None:
            self._buf.copy_(new.expand_as(self._buf))
            return self._pixels()
        nxt = torch.cat([self._buf[:, :, 1:], new], dim=2)
        nxt = torch.where(first.view(-1, 1, 1, 1, 1, 1), new, nxt)
        if keep is not None:
            nxt = torch.where(keep.view(-1, 1, 1, 1, 1, 1), self._buf, nxt)
        self._buf.copy_(nxt)
        return self._pixels()

    def restart(self):
        """every stack starts over from the state the env is in now (after load_checkpoint_state / set_state: the frames are not part of it)"""
        return self._update(None, None)

    def reset(self, mask=None):
        self.lidar = self.env.reset(mask)
        if mask is None:
            return self._update(None, None)
        m = torch.as_tensor(mask).to(device=self.device).view(-1) != 0
        return self._update(m, ~m)

    def _stepped(self, res):
        obs, reward, done, info = res
        info.lidar = obs
        first = (info.status & STATUS_WAS_RESET) != 0
        keep = (info.status & STATUS_NOT_READY) != 0
        return self._update(first & ~keep, keep), reward, done, info

    def step(self, actions):
        return self._stepped(self.env.step(actions))

    def step_thrust(self, thrust):
        return self._stepped(self.env.step_thrust(thrust))
