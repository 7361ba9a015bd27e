"""An independent numpy fp64 restatement of the picture rr_render_ego specifies (include/roborugby_amd.h), for the CPU and GPU tests.

Unlike tests/render_ref.py, which evaluates the shapes at the fp32 sample coordinates, this one computes the SAMPLE POINTS in fp64 as well,
from the fp64 pose: it does not imitate the kernel's fp32 path (camera trig, view constants, rotation).  The shapes are evaluated as
render_ref.frame does; on top comes the OUTSIDE layer, and the relative palette for a grumpy viewer.  The boundary-distance map holds, for
every pixel, the smallest distance (arena units) of any of its samples to any layer boundary -- render_ref's, plus the four wall lines.

The rule is render_ref.check's: a frame is exact outside a band of TOL = 1e-3 around the layer boundaries; exempt pixels must be palette
colours (S = 1) or lie within the palette's channel-wise range (S > 1); at most CAP = 0.2 % of a frame's pixels may be exempt.

Why the tolerance holds: an fp32 numpy restatement of the specified arithmetic, on the recorded states of G, Dwide, T and X at span <= 512,
puts a sample at most 2.3e-4 from the fp64 point; device cosf / sinf add about one ulp times a lever arm of <= 420 units, roughly 5e-5, and
FMA contraction is of the same order.  Why the cap is safe: on every robot of every state of render_ref.golden_states for G, Dwide, T and X,
at (width, height, S, span, ahead) = (64, 64, 1, 400, 0), (64, 48, 1, 400, 100), (32, 32, 2, 400, 100) and (96, 96, 1, 500, 60), the worst
exempt share of this reference alone is 0.098 % -- one pixel of a 32 x 32 frame.  Frames under 512 pixels are not held to the cap (one pixel
of 256 is already 0.39 %); and a span and width that put sample offsets on integers (span 256 at 16 px with S = 4) are to be avoided: the
viewing robot's own edges are axis-aligned in its view."""
import numpy as np

import render_ref as ref

TOL, CAP = ref.TOL, ref.CAP
OUTSIDE = (96, 96, 96)
PALETTE = np.concatenate([ref.PALETTE, np.array([OUTSIDE], np.int64)])
CONFIGS = [(64, 64, 1, 400.0, 0.0), (64, 48, 1, 400.0, 100.0), (32, 32, 2, 400.0, 100.0), (96, 96, 1, 500.0, 60.0)]  # width, height, S, span, ahead


def swap_palette(rgb):
    """the three colour pairs exchanged -- team, ball, goal -- in an S = 1 frame [.., 3]: what a grumpy viewer's relative frame must be"""
    a = np.asarray(rgb)
    out = a.copy()
    for x, y in ((ref.TEAM_HAPPY, ref.TEAM_GRUMPY), (ref.BALL_POS, ref.BALL_NEG), (ref.GOAL_HAPPY, ref.GOAL_GRUMPY)):
        out[(a == x).all(axis=-1)] = y
        out[(a == y).all(axis=-1)] = x
    return out


def sample_points(cx, cy, rot, width, height, S, span, ahead):
    """the arena coordinates (X, Y) [height*S, width*S] of every sample, all in fp64"""
    th = np.radians(360.0 - rot)
    c, s = np.cos(th), np.sin(th)
    f = span / (width * S)
    p = (np.arange(width * S) + 0.5) * f - span * 0.5
    q = (np.arange(height * S) + 0.5) * f - span * 0.5 * height / width
    P, Q = np.meshgrid(p, q)
    fwd = ahead - Q
    return cx + (fwd * c - P * s), cy + (fwd * s + P * c)


def frame(W, H, nr_happy, nb_pos, robots, balls, viewer, width, height, S=1, span=400.0, ahead=0.0, relative=False):
    """robots [NR,>=7] (x, y, ..., rot at 6), balls [NB,>=2] of ONE arena, seen from robot `viewer` ->
    (rgb uint8 [height,width,3], dist float64 [height,width]); an all-zero frame (dist +inf) for a viewer with a non-finite pose"""
    robots, balls = np.asarray(robots, np.float64), np.asarray(balls, np.float64)
    vx, vy, vrot = robots[viewer, 0], robots[viewer, 1], robots[viewer, 6]
    if not (np.isfinite(vx) and np.isfinite(vy) and np.isfinite(vrot)):
        return np.zeros((height, width, 3), np.uint8), np.full((height, width), np.inf)
    swap = bool(relative) and viewer >= nr_happy
    goal_g, goal_h = (ref.GOAL_HAPPY, ref.GOAL_GRUMPY) if swap else (ref.GOAL_GRUMPY, ref.GOAL_HAPPY)
    team = (ref.TEAM_GRUMPY, ref.TEAM_HAPPY) if swap else (ref.TEAM_HAPPY, ref.TEAM_GRUMPY)  # (of the happy robots, of the grumpy ones)
    ball = (ref.BALL_NEG, ref.BALL_POS) if swap else (ref.BALL_POS, ref.BALL_NEG)
    X, Y = sample_points(vx, vy, vrot, width, height, S, span, ahead)
    col = np.empty(X.shape + (3,), np.int64)
    col[:] = ref.BACKGROUND
    dist = np.minimum(np.abs(X + Y - 240.0), np.abs((W - X) + (H - Y) - 240.0)) / np.sqrt(2.0)
    col[X + Y <= 240.0] = goal_g
    col[(W - X) + (H - Y) <= 240.0] = goal_h
    for r, row in enumerate(robots):
        cx, cy, rot = row[0], row[1], row[6]
        if not (np.isfinite(cx) and np.isfinite(cy) and np.isfinite(rot)):
            continue
        th = np.radians(360.0 - rot)
        c, s = np.cos(th), np.sin(th)
        dx, dy = X - cx, Y - cy
        u, v = dx * c + dy * s, -dx * s + dy * c
        au, av = np.abs(u), np.abs(v)
        inside = (au <= 10.0) & (av <= 20.0)
        edge = inside & ((au > 9.0) | (av > 19.0))
        front = inside & ~edge & (u > 7.0)
        col[inside] = team[0] if r < nr_happy else team[1]
        col[front] = ref.FRONT
        col[edge] = ref.BLACK
        d = np.minimum(ref._rect_boundary(au, av, 10.0, 20.0), ref._rect_boundary(au, av, 9.0, 19.0))
        d = np.minimum(d, np.hypot(u - 7.0, np.maximum(av - 19.0, 0.0)))  # the front line: u = 7, |v| <= 19
        dist = np.minimum(dist, d)
    for b, row in enumerate(balls):
        cx, cy = row[0], row[1]
        if not (np.isfinite(cx) and np.isfinite(cy)):
            continue
        rad = np.hypot(X - cx, Y - cy)
        inside = rad <= 7.0
        col[inside] = ball[0] if b < nb_pos else ball[1]
        col[inside & (rad > 6.0)] = ref.BLACK
        dist = np.minimum(dist, np.minimum(np.abs(rad - 7.0), np.abs(rad - 6.0)))
    col[(X < 0.0) | (X > W) | (Y < 0.0) | (Y > H)] = OUTSIDE
    dist = np.minimum(dist, np.minimum(np.minimum(np.abs(X), np.abs(X - W)), np.minimum(np.abs(Y), np.abs(Y - H))))  # the four wall lines
    if S > 1:
        col = (col.reshape(height, S, width, S, 3).sum(axis=(1, 3)) + (S * S) // 2) // (S * S)
        dist = dist.reshape(height, S, width, S).min(axis=(1, 3))
    return col.astype(np.uint8), dist


def check(got, want, dist, S=1, what=""):
    """render_ref.check's rule for ONE frame [h, w, 3], with OUTSIDE in the palette; returns the exempt share (asserted <= CAP for frames
    of at least 512 pixels)"""
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    exempt = dist < TOL
    share = float(exempt.mean())
    bad = (got != want).any(axis=-1) & ~exempt
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5].tolist(), want[bad][:5].tolist())
    e = got[exempt].astype(np.int64)
    if S == 1:
        assert (e[:, None, :] == PALETTE[None]).all(axis=-1).any(axis=-1).all(), (what, "an exempt pixel is no palette colour")
    else:
        assert ((e >= PALETTE.min(axis=0)) & (e <= PALETTE.max(axis=0))).all(), (what, "an exempt pixel is outside the palette's range")
    if exempt.size >= 512:
        assert share <= CAP, (what, f"{100 * share:.3f} % of the pixels are exempt: above the cap")
    return share
