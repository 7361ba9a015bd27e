"""ctypes binding of the host-emulated hive-mind kernel (tests/emu/rr_hive_emu.cpp) -- test harness only -- and the numpy
restatement of the greedy assignment rule the CPU and GPU tests compare with."""
import ctypes as C

import numpy as np

import emu_build as eb
import oracle_lib as ol

# lanes per arena the tests run the emulation at (rows of EMU_HIVE_TABLE, tests/emu/emu_common.hpp): the product's width of the shape
# (csrc/rr_kstep.hpp; X, W, R: build.shape_lanes), wider groups and 64
LANES = {"T": (2, 4, 64), "G": (8, 16, 32, 64), "D": (4, 64), "X": (8, 64), "W": (16, 64), "R": (8, 64)}
LANES.update({wide: LANES[shape] for wide, shape in ol.SHAPE.items()})  # the non-square ids run their shape's build at their own W, H


def build():
    return eb.build(eb.LIBS["hive"])


def lib():
    L = eb.load(eb.LIBS["hive"])
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.hive_emu.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, dp, dp, C.c_uint32, C.c_int, ip, dp]
    return L


def hive_observe(preset, robots, balls, mask, kind, vw, f32=False):
    """robots [n,NR,10], balls [n,NB,8] (canonical layout) -> (assign int32 [n,NR], obs float64 [n,NR,11]) of the kernel source"""
    cfg = ol.PRESETS[preset]
    r, b = eb.canonical(preset, robots, balls)
    n, nr = r.shape[:2]
    assign = np.full((n, nr), -7, np.int32)
    obs = np.full((n, nr, 11), np.nan)
    rc = lib().hive_emu(eb.PRESET_ID[preset], int(vw), int(f32), cfg["W"], cfg["H"], n, eb.ptr(r, C.c_double), eb.ptr(b, C.c_double), int(mask),
                        int(kind), eb.ptr(assign, C.c_int32), eb.ptr(obs, C.c_double))
    assert rc == 0, (preset, vw, f32)
    return assign, obs


def in_goal(x, y, W, H):
    """centre inside the happy or the grumpy goal triangle: RightTriangle.contains_point as the reference evaluates it -- bounding box,
    then slope from the hypotenuse's origin >= the hypotenuse's slope, with x / 0 = +-inf by the sign of x"""
    def slope(dy, dx):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(dx != 0, dy / np.where(dx != 0, dx, 1.0), np.where(dy > 0, np.inf, np.where(dy < 0, -np.inf, 0.0)))
    happy = (W - 240 <= x) & (x <= W) & (H - 240 <= y) & (y <= H) & (slope(y - H, x - (W - 240)) >= slope(-240.0, 240.0))
    grumpy = (0 <= x) & (x <= 240) & (0 <= y) & (y <= 240) & (slope(y - 0.0, x - 240.0) >= slope(240.0, -240.0))
    return happy | grumpy


def tie_bound(dtype):
    """relative distance gap below which the order of two pairs is not the reference's to decide: 1e-9, or four epsilon of the arithmetic
    the distances are compared in where that is coarser (fp32)"""
    return max(1e-9, 4 * float(np.finfo(dtype).eps))


def greedy_assign(rxy, bxy, mask, W, H, dtype=np.float64):
    """The rule of include/roborugby_amd.h (rr_hive_observe) for ONE arena: rxy [NR,2], bxy [NB,2] -> (assign [NR], near_tie).
    near_tie: two candidate pairs' distances differ by less than tie_bound relative (the tie order is ours, not the reference's)."""
    rxy, bxy = np.asarray(rxy, dtype), np.asarray(bxy, dtype)
    nr, nb = len(rxy), len(bxy)
    cand = ~in_goal(bxy[:, 0], bxy[:, 1], dtype(W), dtype(H)) & (bxy[:, 0] > -900)
    pairs = [(np.sqrt((bxy[b, 0] - rxy[r, 0]) ** 2 + (bxy[b, 1] - rxy[r, 1]) ** 2), b, r)
             for b in range(nb) if cand[b] for r in range(nr) if (mask >> r) & 1]
    pairs.sort(key=lambda t: t[0])  # stable: ball index, then robot index among equal distances
    d = np.array([float(t[0]) for t in pairs])
    near = bool(len(d) > 1 and np.any(np.diff(d) < tie_bound(dtype) * np.maximum(d[1:], 1e-300)))
    assign = np.full(nr, -1, np.int32)
    taken = set()
    for _, b, r in pairs:
        if b not in taken and assign[r] < 0:
            taken.add(b)
            assign[r] = b
    return assign, near


def greedy_assign_batch(rxy, bxy, mask, W, H, dtype=np.float64):
    """greedy_assign for [n] arenas at once: rxy [n,NR,2], bxy [n,NB,2] -> (assign [n,NR], near_tie [n]).  Walking the stably sorted
    list is taking, min(NR, NB) times, the closest pair whose robot and ball are still free -- the first one in (ball, robot)
    order among equals, which is what argmin over the ball-major pair axis returns."""
    rxy, bxy = np.asarray(rxy, dtype), np.asarray(bxy, dtype)
    n, nr, nb = rxy.shape[0], rxy.shape[1], bxy.shape[1]
    cand = ~in_goal(bxy[:, :, 0], bxy[:, :, 1], dtype(W), dtype(H)) & (bxy[:, :, 0] > -900)
    d = np.sqrt((bxy[:, :, None, 0] - rxy[:, None, :, 0]) ** 2 + (bxy[:, :, None, 1] - rxy[:, None, :, 1]) ** 2).astype(np.float64)
    hive = ((mask >> np.arange(nr)) & 1).astype(bool)
    d = np.where(cand[:, :, None] & hive[None, None, :], d, np.inf)          # [n, NB, NR]: ball-major
    flat = np.sort(d.reshape(n, -1), axis=1)
    with np.errstate(invalid="ignore"):
        gap = np.diff(flat, axis=1) < tie_bound(dtype) * np.maximum(flat[:, 1:], 1e-300)
    near = np.any(gap & np.isfinite(flat[:, 1:]), axis=1)
    assign = np.full((n, nr), -1, np.int32)
    rows = np.arange(n)
    for _ in range(min(nr, nb)):
        p = np.argmin(d.reshape(n, -1), axis=1)
        b, r = p // nr, p % nr
        ok = np.isfinite(d[rows, b, r])
        assign[rows[ok], r[ok]] = b[ok]
        d[rows[ok], b[ok], :] = np.inf
        d[rows[ok], :, r[ok]] = np.inf
    return assign, near


def random_layouts(rng, n, nr, nb, W, H):
    """robots / balls in canonical layout (centres only matter): uniform over the arena, a third of the balls thrown into the goal
    corners, and every 16th layout degenerate -- all balls in goals, or all but one"""
    robots = np.zeros((n, nr, 10))
    balls = np.zeros((n, nb, 8))
    robots[:, :, 0] = rng.uniform(30, W - 30, (n, nr))
    robots[:, :, 1] = rng.uniform(30, H - 30, (n, nr))
    robots[:, :, 6] = rng.uniform(0, 360, (n, nr))
    balls[:, :, 0] = rng.uniform(8, W - 8, (n, nb))
    balls[:, :, 1] = rng.uniform(8, H - 8, (n, nb))
    corner = rng.random((n, nb)) < 1 / 3
    corner[::16] = True
    keep_one = np.arange(n) % 32 == 16
    corner[keep_one, rng.integers(0, nb, keep_one.sum())] = False
    u, v = rng.uniform(0, 110, (n, nb)), rng.uniform(0, 110, (n, nb))  # u + v < 240: inside a triangle with legs of 240
    far = rng.random((n, nb)) < .5
    balls[:, :, 0] = np.where(corner, np.where(far, W - 5 - u, 5 + u), balls[:, :, 0])
    balls[:, :, 1] = np.where(corner, np.where(far, H - 5 - v, 5 + v), balls[:, :, 1])
    return robots, balls
