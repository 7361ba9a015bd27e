"""ctypes binding of the host-emulated hive transition kernel (tests/emu/rr_hive_transition_emu.cpp) -- test harness only -- and the
numpy restatement of the per-robot reward and of the validity rules (include/roborugby_amd.h: rr_hive_transition) the CPU and GPU
tests compare with."""
import ctypes as C
import math

import numpy as np

import emu_build as eb
import oracle_lib as ol

WAS_RESET, NOT_READY, STEP_AFTER_DONE = 1024, 16384, 64
NOT_STEPPED = WAS_RESET | NOT_READY | STEP_AFTER_DONE
counts = eb.counts


def build():
    return eb.build(eb.LIBS["hive_transition"])  # (its own library for its -fno-builtin: emu_build.LIBS says why)


def lib():
    L = eb.load(eb.LIBS["hive_transition"])
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    L.hive_transition_emu.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, dp, dp, dp, dp, C.c_uint32, C.c_int,
                                      ip, ip, bp, dp, dp, bp, bp]
    return L


def hive_transition(preset, robots0, balls0, robots1, balls1, mask, kind, assign, status, done, vw, f32=False):
    """The kernel source on n transitions.  robots0 / balls0 [n,NR,10] / [n,NB,8]: the state before the step (its extras_begin copies are
    the snapshot); robots1 / balls1: the state after it (the record); assign [n,NR], status [n], done [n]
    -> (next_obs float64 [n,NR,11], reward float64 [n,NR], terminal uint8 [n,NR], valid uint8 [n,NR]); the outputs start as
    NaN / 255, so an element the kernel source does not write shows."""
    cfg = ol.PRESETS[preset]
    r0, b0 = eb.canonical(preset, robots0, balls0)
    n, nr = r0.shape[:2]
    r1, b1 = eb.canonical(preset, robots1, balls1)
    assert r1.shape[0] == n
    a = np.ascontiguousarray(assign, np.int32).reshape(n, nr)
    st = np.ascontiguousarray(status, np.int32).reshape(n)
    dn = np.ascontiguousarray(done, np.uint8).reshape(n)
    obs = np.full((n, nr, 11), np.nan)
    rew = np.full((n, nr), np.nan)
    term = np.full((n, nr), 255, np.uint8)
    val = np.full((n, nr), 255, np.uint8)
    d, i, u8 = C.c_double, C.c_int32, C.c_uint8
    rc = lib().hive_transition_emu(eb.PRESET_ID[preset], int(vw), int(f32), cfg["W"], cfg["H"], n, eb.ptr(r0, d), eb.ptr(b0, d), eb.ptr(r1, d),
                                   eb.ptr(b1, d), int(mask), int(kind), eb.ptr(a, i), eb.ptr(st, i), eb.ptr(dn, u8), eb.ptr(obs, d), eb.ptr(rew, d),
                                   eb.ptr(term, u8), eb.ptr(val, u8))
    assert rc == 0, (preset, vw, f32)
    return obs, rew, term, val


_pow = np.frompyfunc(math.pow, 2, 1)  # libm's pow element by element, as CPython's `**` on floats (numpy's own power takes other routes)


def _dist(ax, ay, bx, by):
    """MyUtils.distance (MyUtils.py:40-41): ((bx - ax) ** 2 + (by - ay) ** 2) ** .5"""
    dx, dy = np.asarray(bx - ax, np.float64), np.asarray(by - ay, np.float64)
    return _pow(_pow(dx, 2.0).astype(np.float64) + _pow(dy, 2.0).astype(np.float64), .5).astype(np.float64)


def restate(preset, rxy0, bxy0, rxy1, bxy1, mask, assign, status, done, W=None, H=None):
    """The definition, in numpy, in fp64 and in the header's order.  rxy0 [n,NR,2] / bxy0 [n,NB,2]: centres before the
    step (the snapshot holds FloatRect.copy()'s arithmetic of them: 10 + (x - 10), 20 + (y - 20) for a robot, 7 + (x - 7) for a ball);
    rxy1 / bxy1: centres after it.  -> (reward float64 [n,NR], terminal uint8 [n,NR], valid bool [n,NR])"""
    cfg = ol.PRESETS[preset]
    nrh, nr, nbp, nb = counts(preset)
    W, H = cfg["W"] if W is None else W, cfg["H"] if H is None else H
    t = np.float64
    mb = 200000.0 / math.pow(W * W + H * H, .5)
    mult_ball, mult_robot = t(mb), t(mb / 100)
    rxy0, bxy0, rxy1, bxy1 = (np.asarray(x, np.float64).astype(t) for x in (rxy0, bxy0, rxy1, bxy1))
    assign, status, done = np.asarray(assign, np.int64), np.asarray(status, np.int64), np.asarray(done).astype(np.uint8)
    n = rxy0.shape[0]
    in_mask = ((int(mask) >> np.arange(nr)) & 1).astype(bool)[None, :]
    ranged = (assign >= 0) & (assign < nb)
    b = np.where(ranged, assign, 0)
    rows = np.arange(n)[:, None]
    in_play = bxy1[rows, b, 0] > t(-900)
    valid = in_mask & ranged & ((status & NOT_STEPPED) == 0)[:, None] & in_play
    prx, pry = t(10) + (rxy0[:, :, 0] - t(10)), t(20) + (rxy0[:, :, 1] - t(20))
    pbx, pby = t(7) + (bxy0[rows, b, 0] - t(7)), t(7) + (bxy0[rows, b, 1] - t(7))
    bx, by = bxy1[rows, b, 0], bxy1[rows, b, 1]
    naughty = ((status[:, None] >> (16 + np.arange(nr))[None, :]) & 1).astype(bool)
    rew = np.zeros((n, nr), t)
    rew = np.where(naughty, rew - t(.005), rew)
    rew = rew + (_dist(prx, pry, bx, by) - _dist(rxy1[:, :, 0], rxy1[:, :, 1], bx, by)) * mult_robot
    zero = np.zeros_like(bx)
    push = (_dist(zero, zero, bx, by) - _dist(zero, zero, pbx, pby)) * mult_ball
    flip = (np.arange(nr) < nrh)[None, :] != (b < nbp)
    rew = np.where(flip, rew - push, rew + push)
    assert rew.dtype == t
    rew = np.where(valid, rew, t(0)).astype(np.float64)
    return rew, np.where(valid, done[:, None], 0).astype(np.uint8), valid


def fp32_bound(W, H):
    """|fp32 reward - fp64 reward| <= 16 * 2^-24 * diag * mult_ball: each term is a difference of two distances <= diag rounded to fp32"""
    diag = float(np.sqrt(W * W + H * H))
    return 16 * 2.0 ** -24 * diag * (200000.0 / diag)
