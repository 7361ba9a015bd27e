"""ctypes binding of the host-emulated hive transition kernel (tests/emu/rr_hive_transition_emu.cpp) -- test harness only -- and the
numpy restatement of the per-robot reward and of the validity rules (include/roborugby_amd.h: rr_hive_transition) the CPU and GPU
tests compare with."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import hive_emu_lib as he
import oracle_lib as ol

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "emu", "librr_hive_transition_emu.so")
SRC = [os.path.join(HERE, "emu", "rr_hive_transition_emu.cpp")] + he.SRC[1:]
WAS_RESET, NOT_READY, STEP_AFTER_DONE = 1024, 16384, 64
NOT_STEPPED = WAS_RESET | NOT_READY | STEP_AFTER_DONE


def build():
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(s) for s in SRC):
        tmp = SO + f".tmp{os.getpid()}"
        # hive_emu_lib's flags + -fno-builtin: the rewards' distances are the reference's pow(x, 2.0) / pow(x, .5) and must stay the libm
        # calls CPython makes (g++ would fold the former to x * x), as oracle/Makefile keeps them for the oracle
        subprocess.check_call(["g++", "-O2", "-fPIC", "-ffp-contract=off", "-fno-builtin", "-std=c++17", "-shared", "-o", tmp, SRC[0]])
        os.replace(tmp, SO)
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        _lib.hive_transition_emu.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, dp, dp, dp, dp, C.c_uint32, C.c_int,
                                             ip, ip, bp, dp, dp, bp, bp]
    return _lib


def counts(preset):
    cfg = ol.PRESETS[preset]
    return cfg["nr_h"], cfg["nr_h"] + cfg["nr_g"], cfg["nb_p"], cfg["nb_p"] + cfg["nb_n"]


def hive_transition(preset, robots0, balls0, robots1, balls1, mask, kind, assign, status, done, vw, f32=False):
    """The kernel source on n transitions.  robots0 / balls0 [n,NR,10] / [n,NB,8]: the state before the step (its extras_begin copies are
    the snapshot); robots1 / balls1: the state after it (the record); assign [n,NR], status [n], done [n]
    -> (next_obs float64 [n,NR,11], reward float64 [n,NR], terminal uint8 [n,NR], valid uint8 [n,NR]); the outputs start as
    NaN / 255, so an element the kernel source does not write shows."""
    cfg = ol.PRESETS[preset]
    _, nr, _, nb = counts(preset)
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    r0 = np.ascontiguousarray(robots0, np.float64).reshape(-1, nr, 10)
    n = r0.shape[0]
    b0 = np.ascontiguousarray(balls0, np.float64).reshape(n, nb, 8)
    r1 = np.ascontiguousarray(robots1, np.float64).reshape(n, nr, 10)
    b1 = np.ascontiguousarray(balls1, np.float64).reshape(n, nb, 8)
    a = np.ascontiguousarray(assign, np.int32).reshape(n, nr)
    st = np.ascontiguousarray(status, np.int32).reshape(n)
    dn = np.ascontiguousarray(done, np.uint8).reshape(n)
    obs = np.full((n, nr, 11), np.nan)
    rew = np.full((n, nr), np.nan)
    term = np.full((n, nr), 255, np.uint8)
    val = np.full((n, nr), 255, np.uint8)
    rc = lib().hive_transition_emu(he.PRESET_ID[preset], int(vw), int(f32), cfg["W"], cfg["H"], n, r0.ctypes.data_as(dp), b0.ctypes.data_as(dp),
                                   r1.ctypes.data_as(dp), b1.ctypes.data_as(dp), int(mask), int(kind), a.ctypes.data_as(ip),
                                   st.ctypes.data_as(ip), dn.ctypes.data_as(bp), obs.ctypes.data_as(dp), rew.ctypes.data_as(dp),
                                   term.ctypes.data_as(bp), val.ctypes.data_as(bp))
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
