"""ctypes binding of the host-emulated frame kernel (tests/emu/rr_render_emu.cpp: g++ build of csrc/rr_render.hpp) -- test harness only."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as ol

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "emu", "librr_render_emu.so")
CSRC = os.path.join(ol.REPO, "roborugby_amd", "csrc")
SRC = [os.path.join(HERE, "emu", "rr_render_emu.cpp")] + [os.path.join(CSRC, f) for f in ("rr_render.hpp", "rr_sim.hpp")]
FLAGS = ["-O2", "-ffp-contract=off", "-std=c++17"]


def build():
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(s) for s in SRC):
        tmp = SO + f".tmp{os.getpid()}"
        subprocess.check_call(["g++"] + FLAGS + ["-fPIC", "-shared", "-o", tmp, SRC[0]])
        os.replace(tmp, SO)
    return SO


def build_program(path, extra=()):
    """the same source as a stand-alone program with its own main (crafted arenas at 4x1 and 96x96, S = 1 and 4), e.g. with
    extra=("-fsanitize=address,undefined", "-g")"""
    subprocess.check_call(["g++"] + FLAGS + list(extra) + ["-DRR_RENDER_EMU_MAIN", "-o", path, SRC[0]])
    return path


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        _lib.render_emu.argtypes = [C.c_int] * 5 + [C.c_double, C.c_double, C.c_int, dp, dp, ip, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.POINTER(C.c_uint8)]
    return _lib


def render(preset, robots, balls, width, height, samples=1, arenas=None, f32=False):
    """robots [n,NR,10], balls [n,NB,8] (canonical layout) -> uint8 [m,height,width,3] of the kernel source; f32: fp32 records"""
    cfg = ol.PRESETS[preset]
    nr, nb = cfg["nr_h"] + cfg["nr_g"], cfg["nb_p"] + cfg["nb_n"]
    r = np.ascontiguousarray(robots, np.float64).reshape(-1, nr, 10)
    b = np.ascontiguousarray(balls, np.float64).reshape(-1, nb, 8)
    n = r.shape[0]
    assert b.shape[0] == n
    idx = None if arenas is None else np.ascontiguousarray(arenas, np.int32)
    m = n if idx is None else len(idx)
    rgb = np.full((m, height, width, 3), 0xAB, np.uint8)
    rc = lib().render_emu(int(f32), nr, cfg["nr_h"], nb, cfg["nb_p"], cfg["W"], cfg["H"], n, r.ctypes.data_as(C.POINTER(C.c_double)),
                          b.ctypes.data_as(C.POINTER(C.c_double)), None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_int32)), m,
                          int(width), int(height), int(samples), rgb.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rc == 0, (preset, width, height, samples)
    return rgb
