"""ctypes binding of the host-emulated frame kernel (tests/emu/rr_render_emu.cpp: g++ build of csrc/rr_render.hpp) -- test harness only."""
import ctypes as C

import numpy as np

import emu_build as eb
import oracle_lib as ol

LIB = eb.LIBS["render"]


def build():
    return eb.build(LIB)


def build_program(path, extra=()):
    """the same source as a stand-alone program with its own main (crafted arenas at 4x1 and 96x96, S = 1 and 4), e.g. with
    extra=("-fsanitize=address,undefined", "-g")"""
    return eb.build_program(LIB, path, extra)


def lib():
    L = eb.load(LIB)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.render_emu.argtypes = [C.c_int] * 5 + [C.c_double, C.c_double, C.c_int, dp, dp, ip, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8)]
    return L


def render(preset, robots, balls, width, height, samples=1, arenas=None, f32=False):
    """robots [n,NR,10], balls [n,NB,8] (canonical layout) -> uint8 [m,height,width,3] of the kernel source; f32: fp32 records"""
    cfg = ol.PRESETS[preset]
    nrh, nr, nbp, nb = eb.counts(preset)
    r, b = eb.canonical(preset, robots, balls)
    n = r.shape[0]
    idx = None if arenas is None else np.ascontiguousarray(arenas, np.int32)
    m = n if idx is None else len(idx)
    rgb = np.full((m, height, width, 3), 0xAB, np.uint8)
    rc = lib().render_emu(int(f32), nr, nrh, nb, nbp, cfg["W"], cfg["H"], n, eb.ptr(r, C.c_double), eb.ptr(b, C.c_double), eb.ptr(idx, C.c_int32), m,
                          int(width), int(height), int(samples), eb.ptr(rgb, C.c_uint8))
    assert rc == 0, (preset, width, height, samples)
    return rgb
