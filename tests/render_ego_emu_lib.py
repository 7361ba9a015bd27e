"""ctypes binding of the host-emulated egocentric frame kernel (tests/emu/rr_render_ego_emu.cpp: g++ build of csrc/rr_render.hpp) -- test
harness only."""
import ctypes as C

import numpy as np

import emu_build as eb
import oracle_lib as ol

LIB = eb.LIBS["render_ego"]
RELATIVE, PLANAR = 1, 2


def build():
    return eb.build(LIB)


def build_program(path, extra=()):
    """the same source as a stand-alone program with its own main (crafted arenas at 4x1, 64x48 and 96x96, S = 1 and 4, every flag
    combination), e.g. with extra=("-fsanitize=address,undefined", "-g")"""
    return eb.build_program(LIB, path, extra)


def lib():
    L = eb.load(LIB)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.render_ego_emu.argtypes = [C.c_int] * 5 + [C.c_double, C.c_double, C.c_int, dp, dp, ip, ip, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_float, C.c_float, C.c_int, C.POINTER(C.c_uint8)]
    return L


def render(preset, robots, balls, width, height, samples=1, span=400.0, ahead=0.0, arenas=None, viewers=None, relative=False, planar=False,
           f32=False, rc=False, out=None):
    """robots [n,NR,10], balls [n,NB,8] (canonical layout) -> uint8 [m,height,width,3] ([m,3,height,width] when planar) of the kernel
    source; f32: fp32 records; arenas / viewers: [m] index lists or None (arena k, robot 0); rc: return the entry's return code instead;
    out: a contiguous uint8 array to write the frames to the start of (it may be longer: what lies behind them must stay as it is)"""
    cfg = ol.PRESETS[preset]
    nrh, nr, nbp, nb = eb.counts(preset)
    r, b = eb.canonical(preset, robots, balls)
    n = r.shape[0]
    idx = None if arenas is None else np.ascontiguousarray(arenas, np.int32)
    vw = None if viewers is None else np.ascontiguousarray(viewers, np.int32)
    m = len(idx) if idx is not None else len(vw) if vw is not None else n
    assert all(x is None or len(x) == m for x in (idx, vw))
    shape = (m, 3, height, width) if planar else (m, height, width, 3)
    rgb = np.full(shape, 0xAB, np.uint8) if out is None else out
    assert rgb.dtype == np.uint8 and rgb.flags.c_contiguous and rgb.size >= m * height * width * 3
    code = lib().render_ego_emu(int(f32), nr, nrh, nb, nbp, cfg["W"], cfg["H"], n, eb.ptr(r, C.c_double), eb.ptr(b, C.c_double),
                                eb.ptr(idx, C.c_int32), eb.ptr(vw, C.c_int32), m, int(width), int(height), int(samples), float(span),
                                float(ahead), (RELATIVE if relative else 0) | (PLANAR if planar else 0), eb.ptr(rgb, C.c_uint8))
    if rc:
        return code
    assert code == 0, (preset, width, height, samples, span, ahead)
    return rgb if out is None else rgb.reshape(-1)[:m * height * width * 3].reshape(shape)
