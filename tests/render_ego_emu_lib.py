"""ctypes binding of the host-emulated egocentric frame kernel (tests/emu/rr_render_ego_emu.cpp: g++ build of csrc/rr_render.hpp) -- test
harness only."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as ol

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "emu", "librr_render_ego_emu.so")
CSRC = os.path.join(ol.REPO, "roborugby_amd", "csrc")
SRC = [os.path.join(HERE, "emu", "rr_render_ego_emu.cpp")] + [os.path.join(CSRC, f) for f in ("rr_render.hpp", "rr_sim.hpp")]
FLAGS = ["-O2", "-ffp-contract=off", "-std=c++17"]
RELATIVE, PLANAR = 1, 2


def build():
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(s) for s in SRC):
        tmp = SO + f".tmp{os.getpid()}"
        subprocess.check_call(["g++"] + FLAGS + ["-fPIC", "-shared", "-o", tmp, SRC[0]])
        os.replace(tmp, SO)
    return SO


def build_program(path, extra=()):
    """the same source as a stand-alone program with its own main (crafted arenas at 4x1, 64x48 and 96x96, S = 1 and 4, every flag
    combination), e.g. with extra=("-fsanitize=address,undefined", "-g")"""
    subprocess.check_call(["g++"] + FLAGS + list(extra) + ["-DRR_RENDER_EGO_EMU_MAIN", "-o", path, SRC[0]])
    return path


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        _lib.render_ego_emu.argtypes = [C.c_int] * 5 + [C.c_double, C.c_double, C.c_int, dp, dp, ip, ip, C.c_int, C.c_int, C.c_int, C.c_int,
                                                       C.c_float, C.c_float, C.c_int, C.POINTER(C.c_uint8)]
    return _lib


def render(preset, robots, balls, width, height, samples=1, span=400.0, ahead=0.0, arenas=None, viewers=None, relative=False, planar=False,
           f32=False, rc=False, out=None):
    """robots [n,NR,10], balls [n,NB,8] (canonical layout) -> uint8 [m,height,width,3] ([m,3,height,width] when planar) of the kernel
    source; f32: fp32 records; arenas / viewers: [m] index lists or None (arena k, robot 0); rc: return the entry's return code instead;
    out: a contiguous uint8 array to write the frames to the start of (it may be longer: what lies behind them must stay as it is)"""
    cfg = ol.PRESETS[preset]
    nr, nb = cfg["nr_h"] + cfg["nr_g"], cfg["nb_p"] + cfg["nb_n"]
    r = np.ascontiguousarray(robots, np.float64).reshape(-1, nr, 10)
    b = np.ascontiguousarray(balls, np.float64).reshape(-1, nb, 8)
    n = r.shape[0]
    assert b.shape[0] == n
    ip = C.POINTER(C.c_int32)
    idx = None if arenas is None else np.ascontiguousarray(arenas, np.int32)
    vw = None if viewers is None else np.ascontiguousarray(viewers, np.int32)
    m = len(idx) if idx is not None else len(vw) if vw is not None else n
    assert all(x is None or len(x) == m for x in (idx, vw))
    shape = (m, 3, height, width) if planar else (m, height, width, 3)
    rgb = np.full(shape, 0xAB, np.uint8) if out is None else out
    assert rgb.dtype == np.uint8 and rgb.flags.c_contiguous and rgb.size >= m * height * width * 3
    code = lib().render_ego_emu(int(f32), nr, cfg["nr_h"], nb, cfg["nb_p"], cfg["W"], cfg["H"], n, r.ctypes.data_as(C.POINTER(C.c_double)),
                                b.ctypes.data_as(C.POINTER(C.c_double)), None if idx is None else idx.ctypes.data_as(ip),
                                None if vw is None else vw.ctypes.data_as(ip), m, int(width), int(height), int(samples), float(span),
                                float(ahead), (RELATIVE if relative else 0) | (PLANAR if planar else 0), rgb.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc:
        return code
    assert code == 0, (preset, width, height, samples, span, ahead)
    return rgb if out is None else rgb.reshape(-1)[:m * height * width * 3].reshape(shape)
