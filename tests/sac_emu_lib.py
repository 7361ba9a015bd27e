"""ctypes binding of the host-emulated epilogue of rr_sac_act (tests/emu/rr_sac_emu.cpp: g++ build of csrc/rr_sac.hpp) -- test harness
only.  The library is this module's own emu_build.Lib: built on first use, by content hash like the registered ones."""
import ctypes as C

import numpy as np

import emu_build as eb

LIB = eb.Lib(eb._emu("rr_sac_emu.cpp"), "librr_sac_emu.so", eb._STRICT, ("sac_uniforms_emu", "sac_draw_emu", "sac_squash_emu"), "RR_SAC_EMU_MAIN")
_vp = C.c_void_p
_p = eb.ptr


def build():
    return eb.build(LIB)


def build_program(path, extra=()):
    """the same source as a stand-alone program with its own main, e.g. with extra=("-fsanitize=address,undefined", "-g")"""
    return eb.build_program(LIB, path, extra)


def lib():
    L = eb.load(LIB)
    L.sac_uniforms_emu.argtypes = [C.c_uint64, C.c_uint32, C.c_int32, _vp]
    L.sac_uniforms_emu.restype = None
    L.sac_draw_emu.argtypes = [C.c_uint64, C.c_uint32, C.c_int32, _vp]
    L.sac_draw_emu.restype = None
    L.sac_squash_emu.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_float, _vp, _vp]
    return L


def uniforms(seed, n, call):
    """[n, 2, 2] float32: (pair, (u1, u2))"""
    u = np.full((n, 2, 2), np.nan, np.float32)
    lib().sac_uniforms_emu(seed, call & 0xFFFFFFFF, n, _p(u))
    return u


def draw(seed, n, call):
    """[n, 4] float32"""
    z = np.full((n, 4), np.nan, np.float32)
    lib().sac_draw_emu(seed, call & 0xFFFFFFFF, n, _p(z))
    return z


def squash(head, z, max_action=1.0):
    """(return code, actions [n, A], log_prob [n]) from head [n, 2A] and z [n, A], both float32"""
    head, z = np.ascontiguousarray(head, np.float32), np.ascontiguousarray(z, np.float32)
    n, A = z.shape
    actions, lp = np.full((n, A), np.nan, np.float32), np.full(n, np.nan, np.float32)
    rc = lib().sac_squash_emu(_p(head), _p(z), n, A, max_action, _p(actions), _p(lp))
    return rc, actions, lp
