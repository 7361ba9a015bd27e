"""ctypes binding of the host-emulated per-row arithmetic of rr_sac_targets (tests/emu/rr_sac_targets_emu.cpp: g++ build of
csrc/rr_sac.hpp) -- test harness only.  The library is this module's own emu_build.Lib: built on first use, by content hash like the
registered ones."""
import ctypes as C

import numpy as np

import emu_build as eb

LIB = eb.Lib(eb._emu("rr_sac_targets_emu.cpp"), "librr_sac_targets_emu.so", eb._STRICT + ("-Wall", "-Wextra", "-Werror"),
             ("sac_targets_stream_emu", "sac_targets_uniforms_emu", "sac_targets_draw_emu", "sac_ring_row_ok_emu", "sac_targets_close_emu"),
             "RR_SAC_TARGETS_EMU_MAIN")
_vp = C.c_void_p
_p = eb.ptr


def build():
    return eb.build(LIB)


def build_program(path, extra=()):
    """the same source as a stand-alone program with its own main, e.g. with extra=("-fsanitize=address,undefined", "-g")"""
    return eb.build_program(LIB, path, extra)


def lib():
    L = eb.load(LIB)
    L.sac_targets_stream_emu.argtypes, L.sac_targets_stream_emu.restype = [], C.c_uint32
    L.sac_targets_uniforms_emu.argtypes, L.sac_targets_uniforms_emu.restype = [C.c_uint64, C.c_uint32, C.c_int32, _vp], None
    L.sac_targets_draw_emu.argtypes, L.sac_targets_draw_emu.restype = [C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, _vp], None
    L.sac_ring_row_ok_emu.argtypes, L.sac_ring_row_ok_emu.restype = [_vp, C.c_int32, C.c_int64, _vp], None
    L.sac_targets_close_emu.argtypes = [_vp, C.c_int32, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, C.c_float, C.c_float, _vp, _vp]
    return L


def stream_word():
    return int(lib().sac_targets_stream_emu())


def uniforms(seed, n, call):
    """[n, 2, 2] float32: (pair, (u1, u2))"""
    u = np.full((n, 2, 2), np.nan, np.float32)
    lib().sac_targets_uniforms_emu(seed, call & 0xFFFFFFFF, n, _p(u))
    return u


def draw(seed, n, call, stream_default=False):
    """[n, 4] float32: sac_draw on the targets' stream word (stream_default: without the stream argument)"""
    z = np.full((n, 4), np.nan, np.float32)
    lib().sac_targets_draw_emu(seed, call & 0xFFFFFFFF, n, 1 if stream_default else 0, _p(z))
    return z


def ring_row_ok(index, mem_rows):
    index = np.ascontiguousarray(index, np.int64)
    ok = np.full(index.shape[0], 7, np.uint8)
    lib().sac_ring_row_ok_emu(_p(index), index.shape[0], mem_rows, _p(ok))
    return ok


def close(index, mem_rows, reward, terminal, q1, q2, log_prob, v_next, reward_scale, gamma):
    """(return code, value_target [n], q_hat [n]): reward / terminal are rings of mem_rows rows, the others batch vectors"""
    f = np.float32
    index = np.ascontiguousarray(index, np.int64)
    reward, terminal = np.ascontiguousarray(reward, f), np.ascontiguousarray(terminal, np.uint8)
    assert reward.shape[0] >= mem_rows and terminal.shape[0] >= mem_rows
    q1, q2, log_prob, v_next = (np.ascontiguousarray(a, f) for a in (q1, q2, log_prob, v_next))
    n = index.shape[0]
    vt, qh = np.full(n, 7.0, f), np.full(n, 7.0, f)
    rc = lib().sac_targets_close_emu(_p(index), n, mem_rows, _p(reward), _p(terminal), _p(q1), _p(q2), _p(log_prob), _p(v_next), reward_scale,
                                     gamma, _p(vt), _p(qh))
    return rc, vt, qh
