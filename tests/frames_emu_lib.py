"""ctypes binding of the host-emulated frame-replay kernels (tests/emu/rr_frames_emu.cpp: g++ build of csrc/rr_frames.hpp) -- test harness
only."""
import ctypes as C
import os
import subprocess

import numpy as np

import frames_ref as fr

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SO = os.path.join(HERE, "emu", "librr_frames_emu.so")
CSRC = os.path.join(REPO, "roborugby_amd", "csrc")
SRC = [os.path.join(HERE, "emu", "rr_frames_emu.cpp")] + [os.path.join(CSRC, f) for f in ("rr_frames.hpp", "rr_dqn_shared.hpp")]
FLAGS = ["-O2", "-std=c++17"]


def build():
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(s) for s in SRC):
        tmp = SO + f".tmp{os.getpid()}"
        subprocess.check_call(["g++"] + FLAGS + ["-fPIC", "-shared", "-o", tmp, SRC[0]])
        os.replace(tmp, SO)
    return SO


def build_program(path, extra=()):
    """the same source as a stand-alone program with its own main (rings pushed past three wraps and sampled both ways, every block a heap
    block of exactly its size), e.g. with extra=("-fsanitize=address,undefined", "-g")"""
    subprocess.check_call(["g++"] + FLAGS + list(extra) + ["-DRR_FRAMES_EMU_MAIN", "-o", path, SRC[0]])
    return path


_lib = None
_vp = C.c_void_p


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.frames_push_emu.argtypes = [_vp, C.c_int64, _vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int64, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp]
        _lib.frames_sample_emu.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _vp, C.c_uint64,
                                           C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    return _lib


def _p(a):
    return None if a is None else _vp(a.ctypes.data)


def push(ring, src, stride=None, first=None, action=None, reward=None, done=None, valid=None, offset=0):
    """the emulated rr_frames_push of push number ring.head into a frames_ref.Ring (its arrays are written in place); src: a contiguous
    uint8 array, the frames start `offset` bytes in and lie `stride` bytes apart (None: frame_bytes).  Returns the entry's return code."""
    stride = ring.frame_bytes if stride is None else stride
    rc = lib().frames_push_emu(_vp(src.ctypes.data + offset), stride, _p(first), _p(action), _p(reward), _p(done), _p(valid), ring.rows,
                               ring.frame_bytes, ring.slots, ring.head, _p(ring.frames), _p(ring.age), _p(ring.action), _p(ring.reward), _p(ring.flags))
    if rc == 0:
        ring.head += 1
    return rc


def sample(ring, stack, batch, index=None, seed=0, call=0, pad=8, out=None):
    """the emulated rr_frames_sample into poisoned outputs of batch + pad rows: (return code, dict of numpy arrays)"""
    out = fr.poisoned_outputs(batch, stack, ring.frame_bytes, pad) if out is None else out
    idx = None if index is None else np.ascontiguousarray(index, np.int64)
    rc = lib().frames_sample_emu(_p(ring.frames), _p(ring.age), _p(ring.action), _p(ring.reward), _p(ring.flags), ring.rows, ring.frame_bytes,
                                 ring.slots, ring.head, stack, batch, _p(idx), seed, call, *[_p(out[f]) for f in fr.OUT_FIELDS])
    return rc, out
