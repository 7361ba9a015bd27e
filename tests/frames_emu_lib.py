"""ctypes binding of the host-emulated frame-replay kernels (tests/emu/rr_frames_emu.cpp: g++ build of csrc/rr_frames.hpp) -- test harness
only."""
import ctypes as C

import numpy as np

import emu_build as eb
import frames_ref as fr

LIB = eb.LIBS["frames"]
_vp = C.c_void_p
_p = eb.ptr  # an array's data as a void *, None for None


def build():
    return eb.build(LIB)


def build_program(path, extra=()):
    """the same source as a stand-alone program with its own main (rings pushed past three wraps and sampled both ways, every block a heap
    block of exactly its size), e.g. with extra=("-fsanitize=address,undefined", "-g")"""
    return eb.build_program(LIB, path, extra)


def lib():
    L = eb.load(LIB)
    L.frames_push_emu.argtypes = [_vp, C.c_int64, _vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int64, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp]
    L.frames_sample_emu.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _vp, C.c_uint64,
                                    C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    return L


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
