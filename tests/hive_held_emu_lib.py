"""ctypes binding of the host-emulated held-row kernels of the hive (tests/emu/rr_hive_held_emu.cpp) -- test harness only."""
import ctypes as C
import os
import subprocess

import numpy as np

import hive_emu_lib as he
import oracle_lib as ol

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "emu", "librr_hive_held_emu.so")
SRC = [os.path.join(HERE, "emu", "rr_hive_held_emu.cpp")] + he.SRC[1:]
LANES = {"T": (2, 64), "G": (8, 64)}  # lanes per arena the emulation is built for


def build():
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(s) for s in SRC):
        tmp = SO + f".tmp{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-fPIC", "-ffp-contract=off", "-std=c++17", "-shared", "-o", tmp, SRC[0]])
        os.replace(tmp, SO)
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def hive_observe_held(preset, robots, balls, parked, mask, kind, vw, assign, obs):
    """k_hive_held's body on robots [n,NR,10], balls [n,NB,8]; parked [n]: the record carries the parked mark.  assign int32 [n,NR] and
    obs float64 [n,NR,11] are written IN PLACE (rows of parked arenas must stay); -> held uint8 [n]"""
    cfg = ol.PRESETS[preset]
    nr, nb = cfg["nr_h"] + cfg["nr_g"], cfg["nb_p"] + cfg["nb_n"]
    r = np.ascontiguousarray(robots, np.float64).reshape(-1, nr, 10)
    b = np.ascontiguousarray(balls, np.float64).reshape(-1, nb, 8)
    n = r.shape[0]
    pk = np.ascontiguousarray(parked, np.uint8)
    assert b.shape[0] == n and pk.shape == (n,) and assign.shape == (n, nr) and obs.shape == (n, nr, 11)
    assert assign.dtype == np.int32 and obs.dtype == np.float64 and assign.flags.c_contiguous and obs.flags.c_contiguous
    held = np.full(n, 9, np.uint8)
    rc = lib().hive_held_emu(he.PRESET_ID[preset], int(vw), C.c_double(cfg["W"]), C.c_double(cfg["H"]), n, _p(r, C.c_double), _p(b, C.c_double),
                             _p(pk, C.c_uint8), C.c_uint32(int(mask)), int(kind), _p(assign, C.c_int32), _p(obs, C.c_double), _p(held, C.c_uint8))
    assert rc == 0, (preset, vw)
    return held


def hive_commit(nr, mask, fresh, assign, held, accepted, thrust):
    """k_hive_commit's loop; accepted int32 [n,nr] and thrust float32 [n,2*nr] are written IN PLACE"""
    n = fresh.shape[0]
    for a, t, shape in ((fresh, np.int32, (n, nr)), (assign, np.int32, (n, nr)), (held, np.uint8, (n,)), (accepted, np.int32, (n, nr)),
                        (thrust, np.float32, (n, 2 * nr))):
        assert a.dtype == t and a.shape == shape and a.flags.c_contiguous
    rc = lib().hive_commit_emu(n, nr, C.c_uint32(int(mask)), _p(fresh, C.c_int32), _p(assign, C.c_int32), _p(held, C.c_uint8),
                               _p(accepted, C.c_int32), _p(thrust, C.c_float))
    assert rc == 0


def hive_idle(preset, vw, status, next_obs, reward, terminal, valid):
    """the held transition kernel's early return; the four outputs are written IN PLACE for arenas that did not step; -> wrote uint8 [n]"""
    n = status.shape[0]
    wrote = np.full(n, 9, np.uint8)
    rc = lib().hive_idle_emu(he.PRESET_ID[preset], int(vw), n, _p(status, C.c_int32), _p(next_obs, C.c_double), _p(reward, C.c_double),
                             _p(terminal, C.c_uint8), _p(valid, C.c_uint8), _p(wrote, C.c_uint8))
    assert rc == 0, (preset, vw)
    return wrote
