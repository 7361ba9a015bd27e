"""ctypes binding of the host-emulated held-row kernels of the hive (tests/emu/rr_hive_emu.cpp: hive_held_emu, hive_commit_emu,
hive_idle_emu) -- test harness only."""
import ctypes as C

import numpy as np

import emu_build as eb
import hive_emu_lib as he
import oracle_lib as ol

LANES = {"T": (2, 64), "G": (8, 64)}  # lanes per arena the tests run the emulation at
build, lib = he.build, he.lib  # one library with the hive's own entry
_p = eb.ptr


def hive_observe_held(preset, robots, balls, parked, mask, kind, vw, assign, obs):
    """k_hive_held's body on robots [n,NR,10], balls [n,NB,8]; parked [n]: the record carries the parked mark.  assign int32 [n,NR] and
    obs float64 [n,NR,11] are written IN PLACE (rows of parked arenas must stay); -> held uint8 [n]"""
    cfg = ol.PRESETS[preset]
    r, b = eb.canonical(preset, robots, balls)
    n, nr = r.shape[:2]
    pk = np.ascontiguousarray(parked, np.uint8)
    assert pk.shape == (n,) and assign.shape == (n, nr) and obs.shape == (n, nr, 11)
    assert assign.dtype == np.int32 and obs.dtype == np.float64 and assign.flags.c_contiguous and obs.flags.c_contiguous
    held = np.full(n, 9, np.uint8)
    rc = lib().hive_held_emu(eb.PRESET_ID[preset], int(vw), C.c_double(cfg["W"]), C.c_double(cfg["H"]), n, _p(r, C.c_double), _p(b, C.c_double),
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
    rc = lib().hive_idle_emu(eb.PRESET_ID[preset], int(vw), n, _p(status, C.c_int32), _p(next_obs, C.c_double), _p(reward, C.c_double),
                             _p(terminal, C.c_uint8), _p(valid, C.c_uint8), _p(wrote, C.c_uint8))
    assert rc == 0, (preset, vw)
    return wrote
