"""The one builder of the host-emulation harness (tests/emu/*.cpp: g++ builds of the kernels' own headers) and what its ctypes bindings
(tests/*_lib.py) share -- test harness only.

Staleness is decided by CONTENT, as roborugby_amd/build.py decides it for the product library: the sha256 of the flags and of every
dependency is written next to the library (<so>.srchash); a library whose recorded hash differs is rebuilt before anything loads it.
The dependency set is the same for every library and over-approximate on purpose -- the library's own .cpp, every .hpp next to it and
every roborugby_amd/csrc/*.hpp -- so there is no per-library header list to forget (tests/test_emu_build.py holds it to g++ -MM)."""
import ctypes as C
import glob
import hashlib
import os
import shutil
import subprocess
from typing import NamedTuple

import numpy as np

import oracle_lib as ol

EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
CSRC = os.path.join(ol.REPO, "roborugby_amd", "csrc")
_O2 = ("-O2", "-std=c++17")
_STRICT = _O2 + ("-ffp-contract=off",)  # no fused multiply-adds: bit-exact comparisons with the oracle and with recorded vectors


class Lib(NamedTuple):
    source: str          # the translation unit; its directory also receives the library
    out: str             # file name of the shared library
    flags: tuple         # compile flags and defines (without -fPIC -shared)
    exports: tuple = ()  # entry points the Python side binds
    main: str = None     # the define that turns the source into a stand-alone program

    @property
    def so(self):
        return os.path.join(os.path.dirname(self.source), self.out)


def _emu(name):
    return os.path.join(EMU, name)


LIBS = {
    "emu": Lib(_emu("rr_emu.cpp"), "librr_emu.so", _STRICT, (
        "emu_create", "emu_destroy", "emu_set_state", "emu_get_state", "emu_set_poses", "emu_set_scratch_rect", "emu_get_scratch_rect", "emu_step",
        "emu_step_budget", "emu_park_seed", "emu_step_thrust", "emu_observe", "emu_reset", "emu_set_program", "emu_observe_kind",
        "emu_set_goal_scoring", "emu_goal_scores", "emu_py_mod360", "emu_sincos", "emu_debug_set_substeps", "emu_debug_trace", "emu_debug_memo",
        "emu_debug_scrub", "emu_shape_lanes")),
    "hive": Lib(_emu("rr_hive_emu.cpp"), "librr_hive_emu.so", _STRICT, ("hive_emu", "hive_held_emu", "hive_commit_emu", "hive_idle_emu")),
    # the hive's flags + -fno-builtin: the rewards' distances are the reference's pow(x, 2.0) / pow(x, .5) and must stay the libm calls
    # CPython makes (g++ would fold the former to x * x), as oracle/Makefile keeps them for the oracle
    "hive_transition": Lib(_emu("rr_hive_transition_emu.cpp"), "librr_hive_transition_emu.so", _STRICT + ("-fno-builtin",), ("hive_transition_emu",)),
    "render": Lib(_emu("rr_render_emu.cpp"), "librr_render_emu.so", _STRICT, ("render_emu",), "RR_RENDER_EMU_MAIN"),
    "render_ego": Lib(_emu("rr_render_ego_emu.cpp"), "librr_render_ego_emu.so", _STRICT, ("render_ego_emu",), "RR_RENDER_EGO_EMU_MAIN"),
    "frames": Lib(_emu("rr_frames_emu.cpp"), "librr_frames_emu.so", _O2, ("frames_push_emu", "frames_sample_emu"), "RR_FRAMES_EMU_MAIN"),
}
# the same source with -DRR_EXACT_TRIG=1 (the exact-trig parity build)
LIBS["emu_exact"] = LIBS["emu"]._replace(out="librr_emu_exact.so", flags=_STRICT + ("-DRR_EXACT_TRIG=1",))


def deps(lib):
    d = os.path.dirname(lib.source)
    return [lib.source] + sorted(glob.glob(os.path.join(d, "*.hpp"))) + sorted(glob.glob(os.path.join(CSRC, "*.hpp")))


def source_hash(lib):
    h = hashlib.sha256(" ".join(lib.flags).encode())
    for d in deps(lib):
        with open(d, "rb") as f:
            h.update(os.path.basename(d).encode() + b"\0" + f.read())
    return h.hexdigest()


def is_stale(lib):
    if not os.path.exists(lib.so) or not os.path.exists(lib.so + ".srchash"):
        return True
    with open(lib.so + ".srchash") as f:
        return f.read().strip() != source_hash(lib)


def build(lib, verbose=False):
    """g++ ... -> lib.so, if it is stale; never returns a stale library"""
    if not is_stale(lib):
        return lib.so
    if not shutil.which("g++"):
        raise RuntimeError(f"{lib.out} is missing or older than its sources and there is no g++ to rebuild it")
    digest = source_hash(lib)
    tmp = lib.so + f".tmp{os.getpid()}"
    cmd = ["g++", *lib.flags, "-fPIC", "-shared", "-o", tmp, lib.source]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(tmp, lib.so)  # atomic: a concurrent loader sees the old or the new library, never half of one
    with open(lib.so + ".srchash", "w") as f:
        f.write(digest + "\n")
    return lib.so


def build_all(verbose=False):
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(len(LIBS), os.cpu_count() or 1)) as ex:  # one g++ process per library, side by side
        return list(ex.map(lambda lib: build(lib, verbose), LIBS.values()))


def build_program(lib, path, extra=()):
    """the library's source as a stand-alone program with its own main, e.g. with extra=("-fsanitize=address,undefined", "-g")"""
    subprocess.check_call(["g++", *lib.flags, *extra, "-D" + lib.main, "-o", path, lib.source])
    return path


_loaded = {}


def load(lib):
    if lib.so not in _loaded:
        _loaded[lib.so] = C.CDLL(build(lib))
    return _loaded[lib.so]


# ---- what the bindings share
# the emulations' preset ids; the non-square ids run their shape's build at their own W, H
PRESET_ID = {"T": 0, "G": 1, "D": 2, "X": 3, "Y": 4, "W": 5, "R": 6, "Q": 7, "P": 8}
PRESET_ID.update({wide: PRESET_ID[shape] for wide, shape in ol.SHAPE.items()})


def ptr(a, ctype=None):
    """a numpy array's data as a POINTER(ctype) (void * without one); None stays None"""
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype) if ctype else C.c_void_p)


def counts(preset):
    """(nrh, nr, nbp, nb) of a preset"""
    cfg = ol.PRESETS[preset]
    return cfg["nr_h"], cfg["nr_h"] + cfg["nr_g"], cfg["nb_p"], cfg["nb_p"] + cfg["nb_n"]


def canonical(preset, robots, balls):
    """robots, balls in canonical layout as contiguous float64 [n,NR,10], [n,NB,8]"""
    _, nr, _, nb = counts(preset)
    r = np.ascontiguousarray(robots, np.float64).reshape(-1, nr, 10)
    return r, np.ascontiguousarray(balls, np.float64).reshape(r.shape[0], nb, 8)
