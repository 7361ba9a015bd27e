"""The hive-mind entries of the C-ABI: declared in include/roborugby_amd.h, mirrored in roborugby_amd/_lib.py, exported by both libraries.
(What they refuse -- null pointers, an unknown kind, a mask bit >= NR, an empty mask -- needs a handle, hence a device:
tests/test_gpu_hive.py::test_hive_observe_refuses_bad_arguments_with_a_message.)"""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rr_hive_observe", "rr_hive_observe_f64")


def test_hive_entries_are_declared_mirrored_and_exported():
    from roborugby_amd import _lib
    header = open(os.path.join(REPO, "include", "roborugby_amd.h")).read()
    assert re.search(r"#define RR_ABI_VERSION 4\b", header)  # additive: the version stays
    for name, out in zip(NAMES, ("float", "double")):
        m = re.search(r"int %s\(rr_env \*env, uint32_t robot_mask, int32_t kind, int32_t \*assign, %s \*obs, void \*stream\);" % (name, out), header)
        assert m, name
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args == [C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_EXACT):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built (__graft_entry__.build() builds both libraries)")
        lib = C.CDLL(path)
        for name in NAMES:
            assert hasattr(lib, name), (path, name)


def test_one_shape_library_exports_the_hive_entries():
    from roborugby_amd import build
    path = build.shape_lib_path(2, 1, 2, 3)
    if not os.path.exists(path):
        pytest.fail(f"{path} is not built (__graft_entry__.build() builds preset X's library)")
    lib = C.CDLL(path)
    for name in NAMES:
        assert hasattr(lib, name), name
