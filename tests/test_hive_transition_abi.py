"""The hive-training entries of the C-ABI: declared in include/roborugby_amd.h, mirrored in roborugby_amd/_lib.py, exported by the two
libraries and by the one-shape library -- additive, the ABI version stays.  (What they refuse needs a handle, hence a device:
tests/test_gpu_hive_transition.py::test_refusals_return_minus_one_with_a_message_and_touch_nothing.)"""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rr_hive_transition", "rr_hive_transition_f64")


def test_transition_entries_are_declared_mirrored_and_exported():
    from roborugby_amd import _lib, build
    header = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "roborugby_amd.h")).read())
    assert re.search(r"#define RR_ABI_VERSION 4\b", header)
    for name, out in zip(NAMES, ("float", "double")):
        decl = (r"int %s\(rr_env \*env, uint32_t robot_mask, int32_t kind, const int32_t \*assign, const int32_t \*status, "
                r"const uint8_t \*done, %s \*next_obs, %s \*reward, uint8_t \*terminal, uint8_t \*valid, void \*stream\);" % (name, out, out))
        assert re.search(decl, header), name
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args == [C.c_void_p, C.c_uint32, C.c_int32] + [C.c_void_p] * 8
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_EXACT, build.shape_lib_path(2, 1, 2, 3)):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built (__graft_entry__.build() builds the two libraries and preset X's)")
        lib = C.CDLL(path)
        for name in NAMES:
            assert hasattr(lib, name), (path, name)


def test_env_and_hive_carry_the_python_surface():
    import inspect
    from roborugby_amd import dqn, env, players
    assert list(inspect.signature(env.BatchedRoboRugbyEnv.hive_transition).parameters)[1:] == [
        "assign", "status", "done", "robot_mask", "observer", "f64", "out"]
    assert list(inspect.signature(env.BatchedRoboRugbyEnv.track_prior_step).parameters)[1:] == ["on"]
    assert list(inspect.signature(players.Hive.transition).parameters)[1:] == ["done", "status"]
    assert list(inspect.signature(players.Hive.store).parameters)[1:] == ["agent", "done", "status"]
    sig = inspect.signature(dqn.train_hive).parameters
    assert list(sig)[:8] == ["num_envs", "steps", "preset", "robots", "opponents", "resume", "checkpoint", "updates_per_step"]
    assert sig["preset"].default == "G" and sig["opponents"].default == "og_twitchy" and sig["updates_per_step"].default == 4
