"""The held-row entries of the C-ABI (the hive under the budgeted step): declared in include/roborugby_amd.h, mirrored in
roborugby_amd/_lib.py, exported by the two libraries and by the one-shape library -- additive, the ABI version stays.  (What they refuse
needs a handle, hence a device: tests/test_gpu_hive_budget.py.)"""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = C.c_void_p
DECLS = {
    "rr_hive_observe_held": (r"rr_env \*env, uint32_t robot_mask, int32_t kind, int32_t \*assign, float \*obs, uint8_t \*held, void \*stream",
                             [VP, C.c_uint32, C.c_int32, VP, VP, VP, VP]),
    "rr_hive_observe_held_f64": (r"rr_env \*env, uint32_t robot_mask, int32_t kind, int32_t \*assign, double \*obs, uint8_t \*held, void \*stream",
                                 [VP, C.c_uint32, C.c_int32, VP, VP, VP, VP]),
    "rr_hive_commit": (r"rr_env \*env, uint32_t robot_mask, const int32_t \*fresh, const int32_t \*assign, const uint8_t \*held, "
                       r"int32_t \*accepted, float \*thrust, void \*stream", [VP, C.c_uint32, VP, VP, VP, VP, VP, VP]),
    "rr_hive_transition_held": (r"rr_env \*env, uint32_t robot_mask, int32_t kind, const int32_t \*assign, const int32_t \*status, "
                                r"const uint8_t \*done, float \*next_obs, float \*reward, uint8_t \*terminal, uint8_t \*valid, void \*stream",
                                [VP, C.c_uint32, C.c_int32] + [VP] * 8),
    "rr_hive_transition_held_f64": (r"rr_env \*env, uint32_t robot_mask, int32_t kind, const int32_t \*assign, const int32_t \*status, "
                                    r"const uint8_t \*done, double \*next_obs, double \*reward, uint8_t \*terminal, uint8_t \*valid, void \*stream",
                                    [VP, C.c_uint32, C.c_int32] + [VP] * 8),
}


def test_held_entries_are_declared_mirrored_and_exported():
    from roborugby_amd import _lib, build
    header = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "roborugby_amd.h")).read())
    assert re.search(r"#define RR_ABI_VERSION 4\b", header)
    for name, (params, args) in DECLS.items():
        assert re.search(r"int %s\(%s\);" % (name, params), header), name
        assert params.count(",") + 1 == len(args)  # (the arity this file states twice)
        res, got = _lib.SYMBOLS[name]
        assert res is C.c_int and got == args, name
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_EXACT, build.shape_lib_path(2, 1, 2, 3)):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built (__graft_entry__.build() builds the two libraries and preset X's)")
        lib = C.CDLL(path)
        for name in DECLS:
            assert hasattr(lib, name), (path, name)


def test_env_hive_and_trainers_carry_the_python_surface():
    import inspect
    from roborugby_amd import dqn, env, players
    E = env.BatchedRoboRugbyEnv
    sig = inspect.signature(E.hive_observe).parameters
    assert list(sig)[1:] == ["robot_mask", "observer", "f64", "out", "held"] and sig["held"].default is False
    assert list(inspect.signature(E.hive_transition_held).parameters) == list(inspect.signature(E.hive_transition).parameters)
    assert list(inspect.signature(E.hive_commit).parameters)[1:] == ["fresh", "assign", "held", "accepted", "thrust", "robot_mask"]
    assert isinstance(E.has_had_budget, property) and isinstance(players.Hive.held, property)
    for fn in (dqn.play_hive, dqn.train_hive):
        assert inspect.signature(fn).parameters["step_budget_clocks"].default == 0


def test_the_docs_no_longer_say_the_hive_refuses_the_budgeted_step():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "rr_hive_transition_held" in design
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in DECLS:
        assert f"`{name}`" in integration, name
