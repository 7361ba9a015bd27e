"""rr_render in the C-ABI: declared in include/roborugby_amd.h, mirrored in roborugby_amd/_lib.py, exported by the two libraries and by
the one-shape library -- additive, the ABI version stays -- and the Python surface that goes with it.  (What the entry refuses needs a
handle, hence a device: tests/test_gpu_render.py.)"""
import ctypes as C
import inspect
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = C.c_void_p
PARAMS = (r"rr_env \*env, const int32_t \*arenas, int32_t m, int32_t width, int32_t height, int32_t samples, uint8_t \*rgb, "
          r"void \*stream")
ARGS = [VP, VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, VP, VP]


def test_rr_render_is_declared_mirrored_and_exported():
    from roborugby_amd import _lib, build
    header = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "roborugby_amd.h")).read())
    assert re.search(r"#define RR_ABI_VERSION 4\b", header)
    assert re.search(r"int rr_render\(%s\);" % PARAMS, header)
    assert PARAMS.count(",") + 1 == len(ARGS)
    res, got = _lib.SYMBOLS["rr_render"]
    assert res is C.c_int and got == ARGS
    assert os.path.join(build.HERE, "csrc", "rr_render.hpp") in build.DEPS  # an edited kernel is a stale library
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_EXACT, build.shape_lib_path(2, 1, 2, 3)):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built (__graft_entry__.build() builds the two libraries and preset X's)")
        assert hasattr(C.CDLL(path), "rr_render"), path


def test_the_python_surface_is_there():
    from roborugby_amd import dqn, env, render
    sig = inspect.signature(env.BatchedRoboRugbyEnv.render_batch).parameters
    assert list(sig)[1:] == ["arenas", "width", "height", "samples", "out"]
    assert [sig[k].default for k in list(sig)[1:]] == [None, None, None, 1, None]
    assert list(inspect.signature(render.contact_sheet).parameters) == ["frames", "cols", "pad"]
    assert list(inspect.signature(render.save_gif).parameters) == ["path", "images", "fps"]
    ph = inspect.signature(dqn.play_hive).parameters
    assert [ph[k].default for k in ("record", "record_arenas", "record_size", "record_every")] == [None, 16, 96, 1]
    assert '"--record"' in inspect.getsource(dqn.main)
    # render() and the single-arena view keep their signatures
    assert list(inspect.signature(env.BatchedRoboRugbyEnv.render).parameters) == ["self", "mode", "arena"]
    assert list(inspect.signature(env.RoboRugbyEnv.render).parameters) == ["self", "mode"]


def test_the_kernel_colours_are_the_host_picture_s():
    """csrc/rr_render.hpp states the colours roborugby_amd/render.py carries (and tests/render_ref.py, independently, a third time)"""
    from roborugby_amd import render
    import render_ref as ref
    src = open(os.path.join(REPO, "roborugby_amd", "csrc", "rr_render.hpp")).read()
    for name, rgb in (("RENDER_BACKGROUND", render.COLOR_BACKGROUND), ("RENDER_GOAL_GRUMPY", render.COLOR_GOAL_GRUMPY),
                      ("RENDER_GOAL_HAPPY", render.COLOR_GOAL_HAPPY), ("RENDER_BALL_POS", render.COLOR_BALL_POS),
                      ("RENDER_BALL_NEG", render.COLOR_BALL_NEG)):
        assert re.search(r"%s = render_rgb\(%d, %d, %d\)" % ((name,) + tuple(rgb)), src), name
    assert (ref.BACKGROUND, ref.GOAL_GRUMPY, ref.GOAL_HAPPY, ref.BALL_POS, ref.BALL_NEG) == (
        render.COLOR_BACKGROUND, render.COLOR_GOAL_GRUMPY, render.COLOR_GOAL_HAPPY, render.COLOR_BALL_POS, render.COLOR_BALL_NEG)


def test_the_docs_name_the_entry():
    for doc in ("DESIGN.md", "INTEGRATION.md", "README.md"):
        text = open(os.path.join(REPO, doc)).read()
        assert "render_batch" in text, doc
    assert "`rr_render`" in open(os.path.join(REPO, "INTEGRATION.md")).read()
