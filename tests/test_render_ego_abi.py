"""rr_render_ego in the C-ABI: declared in include/roborugby_amd.h, mirrored in roborugby_amd/_lib.py, exported by the two libraries and by
the one-shape library -- additive, the ABI version stays -- and the Python surface that goes with it.  (What the entry refuses needs a
handle, hence a device: tests/test_gpu_render_ego.py.)"""
import ctypes as C
import inspect
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = C.c_void_p
PARAMS = (r"rr_env \*env, const int32_t \*arenas, const int32_t \*robots, int32_t m, int32_t width, int32_t height, int32_t samples, "
          r"float span, float ahead, int32_t flags, uint8_t \*rgb, void \*stream")
ARGS = [VP, VP, VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32, VP, VP]


def test_rr_render_ego_is_declared_mirrored_and_exported():
    from roborugby_amd import _lib, build
    header = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "roborugby_amd.h")).read())
    assert re.search(r"#define RR_ABI_VERSION 4\b", header)
    assert re.search(r"int rr_render_ego\(%s\);" % PARAMS, header)
    assert re.search(r"#define RR_EGO_RELATIVE 1\b", header) and re.search(r"#define RR_EGO_PLANAR 2\b", header)
    assert PARAMS.count(",") + 1 == len(ARGS)
    res, got = _lib.SYMBOLS["rr_render_ego"]
    assert res is C.c_int and got == ARGS
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_EXACT, build.shape_lib_path(2, 1, 2, 3)):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built (__graft_entry__.build() builds the two libraries and preset X's)")
        lib = C.CDLL(path)
        assert hasattr(lib, "rr_render_ego") and hasattr(lib, "rr_render"), path
    assert _lib.load().rr_abi_version() == 4


def test_the_python_surface_is_there():
    import roborugby_amd as rr
    from roborugby_amd import dqn, env, pixels
    sig = inspect.signature(env.BatchedRoboRugbyEnv.render_ego).parameters
    assert list(sig)[1:] == ["arenas", "robots", "width", "height", "span", "ahead", "samples", "relative", "planar", "out"]
    assert [sig[k].default for k in list(sig)[1:]] == [None, None, 64, None, 400.0, 0.0, 1, True, False, None]
    assert rr.PixelObservation is pixels.PixelObservation and "PixelObservation" in rr.__all__
    sig = inspect.signature(pixels.PixelObservation).parameters
    assert list(sig) == ["env", "robots", "size", "span", "ahead", "samples", "relative", "stack"]
    assert [sig[k].default for k in list(sig)[1:]] == [0, 64, 400.0, 0.0, 1, True, 1]
    for name, params in (("reset", ["self", "mask"]), ("step", ["self", "actions"]), ("step_thrust", ["self", "thrust"])):
        assert list(inspect.signature(getattr(pixels.PixelObservation, name)).parameters) == params
    ph = inspect.signature(dqn.play_hive).parameters
    assert ph["record_view"].default == "field"
    assert [ph[k].default for k in ("record", "record_arenas", "record_size", "record_every")] == [None, 16, 96, 1]  # unchanged
    assert '"--record-view"' in inspect.getsource(dqn.main)
    # render_batch keeps its signature
    assert list(inspect.signature(env.BatchedRoboRugbyEnv.render_batch).parameters)[1:] == ["arenas", "width", "height", "samples", "out"]


def test_the_outside_colour_is_stated_the_same_everywhere():
    from roborugby_amd import render
    import render_ego_ref as ego
    src = open(os.path.join(REPO, "roborugby_amd", "csrc", "rr_render.hpp")).read()
    assert render.COLOR_OUTSIDE == (96, 96, 96) == ego.OUTSIDE
    assert re.search(r"RENDER_OUTSIDE = render_rgb\(%d, %d, %d\)" % render.COLOR_OUTSIDE, src)
    assert re.search(r"RENDER_EGO_RELATIVE = 1, RENDER_EGO_PLANAR = 2\b", src)
    assert "k_render_ego" in src


def test_the_docs_name_the_entry():
    for doc in ("DESIGN.md", "INTEGRATION.md", "README.md"):
        text = open(os.path.join(REPO, doc)).read()
        assert "render_ego" in text, doc
    assert "`rr_render_ego`" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert "PixelObservation" in open(os.path.join(REPO, "DESIGN.md")).read()
