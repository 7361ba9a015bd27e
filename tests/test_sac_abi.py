"""rr_sac_act's place in the C-ABI: declared in include/roborugby_amd.h with its flag, mirrored in _lib.SYMBOLS, exported by the built
libraries, compiled by roborugby_amd/build.py from its own translation unit, named in INTEGRATION.md.  CPU only."""
import ctypes as C
import os
import re

import pytest

import oracle_lib as ol

HEADER = os.path.join(ol.REPO, "include", "roborugby_amd.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_entry_and_its_flag():
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int rr_sac_act\((.*?)\);", code, re.S)
    assert m, "rr_sac_act is not declared"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["rr_dqn *dqn", "const float *const params[8]", "const float *obs", "int32_t n", "int32_t n_actions", "float max_action",
                    "int32_t flags", "uint64_t seed", "uint32_t call", "float *actions", "float *log_prob", "float *head", "float *noise",
                    "void *stream"]
    assert re.search(r"^#define RR_SAC_DETERMINISTIC 1\b", code, re.M)
    for word in ("0x5AC7", "Philox4x32-10", "clamp(raw, 1e-6, 1)", "multiple of 64", "rr_dqn_last_error"):  # the comment is the specification
        assert word in text, word


def test_symbols_mirror_the_declaration():
    torch = pytest.importorskip("torch")  # noqa: F841  (_lib imports it first)
    from roborugby_amd import _lib
    res, args = _lib.SYMBOLS["rr_sac_act"]
    vp = C.c_void_p
    assert res is C.c_int
    assert args[0] is vp and args[2] is vp and args[3:9] == [C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_uint64, C.c_uint32]
    assert args[1]._type_._length_ == 8 and args[9:] == [vp] * 5
    assert _lib.RR_SAC_DETERMINISTIC == 1
    assert hasattr(_lib.DqnHandle, "sac_act")


def test_built_libraries_export_it():
    pytest.importorskip("torch")
    from roborugby_amd import _lib, build  # noqa: F401  (_lib: torch's HIP runtime is loaded before the library's)
    assert build.SRC_SAC in build.DEPS and os.path.join(build.HERE, "csrc", "rr_sac.hpp") in build.DEPS
    assert os.path.join(build.HERE, "csrc", "rr_dqn_tile.hpp") in build.DEPS  # an edited tile is a stale library
    libs = [build.LIB, build.LIB_EXACT, build.shape_lib_path(2, 1, 2, 3)]
    for path in libs:
        assert os.path.exists(path), f"{path}: __graft_entry__.build() makes it"
        assert hasattr(C.CDLL(path), "rr_sac_act"), path


def test_integration_notes_name_the_entry():
    with open(os.path.join(ol.REPO, "INTEGRATION.md")) as f:
        text = f.read()
    assert "rr_sac_act" in text and "RR_SAC_DETERMINISTIC" in text


def test_package_exports_the_agent():
    pytest.importorskip("torch")
    import roborugby_amd as rr
    from roborugby_amd import sac
    assert rr.BatchedSACAgent is sac.BatchedSACAgent and "BatchedSACAgent" in rr.__all__
