"""rr_sac_targets' place in the C-ABI: the struct and the entry declared in include/roborugby_amd.h with the specification in the comment,
mirrored in _lib (SYMBOLS, the ctypes struct, DqnHandle.sac_targets), exported by the built libraries, named in INTEGRATION.md.  CPU only."""
import ctypes as C
import os
import re

import pytest

import oracle_lib as ol

HEADER = os.path.join(ol.REPO, "include", "roborugby_amd.h")
FIELDS = ["struct_size", "batch", "n_actions", "flags", "actor", "critic_1", "critic_2", "target_value", "state_memory", "new_state_memory",
          "action_memory", "reward_memory", "terminal_memory", "mem_rows", "batch_index", "noise", "max_action", "gamma", "reward_scale", "seed",
          "call", "value_target", "q_hat", "state", "action", "policy_action", "log_prob", "head", "noise_out", "q1", "q2", "v_next"]


def _header():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_struct_and_the_entry():
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int rr_sac_targets\(\s*rr_dqn \*dqn,\s*const rr_sac_targets_args \*args,\s*void \*stream\);", code)
    m = re.search(r"typedef struct rr_sac_targets_args \{(.*?)\} rr_sac_targets_args;", code, re.S)
    assert m, "rr_sac_targets_args is not declared"
    names = []
    for stmt in m.group(1).split(";"):
        stmt = " ".join(stmt.split())
        if stmt:
            names += [re.sub(r"\[\d+\]", "", part).split()[-1].lstrip("*") for part in stmt.split(",")]
    assert names == FIELDS
    assert re.search(r"^#define RR_ABI_VERSION 4\b", code, re.M)  # additive
    for word in ("0x5A7A", "0x5AC7", "batch_index", "never used as an", "NaN", "fminf(q1, q2) - log_prob", "bit-identical", "RR_DQN_WGS",
                 "rr_dqn_last_error", "multiple of 64", "BATCH POSITION"):  # the comment is the specification
        assert word in text, word


def test_symbols_and_struct_mirror_the_declaration():
    torch = pytest.importorskip("torch")  # noqa: F841  (_lib imports it first)
    from roborugby_amd import _lib
    res, args = _lib.SYMBOLS["rr_sac_targets"]
    assert res is C.c_int and args[0] is C.c_void_p and args[2] is C.c_void_p and args[1]._type_ is _lib.RRSacTargetsArgs
    S = _lib.RRSacTargetsArgs
    assert [f[0] for f in S._fields_] == FIELDS
    assert S.actor.size == 64 and S.critic_1.size == S.critic_2.size == S.target_value.size == 48
    assert S.mem_rows.offset % 8 == 0 and S.seed.offset % 8 == 0 and S.value_target.offset % 8 == 0
    assert C.sizeof(S) == 408  # what a C compiler gives the declaration on an LP64 target
    assert hasattr(_lib.DqnHandle, "sac_targets")


def test_built_libraries_export_it():
    pytest.importorskip("torch")
    from roborugby_amd import _lib, build  # noqa: F401  (_lib: torch's HIP runtime is loaded before the library's)
    for path in (build.LIB, build.LIB_EXACT, build.shape_lib_path(2, 1, 2, 3)):
        assert os.path.exists(path), f"{path}: __graft_entry__.build() makes it"
        assert hasattr(C.CDLL(path), "rr_sac_targets"), path


def test_struct_size_matches_a_c_compiler(tmp_path):
    import subprocess
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "roborugby_amd.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(rr_sac_targets_args), '
                   '__builtin_offsetof(rr_sac_targets_args, seed), __builtin_offsetof(rr_sac_targets_args, value_target)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["g++", "-x", "c", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    pytest.importorskip("torch")
    from roborugby_amd import _lib
    S = _lib.RRSacTargetsArgs
    assert subprocess.check_output([str(exe)], text=True).split() == [str(C.sizeof(S)), str(S.seed.offset), str(S.value_target.offset)]


def test_integration_notes_name_the_entry():
    with open(os.path.join(ol.REPO, "INTEGRATION.md")) as f:
        text = f.read()
    assert "rr_sac_targets" in text and "rr_sac_targets_args" in text


def test_stream_word_is_listed_next_to_the_others():
    with open(os.path.join(ol.REPO, "roborugby_amd", "csrc", "rr_sac.hpp")) as f:
        text = f.read()
    assert re.search(r"SAC_TARGETS_STREAM = 0x5A7Au", text) and "uint32_t stream = SAC_STREAM" in text
