"""rr_sac_grads' place in the C-ABI: the struct and the entry declared in include/roborugby_amd.h with the specification in the comment,
mirrored in _lib (SYMBOLS, the ctypes struct, DqnHandle.sac_grads), exported by the built libraries, named in INTEGRATION.md; the agent's
fused_grads keyword refuses a CPU device.  CPU only."""
import ctypes as C
import os
import re

import pytest

import oracle_lib as ol

HEADER = os.path.join(ol.REPO, "include", "roborugby_amd.h")
FIELDS = ["struct_size", "batch", "n_actions", "flags", "value", "critic_1", "critic_2", "state", "action", "value_target", "q_hat",
          "grad_value", "grad_critic_1", "grad_critic_2", "loss"]


def _header():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_struct_and_the_entry():
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int rr_sac_grads\(\s*rr_dqn \*dqn,\s*const rr_sac_grads_args \*args,\s*void \*stream\);", code)
    m = re.search(r"typedef struct rr_sac_grads_args \{(.*?)\} rr_sac_grads_args;", code, re.S)
    assert m, "rr_sac_grads_args is not declared"
    names = []
    for stmt in m.group(1).split(";"):
        stmt = " ".join(stmt.split())
        if stmt:
            names += [re.sub(r"\[\d+\]", "", part).split()[-1].lstrip("*") for part in stmt.split(",")]
    assert names == FIELDS
    assert re.search(r"^#define RR_ABI_VERSION 4\b", code, re.M)  # additive
    spec = text[text.index("k_sac_grads"):text.index("typedef struct rr_sac_grads_args")]
    for word in ("Training_SAC_pytorch.py:344-383", "(f_b - y_b) / B", "0.5 * mean", "loss[1] + loss[2]", "h > 0", "bit-identical", "RR_DQN_WGS",
                 "NOT promised identical across grid sizes", "NaN", "rr_dqn_last_error", "multiple of 64", "no atomics",
                 "Every element of every output is written"):  # the comment is the specification
        assert word in spec, word


def test_symbols_and_struct_mirror_the_declaration():
    torch = pytest.importorskip("torch")  # noqa: F841  (_lib imports it first)
    from roborugby_amd import _lib
    res, args = _lib.SYMBOLS["rr_sac_grads"]
    assert res is C.c_int and args[0] is C.c_void_p and args[2] is C.c_void_p and args[1]._type_ is _lib.RRSacGradsArgs
    S = _lib.RRSacGradsArgs
    assert [f[0] for f in S._fields_] == FIELDS
    assert all(getattr(S, k).size == 48 for k in ("value", "critic_1", "critic_2", "grad_value", "grad_critic_1", "grad_critic_2"))
    assert S.value.offset == 16 and S.state.offset % 8 == 0 and S.loss.offset == C.sizeof(S) - 8
    assert C.sizeof(S) == 344  # what a C compiler gives the declaration on an LP64 target
    assert hasattr(_lib.DqnHandle, "sac_grads")


def test_built_libraries_export_it():
    pytest.importorskip("torch")
    from roborugby_amd import _lib, build  # noqa: F401  (_lib: torch's HIP runtime is loaded before the library's)
    for path in (build.LIB, build.LIB_EXACT, build.shape_lib_path(2, 1, 2, 3)):
        assert os.path.exists(path), f"{path}: __graft_entry__.build() makes it"
        assert hasattr(C.CDLL(path), "rr_sac_grads"), path


def test_struct_size_matches_a_c_compiler(tmp_path):
    import subprocess
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "roborugby_amd.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(rr_sac_grads_args), '
                   '__builtin_offsetof(rr_sac_grads_args, state), __builtin_offsetof(rr_sac_grads_args, grad_value), '
                   '__builtin_offsetof(rr_sac_grads_args, loss)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["g++", "-x", "c", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    pytest.importorskip("torch")
    from roborugby_amd import _lib
    S = _lib.RRSacGradsArgs
    assert subprocess.check_output([str(exe)], text=True).split() == [str(C.sizeof(S)), str(S.state.offset), str(S.grad_value.offset),
                                                                      str(S.loss.offset)]


def test_integration_notes_name_the_entry():
    with open(os.path.join(ol.REPO, "INTEGRATION.md")) as f:
        text = f.read()
    assert "rr_sac_grads" in text and "rr_sac_grads_args" in text


def test_fused_grads_needs_a_gpu():
    pytest.importorskip("torch")
    from roborugby_amd.sac import BatchedSACAgent
    with pytest.raises(ValueError, match="fused_grads"):
        BatchedSACAgent(n_actions=2, max_mem_size=64, batch_size=64, device="cpu", fused=False, fused_grads=True)
    ag = BatchedSACAgent(n_actions=2, max_mem_size=64, batch_size=64, device="cpu", fused=False)  # the default: off
    assert ag.fused_grads is False
    ag.close()
