"""The one builder of the host-emulation harness (tests/emu_build.py): staleness goes by content and not by file times, the hashed
dependency set covers every file a library's source includes, and every registered library builds, loads and exports what its Python
side binds.  CPU only."""
import ctypes as C
import os
import subprocess

import pytest

import emu_build as eb
import emu_lib
import frames_emu_lib
import hive_emu_lib
import hive_held_emu_lib
import hive_transition_lib
import render_ego_emu_lib
import render_emu_lib


def test_staleness_goes_by_content_not_by_time(tmp_path):
    src, hdr = tmp_path / "answer.cpp", tmp_path / "answer.hpp"
    hdr.write_text("#define ANSWER 41\n")
    src.write_text('#include "answer.hpp"\nextern "C" int answer() { return ANSWER + BIAS; }\n// (three lines)\n')
    lib = eb.Lib(str(src), "libanswer.so", ("-O2", "-DBIAS=0"), ("answer",))
    assert eb.is_stale(lib)
    assert eb.build(lib) == str(tmp_path / "libanswer.so") and not eb.is_stale(lib)
    assert C.CDLL(lib.so).answer() == 41
    built = os.stat(lib.so).st_mtime_ns
    for k, f in enumerate((src, hdr, tmp_path / "libanswer.so")):  # sources newer than the library, and all of them in the future
        os.utime(f, ns=(built + (5 - k) * 10 ** 12,) * 2)
    moved = os.stat(lib.so).st_mtime_ns
    assert moved > built and os.stat(src).st_mtime_ns > moved
    assert not eb.is_stale(lib)
    assert eb.build(lib) == lib.so and os.stat(lib.so).st_mtime_ns == moved  # (not rebuilt)
    hdr.write_text("#define ANSWER 42\n")  # one byte of the header
    assert eb.is_stale(lib)
    eb.build(lib)
    assert not eb.is_stale(lib)
    flagged = lib._replace(flags=("-O2", "-DBIAS=1"))
    assert eb.is_stale(flagged)
    eb.build(flagged)
    assert not eb.is_stale(flagged) and eb.is_stale(lib)
    # (a library that is loaded stays mapped under its path: read the rebuilt one through a copy)
    copy = tmp_path / "rebuilt.so"
    copy.write_bytes((tmp_path / "libanswer.so").read_bytes())
    assert C.CDLL(str(copy)).answer() == 43
    assert not [f for f in os.listdir(tmp_path) if ".tmp" in f]


def test_a_stale_library_without_a_compiler_is_an_error_that_names_it(tmp_path, monkeypatch):
    src = tmp_path / "answer.cpp"
    src.write_text('extern "C" int answer() { return 1; }\n')
    lib = eb.Lib(str(src), "libanswer.so", ("-O2",))
    monkeypatch.setenv("PATH", str(tmp_path))
    with pytest.raises(RuntimeError, match="libanswer.so"):
        eb.build(lib)


@pytest.mark.parametrize("name", sorted(eb.LIBS))
def test_hashed_dependencies_cover_what_the_source_includes(name):
    """g++ -MM with the library's own defines: every non-system file it names lies in the hashed set (rr_emu.cpp's rr_extras.hpp was
    missing from the hand-kept list this replaced)"""
    lib = eb.LIBS[name]
    out = subprocess.check_output(["g++", *lib.flags, "-MM", lib.source], text=True)
    named = {os.path.realpath(f) for f in out.replace("\\\n", " ").split()[1:]}
    hashed = {os.path.realpath(f) for f in eb.deps(lib)}
    assert os.path.realpath(lib.source) in named and len(named) > 1
    assert named <= hashed, sorted(named - hashed)


def test_every_registered_library_builds_loads_and_exports_its_entries():
    assert eb.build_all() == [lib.so for lib in eb.LIBS.values()]
    assert len({lib.so for lib in eb.LIBS.values()}) == len(eb.LIBS)
    for name, lib in eb.LIBS.items():
        assert not eb.is_stale(lib), name
        assert lib.exports, name
        loaded = eb.load(lib)
        assert eb.load(lib) is loaded  # cached
        for entry in lib.exports:
            assert hasattr(loaded, entry), (name, entry)
    # the bindings themselves: each sets the argument types of the entries it calls, which fails on a missing one
    for bind in (lambda: emu_lib.lib(False), lambda: emu_lib.lib(True), hive_emu_lib.lib, hive_held_emu_lib.lib, hive_transition_lib.lib,
                 render_emu_lib.lib, render_ego_emu_lib.lib, frames_emu_lib.lib):
        assert bind() is not None
    assert hive_held_emu_lib.lib() is hive_emu_lib.lib()  # the held-row entries live in the hive's library
