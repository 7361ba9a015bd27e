"""The checked-call path of the Python binding (roborugby_amd/_lib.py: EnvHandle.call / .launch, ptr) against a stand-in library: no GPU,
no compiled code."""
import pytest

torch = pytest.importorskip("torch")

from roborugby_amd import _lib  # noqa: E402


class StandIn:
    """a library whose rr_* entries record their arguments and return `rc`"""

    def __init__(self, rc=0, message=b"rr_thing: the stand-in says no"):
        self.rc, self.message, self.calls = rc, message, []

    def __getattr__(self, name):
        if not name.startswith("rr_"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or self.rc

    def rr_last_error(self):
        return self.message


def _handle(rc=0):
    lib = StandIn(rc)
    return lib, _lib.EnvHandle(lib, 1234, torch.device("cpu"))


def test_a_call_that_returns_zero_gives_none_and_passes_the_handle_first():
    lib, h = _handle()
    assert h.call("rr_thing", 5, None, "x") is None
    assert lib.calls == [("rr_thing", (1234, 5, None, "x"))]


def test_the_stream_is_appended_exactly_when_asked_for(monkeypatch):
    lib, h = _handle()
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device: type("S", (), {"cuda_stream": 77, "device": device}))
    h.call("rr_thing", 1, 2)
    h.launch("rr_thing", 1, 2)
    (_, plain), (_, launched) = lib.calls
    assert plain == (1234, 1, 2)
    assert launched[:3] == (1234, 1, 2) and len(launched) == 4 and launched[3].value == 77
    assert h.stream().value == 77 and _lib.current_stream(torch.device("cpu")).value == 77


@pytest.mark.parametrize("method", ["call", "launch"])
def test_a_failure_names_the_symbol_called_the_code_and_the_librarys_message(method, monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device: type("S", (), {"cuda_stream": 0}))
    lib, h = _handle(rc=-3)
    with pytest.raises(_lib.RRError) as e:
        getattr(h, method)("rr_other_f64", 1)
    text = str(e.value)
    assert "rr_other_f64" in text and "-3" in text and "the stand-in says no" in text
    assert lib.calls[0][0] == "rr_other_f64"


def test_close_destroys_once_and_leaves_no_handle():
    lib, h = _handle()
    h.close()
    h.close()
    assert lib.calls == [("rr_destroy", (1234,))] and h.h is None


def test_ptr():
    assert _lib.ptr(None) is None
    t = torch.arange(8, dtype=torch.int32)
    assert _lib.ptr(t).value == t.data_ptr() and _lib.ptr(t, 12).value == t.data_ptr() + 12
