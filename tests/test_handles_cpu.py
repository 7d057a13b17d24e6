"""The one close / __del__ of the handle classes (zkp_hip._Handle) against a recording stub in the library's place: no device, no
library needed."""
import ctypes as C

import pytest

import zkp_hip as zkp
from zkp_hip import nova

HANDLE_CLASSES = [zkp.G1Bases, zkp.PlonkTranscript, zkp.KzgOpener, zkp.KzgRecoverer, zkp.KzgCellVerifier, zkp.PlonkProver, nova.NovaR1CS,
                  nova.NovaTranscript]


class _Recorder:
    """Stands where the loaded library stands: every entry is callable and records (name, args); `fail` makes them raise."""

    def __init__(self, fail=False):
        self.calls, self.fail = [], fail

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            if self.fail:
                raise OSError("stub: " + name)
        return entry


@pytest.fixture
def stub(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(zkp, "lib", lambda: rec)
    return rec


def test_every_handle_class_is_listed():
    found = {c for mod in (zkp, nova) for c in vars(mod).values() if isinstance(c, type) and issubclass(c, zkp._Handle) and c is not zkp._Handle}
    assert found == set(HANDLE_CLASSES)
    own = [c.__name__ for c in HANDLE_CLASSES if "close" in vars(c) or "__del__" in vars(c)]
    assert own == [], "close and __del__ are _Handle's alone"


@pytest.mark.parametrize("cls", HANDLE_CLASSES, ids=lambda c: c.__name__)
def test_destroy_symbol_is_exported(cls):
    assert cls._destroy in zkp.exported_symbols()
    assert cls._destroy.endswith("_destroy")
    assert len({c._destroy for c in HANDLE_CLASSES}) == len(HANDLE_CLASSES)


@pytest.mark.parametrize("cls", HANDLE_CLASSES, ids=lambda c: c.__name__)
def test_close_without_a_handle_calls_nothing(cls, stub):
    never_assigned = object.__new__(cls)
    never_assigned.close()
    assert never_assigned._h is None
    null = object.__new__(cls)
    null._h = C.c_void_p()
    null.close()
    assert null._h is None
    del never_assigned, null
    assert stub.calls == []


@pytest.mark.parametrize("cls", HANDLE_CLASSES, ids=lambda c: c.__name__)
def test_close_destroys_once(cls, stub):
    obj = object.__new__(cls)
    obj._h = h = C.c_void_p(0x1000)
    obj.close()
    assert stub.calls == [(cls._destroy, (h,))]
    assert obj._h is None
    obj.close()
    del obj
    assert len(stub.calls) == 1


@pytest.mark.parametrize("cls", HANDLE_CLASSES, ids=lambda c: c.__name__)
def test_del_swallows_what_destroy_raises(cls, stub):
    stub.fail = True
    closed, dropped = object.__new__(cls), object.__new__(cls)
    closed._h, dropped._h = C.c_void_p(0x1000), C.c_void_p(0x2000)
    with pytest.raises(OSError):
        closed.close()
    dropped.__del__()
    assert [name for name, _ in stub.calls] == [cls._destroy] * 2
    assert closed._h is None and dropped._h is None  # neither is tried again
