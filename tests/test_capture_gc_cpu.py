"""ops.CapturedGraph keeps Python's cyclic garbage collector off between begin() and end(): a collection inside a
capture would run finalizers of unreachable models (hipGraphExecDestroy, a device synchronize) that invalidate the
capture.  Checked without a GPU: the C entry points are replaced by a recorder."""
import gc

import pytest


@pytest.fixture
def recorder(monkeypatch):
    from arx import ops
    seen = []

    def fake_call(name, *args):
        seen.append((name, gc.isenabled()))
        if name == "arx_capture_end" and getattr(fake_call, "fail_end", False):
            raise RuntimeError("end failed")
        return 0
    monkeypatch.setattr(ops, "call", fake_call)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    return ops, seen, fake_call


def test_gc_is_off_inside_a_capture_and_restored(recorder):
    ops, seen, _ = recorder
    assert gc.isenabled()
    g = ops.CapturedGraph()
    g.begin()
    assert not gc.isenabled()
    g.end()
    assert gc.isenabled()
    assert seen == [("arx_capture_begin", False), ("arx_capture_end", False)]


def test_gc_restored_when_end_raises_and_left_off_if_it_was_off(recorder):
    ops, seen, fake_call = recorder
    g = ops.CapturedGraph()
    g.begin()
    fake_call.fail_end = True
    with pytest.raises(RuntimeError):
        g.end()
    assert gc.isenabled()
    fake_call.fail_end = False
    gc.disable()
    try:
        g = ops.CapturedGraph()
        g.begin()
        g.end()
        assert not gc.isenabled()                       # the caller's choice stands
    finally:
        gc.enable()
