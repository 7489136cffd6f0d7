"""engines.capture: graph captures run with the cyclic garbage collector out of the way.  A dropped engine and its
graph programs refer to each other; were the collector to find them in the middle of a capture, their device frees
and graph destruction would be refused by the runtime there and abort the process.  The guard itself needs no GPU:
the capture context manager is replaced by a recorder."""
import contextlib
import gc
import weakref

import torch

import shai_amd.engines as engines


class _Node:
    pass


def test_capture_collects_first_and_keeps_the_collector_off(monkeypatch):
    seen = {}

    @contextlib.contextmanager
    def fake_graph(graph, **kw):
        seen["enter"] = (gc.isenabled(), ref() is None, kw)
        yield
        seen["exit"] = gc.isenabled()

    monkeypatch.setattr(torch.cuda, "graph", fake_graph)
    gc.collect()
    was = gc.isenabled()
    gc.disable()          # (so that the cycle below is certainly still there when capture() starts)
    try:
        a, b = _Node(), _Node()
        a.other, b.other = b, a
        ref = weakref.ref(a)
        del a, b
        assert ref() is not None
        gc.enable()
        with engines.capture(object(), pool=None):
            assert not gc.isenabled()
        assert gc.isenabled()
    finally:
        gc.enable() if was else gc.disable()
    # the dead cycle went before the capture began, the collector stayed off to its end
    assert seen["enter"] == (False, True, {"pool": None}) and seen["exit"] is False


def test_capture_leaves_a_disabled_collector_disabled_and_survives_errors(monkeypatch):
    @contextlib.contextmanager
    def fake_graph(graph, **kw):
        yield

    monkeypatch.setattr(torch.cuda, "graph", fake_graph)
    was = gc.isenabled()
    try:
        gc.disable()
        with engines.capture(object()):
            pass
        assert not gc.isenabled()
        gc.enable()
        try:
            with engines.capture(object()):
                raise RuntimeError("capture failed")
        except RuntimeError:
            pass
        assert gc.isenabled()
    finally:
        gc.enable() if was else gc.disable()


def test_every_engine_captures_through_the_guard():
    import inspect
    import shai_amd.engines.diffusion as d
    import shai_amd.engines.encoders as e
    import shai_amd.engines.flux as f
    import shai_amd.engines.llm as l
    for mod in (d, e, f, l):
        src = inspect.getsource(mod)
        assert "torch.cuda.graph(" not in src and "capture(" in src, mod.__name__
