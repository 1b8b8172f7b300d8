"""ops.Graph keeps Python's cyclic collector off for the length of a capture (host side, no GPU): a collection inside the window can run
destructors that free device memory, which the runtime refuses on a capturing thread."""
import gc

import pytest


class _FakeLib:
    def __init__(self, begin_rc=0):
        self.begin_rc, self.inside = begin_rc, []

    def cover_graph_begin(self, stream):
        return self.begin_rc

    def cover_graph_end(self, stream, handle):
        self.inside.append(gc.isenabled())
        return 0


def test_graph_capture_runs_with_the_collector_off_and_restores_it(monkeypatch):
    from cover_vla_amd import graphs, ops
    fake = _FakeLib()
    monkeypatch.setattr(graphs.L, "lib", lambda: fake)
    monkeypatch.setattr(graphs, "_stream", lambda: 0)       # ops.Graph is graphs.Graph: it reads its stream there
    assert gc.isenabled()
    with ops.Graph():
        assert not gc.isenabled()
    assert gc.isenabled() and fake.inside == [False]
    with pytest.raises(RuntimeError):                      # an error inside the block still ends the capture and restores the collector
        with ops.Graph():
            raise RuntimeError("body failed")
    assert gc.isenabled()
    gc.disable()                                           # a caller that runs with the collector off keeps it off
    try:
        with ops.Graph():
            assert not gc.isenabled()
        assert not gc.isenabled()
    finally:
        gc.enable()
    fake.begin_rc = 1                                      # a capture that does not begin leaves the collector as it was
    with pytest.raises(ops.L.CoverError):
        ops.Graph().__enter__()
    assert gc.isenabled()
