"""graphs.ReplayGraph's policy on the host (no GPU): eager once, then captured; replayed until the generation moves; nothing kept from a
body that raised. graphs.capture is replaced by a fake that calls fn once and returns an object counting its launches."""
import pytest


class _FakeGraph:
    def __init__(self):
        self.launches = 0

    def launch(self):
        self.launches += 1


class _Rig:
    """A counting body, a mutable generation and the fake capture. body call `fail_on` (1-based, counted per run() through `in_run`) raises;
    the first body call ever bumps the generation, as an eager pass that grows a workspace does."""

    def __init__(self, monkeypatch, gen=True):
        from cover_vla_amd import graphs
        self.calls, self.in_run, self.fail_on, self.generation, self.graphs = 0, 0, None, [0], []
        monkeypatch.setattr(graphs, "capture", self.capture)
        self.rg = graphs.ReplayGraph(self.body, "cpu", gen=(lambda: self.generation[0]) if gen else None)

    def body(self):
        self.calls += 1
        self.in_run += 1
        if self.calls == 1:
            self.generation[0] += 1
        if self.in_run == self.fail_on:
            raise RuntimeError("body failed")

    def capture(self, fn, device):
        g = _FakeGraph()
        self.graphs.append(g)
        return g, fn()

    def run(self, fail_on=None):
        """-> (body calls, launches) of this run()."""
        self.in_run, self.fail_on = 0, fail_on
        calls, launches = self.calls, self.launches
        self.rg.run()
        return self.calls - calls, self.launches - launches

    @property
    def launches(self):
        return sum(g.launches for g in self.graphs)


def test_first_run_is_eager_then_captured_and_later_runs_replay(monkeypatch):
    r = _Rig(monkeypatch)
    assert not r.rg.captured and r.rg.gen is None
    assert r.run() == (2, 0)                               # eager, then under capture; nothing launched
    assert r.rg.captured and r.rg.gen == 1 == r.generation[0]   # the generation read AFTER the eager pass, which bumped it
    assert r.run() == (0, 1) and r.run() == (0, 1)         # replays, no re-capture
    assert len(r.graphs) == 1


def test_a_moved_generation_drops_the_graph_and_captures_again(monkeypatch):
    r = _Rig(monkeypatch)
    r.run(), r.run()
    r.generation[0] = 7
    assert r.run() == (2, 0)
    assert r.rg.captured and r.rg.gen == 7 and len(r.graphs) == 2
    assert r.run() == (0, 1)
    assert (r.graphs[0].launches, r.graphs[1].launches) == (1, 1)   # the stale graph is never launched again


def test_without_a_generation_the_graph_is_never_stale(monkeypatch):
    r = _Rig(monkeypatch, gen=False)
    assert r.run() == (2, 0) and r.rg.captured and r.rg.gen is None
    r.generation[0] = 7
    assert r.run() == (0, 1) and r.run() == (0, 1) and len(r.graphs) == 1


@pytest.mark.parametrize("fail_on", [1, 2], ids=["eager", "under_capture"])
@pytest.mark.parametrize("held", [False, True], ids=["first_capture", "re_capture"])
def test_a_body_that_raises_leaves_nothing_behind(monkeypatch, fail_on, held):
    r = _Rig(monkeypatch)
    if held:                                               # a stale graph must not survive the failed re-capture either
        r.run()
        r.generation[0] = 7
    with pytest.raises(RuntimeError, match="body failed"):
        r.run(fail_on=fail_on)
    assert not r.rg.captured and r.rg.gen is None
    assert r.run() == (2, 0)                               # the next run() starts over
    assert r.rg.captured and r.rg.gen == r.generation[0]
    assert r.run() == (0, 1)
