"""hipGraph capture and replay (and the hipEvent timer): capture() is the package's one fork-capture-join block, ReplayGraph and
PooledGraph are its two replay policies. ops re-exports Graph, PooledGraph and Timer."""
import ctypes as C
import gc
import threading

import torch

from . import _lib as L


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class Graph:
    """hipGraph captured from whatever runs on the current stream inside the `with` block."""

    def __init__(self):
        self.handle = C.c_void_p()
        self.stream = None

    def __enter__(self):
        self.stream = _stream()
        # no cyclic collection inside the capture: garbage that owns device memory (a torch.cuda.MemPool behind a reference cycle, as
        # PooledGraph's in the verifier) frees it in its destructor, and a hipFree on the capturing thread aborts the process
        self._gc = gc.isenabled()
        gc.disable()
        try:
            L.check(L.lib().cover_graph_begin(self.stream), "graph_begin")
        except BaseException:
            self._gc and gc.enable()
            raise
        return self

    def __exit__(self, et, ev, tb):
        rc = L.lib().cover_graph_end(self.stream, C.byref(self.handle))
        if self._gc:
            gc.enable()
        if et is None:
            L.check(rc, "graph_end")
        return False

    def launch(self):
        L.check(L.lib().cover_graph_launch(self.handle, _stream()), "graph_launch")


# One capture stream per device and host thread, created on first use. Per thread: captures are thread-local and two host threads capture
# (the policy's graphs on the main one, the verifier's PooledGraph on the one that queues the towers), which one stream cannot serve at once.
_capture_streams = {}


def capture(fn, device):
    """Record fn()'s launches into a Graph on the capture stream, forked from the current stream and joined back to it. Launches nothing.
    -> (Graph, what fn returned under capture)."""
    key = (torch.device(device), threading.get_ident())
    if key not in _capture_streams:
        _capture_streams[key] = torch.cuda.Stream(device=device)
    cap, cur = _capture_streams[key], torch.cuda.current_stream()
    cap.wait_stream(cur)
    with torch.cuda.stream(cap):
        with Graph() as g:
            out = fn()
    cur.wait_stream(cap)
    return g, out


class ReplayGraph:
    """A launch sequence on static buffers: run eagerly once, then captured, then replayed for as long as the captured pointers stay valid.
    body: no arguments, launches only. gen: no arguments, the generation of whatever those pointers depend on (a workspace's ws_gen);
    None = never stale. A graph replayed over a moved workspace writes through a freed pointer, so run() compares the generation with the
    one stored at capture (self.gen) before every launch. A body that raises leaves no graph and no generation behind."""

    def __init__(self, body, device, gen=None):
        self.body, self.dev, self._gen_of = body, device, gen or (lambda: None)
        self._graph = self.gen = None

    @property
    def captured(self) -> bool:
        return self._graph is not None

    def run(self):
        if self.captured and self._gen_of() != self.gen:
            self._graph = self.gen = None                      # stale: capture again
        if self.captured:
            return self._graph.launch()
        self.body()                                            # eager: this call's results (it also sizes every workspace)
        gen = self._gen_of()                                   # after the eager pass, which is what may have moved a workspace
        self._graph, _ = capture(self.body, self.dev)
        self.gen = gen


class PooledGraph:
    """A launch sequence that ALLOCATES its intermediates (ordinary op wrappers) as one replayable hipGraph.

    call 1 runs `fn()` eagerly inside a private torch memory pool (this sizes every intermediate and leaves their blocks in the pool),
    call 2 captures it inside the same pool (every allocation is served from the pool's cache: no hipMalloc under capture), later calls
    replay. The pool belongs to this object alone, so the blocks the captured kernels write to are never handed to anybody else between
    replays. `fn` takes no arguments: it reads static input tensors the caller refreshes before every call, and returns tensors that stay
    valid (static) from the capture on. Streams that `fn` forks to and joins from become parallel branches of the graph."""

    def __init__(self, fn, device):
        self.fn, self.dev = fn, device
        self.pool = torch.cuda.MemPool()
        self.graph, self.out, self.calls = None, None, 0

    def __call__(self):
        self.calls += 1
        if self.graph is None:
            with torch.cuda.use_mem_pool(self.pool, device=self.dev):
                if self.calls == 1:
                    # (this call's outputs live in the pool until the caller drops them; the capture of call 2 then allocates its own)
                    return self.fn()
                self.graph, self.out = capture(self.fn, self.dev)    # executes nothing: the launch below is this call's run
        self.graph.launch()
        return self.out


class Timer:
    """hipEvent pair recorded on the current stream."""

    def __init__(self):
        self.h = C.c_void_p()
        L.check(L.lib().cover_timer_create(C.byref(self.h)), "timer_create")

    def start(self):
        L.check(L.lib().cover_timer_start(self.h, _stream()), "timer_start")

    def stop(self) -> float:
        ms = C.c_float()
        L.check(L.lib().cover_timer_stop(self.h, _stream(), C.byref(ms)), "timer_stop")
        return ms.value
