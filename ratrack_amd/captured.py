"""Warm-up, capture and replay of a step whose launches are recorded in hipGraphs -- the state machine that `train.Trainer` and
`tracker.BatchedTracker` share.  Nothing here touches the device: how a capture is made (one graph or two, what is allocated before
it) and what a replay consists of (what runs between or after the graphs) belong to the caller's callbacks."""
import torch


def signature(tensors):
    """The key of a flat list of tensors (entries may be None): their shapes and dtypes."""
    return tuple(None if t is None else (tuple(t.shape), t.dtype) for t in tensors)


def capture_graph(fn):
    """fn() recorded into a new hipGraph -> (graph, fn's return value)."""
    g = torch.cuda.CUDAGraph()
    import torch.distributed as dist
    # with a process group alive, its watchdog thread polls events while we capture: only this thread's calls may
    # invalidate the capture
    mode = "thread_local" if dist.is_available() and dist.is_initialized() else "global"
    with torch.cuda.graph(g, capture_error_mode=mode):
        out = fn()
    return g, out


class CapturedStep:
    """step = CapturedStep(warmup, copy);  out = step(key, args, eager, capture)

    The first `warmup` calls under a key return eager(args): real steps on the caller's tensors.  The next one clones `args` into
    static buffers and calls capture(static) -> (out, replay) once; it and every later call run copy([(static, arg), ...]) over the
    entries that are not None, then replay(), and return `out`.  One slot: a new key forgets the graph, the statics and the warm-up
    count.  A capture that raises leaves no graph behind, and the next call with that key captures again.
    Read only: `captured` (the last call was a replay), `ready` (a graph exists for the current key), `warmups` (eager steps taken
    under the current key)."""

    def __init__(self, warmup, copy):
        self._warm, self._copy = int(warmup), copy
        self._key = self._static = self._out = self._replay = None
        self.captured, self.warmups = False, 0

    @property
    def ready(self):
        return self._replay is not None

    def __call__(self, key, args, eager, capture):
        if key != self._key:
            self._key, self._static, self._out, self._replay, self.warmups = key, None, None, None, 0
        self.captured = False
        if not self.ready and self.warmups < self._warm:
            self.warmups += 1
            return eager(args)
        if not self.ready:
            static = [None if t is None else t.clone(memory_format=torch.contiguous_format) for t in args]
            self._out, self._replay = capture(static)
            self._static = static
        self._copy([(dst, src) for dst, src in zip(self._static, args) if dst is not None])
        self._replay()
        self.captured = True
        return self._out
