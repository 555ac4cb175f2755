"""A launch sequence as ONE replayed hipGraph: the capture-and-replay driver of every hot path (CapturedStep: the decoders' train steps,
SURVEY 8a, text_generation_model.py:425-438 and text_generation_model_v2.py:262-287; the joint model's step behind the encoder; the
encoder pass, whole or as trunk + top) and the joint model's choice between replaying and issuing eagerly (PathChooser).

The decoder-only configurations (BASELINE configs[0] / configs[1]) are chains of 60 - 150 kernels of 5 - 20 us each: issued one by one
from Python the host is the bottleneck (10 us per launch through ctypes), not the GPU.  Here the step is enqueued once into a hipGraph
-- forward, loss, backward, the optimizer's launch (ops.amsgrad_step, or ops.optimizer_step
for Adam without amsgrad and SGD) -- and replayed; what changes from step to step reaches the kernels through persistent device
buffers:

  * PackedInputs: the host's per-step words (token ids, masks, targets, index tables, Keras' lr_t, the dropout stream position) packed
    into ONE buffer and moved with ONE asynchronous copy from a small ring of page-locked buffers;
  * the RoI features: copied into a persistent device tensor (device -> device, or one upload when the caller holds them on the host).

Values that Python computed while the capture ran (optimizer.iterations, the dropout step counter) are advanced by hand on every replay.
Replays are bit-identical to the eager step: the same launches with the same arguments (tests/test_gpu_models.py).
"""
import os
import warnings

import numpy as np
import torch

from . import ops


def enabled():
    """DCAP_STEP_GRAPH=0 issues every step eagerly (the same launches, one by one)."""
    return os.environ.get("DCAP_STEP_GRAPH", "1") != "0"


class PackedInputs(object):
    """Per-step host inputs as 4-byte words in ONE persistent device buffer, filled by ONE asynchronous copy per step.
    sizes: [(key, n_words)]; every part starts 16-byte aligned.  The device side has fixed addresses (a captured hipGraph replays
    them); the host side is a ring of page-locked buffers, each guarded by the event of its last copy, so the host never waits for the
    device and never rewrites a buffer whose copy is still queued."""
    SLOTS = 4

    def __init__(self, device, sizes):
        self.off, pos = {}, 0
        for k, n in sizes:
            self.off[k] = (pos, int(n))
            pos += (int(n) + 3) // 4 * 4
        self.words = max(pos, 4)
        self.dev = torch.zeros(self.words, dtype=torch.int32, device=device)
        self.pins = [torch.zeros(self.words, dtype=torch.int32, pin_memory=True) for _ in range(self.SLOTS)]
        self.events = [None] * self.SLOTS
        self.k = 0

    def view(self, key, dtype=torch.int32):
        o, n = self.off[key]
        v = self.dev[o:o + n]
        return v if dtype == torch.int32 else v.view(dtype)

    def bytes_view(self, key, nbytes):
        """The first nbytes of a part as uint8 (Keras masks travel as bytes)."""
        o, n = self.off[key]
        if nbytes > 4 * n:
            raise ValueError("%s: %d bytes do not fit the %d reserved" % (key, nbytes, 4 * n))
        return self.dev[o:o + n].view(torch.uint8)[:nbytes]

    def upload(self, parts):
        """parts: {key: numpy array of int32 / float32 / uint32 words, or uint8 bytes}; missing keys are zero."""
        k = self.k
        self.k = (k + 1) % self.SLOTS
        if self.events[k] is not None:
            self.events[k].synchronize()                    # (SLOTS steps old: complete long ago unless the host runs far ahead)
        host = self.pins[k].numpy()
        host[:] = 0
        for key, a in parts.items():
            o, n = self.off[key]
            a = np.ascontiguousarray(a).reshape(-1)
            if a.dtype == np.uint8 or a.dtype == np.bool_:
                if a.size > 4 * n:
                    raise ValueError("%s: %d bytes do not fit the %d reserved" % (key, a.size, 4 * n))
                host[o:o + n].view(np.uint8)[:a.size] = a.view(np.uint8)
                continue
            if a.size > n:
                raise ValueError("%s: %d words do not fit the %d reserved" % (key, a.size, n))
            if a.dtype.itemsize != 4:
                raise TypeError("%s: 4-byte words expected, got %s" % (key, a.dtype))
            host[o:o + a.size] = a if a.dtype == np.int32 else a.view(np.int32)
        self.dev.copy_(self.pins[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[k] = ev


class CapturedStep(object):
    """ONE launch sequence as a replayed hipGraph -- a model's train step for one batch shape, an encoder pass or one half of it: eager
    calls first (they size every buffer and workspace), then a capture, then replays.  The only place of the package that builds,
    captures and replays a graph.  What a captured step holds for as long as its graph exists: the graph, the body's outputs, every
    scratch buffer ops.WORKSPACE handed out during the capture (`kept`: {(device, stream handle): [buffers]} -- the capture stream's
    and those of streams the capture pulled in; a later, larger request on one of those streams replaces WORKSPACE's entry, not the
    memory the graph's launches point into) and `bufs`, a scratch-buffer dictionary private to this step that a model swaps in around
    run(), so that another batch shape or a predict() call in between can never free a buffer whose address the graph has baked."""

    def __init__(self):
        self.graph = None
        self.out = None
        self.warm = 0
        self.bufs = {}
        self.kept = {}
        self.failed = None            # the error text when the capture failed: this step then stays eager
        self.last = None              # what the last run() did: "eager" | "capture" | "replay"

    def run(self, body, counters_get=None, counters_set=None, on_replay=None, warm_calls=2, propagate=False, on_failure=None):
        """body(): enqueue the launches, return the output tensor(s).  The first warm_calls calls run it eagerly, the next one captures
        it (and replays once: that call's work), later ones replay.  counters_get() / counters_set(v): the host-side counters body()
        advances (restored when a capture fails, since the eager retry advances them again); on_replay(): advance them by one step.
        A capture that raises: warn, restore the counters, synchronise, on_failure(error text), run body() eagerly and stay eager --
        or, with propagate, raise (an encoder pass must not silently become a hundred eager launches)."""
        if self.graph is not None:
            self.last = "replay"
            self.graph.replay()
            if on_replay is not None:
                on_replay()
            return self.out
        self.last = "eager"
        if self.failed is not None or self.warm < warm_calls:
            self.warm += 1
            return body()
        saved = counters_get() if counters_get is not None else None
        try:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            # thread-local capture: the RCCL watchdog thread of a multi-GPU run polls events while this thread captures; under the
            # default (global) mode that would invalidate the capture
            with ops.no_gc_during_capture(), ops.WORKSPACE.handed_out() as kept, torch.cuda.graph(graph, capture_error_mode="thread_local"):
                out = body()
        except RuntimeError as e:                            # a capture error (torch raises RuntimeError)
            if propagate:
                raise
            warnings.warn("hipGraph capture failed (%s); running eagerly" % (repr(e)[:200],))
            self.failed = repr(e)[:200]
            if counters_set is not None:
                counters_set(saved)
            torch.cuda.synchronize()
            if on_failure is not None:
                on_failure(self.failed)
            return body()
        self.graph, self.out, self.kept, self.last = graph, out, kept, "capture"
        graph.replay()                                       # (a capture records, it does not run: this is the call's work itself)
        return out

    def drop(self):
        """Let go of the graph, then of what its launches point into: outputs, kept scratch buffers, the private buffers."""
        self.graph = None
        self.out = None
        self.kept = {}
        self.bufs = {}


def drop_all(steps):
    """drop() every CapturedStep of a dictionary (something they baked has moved); returns the empty dictionary that replaces it."""
    for cs in steps.values():
        cs.drop()
    return {}


class PathChooser(object):
    """Replay the captured step or issue its launches eagerly?  Automatic mode times SAMPLES steps of either path with event pairs
    around whole steps and keeps the faster one (the minimum of its samples; a tie keeps the graph).  pin() -- an explicit choice --
    ends the automatic mode.  decide() never waits: while the end event of a recorded pair has not completed it returns without
    deciding and is asked again at the start of the next step."""
    SAMPLES = 2

    def __init__(self, use_graph, auto):
        self.use_graph, self.auto = bool(use_graph), bool(auto)
        self.choice = None                                   # dict(eager_ms, graph_ms, kept) once the automatic choice has been made
        self._events = {"eager": [], "graph": []}

    def pin(self, use_graph):
        self.use_graph, self.auto = bool(use_graph), False

    def wants(self, kind):
        """Is a step of this kind ("eager" | "graph") still to be timed?"""
        return self.auto and self.use_graph and len(self._events[kind]) < self.SAMPLES

    def add(self, kind, start, end):
        self._events[kind].append((start, end))

    def decide(self):
        ev = self._events
        if not self.auto or any(len(v) < self.SAMPLES for v in ev.values()):
            return
        if not all(end.query() for v in ev.values() for _, end in v):
            return
        t = {k: min(a.elapsed_time(b) for a, b in v) for k, v in ev.items()}
        keep_graph = t["graph"] <= t["eager"]
        self.pin(keep_graph)
        self.choice = dict(eager_ms=round(t["eager"], 4), graph_ms=round(t["graph"], 4), kept="graph" if keep_graph else "eager")


def lr_word(opt):
    """The step word of the update the NEXT step ends with (t = iterations + 1; Adam / AMSGrad: Keras' lr_t = lr_d * sqrt(1 - b2^t) /
    (1 - b1^t), SGD: lr_d -- params.Optimizer.step_word), as the float32 word the eager launch would carry as its argument."""
    return np.array([opt.step_word(opt.iterations + 1)], np.float32)
