"""include/rsu.h: "`stream` is a hipStream_t ... All calls are asynchronous on that stream and re-entrant per stream." on_stream() holds a
fenced case to the first half of that sentence, on a stream that is NOT the null stream and that is busy when the call is made.

A Gate is a device-side sleep of a known length on a stream with an event behind it: while the event has not fired the gate is closed,
and whatever was queued on that stream behind it has not run. Gated (a test_gpu_aligned_min.Recorder) puts a gate in front of every
library call, on the stream that is current at that moment, and notes after the call whether the gate was still closed. Torch's pool
streams are created non-blocking -- the null stream does not wait for them -- so under a gate:

  * an entry that waits for the device (a synchronising copy, a hipStreamSynchronize, a hipDeviceSynchronize) returns with its gate OPEN:
    GateOpen, an error class of its own, so that a gate that was too short is never taken for a wrong result nor the other way round;
  * a kernel of the entry that went to another stream runs at once, in front of everything still queued behind the gate. What it writes is
    lost: behind the gate, in front of the call, Gated writes every arena of the case back with the bytes it held in front of the gate
    (a copy of the arena onto itself in stream order: nothing for launches that keep to their stream; an Arena build ends with blocking
    copies from the host, so without this a first launch on the wrong stream would find its inputs ready and its output untouched).
    The case's own comparison or the byte comparison of on_stream then fails (StreamError, an AssertionError).

Gated also wraps fence_util.Arena.__init__ for the run (a gate in front of every arena build; restored in __exit__) and gates only the
calls `where` selects: "all", "main" (issued on the stream that was current when the run began) or "side" (on any other) -- the net-level
tests of tests/test_gpu_streams.py shift the two queues of the training step against each other with it.

Everything that touches the device goes through a Device object; tests/test_streams_host.py runs Gated and on_stream on CPU tensors with
a fake one (a library of Python callables, gates that a fake "synchronise" opens)."""
import os
import time

import torch

from tests import align_util as au
from tests import fence_util as F
from tests import ws_util as WU
from tests.test_gpu_aligned_min import Recorder, device_pointers

NEWEST = ("rsu_paths.h", "rsu_routes.h")      # the two headers behind align_util.HEADERS (its counts are those of ten headers)
FLOOR_MS, FACTOR = 1.0, 20.0                   # gate length = max(FLOOR_MS, FACTOR x the longest host time of one call): host jitter
RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r33", "streams.txt")


def prototypes():
    """align_util.prototypes() over all twelve headers"""
    ten = au.HEADERS
    au.HEADERS = tuple(ten) + tuple(h for h in NEWEST if h not in ten)
    try:
        return au.prototypes()
    finally:
        au.HEADERS = ten


def launching(protos=None):
    """every `int rsu_*` with an rsu_stream_t parameter"""
    return au.launching(protos or prototypes())


def wrapped_entries():
    """what Gated wraps: the entries of align_util.ALIGN (the launching ones of ten headers and the table-filling calls) and the launching
    entries of the two newest headers"""
    return sorted(set(au.ALIGN) | set(launching()))


class GateOpen(Exception):
    """a gated call returned with its gate open: .entry, .host_ms (the call's time on the host), .gate_ms"""

    def __init__(self, entry, host_ms, gate_ms, others=()):
        self.entry, self.host_ms, self.gate_ms = entry, host_ms, gate_ms
        Exception.__init__(self, "%s returned with its gate open: %.3f ms on the host under a gate of %.3f ms%s -- the entry waits for the "
                           "device (or the gate was too short for this host)" % (entry, host_ms, gate_ms,
                                                                                  "; also %s" % ", ".join(others) if others else ""))


class StreamError(AssertionError):
    """.found = [(arena index, spec name, bytes changed, first offset)]"""

    def __init__(self, found):
        self.found = found
        lines = ["arena %d %s: %d byte(s) differ from the run on the default stream, first at offset %d" % f for f in found]
        AssertionError.__init__(self, "a gated side stream changed a result: %s" % "; ".join(lines))


_CYCLES_PER_MS = None


BY_HAND = ("## by hand (kept by every run)", "## end by hand")


def record(line, fresh=False):
    """one line into profiles/r33/streams.txt; fresh: start the file again, keeping the block between the BY_HAND lines (what no test
    writes: the one-off scratch build, findings)"""
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    kept = []
    if fresh and os.path.exists(RECORD):
        with open(RECORD) as f:
            old = f.read().splitlines()
        if BY_HAND[0] in old and BY_HAND[1] in old[old.index(BY_HAND[0]):]:
            kept = old[old.index(BY_HAND[0]):old.index(BY_HAND[1], old.index(BY_HAND[0])) + 1]
    with open(RECORD, "w" if fresh else "a") as f:
        f.write("\n".join([line.rstrip("\n")] + kept) + "\n")


def calibrate():
    """cycles of torch.cuda._sleep per millisecond, measured once per session between two timing events at two counts (the difference
    drops the launch overhead); starts profiles/r33/streams.txt"""
    global _CYCLES_PER_MS
    if _CYCLES_PER_MS is None:
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        ms = []
        counts = (2_000_000, 20_000_000)
        for c in counts:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(c)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        assert ms[1] > ms[0] > 0.0, ms
        _CYCLES_PER_MS = (counts[1] - counts[0]) / (ms[1] - ms[0])
        record("# the stream contract of include/rsu.h: tests/test_gpu_streams.py (written by that run; tests/stream_util.py)", fresh=True)
        record("calibration: torch.cuda._sleep(%d) %.3f ms, (%d) %.3f ms -> %.0f cycles per ms; gate = max(%.0f ms, %.0f x longest host call)"
               % (counts[0], ms[0], counts[1], ms[1], _CYCLES_PER_MS, FLOOR_MS, FACTOR))
    return _CYCLES_PER_MS


class Gate:
    """a sleep of `ms` queued on `stream`, an event behind it"""

    def __init__(self, stream, ms):
        cycles = int(ms * calibrate())
        self.event = torch.cuda.Event()
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)
            self.event.record(stream)

    def closed(self):
        return not self.event.query()


class Device:
    """the real device: torch's streams, Gate, the loaded library (or `library`: an object whose attributes `entries` are the callables to
    wrap -- the stand-in entries of the positive controls)"""

    def __init__(self, library=None, entries=None):
        self.library, self.entries = library, entries

    def lib(self):
        if self.library is not None:
            return self.library
        from road_segmentation_unet_amd._lib import lib
        return lib()

    def names(self):
        return list(self.entries) if self.entries is not None else wrapped_entries()

    def current(self):
        return torch.cuda.current_stream()

    def key(self, stream):
        return stream.cuda_stream

    def gate(self, stream, ms):
        return Gate(stream, ms)

    def fresh(self):
        return torch.cuda.Stream()

    def on(self, stream):
        return torch.cuda.stream(stream)

    def drain(self, stream):
        stream.synchronize()


def _pointers(entry, args, placement):
    """the device pointers of a call of a fenced case (none for the two newest headers, which align_util.ALIGN does not hold, and none for
    the calls of a net, which builds no arena)"""
    return device_pointers(entry, args) if entry in au.ALIGN and placement.arenas else []


class Timed(Recorder):
    """Recorder over Device.names(), which also keeps the time every call took on the host: .host_ms = [ms per call]"""

    def __init__(self, placement, device=None):
        Recorder.__init__(self, placement)
        self.device, self.host_ms = device or Device(), []

    def __enter__(self):
        L = self.L = self.device.lib()
        self.saved = {e: getattr(L, e) for e in self.device.names()}
        for e, fn in self.saved.items():
            setattr(L, e, self._wrap(e, fn))
        return self

    def _wrap(self, entry, fn):
        def wrapped(*args):
            self.calls.append((entry, _pointers(entry, args, self.placement)))
            t0 = time.perf_counter()
            rc = fn(*args)
            self.host_ms.append((time.perf_counter() - t0) * 1e3)
            return rc
        return wrapped


class Gated(Timed):
    """see the module. .noted = [(entry, gate still closed when the call returned, host ms)] of the gated calls; .arena_gates = the gates put
    in front of arena builds; .skipped = the calls `where` left ungated"""

    def __init__(self, placement, ms, where="all", device=None):
        assert where in ("all", "main", "side"), where
        Timed.__init__(self, placement, device)
        self.ms, self.where, self.noted, self.arena_gates, self.skipped = ms, where, [], 0, 0

    def _selected(self, stream):
        on_main = self.device.key(stream) == self.main
        return self.where == "all" or (self.where == "main") == on_main

    def __enter__(self):
        self.main = self.device.key(self.device.current())
        Timed.__enter__(self)
        self.arena_init = real = F.Arena.__init__
        gated = self

        def init(arena, *args, **kw):
            cur = gated.device.current()
            if gated._selected(cur):
                gated.device.gate(cur, gated.ms)
                gated.arena_gates += 1
            real(arena, *args, **kw)
        F.Arena.__init__ = init
        return self

    def __exit__(self, *exc):
        F.Arena.__init__ = self.arena_init
        Timed.__exit__(self, *exc)

    def _wrap(self, entry, fn):
        def wrapped(*args):
            cur = self.device.current()
            self.calls.append((entry, _pointers(entry, args, self.placement)))
            if not self._selected(cur):
                self.skipped += 1
                return fn(*args)
            # (the copies are taken in front of the gate: an allocation may wait for the device, the gated call must not)
            kept = [A.mem.clone() for A in self.placement.arenas]
            gate = self.device.gate(cur, self.ms)
            for A, k in zip(self.placement.arenas, kept):
                A.mem.copy_(k)
            t0 = time.perf_counter()
            rc = fn(*args)
            ms = (time.perf_counter() - t0) * 1e3
            self.noted.append((entry, gate.closed(), ms))
            self.host_ms.append(ms)
            return rc
        return wrapped


def compare(want, got):
    """[(arena index, spec name, bytes changed, first offset)] over the payloads of ws_util.results"""
    assert sorted(want) == sorted(got), (sorted(want), sorted(got))
    found = []
    for key in sorted(want):
        diff = (got[key] != want[key]).nonzero().reshape(-1)
        if diff.numel():
            found.append((key[0], key[1], int(diff.numel()), int(diff.min())))
    return found


def on_stream(case, entries, *args, addresses=(), name=None, device=None, log=record, **kw):
    """`case(*args, placement=..., **kw)` twice on the default stream (the first run warms lazy code-object loads and attribute calls, the
    second is the reference: its calls, its arena layout, the bytes of every output and state, the host time of every call), then once
    under a fresh stream with a gate in front of every call and every arena build. The same calls, the same layout, the same bytes
    (StreamError), and every gated call back on the host with its gate closed (GateOpen). `entries`: what the registry says this case
    runs; `addresses`: outputs compared with ws_util.rebased. Returns the Gated run."""
    device = device or Device()
    for _ in range(2):
        first = F.Placement("aligned")
        with Timed(first, device) as r1:
            case(*args, placement=first, **kw)
    calls = [e for e, _ in r1.calls]
    assert set(entries) <= set(calls), "the registry names %s for this case, it ran %s" % (sorted(set(entries) - set(calls)), sorted(set(calls)))
    want, lay = WU.results(first, addresses), WU.layout(first)
    assert want, "no arena of this case holds an output or a state"
    longest = max(r1.host_ms)
    gate_ms = max(FLOOR_MS, FACTOR * longest)
    what = name or getattr(case, "__name__", "case")
    stream = device.fresh()
    second = F.Placement("aligned")
    try:
        with device.on(stream):
            with Gated(second, gate_ms, "all", device) as g:
                case(*args, placement=second, **kw)
            got = WU.results(second, addresses)
            device.drain(stream)
    except AssertionError:
        log("%-32s calls %3d  longest host call %8.3f ms  gate %8.3f ms  the case's own assertion FAILED on the gated stream"
            % (what, len(calls), longest, gate_ms))
        raise
    opened = [(e, ms) for e, closed, ms in g.noted if not closed]
    log("%-32s calls %3d  longest host call %8.3f ms  gate %8.3f ms  gated %3d (+%d arena builds)  returned open %d"
        % (what, len(calls), longest, gate_ms, len(g.noted), g.arena_gates, len(opened)))
    assert [e for e, _ in g.calls] == calls, "other calls on the side stream: %s, on the default stream %s" % ([e for e, _ in g.calls], calls)
    assert WU.layout(second) == lay, "other arenas on the side stream"
    assert len(g.noted) == len(calls) and g.arena_gates == len(second.arenas), (len(g.noted), len(calls), g.arena_gates)
    found = compare(want, got)
    if found:
        log("%-32s -> %s" % (what, StreamError(found)))
        raise StreamError(found)
    if opened:
        err = GateOpen(opened[0][0], opened[0][1], gate_ms, sorted({e for e, _ in opened[1:]} - {opened[0][0]}))
        log("%-32s -> %s" % (what, err))
        raise err
    return g
