"""No GPU: tests/test_gpu_streams.py leaves no entry that takes a stream out, and stream_util.Gated / on_stream have teeth. The registry
check parses the prototypes of all twelve headers: every `int rsu_*` with an rsu_stream_t parameter is in exactly one of STREAMED and
NOT_STREAMED, every case id named exists and names the entry, and an entry may only be excused where its body in csrc/rsu_api.hip uses
no hipStream_t. Gated and on_stream run on CPU tensors with a fake device: a library of Python callables, named streams, and gates that
stay closed until their stream is "synchronised" -- the call list, the layout and the byte comparison fail when they should, a call
that waits raises GateOpen, Arena.__init__ and the library are restored whatever happens inside, and `where` selects the right calls."""
import contextlib
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import align_util as au
from tests import fence_util as F
from tests import stream_util as SU

BAND = 4096


# ------------------------------------------------------------------------------------------- the registry covers the twelve headers
def _api_text():
    with open(os.path.join(au._root(), "road_segmentation_unet_amd", "csrc", "rsu_api.hip")) as f:
        return f.read()


def body_of(entry, text):
    """the body of `extern "C" int <entry>(...) { ... }` in csrc/rsu_api.hip, by matching braces"""
    m = re.search(r'^extern "C" int %s\(' % re.escape(entry), text, flags=re.M)
    assert m, "%s is not defined in rsu_api.hip" % entry
    start = text.index(") {", m.end()) + 2      # (the parameter list holds no brace)
    assert ";" not in text[m.end():start], entry
    depth, at = 0, start
    while True:
        c = text[at]
        depth += (c == "{") - (c == "}")
        at += 1
        if depth == 0:
            return text[start:at]


def launches_nothing(entry, text):
    return "hipStream_t" not in body_of(entry, text) and "stream" not in body_of(entry, text)


def check_registry(streamed, not_streamed, cases):
    protos = SU.prototypes()
    takes = SU.launching(protos)
    assert len(takes) >= 75 and len(protos) > len(au.prototypes()), len(takes)
    for probe in ("rsu_conv2d_fwd", "rsu_wgrad_group_run", "rsu_head_fwd_bwd", "rsu_update_table_run_adam_decay", "rsu_mask_thin",
                  "rsu_line_segments", "rsu_segment_paths", "rsu_graph_routes", "rsu_route_score"):
        assert probe in takes, probe
    for e in takes:
        assert (e in streamed) != (e in not_streamed), "%s: in exactly one of STREAMED and NOT_STREAMED" % e
    assert set(streamed) | set(not_streamed) <= set(takes), sorted((set(streamed) | set(not_streamed)) - set(takes))
    for e, ids in streamed.items():
        assert ids, e
        for cid in ids:
            assert cid in cases and e in cases[cid][3], (e, cid)
    text = _api_text()
    for e, reason in not_streamed.items():
        assert isinstance(reason, str) and len(reason.strip()) > 20, e
        assert launches_nothing(e, text), "%s is excused, but its body in rsu_api.hip uses a stream" % e


def test_every_entry_that_takes_a_stream_is_run_on_a_gated_side_stream_or_excused():
    from tests import test_gpu_streams as S
    check_registry(S.STREAMED, S.NOT_STREAMED, S.CASES)
    assert set(S.CASES) == set(S.H.ALL) | set(S.NEWEST) and not set(S.H.ALL) & set(S.NEWEST)
    assert S.NEWEST["paths_uneven"][:2] == (S.GP._case, ("uneven",)) and S.NEWEST["routes_pruned"][:2] == (S.GR._case, ("pruned",))
    import inspect
    for cid, (fn, _args, _env, _entries) in S.CASES.items():
        assert "placement" in inspect.signature(fn).parameters and fn.__module__.endswith("fenced"), cid
    # Gated wraps every entry the registry names (and the table-filling calls of align_util.ALIGN)
    assert set(S.STREAMED) <= set(SU.wrapped_entries()) and "rsu_pack_table_add" in SU.wrapped_entries()
    # the re-entrant runs and the net-level kinds the issue names
    assert sorted(S.REENTRANT) == ["conv2d_bwd_weight", "conv2d_fwd", "graph_routes", "head_fwd_bwd", "mask_thin"]
    assert S.WHERE == ("main", "side", "all") and sorted(S.H.NETS) == ["dilated", "every_term", "plain"]


def test_the_registry_check_fails_when_an_entry_is_left_out_or_wrongly_excused():
    from tests import test_gpu_streams as S
    for gone in ("rsu_graph_routes", "rsu_conv2d_fwd", "rsu_ema_step"):
        fewer = {e: ids for e, ids in S.STREAMED.items() if e != gone}
        with pytest.raises(AssertionError, match=gone):
            check_registry(fewer, S.NOT_STREAMED, S.CASES)
        with pytest.raises(AssertionError, match="uses a stream"):      # an entry that launches cannot be excused
            check_registry(fewer, {gone: "a reason that is long enough to be one"}, S.CASES)
        with pytest.raises(AssertionError):                             # nor named twice
            check_registry(S.STREAMED, {gone: "a reason that is long enough to be one"}, S.CASES)
    with pytest.raises(AssertionError):                                 # a case id that does not exist
        check_registry(dict(S.STREAMED, rsu_ema_step=["no_such_case"]), S.NOT_STREAMED, S.CASES)
    with pytest.raises(AssertionError):                                 # a case that does not run the entry
        check_registry(dict(S.STREAMED, rsu_ema_step=["dropout"]), S.NOT_STREAMED, S.CASES)
    with pytest.raises(AssertionError):                                 # an entry that takes no stream belongs in neither
        check_registry(S.STREAMED, {"rsu_wgrad_group_plan": "fills a host table and launches nothing"}, S.CASES)
    # what "launches nothing" means: the table-filling calls use no stream, a launcher does
    text = _api_text()
    assert launches_nothing("rsu_wgrad_group_plan", text) and launches_nothing("rsu_pack_table_add", text)
    assert not launches_nothing("rsu_wgrad_group_run", text) and not launches_nothing("rsu_route_score", text)


def test_the_two_newest_headers_are_read_here_and_align_util_keeps_its_ten():
    assert len(au.HEADERS) == 10 and not set(SU.NEWEST) & set(au.HEADERS)
    ten, twelve = au.prototypes(), SU.prototypes()
    assert au.HEADERS == tuple(h for h in au.HEADERS) and len(au.HEADERS) == 10           # prototypes() puts the list back
    assert set(twelve) - set(ten) >= {"rsu_segment_paths", "rsu_graph_routes", "rsu_route_score"} and set(ten) <= set(twelve)


def test_a_fresh_record_keeps_the_block_written_by_hand(tmp_path, monkeypatch):
    monkeypatch.setattr(SU, "RECORD", str(tmp_path / "r33" / "streams.txt"))
    SU.record("# header", fresh=True)
    SU.record("a case")
    with open(SU.RECORD, "a") as f:
        f.write("\n".join([SU.BY_HAND[0], "the scratch build", SU.BY_HAND[1], "an older run's line"]) + "\n")
    SU.record("# header again", fresh=True)
    SU.record("another case")
    with open(SU.RECORD) as f:
        assert f.read().splitlines() == ["# header again", SU.BY_HAND[0], "the scratch build", SU.BY_HAND[1], "another case"]


# ------------------------------------------------------------------------------------------- a fake device
class _Stream:
    def __init__(self, name):
        self.name = name


class _Gate:
    def __init__(self, stream, ms):
        self.stream, self.ms, self.open = stream, ms, False

    def closed(self):
        return not self.open


class FakeDevice(SU.Device):
    """named streams; a gate opens when its stream is drained (the fake of a wait on the host); CPU tensor work is immediate"""

    def __init__(self, library, entries):
        SU.Device.__init__(self, library, entries)
        self.default = self.cur = _Stream("default")
        self.gates, self.made = [], 0

    def current(self):
        return self.cur

    def key(self, stream):
        return stream.name

    def gate(self, stream, ms):
        self.gates.append(_Gate(stream, ms))
        return self.gates[-1]

    def fresh(self):
        self.made += 1
        return _Stream("fresh%d" % self.made)

    @contextlib.contextmanager
    def on(self, stream):
        keep, self.cur = self.cur, stream
        try:
            yield
        finally:
            self.cur = keep

    def drain(self, stream):
        for g in self.gates:
            if g.stream is stream:
                g.open = True


X = np.arange(1, 33, dtype=np.float32)


def _world(fault=None):
    """(case, device, library): a library of two entries on CPU tensors -- rsu_double (y = 2 x) and rsu_add (acc += y) -- and a case that
    builds one arena and calls both. `fault` makes them wrong away from the default stream only."""
    lib = types.SimpleNamespace()
    dev = FakeDevice(lib, ["rsu_double", "rsu_add"])
    away = lambda: dev.current() is not dev.default  # noqa: E731

    def rsu_double(x, y):
        torch.mul(x, 3.0 if fault == "bytes" and away() else 2.0, out=y)
        if fault == "waits" and away():
            dev.drain(dev.current())
        return 0

    def rsu_add(acc, y):
        acc.add_(y)
        return 0
    lib.rsu_double, lib.rsu_add = rsu_double, rsu_add

    def case(placement="aligned"):
        n = 16 if fault == "layout" and away() else 32
        A = F.Arena("cpu", [F.f32("x", X[:n]), F.out("y", (n,), torch.float32), F.state("acc", np.ones(n, np.float32))], band=BAND, placement=placement)
        assert lib.rsu_double(A["x"], A["y"]) == 0
        assert lib.rsu_add(A["acc"], A["y"]) == 0
        if fault == "calls" and away():
            lib.rsu_add(A["acc"], A["y"])
        if fault == "own":
            assert not away(), "the case's own comparison"
        A.check("fake")
    return case, dev, lib


def _quiet(_line, fresh=False):
    pass


def test_on_stream_passes_a_library_that_keeps_to_its_stream():
    case, dev, lib = _world()
    plain = (lib.rsu_double, lib.rsu_add, F.Arena.__init__)
    lines = []
    g = SU.on_stream(case, ["rsu_double", "rsu_add"], name="fake", device=dev, log=lambda line, fresh=False: lines.append(line))
    assert [e for e, _ in g.calls] == ["rsu_double", "rsu_add"] and [n[:2] for n in g.noted] == [("rsu_double", True), ("rsu_add", True)]
    assert g.arena_gates == 1 and g.where == "all" and g.ms >= SU.FLOOR_MS and dev.made == 1
    # a gate in front of the arena build and of each call, all on the fresh stream, none on the default one
    assert len(dev.gates) == 3 and {x.stream.name for x in dev.gates} == {"fresh1"} and all(x.ms == g.ms for x in dev.gates)
    assert (lib.rsu_double, lib.rsu_add, F.Arena.__init__) == plain and dev.current() is dev.default
    assert len(lines) == 1 and "fake" in lines[0] and "returned open 0" in lines[0]
    with pytest.raises(AssertionError, match="the registry names"):
        SU.on_stream(case, ["rsu_double", "rsu_other"], device=dev, log=_quiet)


def test_the_gate_length_follows_the_longest_host_call():
    case, dev, lib = _world()
    import time
    slow = lib.rsu_add

    def rsu_add(acc, y):
        time.sleep(0.004)
        return slow(acc, y)
    lib.rsu_add = rsu_add
    g = SU.on_stream(case, ["rsu_add"], device=dev, log=_quiet)
    assert SU.FACTOR * 4.0 <= g.ms < SU.FACTOR * 40.0 and SU.FLOOR_MS == 1.0 and SU.FACTOR == 20.0, g.ms


@pytest.mark.parametrize("fault,error,match", [("bytes", SU.StreamError, "arena 0 y"), ("calls", AssertionError, "other calls"),
                                               ("layout", AssertionError, "other arenas"), ("own", AssertionError, "own comparison")])
def test_on_stream_fails_on_other_bytes_other_calls_and_another_layout(fault, error, match):
    case, dev, lib = _world(fault)
    plain = (lib.rsu_double, lib.rsu_add, F.Arena.__init__)
    case()                                                   # on the default stream the fault does not show
    with pytest.raises(error, match=match) as e:
        SU.on_stream(case, ["rsu_double", "rsu_add"], device=dev, log=_quiet)
    assert not isinstance(e.value, SU.GateOpen)
    if fault == "bytes":      # the output and the state that took it up, by name
        assert [f[:2] for f in e.value.found] == [(0, "acc"), (0, "y")] and e.value.found[1][2] > 0
    assert (lib.rsu_double, lib.rsu_add, F.Arena.__init__) == plain and dev.current() is dev.default


def test_a_call_that_waits_for_its_stream_raises_gate_open_and_nothing_else():
    case, dev, lib = _world("waits")
    with pytest.raises(SU.GateOpen) as e:
        SU.on_stream(case, ["rsu_double", "rsu_add"], device=dev, log=_quiet)
    assert e.value.entry == "rsu_double" and e.value.gate_ms >= SU.FLOOR_MS and not isinstance(e.value, AssertionError)
    assert "rsu_double" in str(e.value) and "gate open" in str(e.value)


def test_gated_restores_the_arena_builder_and_the_library_after_an_exception():
    case, dev, lib = _world()
    plain = (lib.rsu_double, lib.rsu_add, F.Arena.__init__)
    with pytest.raises(RuntimeError, match="inside the case"):
        with SU.Gated(F.Placement(), 1.0, "all", dev):
            assert F.Arena.__init__ is not plain[2] and lib.rsu_double is not plain[0]
            case()
            raise RuntimeError("inside the case")
    assert (lib.rsu_double, lib.rsu_add, F.Arena.__init__) == plain
    with pytest.raises(AssertionError):
        SU.Gated(F.Placement(), 1.0, "most", dev)


def test_gated_writes_the_arenas_back_behind_the_gate():
    """what turns a launch on the wrong stream into wrong bytes: in front of a gated call the arena is written back with what it held in
    front of the gate. On the fake device that is immediate, so a call finds the arena as it was -- and the copy was taken before the gate"""
    case, dev, lib = _world()
    p = F.Placement()
    seen = []
    inner = lib.rsu_double

    def rsu_double(x, y):
        seen.append((len(dev.gates), bool(torch.isnan(y).all())))
        return inner(x, y)
    lib.rsu_double = rsu_double
    with SU.Gated(p, 1.0, "all", dev):
        case(placement=p)
    assert seen == [(2, True)]          # the arena's gate and the call's own are in place; y still holds the pattern


@pytest.mark.parametrize("where", ["all", "main", "side"])
def test_where_selects_the_calls_of_the_main_stream_or_of_the_others(where):
    case, dev, lib = _world()
    side = _Stream("side")
    start = dev.fresh()
    p = F.Placement()
    with dev.on(start):                                   # "main" is the stream that is current when the run begins, not the default one
        with SU.Gated(p, 1.0, where, dev) as g:
            A = F.Arena("cpu", [F.f32("x", X), F.out("y", (32,), torch.float32), F.state("acc", np.ones(32, np.float32))], band=BAND, placement=p)
            lib.rsu_double(A["x"], A["y"])                # on the main stream
            with dev.on(side):
                lib.rsu_add(A["acc"], A["y"])             # on a side stream
                with dev.on(dev.default):
                    lib.rsu_add(A["acc"], A["y"])         # the default stream is a side stream here
            lib.rsu_double(A["x"], A["y"])
    assert [e for e, _ in g.calls] == ["rsu_double", "rsu_add", "rsu_add", "rsu_double"]
    on_main, on_side = [("rsu_double", True)] * 2, [("rsu_add", True)] * 2
    want = {"all": on_main[:1] + on_side + on_main[1:], "main": on_main, "side": on_side}[where]
    assert [n[:2] for n in g.noted] == want and g.skipped == 4 - len(want)
    assert g.arena_gates == (0 if where == "side" else 1)
    names = [x.stream.name for x in dev.gates]
    assert names == {"all": ["fresh1", "fresh1", "side", "default", "fresh1"], "main": ["fresh1"] * 3, "side": ["side", "default"]}[where]
    assert torch.equal(A["acc"], torch.from_numpy(1 + 4 * X))
