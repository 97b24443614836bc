"""A workspace "need not be cleared and holds nothing between calls": history_free() holds a fenced case to that. The fenced files start
every workspace as the pattern 0x7FA5..., which proves initialisation only where that value gives a wrong answer: it is non-zero (a
"skip where the previous launch's counter is 0" never fires on an uncleared counter), large and positive as an integer (an atomicMin
target that was never set to "infinity" works by accident), out of range as an index, and a NaN as a float (but zeros hide a partial sum
that is read and never written). Production hands a kernel none of these: one workspace serves every layer's weight gradient, the head
and the grouped launch in turn, and the evaluation workspaces live across batches.

history_free(case, entries, *args, **kw) runs `case(*args, placement=..., **kw)` under fence_util.Placement(fill="pattern"), keeps the
bytes of every `out` and `state` payload of every arena and of every workspace, then runs it again under "zeros", "ones" and "rolled"
(the workspaces' own leftovers, rolled by a third). In every run the fill is put back into a workspace in front of EVERY library call
that receives it (refiller(): a case hands one workspace to several entries in a row, and each of them must start from the fill, not
from what the entry before left for the same input); rsu_cldice_bwd, which reads what rsu_cldice_fwd left, is the one exception. Each run makes the case's own assertions -- the reference comparison, Arena.check,
the exact workspace size; on top of them every `out` / `state` payload must be BYTE-IDENTICAL to the pattern run's. No tolerance: every
kernel here has a fixed reduction order and uses integer atomics only, and a leak small enough to hide inside a conv tolerance shows.
All runs must issue the same calls (test_gpu_aligned_min.Recorder).

tests/test_ws_history_host.py proves on CPU tensors that this has teeth: a "kernel" that reads a workspace element before writing it,
one that skips work where a workspace counter is 0 and one that takes a minimum with an unset slot each pass under the pattern and fail
under another fill."""
import torch

from tests import fence_util as F

FILLS = ("zeros", "ones", "rolled")      # what a case runs under after its pattern run


class HistoryError(AssertionError):
    """.fill, .found = [(arena index, spec name, bytes changed, first offset)]"""

    def __init__(self, fill, found):
        self.fill, self.found = fill, found
        lines = ["arena %d %s: %d byte(s) differ from the pattern run, first at offset %d" % f for f in found]
        AssertionError.__init__(self, "workspace fill %r changed a result: %s" % (fill, "; ".join(lines)))


# the one entry that READS what another entry left in its workspace (include/rsu_cldice.h: the erosion levels and skeleton states
# rsu_cldice_fwd wrote): its workspace is not refilled in front of it
CARRIED = {"rsu_cldice_bwd": "reads the [2 iters + 1] maps rsu_cldice_fwd left in ws"}


def rebased(t, arena):
    """the bytes of a device table with every 8-byte word that is an address inside `arena` replaced by its offset from the arena's
    start: two runs build their arenas elsewhere, and lay them out alike (a tail of fewer than 8 bytes is kept as it is)"""
    n = t.numel() // 8 * 8
    words = t[:n].clone().view(torch.int64)
    base = arena.mem.data_ptr()
    inside = (words >= base) & (words < base + arena.total)
    words[inside] -= base
    return torch.cat([words.view(torch.uint8), t[n:]]), int(inside.sum())


def results(placement, addresses=()):
    """{(arena index, spec name): bytes} of every `out` and `state` payload of the arenas built with `placement`; those named in
    `addresses` rebased()"""
    out = {}
    for i, A in enumerate(placement.arenas):
        for s in A.specs:
            if s.kind in ("out", "state"):
                out[(i, s.name)] = A.payload_bytes(s.name).clone()
                if s.name in addresses:
                    assert A.place[s.name][0] % 8 == 0, s.name
                    out[(i, s.name)], n = rebased(out[(i, s.name)], A)
                    assert n > 0, "%s holds no address of its arena" % s.name
    return out


def layout(placement):
    return [[(s.name, s.kind, s.nbytes) + A.place[s.name] for s in A.specs] for A in placement.arenas]


class _NoCalls:
    calls, refilled = (), ()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


def refiller(placement):
    """test_gpu_aligned_min.Recorder that, in front of EVERY library call, puts the placement's fill back into each workspace payload
    the call receives (CARRIED excepted): a case hands one workspace to several calls in a row, and without this only the first of
    them would start from the fill -- the others from the leftover of the call before on the same input, alike under every fill.
    .refilled = [(entry, arena index, spec name)]"""
    from tests.test_gpu_aligned_min import Recorder, device_pointers

    class Refiller(Recorder):
        def __init__(self, placement):
            Recorder.__init__(self, placement)
            self.refilled = []

        def _wrap(self, entry, fn):
            def wrapped(*args):
                ptrs = device_pointers(entry, args)
                self.calls.append((entry, ptrs))
                for _key, addr in ptrs:
                    hit = self.payload(addr)
                    if hit is None or entry in CARRIED:
                        continue
                    A = self.placement.arenas[hit[0]]
                    if any(s.name == hit[1] and s.kind == "ws" for s in A.specs):
                        assert hit[2] == 0, (entry, hit)      # (a workspace is handed over whole)
                        A.refill(hit[1])
                        self.refilled.append((entry,) + hit[:2])
                return fn(*args)
            return wrapped

    return Refiller(placement)


def takes_a_workspace(entry, protos):
    return any("*" in t and n in ("ws", "kws") for t, n in protos[entry][1])


def history_free(case, entries, *args, fills=FILLS, record=True, addresses=(), **kw):
    """see the module. `entries`: the entries the registry says this case runs; `fills`: the fills to run after the pattern run;
    record=False: the case calls nothing of the library (the CPU controls: one "launch" each); `addresses`: the names of outputs that
    hold device ADDRESSES of the arena's own payloads (the tables of the table-driven launches), compared rebased().
    Returns the entries that started from a freshly filled workspace in every run."""
    first = F.Placement("aligned", fill="pattern")
    with (refiller(first) if record else _NoCalls()) as r1:
        case(*args, placement=first, **kw)
    calls = [e for e, _ in r1.calls]
    assert set(entries) <= set(calls), "the registry names %s for this case, it ran %s" % (sorted(set(entries) - set(calls)), sorted(set(calls)))
    if record:
        from tests import align_util as au
        protos = au.prototypes()
        owed = {e for e in entries if takes_a_workspace(e, protos) and e not in CARRIED}
        got_one = {e for e, _i, _n in r1.refilled}
        assert owed <= got_one, "%s received no workspace of an arena: nothing was filled in front of them" % sorted(owed - got_one)
    want, snaps = results(first, addresses), first.workspaces()
    assert set(addresses) <= {name for _, name in want}, (addresses, sorted(want))
    assert snaps, "no arena of this case holds a workspace"
    assert want, "no arena of this case holds an output or a state"
    for fill in fills:
        assert fill in F.FILLS and fill != "pattern", fill
        p = F.Placement("aligned", fill=fill, snapshots=snaps)
        with (refiller(p) if record else _NoCalls()) as r:
            try:
                case(*args, placement=p, **kw)
            except AssertionError as e:
                raise AssertionError("under the workspace fill %r the case's own assertion fails: %s" % (fill, e)) from e
        assert [e for e, _ in r.calls] == calls and list(r.refilled) == list(r1.refilled) and layout(p) == layout(first), \
            "fill %r: other calls, other workspaces or other arenas" % fill
        got, found = results(p, addresses), []
        for key in sorted(want):
            diff = (got[key] != want[key]).nonzero().reshape(-1)
            if diff.numel():
                found.append((key[0], key[1], int(diff.numel()), int(diff.min())))
        if found:
            raise HistoryError(fill, found)
    return sorted({e for e, _i, _n in r1.refilled})


def bit_equal(a, b):
    """two tensors (or numbers, or nested tuples / lists / dicts of them) hold the same bytes"""
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(bit_equal(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(bit_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and \
            torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))
    import numpy as np
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return isinstance(b, float) and np.float64(a).tobytes() == np.float64(b).tobytes()
    return type(a) is type(b) and a == b
