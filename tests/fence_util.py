"""An arena with fences: ONE torch allocation holds every device buffer of a test, and everything in it that is not a payload is a band
of the 16-bit word 0x7FA5 -- a NaN as bf16, a NaN as float32 (0x7FA57FA5), an absurd value as any integer. The buffer descriptors of the
MFMA kernels are built with num_records = 0x7fffffff: the hardware checks no bound, every tile edge is a hand-written
predicate, and the exact-size torch tensors of the op tests sit in 512-byte allocator blocks that swallow a short overrun.

Layout. A payload starts on a 256-byte boundary -- under Placement("minimum") at a 256-byte boundary plus its own minimum alignment, an
address aligned to exactly that and to nothing larger (the arena itself starts on a 256-byte boundary) -- and ends exactly at its last
byte. Every claim below holds under both placements. In front of and behind every payload lie at least
BAND = 1 MiB of pattern; behind a workspace at least the workspace's own size (a size function that is wrong by a factor of two still
lands inside the arena). The gap between two neighbours is the band behind the first PLUS the band in front of the second, so every
byte of a gap belongs to exactly one (tensor, side). Outputs start as pattern too: an element a kernel never wrote reads as NaN.
A workspace starts as pattern unless the case's Placement carries another fill (zeros, ones, or the rolled leftover of an earlier run:
tests/ws_util.py runs every case under each and asks for byte-identical results).

Arena.check(what), called after the launches of a case, makes one synchronisation and asserts that every band byte still holds the
pattern (compared as raw integers on the device, reduced to one flag) and that every tensor registered as an input still holds the bytes
it was given. A stray WRITE shows there; a stray READ that reaches a result shows as NaN in the output, which the comparisons of
tests/hiputil.py treat as out of tolerance. The failure (FenceError, an AssertionError) names the tensor, the side, the first and last
offending byte and the number of bytes changed. Offsets: `front` counts from the payload's first byte (-1 = the byte just in front of
it), `behind` from the payload's end (0 = the first byte behind it), `input` from the payload's first byte.

The arena takes its device as an argument: tests/test_fence_host.py proves every claim above on CPU tensors."""
import numpy as np
import torch

PATTERN = 0x7FA5
BAND = 1 << 20
ALIGN = 256
FILLS = ("pattern", "zeros", "ones", "rolled")

_BF16, _F32 = torch.bfloat16, torch.float32


class FenceError(AssertionError):
    """.tensor, .side ("front", "behind" or "input"), .first, .last, .count of the first violation; the message lists all of them"""

    def __init__(self, what, found):
        self.tensor, self.side, self.first, self.last, self.count = found[0]
        lines = ["%s %s: %d byte(s) changed, first at offset %+d, last at offset %+d" % (n, s, c, a, b) for n, s, a, b, c in found]
        AssertionError.__init__(self, "fence: %s: %s" % (what, "; ".join(lines)))


class _Spec:
    def __init__(self, name, kind, dtype, shape, data=None, band=None):
        self.name, self.kind, self.dtype, self.shape, self.data, self.band = name, kind, dtype, tuple(int(s) for s in shape), data, band
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size()
        self.minimum = torch.empty(0, dtype=dtype).element_size()    # its minimum alignment: the element size unless a Placement says more
        assert self.nbytes > 0, name


class Placement:
    """Where the payloads of the arenas of ONE case start. "aligned" (the default of Arena): every payload on a 256-byte boundary.
    "minimum": a payload starts at a 256-byte boundary PLUS its own minimum alignment m (a power of two below 256), so its address is a
    multiple of m and of nothing larger -- what a caller who places buffers back to back may hand a kernel. A spec's minimum is its element
    size; minima[i] = {spec name: bytes} raises it for the specs of the i-th arena the case builds (tests/align_util.ALIGN by (entry,
    argument): tests/test_gpu_aligned_min.py). Bands, the attribution of gap bytes, check() and poison_outside() are the same under both.
    The placement keeps the arenas built with it (.arenas), in order.

    fill: what a WORKSPACE payload (kind "ws", nothing else) holds when the case starts. "pattern" (the default: as the bands), "zeros"
    (every byte 0x00), "ones" (every byte 0xFF: -1 as a signed integer, the maximum as an unsigned one, a NaN with another payload as a
    float) or "rolled": the bytes snapshots[(arena index, spec name)] -- what the same workspace held after an earlier run of the case
    (workspaces()) -- rolled by (count // 3) | 1 elements of the spec's element type: real counters, in-range parents, real bit planes
    and real partial sums, all in the wrong places. Bands, inputs, outputs, states and check() are the same under every fill.
    Arena.refill(name) puts the fill back into a workspace later on (tests/ws_util.py: in front of every call that receives it)."""

    def __init__(self, mode="aligned", minima=(), fill="pattern", snapshots=None):
        assert mode in ("aligned", "minimum"), mode
        assert fill in FILLS, fill
        self.mode, self.minima, self.arenas = mode, list(minima), []
        self.fill, self.snapshots = fill, dict(snapshots or {})

    def workspaces(self):
        """{(arena index, spec name): the bytes every workspace of the arenas built so far holds now}: the snapshots of a "rolled" run"""
        return {(i, s.name): A.payload_bytes(s.name).clone() for i, A in enumerate(self.arenas) for s in A.specs if s.kind == "ws"}

    def fill_workspace(self, spec, payload, index):
        """`payload`: the bytes of workspace `spec` of arena `index` (a uint8 view); "pattern" is Arena.refill's own"""
        if self.fill == "zeros":
            payload.zero_()
        elif self.fill == "ones":
            payload.fill_(0xFF)
        elif self.fill == "rolled":
            key = (index, spec.name)
            assert key in self.snapshots, "no snapshot of workspace %s of arena %d" % (spec.name, key[0])
            snap = self.snapshots[key].to(payload.device)
            assert snap.dtype == torch.uint8 and snap.numel() == payload.numel(), key
            esz = spec.nbytes // spec.shape[0]
            payload.copy_(torch.roll(snap.view(-1, esz), roll_shift(spec.shape[0]), 0).reshape(-1))

    def shift(self, spec):
        """bytes between the 256-byte boundary and the start of `spec` in the arena that is being built"""
        if self.mode == "aligned":
            return 0
        over = self.minima[len(self.arenas)] if len(self.arenas) < len(self.minima) else {}
        m = max(spec.minimum, int(over.get(spec.name, 0)))
        assert 0 < m < ALIGN and m & (m - 1) == 0 and m % spec.minimum == 0, (spec.name, m)
        return m


def roll_shift(count):
    """how far a "rolled" workspace of `count` elements is rolled: odd, about a third of it"""
    return (count // 3) | 1


def _cpu(a, dtype):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().to(dtype).contiguous()
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(dtype).contiguous()


def _np_dtype(a):
    a = np.asarray(a)
    return {"float32": _F32, "int64": torch.int64, "uint64": torch.int64, "int32": torch.int32, "uint8": torch.uint8,
            "uint32": torch.int32, "int16": torch.int16, "uint16": torch.int16}[a.dtype.name]


def bf16(name, a):
    """an INPUT of bf16 elements from float data (one round-to-nearest, as hiputil.dev_bf16)"""
    return _Spec(name, "in", _BF16, np.shape(a), _cpu(np.asarray(a, np.float32), _BF16))


def f32(name, a):
    """a float32 INPUT"""
    return _Spec(name, "in", _F32, np.shape(a), _cpu(np.asarray(a, np.float32), _F32))


def raw(name, a):
    """an INPUT with the numpy array's own element type (int64 labels, uint8 images, device tables as bytes)"""
    return _Spec(name, "in", _np_dtype(a), np.shape(a), _cpu(a, _np_dtype(a)))


def out(name, shape, dtype=_BF16):
    """an OUTPUT: starts as pattern"""
    return _Spec(name, "out", dtype, shape)


def state(name, a, dtype=None):
    """a buffer the launches read AND write (weights, optimizer slots, accumulators the caller zeroes): starts as `a`, is not compared"""
    dtype = dtype or _np_dtype(a)
    return _Spec(name, "state", dtype, np.shape(a), _cpu(a, dtype))


def ws(name, count, dtype=_F32, band=None):
    """a WORKSPACE of exactly `count` elements (the advertised size): starts as the placement's fill (pattern by default); the band
    behind it is at least its own size (`band`: another minimum, for a workspace whose planner checks its need on the host)"""
    return _Spec(name, "ws", dtype, (count,), band=band)


def _up(n, a=ALIGN):
    return (n + a - 1) // a * a


class Arena:
    def __init__(self, device, specs, band=BAND, placement="aligned"):
        self.device, self.specs, self.band = device, list(specs), band
        assert len({s.name for s in self.specs}) == len(self.specs), "duplicate names"
        self.placement = placement if isinstance(placement, Placement) else Placement(placement)
        cur = 0
        self.place = {}          # name -> (start, end, band behind)
        for s in self.specs:
            start = _up(cur + band) + self.placement.shift(s)
            behind = _up(max(band, s.nbytes) if s.kind == "ws" and s.band is None else max(band, s.band or 0))
            self.place[s.name] = (start, start + s.nbytes, behind)
            cur = start + s.nbytes + behind
        self.total = _up(cur)
        raw = torch.empty(self.total + ALIGN, dtype=torch.uint8, device=device)    # (the arena itself starts on a 256-byte boundary on any device)
        self.mem = raw[(-raw.data_ptr()) % ALIGN:][:self.total]
        assert self.mem.data_ptr() % ALIGN == 0
        self.mem.view(torch.int16).fill_(PATTERN)
        # the regions: every byte that is no payload, attributed to (tensor, side); offsets are formed from `origin`
        self.regions = []        # (name, side, start, end, origin)
        prev_end = 0
        for i, s in enumerate(self.specs):
            start, end, behind = self.place[s.name]
            self.regions.append((s.name, "front", prev_end, start, start))
            nxt = self.place[self.specs[i + 1].name][0] if i + 1 < len(self.specs) else self.total
            stop = min(end + behind, nxt) if i + 1 < len(self.specs) else self.total
            self.regions.append((s.name, "behind", end, stop, end))
            prev_end = stop
        longest = max(e - s for _, _, s, e, _ in self.regions)
        self.pat = torch.empty(_up(longest + 2, 2), dtype=torch.uint8, device=device)
        self.pat.view(torch.int16).fill_(PATTERN)
        self.t, self.given = {}, {}
        for s in self.specs:
            start, end, _ = self.place[s.name]
            self.t[s.name] = self.mem[start:end].view(s.dtype).reshape(s.shape)
            if s.data is not None:
                self.mem[start:end].copy_(s.data.view(torch.uint8).reshape(-1).to(device))
            if s.kind == "in":
                self.given[s.name] = self.mem[start:end].clone()
        self.index = len(self.placement.arenas)      # which arena of its placement this is
        if self.placement.fill != "pattern":
            for s in self.specs:
                if s.kind == "ws":
                    self.refill(s.name)
        self.placement.arenas.append(self)

    def refill(self, name):
        """workspace `name` as it was when the arena was built: the placement's fill again, whatever the launches since left there
        (tests/ws_util.py does this in front of every library call that receives the workspace)"""
        spec = next(s for s in self.specs if s.name == name)
        assert spec.kind == "ws", name
        start, end, _ = self.place[name]
        if self.placement.fill == "pattern":
            v = self.mem[start:end]         # (the arena's words lie on even offsets: low byte first)
            if start & 1:
                v[0] = PATTERN >> 8
                v = v[1:]
            even = v.numel() // 2 * 2
            v[:even].view(torch.int16).fill_(PATTERN)
            if v.numel() > even:
                v[even] = PATTERN & 0xFF
        else:
            self.placement.fill_workspace(spec, self.mem[start:end], self.index)

    def __getitem__(self, name):
        return self.t[name]

    def payload_bytes(self, name):
        """the payload as the bytes of the arena (a view)"""
        start, end, _ = self.place[name]
        return self.mem[start:end]

    def nbytes(self, name):
        start, end, _ = self.place[name]
        return end - start

    def poison_outside(self, name, oy, ox, h, w):
        """the crop margins of an NHWC bf16 input: everything outside the window [oy, oy + h) x [ox, ox + w) becomes pattern"""
        t = self.t[name].view(torch.int16)
        keep = t[:, oy:oy + h, ox:ox + w, :].clone()
        t.fill_(PATTERN)
        t[:, oy:oy + h, ox:ox + w, :] = keep
        start, end, _ = self.place[name]
        self.given[name] = self.mem[start:end].clone()

    def _diff(self, s, e):
        return self.mem[s:e] != self.pat[(s & 1):(s & 1) + (e - s)]

    def check(self, what):
        counts = [self._diff(s, e).sum() for _, _, s, e, _ in self.regions if e > s]
        names = list(self.given)
        counts += [(self.mem[self.place[n][0]:self.place[n][1]] != self.given[n]).sum() for n in names]
        if int(torch.stack(counts).sum().item()) == 0:      # the one synchronisation
            return
        found = []
        for name, side, s, e, origin in self.regions:
            if e > s:
                idx = self._diff(s, e).nonzero().reshape(-1)
                if idx.numel():
                    found.append((name, side, int(idx.min()) + s - origin, int(idx.max()) + s - origin, int(idx.numel())))
        for n in names:
            idx = (self.mem[self.place[n][0]:self.place[n][1]] != self.given[n]).nonzero().reshape(-1)
            if idx.numel():
                found.append((n, "input", int(idx.min()), int(idx.max()), int(idx.numel())))
        raise FenceError(what, found)
