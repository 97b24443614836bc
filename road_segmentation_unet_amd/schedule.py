"""WHERE and HOW the launches of a backward pass run (unet.UNet says WHAT they compute): which stream, which share of the chip, which
weight-gradient group, which workspace, when the side streams fork and join.

Weight-gradient launches can go to a second stream: they only READ what the main stream produced (dz, activations) and write gradients
nobody reads before the optimizer. Two persistent kernels then share the chip and each fills the other's poorly occupied last round of
tiles. RSU_WGRAD_STREAM=0 keeps everything on one stream.

The two streams SHARE the chip by plan (RSU_SPLIT_CHIP, default _SPLIT_DEFAULT, of 256): while the backward pass runs, launches on the
main stream (backward-data) plan their persistent workgroups for the first number of CUs, launches on the side stream (weight gradients)
for the second, so a backward-data and a weight-gradient kernel are resident together, each on its own CUs, instead of taking turns on
all of them. The weight gradient of a layer is a sum over one partial result PER WORKGROUP (a 295-KB slab each, written and read back by
the reduce kernel): half the workgroups, half that traffic -- and persistent kernels on fewer CUs lose less to their last, partly filled
round of tiles. "0" = both plan for every CU.
"""
import contextlib
import ctypes
import os
import sys

import torch

from . import _lib
from ._lib import RsuWgradJob, call

# RSU_WG_GROUP: how the weight gradients of a backward pass are launched (BackwardSchedule.flush). Default: one launch per layer where a
# side stream runs them beside the backward-data launches (each kernel on half the chip: per layer they are as efficient there as a
# group, and the fine grain keeps both streams busy to the end -- measured, profiles/r03/wg_group_schedules.txt), ONE grouped launch behind
# the pass where everything runs on one stream (alone on the chip a layer's launch pays 75 MB of slabs and a partly filled last round)
_WG_GROUP_TWO_STREAMS, _WG_GROUP_ONE_STREAM = "0", "all"
_WG_ALL = 10 ** 6            # blocks in a group of RSU_WG_GROUP=all
# RSU_RAW_EVENTS=0: fork the side stream through torch events (system-scope release) instead of _lib.hip_fork (agent scope)
_RAW_EVENTS = os.environ.get("RSU_RAW_EVENTS", "1") != "0"
_SPLIT_DEFAULT = "128,128"   # RSU_SPLIT_CHIP: CUs the main stream / each side stream plan for during the backward pass


def cu_shares(full, parts):
    """CUs the backward streams plan for: `parts` = RSU_SPLIT_CHIP as integers ([main, side, ...] out of 256), `full` = the CUs the backward pass
    may use in all (256, or a data-parallel budget that leaves CUs to RCCL's channel workgroups). With the default 128 + 128 and a budget of
    224 .. 255 the weight-gradient stream keeps its 128 -- its pixel splits and workgroup counts per XCD are powers of two: 120 + 120 costs c2
    8 % and c4 5 %, 112 + 128 costs 1.7 % and 3.6 % (profiles/r06/dp_budget.txt) -- and the backward-data stream, whose persistent kernels walk
    tile lists of any length, takes the rest. Below 224 the backward-data stream would starve (80 + 128: -16 %): shares in proportion, in
    steps of 8, at least 32 -- as for every other setting."""
    if full < 256 and list(parts) == [128, 128] and full >= 224:
        return [full - 128, 128]
    return [max(32, v * full // 256 // 8 * 8) for v in parts]


class BackwardSchedule:
    """The stream and CU-share schedule of one net. A backward pass moves through these states; ncu() is the `ncu` argument of a launch
    issued on the current stream in each (0: the library's default budget):

      idle        outside begin() .. end(): ncu() = 0. side() still forks to a side stream (the forward pass of a dilated net runs its
                  twin blocks there) but no share changes hands; join() brings the side streams back.
      whole chip  begin(budget): the main stream plans for the whole budget until something runs beside it.
      shared      from the exit of the pass's FIRST side() that really went to a side stream: the main stream plans for its share
                  (RSU_SPLIT_CHIP through cu_shares), every side() for its stream's share -- or for the whole budget with alone=True,
                  when the caller knows that nothing is left to run beside it. Never entered without side streams, with
                  RSU_SPLIT_CHIP=0 or with RSU_WG_GROUP=all.
      tail        inside tail(alone=True): the level-0 conv1 gradient on the main stream, behind a join, on the whole budget.
      joined      join() behind the last flush; end() (in a `finally`) returns to idle whatever happened.

    Weight gradients: while `grouped`, the caller hands them to queue() and reports block_done() behind a block's conv2 gradient; the
    schedule sends a group to a side stream when RSU_WG_GROUP says it is full, when flush() is called on behalf of a gradient exchange
    that is about to wait for the side streams, and behind the pass. Not `grouped`: the caller launches each one inside side().

    `streams` is the list the owner may empty and restore between passes (UNet.wstreams); workspaces are looked up by stream index, so
    they are found again when the list grows back. The owner allocates them: `ws_side[k]` the weight-gradient workspace of side stream k
    (their slabs are live at the same time; [0] is the main stream's too), `kws` / `kws_side[k]` the split-K workspaces of the conv
    launches (one per stream: whether a layer splits must never depend on which stream its launch went to)."""

    def __init__(self, device, batch, training, launch):
        """launch(tag, flops, entry point, *args): how the owner issues (and, when profiling, times) an ABI call"""
        self.device, self.batch, self.launch = device, batch, launch
        self.streams = []
        if training and device.type == "cuda" and os.environ.get("RSU_WGRAD_STREAM", "1") == "1":
            nside = max(1, len(os.environ.get("RSU_SPLIT_CHIP", _SPLIT_DEFAULT).split(",")) - 1)
            self.streams = [torch.cuda.Stream(device=device) for _ in range(nside)]
        self.ws_side, self.kws, self.kws_side = [], None, []
        self._raw_events = _RAW_EVENTS
        self._split = None     # (full, main, [side ...]) CU budgets while a backward pass shares the chip between the streams
        self._whole = 0        # what the main stream plans for before the chip is shared (0: the library's default budget)
        self._shared = False   # a launch has gone to a side stream in this backward pass
        self._at = None        # (side stream index, alone) inside side(), "tail" inside tail() on the main stream
        self._rr, self._dirty = 0, True
        # grouped weight gradients (rsu.h rsu_wgrad_group_*): the launches of RSU_WG_GROUP consecutive levels / decoder stages of the
        # backward pass go out as ONE launch (0: one launch per layer, as in round 2; "all": one group behind the whole pass)
        self._sizes, self._blocks, self._index = [0], 0, 0   # the policy of this pass, blocks in the open group, groups sent
        self.grouped = False                                 # weight gradients are queued, not launched one by one inside side()
        self._conv, self._convT = [], []                     # queued (job, flops, identity)
        self._plans = {}

    def begin(self, budget):
        """CU shares of the backward pass: `budget` (set by the data-parallel host: CUs left to RCCL's channel workgroups while the
        gradient exchange overlaps the backward pass; the forward pass keeps the whole chip; None: the library's default) shared out
        between the streams. Every launch carries its share as its own `ncu` argument: no library state changes between launches.
        RSU_WG_GROUP for this pass: "n" every group holds n blocks; "a,b,c" the first group a blocks, the second b, ... (the last number
        repeats); "all" one group behind the whole pass; "0" one launch per layer."""
        g = os.environ.get("RSU_WG_GROUP", _WG_GROUP_TWO_STREAMS if self.streams else _WG_GROUP_ONE_STREAM)
        self._sizes = [_WG_ALL] if g == "all" else [max(0, int(v)) for v in g.split(",")]
        self.grouped = self._sizes[0] > 0
        full = budget or _lib.lib().rsu_get_cu_budget()
        self._split, self._whole = None, full if budget else 0
        spec = os.environ.get("RSU_SPLIT_CHIP", _SPLIT_DEFAULT)
        if self.streams and spec not in ("0", "") and self._sizes[0] < _WG_ALL:   # (RSU_WG_GROUP=all: nothing runs beside backward-data)
            try:
                parts = [int(v) for v in spec.split(",")]
            except ValueError:
                return
            if len(parts) == len(self.streams) + 1 and min(parts) >= 1:
                parts = cu_shares(full, parts)
                self._split = (full, parts[0], parts[1:])

    def end(self):
        self._split, self._whole, self._shared, self._at, self._index = None, 0, False, None, 0

    def ncu(self):
        """the CUs a launch issued now, on the current stream, plans for"""
        if self._split is None:
            return self._whole
        full, main, sides = self._split
        if self._at is None:
            return main if self._shared else self._whole
        return full if self._at == "tail" or self._at[1] else sides[self._at[0]]

    @contextlib.contextmanager
    def side(self, alone=False):
        """`with schedule.side() as ws:` -- launches inside go to the next side stream (round robin), which waits for everything issued on
        the main stream so far, and plan for that stream's share of the chip (alone: nothing is left to run beside them on the main
        stream -- the whole budget); ws is its weight-gradient workspace. Without side streams they stay where they are."""
        if not self.streams:
            yield self.ws_side[0] if self.ws_side else None
            return
        k = self._rr % len(self.streams)
        self._rr += 1
        self._dirty = True
        main, stream = torch.cuda.current_stream(self.device), self.streams[k]
        if self._raw_events:
            # the fork costs the MAIN queue an idle gap per weight-gradient launch (the event's packet sits between two backward-data
            # kernels): ~6 us with a torch event, less without the system-scope fence a same-device dependency does not need
            try:
                _lib.hip_fork(main.cuda_stream, stream.cuda_stream, self.device.index)
            except (_lib.RsuError, OSError, AttributeError) as ex:   # no usable runtime handle: torch's events do the same, a little slower
                print("road_segmentation_unet_amd: raw HIP fork events unavailable (%r); using torch events" % (ex,), file=sys.stderr)
                self._raw_events = False
        if not self._raw_events:
            ev = torch.cuda.Event()
            ev.record(main)
            stream.wait_event(ev)
        self._at = (k, alone)
        try:
            with torch.cuda.stream(stream):
                yield self.ws_side[k]
        finally:
            self._at = None   # on error paths too
            if self._split is not None:
                self._shared = True   # from here on the main stream's launches share the chip with the side stream's

    def join(self):
        if not self._dirty:   # nothing has gone to a side stream since the last join: no wait packet on the main queue
            return
        for s in self.streams:
            torch.cuda.current_stream(self.device).wait_stream(s)
        self._dirty = False

    @contextlib.contextmanager
    def tail(self, alone):
        """where the level-0 conv1 gradient runs (as side(): yields its workspace). alone (no dilated twin of level 0 follows): the
        pass's last launch needs the backward-data kernel that has just gone out on the main stream and nothing runs beside it: on the
        main stream it follows back to back -- on the side stream it cost a fork and a join (~24 us of latency in the timeline). The
        side stream's last reduction must be done before the workspace is re-used: joined first. RSU_TAIL_MAIN=0: on a side stream."""
        if self._split is not None and alone and os.environ.get("RSU_TAIL_MAIN", "1") != "0":
            self.join()
            self._at = "tail"
            try:
                yield self.ws_side[0]
            finally:
                self._at = None
        else:
            with self.side(alone=alone) as ws:
                yield ws

    def kws_here(self):
        """the split-K workspace of the stream the next conv launch goes to (None: that launch never splits)"""
        if self._at is None or self._at == "tail":
            return self.kws
        return self.kws_side[self._at[0]] if self._at[0] < len(self.kws_side) else None

    def queue(self, job, flops, ident, transposed=False):
        """one RsuWgradJob for the next group; `ident` names it in the plan cache. (No event per queued job: the group forks where it is
        flushed, through the raw event of side() -- a torch event here would cost the main queue ~5 us between two backward-data kernels.)"""
        (self._convT if transposed else self._conv).append((job, flops, ident))

    def block_done(self):
        """The conv2 gradient of a block has been queued. (Not for level 0 of a net without dilated twins: that is the last group,
        flushed by the caller, which knows that nothing runs beside it.)
        A group closes BEHIND a conv2 gradient: dz of a block's conv2 is there when the block's backward pass begins, so the group
        {conv1 (+ transposed conv) of the block before, conv2 of this one} can run beside ALL of this block's backward-data launches;
        closing it behind conv1 would make it wait for the block's first backward-data launch."""
        self._blocks += 1
        if self._blocks >= self._sizes[min(self._index, len(self._sizes) - 1)]:
            self.flush()

    def flush(self, alone=False):
        """Launch the queued weight gradients as grouped launches on the side stream (everything they read has been produced by launches
        issued on the main stream before this point; side() makes the side stream wait for them). The plan of a group -- which layers,
        which CU share, which workspace -- is made once and kept (host table + its device copy, rsu.h rsu_wgrad_group_plan)."""
        if not self._conv and not self._convT:
            return   # (the data-parallel host asks per bucket boundary: an empty flush must not advance the group schedule)
        self._blocks = 0
        self._index += 1
        for pending, tag in ((self._conv, "conv3x3_bwd_weight"), (self._convT, None)):
            while pending:
                chunk = pending[:_lib.WGRAD_GROUP_MAX]
                del pending[:_lib.WGRAD_GROUP_MAX]
                with self.side(alone=alone) as ws:
                    ncu, st = self.ncu(), ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
                    key = (tuple(k for _, _, k in chunk), ncu, ws.data_ptr())
                    plan = self._plans.get(key)
                    if plan is None:
                        lib = _lib.lib()
                        host = ctypes.create_string_buffer(lib.rsu_wgrad_group_table_bytes())
                        arr = (RsuWgradJob * len(chunk))(*[j for j, _, _ in chunk])
                        _lib.check(lib.rsu_wgrad_group_plan(arr, len(chunk), ctypes.c_void_p(ws.data_ptr()), self.batch, ncu, host),
                                   "rsu_wgrad_group_plan")
                        devt = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(self.device)
                        plan = self._plans[key] = (host, devt)
                    devp = ctypes.c_void_p(plan[1].data_ptr())
                    if tag is None:
                        call("rsu_wgrad_group_run", plan[0], devp, st)
                    else:
                        self.launch(tag, sum(f for _, f, _ in chunk), "rsu_wgrad_group_run", plan[0], devp, st)
