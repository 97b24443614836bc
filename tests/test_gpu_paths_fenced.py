"""-m gpu: the launching entry point of include/rsu_paths.h inside a fenced arena (tests/fence_util.py), as
tests/test_gpu_segments_fenced.py holds that of include/rsu_segments.h, and under the placements and workspace fills that
tests/test_gpu_aligned_min.py and tests/test_gpu_ws_history.py run for the entries of the first ten headers (their registries enumerate
exactly those ten, so this header's runs live here): rsu_segment_paths with pos and without, on a thinned and pruned pair and on a stack
whose images converge at different jump launches (a line of 1400 pixels, a few short ones, nothing), with max_len above the line and
exactly at it. The workspace has exactly rsu_paths_ws_bytes bytes. After Arena.check the results are compared with hostio.segment_paths
byte for byte; elements the entry does not touch must still hold the arena's pattern.

  test_paths_entry                 every payload on a 256-byte boundary, the workspace as pattern;
  test_paths_entry_at_its_minimum  every payload at a 256-byte boundary plus exactly its alignment (int32: 4, ws: 8);
  test_paths_workspace_history     the workspace zeroed, 0xFF-filled and rolled, put back in front of every call: the bytes of the pattern run.

FENCED is the registry tests/test_paths_host.py checks without a GPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import fence_util as F  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests import paths_util as PU  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

PATTERN32 = 0x7FA57FA5      # what an int32 of an arena holds before a launch
CASES = {"thinned": 4096, "uneven": 4096, "uneven_exact": 1400}      # case -> max_len
OUTS = ("paths", "offsets", "kind", "pos", "info", "paths2", "offsets2", "kind2", "info2")
ALIGN = dict({n: 4 for n in ("seg", "edges", "counts") + OUTS}, ws=8)      # the header's align note


def _inputs(case):
    if case == "thinned":
        return PU.bank_inputs("smooth1.5~smooth3", (2, 230, 97), 8, 0)
    return PU.inputs_of(PU.uneven(), cap=8)


def _launch(A, shape, cap, max_len, max_points, st):
    """with pos, then without; the workspace starts from the placement's fill both times"""
    q = lambda n: hu.ptr(A[n])  # noqa: E731
    A.refill("ws")
    call("rsu_segment_paths", q("seg"), q("edges"), q("counts"), 0, cap, max_len, max_points, q("paths"), q("offsets"), q("kind"), q("pos"),
         q("info"), q("ws"), *shape, st)
    A.refill("ws")
    call("rsu_segment_paths", q("seg"), q("edges"), q("counts"), 0, cap, max_len, max_points, q("paths2"), q("offsets2"), q("kind2"), None,
         q("info2"), q("ws"), *shape, st)


def _case(case, placement="aligned"):
    """one fenced run; returns {output name: bytes}"""
    max_len = CASES[case]
    seg, edges, counts = (np.array(a) for a in _inputs(case))
    shape, cap = seg.shape, edges.shape[1]
    max_points = shape[1] * shape[2]
    nbytes = int(lib().rsu_paths_ws_bytes(*shape, cap, max_len))
    assert nbytes == PU.ws_layout(*shape, cap, max_len) and nbytes % 8 == 0
    specs = [F.raw("seg", seg), F.raw("edges", edges), F.raw("counts", counts)]
    for sfx in ("", "2"):
        specs += [F.out("paths" + sfx, (shape[0], max_points), torch.int32), F.out("offsets" + sfx, (shape[0], cap + 1), torch.int32),
                  F.out("kind" + sfx, (shape[0], cap), torch.int32), F.out("info" + sfx, (shape[0], 4), torch.int32)]
    specs += [F.out("pos", shape, torch.int32), F.ws("ws", nbytes // 8, dtype=torch.int64)]
    A = F.Arena(hu.DEV, specs, placement=placement)
    if A.placement.mode == "minimum":      # a multiple of its number and of nothing larger
        for s in specs:
            assert A[s.name].data_ptr() % (2 * ALIGN[s.name]) == ALIGN[s.name], s.name
    _launch(A, shape, cap, max_len, max_points, hu.stream())
    what = "paths fenced %s" % case
    A.check(what)
    got = {n: A[n].cpu().numpy() for n in OUTS}
    want = hostio.segment_paths(seg, edges, counts, 0, max_len, max_points, fill=PATTERN32)
    for sfx in ("", "2"):
        for name, w in zip(PU.NAMES, want):
            if name == "pos" and sfx:
                continue
            assert got[name + sfx].tobytes() == w.tobytes(), (what, name + sfx)
    assert (want[2] == PATTERN32).any() and (want[0] == PATTERN32).any() and want[4][:, 0].max() > 100, what      # untouched elements, and work
    if case != "thinned":      # the line of image 0 is ordered whole; the images need eleven, three and no doublings
        assert want[4].tolist() == [[1400, 1, 0, 0], [15, 3, 0, 0], [0, 0, 0, 0]] and PU.rounds(max_len) >= 11
    return {n: g.tobytes() for n, g in got.items()}


@pytest.mark.parametrize("case", sorted(CASES))
def test_paths_entry(case):
    _case(case)


@pytest.mark.parametrize("case", sorted(CASES))
def test_paths_entry_at_its_minimum(case):
    assert _case(case, F.Placement("minimum", [{"ws": 8}])) == _case(case)


@pytest.mark.parametrize("fill", ("zeros", "ones", "rolled"))
@pytest.mark.parametrize("case", sorted(CASES))
def test_paths_workspace_history(case, fill):
    first = F.Placement("aligned", fill="pattern")
    want = _case(case, first)
    snaps = first.workspaces()
    assert list(snaps) == [(0, "ws")]
    got = _case(case, F.Placement("aligned", fill=fill, snapshots=snaps))
    bad = [n for n in OUTS if got[n] != want[n]]
    assert not bad, "workspace fill %r changed %s" % (fill, bad)


# ------------------------------------------------------------------------------------------- the registry (tests/test_paths_host.py)
FENCED = {"rsu_segment_paths": ["test_paths_entry", "test_paths_entry_at_its_minimum", "test_paths_workspace_history"]}
HELPERS = {n: (_case, _launch) for n in FENCED["rsu_segment_paths"]}
