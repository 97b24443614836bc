"""-m gpu: the launching entry points of include/rsu_components.h inside a fenced arena (tests/fence_util.py), as
tests/test_gpu_lovasz_fenced.py holds those of include/rsu_lovasz.h: rsu_components_label, rsu_components_filter and
rsu_components_pair_count at (3, 63, 65) -- two tiles per image, the second one column wide -- and at (2, 130, 67): three by two tiles,
both axes partial, two merge levels. The workspace has exactly rsu_components_ws_bytes bytes and starts as pattern. After Arena.check the
results are compared with the host restatements of hostio.

FENCED is the registry tests/test_components_host.py checks against include/rsu_components.h without a GPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import components_util as CU  # noqa: E402
from tests import fence_util as F  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

SHAPES = [(3, 63, 65), (2, 130, 67)]
MIN_AREA, MAX_HOLE = 20, 20


def _launch(A, shape, connectivity, st):
    """the labelling of the mask with and of its complement without area and edge, the clean-up into `out` and in place, the pair count"""
    p = lambda n: hu.ptr(A[n])  # noqa: E731
    call("rsu_components_label", p("prob"), CU.THRESHOLD, connectivity, 0, p("labels"), p("area"), p("edge"), p("ws"), *shape, st)
    call("rsu_components_label", p("prob"), CU.THRESHOLD, connectivity, 1, p("labels_inv"), None, None, p("ws"), *shape, st)
    call("rsu_components_filter", p("prob"), CU.THRESHOLD, connectivity, MIN_AREA, MAX_HOLE, p("out"), p("stats"), p("ws"), *shape, st)
    call("rsu_components_filter", p("inplace"), CU.THRESHOLD, connectivity, MIN_AREA, MAX_HOLE, p("inplace"), None, p("ws"), *shape, st)
    call("rsu_components_pair_count", p("prob"), CU.THRESHOLD, p("labels64"), connectivity, p("acc"), p("ws"), *shape, st)


@pytest.mark.parametrize("connectivity", CU.CONNECTIVITIES)
@pytest.mark.parametrize("shape", SHAPES, ids=[CU.shape_id(s) for s in SHAPES])
def test_components_entries(shape, connectivity, placement="aligned"):
    prob = CU.float_bank(shape)
    labels64 = CU.pair_labels(shape)
    nbytes = int(lib().rsu_components_ws_bytes(*shape))
    assert nbytes == 20 * int(np.prod(shape)) + 16 * shape[0]
    specs = [F.f32("prob", prob), F.raw("labels64", labels64), F.out("labels", shape, torch.int32), F.out("area", shape, torch.int32),
             F.out("edge", shape, torch.uint8), F.out("labels_inv", shape, torch.int32), F.out("out", shape, torch.float32),
             F.out("stats", (shape[0], 6), torch.int64), F.state("inplace", prob), F.state("acc", np.zeros(4, np.int64)),
             F.ws("ws", nbytes // 4, dtype=torch.int32)]
    A = F.Arena(hu.DEV, specs, placement=placement)
    _launch(A, shape, connectivity, hu.stream())
    what = "components fenced %s %d" % (shape, connectivity)
    A.check(what)
    got = {n: A[n].cpu().numpy() for n in ("labels", "area", "edge", "labels_inv", "out", "stats", "inplace", "acc")}
    lab, area, edge = hostio.label_components(prob, CU.THRESHOLD, connectivity)
    assert np.array_equal(got["labels"], lab) and np.array_equal(got["area"], area) and np.array_equal(got["edge"], edge), what
    assert np.array_equal(got["labels_inv"], hostio.label_components(prob, CU.THRESHOLD, connectivity, True)[0]), what
    out, stats = hostio.filter_components(prob, CU.THRESHOLD, connectivity, MIN_AREA, MAX_HOLE)
    assert stats[:, 2].sum() > 0 and stats[:, 5].sum() > 0
    assert np.array_equal(CU.bits(got["out"]), CU.bits(out)) and np.array_equal(got["stats"], stats), what
    assert np.array_equal(CU.bits(got["inplace"]), CU.bits(out)), what
    assert np.array_equal(got["acc"], hostio.components_pair_count(prob, CU.THRESHOLD, labels64, connectivity)), what


# ------------------------------------------------------------------------------------------- the registry (tests/test_components_host.py)
# launching entry of include/rsu_components.h -> the cases that launch it inside an arena (HELPERS: what a case calls it through)
FENCED = {
    "rsu_components_label": ["test_components_entries"],
    "rsu_components_filter": ["test_components_entries"],
    "rsu_components_pair_count": ["test_components_entries"],
}
NOT_FENCED = {}
HELPERS = {"test_components_entries": (_launch,)}
