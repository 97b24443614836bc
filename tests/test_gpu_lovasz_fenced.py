"""-m gpu: the launching entry points of include/rsu_lovasz.h inside a fenced arena (tests/fence_util.py), as tests/test_gpu_cldice_fenced.py
holds those of include/rsu_cldice.h: rsu_lovasz_fwd and rsu_lovasz_fwd_bwd at (3, 37, 41) -- one LDS tile per image, most of it padding --
and at (2, 17, 241): 4097 pixels, two tiles per image, the second one pixel and 4095 zero keys, one merge through global memory -- with
tied values and ignored labels. The workspace has exactly rsu_lovasz_ws_bytes bytes. After Arena.check: no NaN in any result (an element
never written, or a stray read of the bands, is one), and the results against the host mirror of tests/test_gpu_lovasz.py.

FENCED is the registry tests/test_lovasz_host.py checks against include/rsu_lovasz.h without a GPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import fence_util as F  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests import lovasz_util as LU  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

SHAPES = [(3, 37, 41), (2, 17, 241)]


def _launch(A, shape, st):
    """the forward alone, then forward + backward overwriting, then accumulating on a given gradient: each with sums of its own"""
    p = lambda n: hu.ptr(A[n])  # noqa: E731
    call("rsu_lovasz_fwd", p("prob"), p("labels"), p("loss_f"), p("ws"), *shape, st)
    call("rsu_lovasz_fwd_bwd", p("prob"), p("labels"), LU.SCALE, 0, p("gprob"), p("loss_b"), p("ws"), *shape, st)
    call("rsu_lovasz_fwd_bwd", p("prob"), p("labels"), LU.SCALE, 1, p("gacc"), p("loss_a"), p("ws"), *shape, st)


@pytest.mark.parametrize("kind", ["quant4", "scattered_ignored"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_lovasz_fwd_and_fwd_bwd(shape, kind, placement="aligned"):
    p, labels = LU.INPUTS[kind](shape)
    if kind == "quant4":
        labels = LU.scattered_ignored(shape)[1]
    assert ((labels != 0) & (labels != 1)).sum() > labels.size // 20
    g0 = np.random.RandomState(3).standard_normal(shape).astype(np.float32)
    nbytes = int(lib().rsu_lovasz_ws_bytes(*shape))
    assert nbytes > 0 and nbytes % 4 == 0
    z2 = lambda name: F.state(name, np.zeros(2, np.float32))  # noqa: E731
    specs = [F.f32("prob", p), F.raw("labels", labels), F.out("gprob", shape, torch.float32), F.state("gacc", g0), z2("loss_f"), z2("loss_b"),
             z2("loss_a"), F.ws("ws", nbytes // 4, dtype=torch.int32)]
    A = F.Arena(hu.DEV, specs, placement=placement)
    _launch(A, shape, hu.stream())
    what = "Lovasz fenced %s %s" % (shape, kind)
    A.check(what)
    for n in ("gprob", "gacc", "loss_f", "loss_b", "loss_a"):
        assert not bool(torch.isnan(A[n]).any()), (what, n)
    got = {n: A[n].cpu().numpy() for n in ("gprob", "gacc", "loss_f", "loss_b", "loss_a")}
    assert np.array_equal(got["gprob"].view(np.uint32), hostio.lovasz_gradient(p, labels, LU.SCALE).view(np.uint32)), what
    assert np.array_equal(got["gacc"].view(np.uint32), hostio.lovasz_gradient(p, labels, LU.SCALE, into=g0).view(np.uint32)), what
    total = float(hostio.lovasz_loss(p, labels).astype(np.float64).sum())
    n = shape[1] * shape[2]
    bound = LU.sum_bound(LU.host_depth(n) + LU.gpu_depth(shape), total)
    for k in ("loss_f", "loss_b", "loss_a"):
        assert abs(float(got[k][0]) - total) <= bound and got[k][1] == shape[0], (what, k, got[k], total, bound)
        assert np.array_equal(got[k].view(np.uint32), got["loss_f"].view(np.uint32)), (what, k)


# ------------------------------------------------------------------------------------------- the registry (tests/test_lovasz_host.py)
# launching entry of include/rsu_lovasz.h -> the cases that launch it inside an arena (HELPERS: what a case calls it through)
FENCED = {
    "rsu_lovasz_fwd": ["test_lovasz_fwd_and_fwd_bwd"],
    "rsu_lovasz_fwd_bwd": ["test_lovasz_fwd_and_fwd_bwd"],
}
NOT_FENCED = {}
HELPERS = {"test_lovasz_fwd_and_fwd_bwd": (_launch,)}
