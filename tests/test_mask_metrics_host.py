"""mask_metrics.layout / decode on the host (no library, no device): for every admissible combination of the --validate_* mask flags the
accumulator's layout is the stated one -- the stage lengths and offsets are written out here as literals, not taken from the module --
and decode() returns the keys evaluate() returned for that combination before the module existed, in that order, with the values of the
hostio functions on each stage's own counters."""
import itertools

import numpy as np
import pytest

from road_segmentation_unet_amd import hostio
from road_segmentation_unet_amd import mask_metrics as MM

SLACK = 3
CC_KEYS = ["components_pred", "components_true", "b0_error"]
DT_KEYS = ["dist_hist", "relaxed_precision", "relaxed_recall", "relaxed_f1", "mean_dist_pred", "mean_dist_true", "far_pred", "far_true"]
CL_KEYS = ["cl_hist", "cl_correctness", "cl_completeness", "cl_quality", "cldice_hard", "cl_len_pred", "cl_len_true", "thin_unconverged"]
JN_KEYS = ["jn_hist", "jn_precision", "jn_recall", "jn_f1", "junctions_pred", "junctions_true", "junction_error", "ends_pred", "ends_true",
           "isolated_pred", "isolated_true"]
SG_KEYS = [k + side for side in ("_pred", "_true") for k in ("segments", "road_length", "seg_len_mean", "dangling", "free", "rings", "multi",
                                                             "segments_dropped", "nodes")] + ["length_ratio"]

# (components, distances, centerlines, min_branch, junctions, segments): 2^3, and under centre-lines every min_branch x junctions x segments
COMBOS = [(cc, dt, False, 0, False, False) for cc, dt in itertools.product((False, True), repeat=2)] \
    + [(cc, dt, True, mb, jn, sg) for cc, dt in itertools.product((False, True), repeat=2)
       for mb, jn, sg in itertools.product((0, 2), (False, True), (False, True))]
assert len(COMBOS) == 4 + 4 * 8


def _same(got, want):
    assert list(got) == list(want)
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert got[k].dtype == np.int64 and got[k].shape == v.shape and np.array_equal(got[k], v), k
        else:
            assert type(got[k]) is type(v) and got[k] == v, (k, got[k], v)


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "cc%d-dt%d-cl%d-mb%d-jn%d-sg%d" % tuple(int(v) for v in c))
def test_layout_and_decode(combo):
    cc, dt, cl, mb, jn, sg = combo
    flags = MM.Flags(*combo)
    gr = cl and (mb > 0 or jn)
    lay = MM.layout(flags)
    # the stages present, in the stated order, each with its literal length; together they cover [0, total) without a gap or an overlap
    stages = [(n, length) for n, on, length in (("components", cc, 4), ("distances", dt, 128), ("centerlines", cl, 128 + 4 + 1),
                                                ("graph", gr, 8 + 128 + 4), ("segments", sg, 16 + 4)) if on]
    total = sum(length for _, length in stages)
    assert [k for k in lay if "." not in k] == [n for n, _ in stages] and MM.total(flags) == total
    at = 0
    for name, length in stages:
        assert lay[name] == slice(at, at + length), (name, lay[name])
        parts = [v for k, v in lay.items() if k.startswith(name + ".")]
        assert parts and parts[0].start == at and parts[-1].stop == at + length and all(a.stop == b.start for a, b in zip(parts, parts[1:]))
        at += length
    assert at == total and all(s.step is None and 0 <= s.start < s.stop <= total for s in lay.values())
    assert {k.split(".")[0] for k in lay} == {n for n, _ in stages}      # a stage that is off has no name, and no part either
    # decode on distinct small integers against the hostio functions on slices cut by the literal offsets
    v = np.arange(1, total + 1, dtype=np.float64)
    c = np.arange(1, total + 1, dtype=np.int64)
    want, at = {}, 0
    if cc:
        want.update(components_pred=int(c[at]), components_true=int(c[at + 1]), b0_error=float(c[at + 2]) / float(c[at + 3]))
        at += 4
    if dt:
        want["dist_hist"] = c[at:at + 128].reshape(2, 64)
        want.update(hostio.relaxed_metrics(want["dist_hist"], SLACK))
        at += 128
    if cl:
        want["cl_hist"] = c[at:at + 128].reshape(2, 64)
        want.update(hostio.centerline_metrics(want["cl_hist"], c[at + 128:at + 132], SLACK))
        want["thin_unconverged"] = int(c[at + 132])
        at += 133
    if gr:
        if mb > 0:      # the pruned lines' pixel counts replace the unpruned ones in place; cldice_hard stays
            want["cl_len_pred"], want["cl_len_true"] = int(c[at]), int(c[at + 4])
        if jn:
            want["jn_hist"] = c[at + 8:at + 136].reshape(2, 64)
            want.update(hostio.graph_metrics(want["jn_hist"], c[at + 136:at + 140], c[at:at + 8], SLACK))
        at += 140
    if sg:
        want.update(hostio.segment_metrics(c[at:at + 16].reshape(2, 8), c[at + 16:at + 20]))
        at += 20
    assert at == total
    got = MM.decode(flags, v, SLACK)
    # the keys evaluate() added for this combination, in its order
    assert list(got) == CC_KEYS * cc + DT_KEYS * dt + CL_KEYS * cl + JN_KEYS * bool(cl and jn) + SG_KEYS * sg
    _same(got, want)
    if total:
        with pytest.raises(ValueError):
            MM.decode(flags, v[:-1], SLACK)


def test_flags_that_need_centerlines_add_nothing_without_them():
    bare = MM.Flags()
    assert not bare.any and MM.layout(bare) == {} and MM.total(bare) == 0 and MM.decode(bare, np.zeros(0), SLACK) == {}
    for kw in (dict(junctions=True), dict(segments=True), dict(min_branch=2), dict(min_branch=2, junctions=True, segments=True)):
        assert MM.Flags(**kw) == bare and MM.layout(MM.Flags(**kw)) == {}
        with_dt = MM.Flags(distances=True, **kw)
        assert with_dt == MM.Flags(distances=True) and list(MM.layout(with_dt)) == ["distances", "distances.hist"]
    cl = MM.Flags(centerlines=True)
    assert cl.any and not cl.graph and MM.Flags(centerlines=True, min_branch=2).graph and MM.Flags(centerlines=True, junctions=True).graph


def test_flags_of_options():
    class O:
        validate_distances, validate_centerlines, centerline_min_branch, validate_segments = True, True, 5, True
    assert MM.Flags.of(O()) == MM.Flags(False, True, True, 5, False, True)
    assert MM.Flags.of(object()) == MM.Flags()
