"""-m gpu: include/rsu_graph.h against the host restatement hostio.skeleton_graph (which tests/test_graph_host.py holds to the topology of
its input and to hand cases): rsu_skeleton_graph over the bank of tests/thin_util.py -- every kind as the prediction against the next as
the truth, raw and pre-thinned -- at shapes from one pixel to the tiling's limits and at min_branch 0, 1, R - 1, R, R + 1, 2 R + 1 and 64;
a line with spurs of 1 .. 2 R + 2 pixels and a ring across a four-tile corner; ignored labels kept verbatim; the float bank; the NULL
variants; in-place outputs; accumulation; two runs byte for byte; ConvolutionalModel.evaluate() with --centerline_min_branch and
--validate_junctions, centerlines() and the command line's --save_centerlines above it. Every comparison is equality of the bytes."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from tests import components_util as CU  # noqa: E402
from tests import graph_util as GU  # noqa: E402
from tests import thin_util as TU  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402

NAMES = ("out_pred", "out_true", "junc_pred", "junc_true", "acc")


def _np(t):
    return None if t is None else t.cpu().numpy()


def _dev(labels):
    return torch.from_numpy(np.array(labels)).to(hu.DEV)   # (a copy: the bank's arrays are read-only)


def _same(got, want, what):
    """byte for byte: the float32 and int64 outputs, acc as int64 [8]; an output not asked for is None on the device side"""
    for name, g, w in zip(NAMES, got, want):
        g = _np(g)
        if g is None:
            continue
        assert w is not None and g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert g.tobytes() == w.tobytes(), (what, name, int((g != w).sum()), g if name == "acc" else None, w if name == "acc" else None)


# ------------------------------------------------------------------------------------------- the bank
@pytest.mark.parametrize("pre_thinned", [False, True], ids=["raw", "thinned"])
@pytest.mark.parametrize("shape", GU.SHAPES, ids=[GU.shape_id(s) for s in GU.SHAPES])
def test_skeleton_graph_equals_the_host_over_the_bank(shape, pre_thinned):
    pruned = nodes = 0
    for name in TU.pair_names():
        prob, labels = GU.pair(name, shape, pre_thinned)
        pt, lt = hu.dev_f32(np.array(prob)), _dev(labels)
        for L in GU.BRANCHES:
            want = GU.host_pair(name, shape, pre_thinned, L)
            _same(GU.run_graph(pt, lt, shape, L), want, (name, shape, pre_thinned, L))
            pruned += int(want[4][0] < GU.host_pair(name, shape, pre_thinned, 0)[4][0])
            nodes += int(want[4][1] > 0 and want[4][3] > 0)
    if min(shape[1:]) > 8:   # the cases are not trivial: pruning removes pixels, and ends and junction pixels exist
        assert pruned > 0 and nodes > 0


def test_spurs_and_a_ring_across_a_four_tile_corner():
    """a line with spurs of 1 .. 2 R + 2 pixels along the last core row above a tile border, crossing three word columns, against a ring
    around the same corners: every delete and regrow launch passes branch tips through the halo. At min_branch L the spurs longer than L
    are whole (away from the line's ends); the ring is untouched at every L"""
    shape = GU.CORNER_SHAPE
    line, ring = GU.corner_line(), GU.corner_ring()
    for pred, true in ((line, ring), (ring, line)):
        prob, labels = CU.prob_of(pred), true.astype(np.int64)
        pt, lt = hu.dev_f32(prob), _dev(labels)
        for L in GU.BRANCHES:
            want = hostio.skeleton_graph(prob, GU.THRESHOLD, labels, L)
            _same(GU.run_graph(pt, lt, shape, L), want, ("corner", L))
            ring_side = want[1] if pred is line else want[0]
            assert np.array_equal(ring_side > 0, ring)
            if pred is line and 0 < L <= GU.R + 1:
                col = (want[0][0] > 0).sum(axis=0) - 1                       # what is left of each spur
                spur = line[0].sum(axis=0) - 1
                far = (np.arange(shape[2]) > L + 1) & (np.arange(shape[2]) < shape[2] - L - 2)
                assert (col[far & (spur > L)] == spur[far & (spur > L)]).all(), L
                # (the spurs stand three columns apart: at larger L the ends of the surviving ones grow back into their neighbours'
                # stubs, the artefact the header documents; at L = 1 nothing is that close)
                assert L > 1 or not col[far & (spur <= L)].any()
                assert want[4][0] < line.sum()


# ------------------------------------------------------------------------------------------- floats and labels
@pytest.mark.parametrize("shape", [(2, 230, 97), (3, 63, 65)], ids=GU.shape_id)
def test_float_bank_and_ignored_labels(shape):
    """the threshold itself, the float below it, -0.0, NaNs and infinities: one float32 comparison decides; labels -1, 2 and
    (1 << 32) | 1 are not counted and not truth, all 64 bits tested; they are background on both sides and stay verbatim in the two
    *_true outputs"""
    p = CU.float_bank(shape)
    labels = TU.mixed_labels(shape)
    ignored = (labels != 0) & (labels != 1)
    assert (labels == ((1 << 32) | 1)).sum() > 100 and (labels == 2).sum() > 100 and (labels == -1).sum() > 100
    for thr, L in ((GU.THRESHOLD, 3), (-0.25, GU.R + 1)):
        want = hostio.skeleton_graph(p, thr, labels, L)
        got = GU.run_graph(hu.dev_f32(p), _dev(labels), shape, L, threshold=thr)
        _same(got, want, (shape, thr))
        for k in (1, 3):
            t = _np(got[k])
            assert np.array_equal(t[ignored], labels[ignored]) and set(np.unique(t[~ignored])) <= {0, 1}
        assert not _np(got[0])[ignored | np.isnan(p)].any() and not _np(got[2])[ignored | np.isnan(p)].any()
    if shape[0] > 1:   # the padding image of an evaluation chunk: nothing in any output, nothing counted
        assert np.array_equal(hostio.skeleton_graph(p[:-1], -0.25, labels[:-1], GU.R + 1)[4], want[4])
        assert not _np(got[0])[-1].any() and (_np(got[1])[-1] == -1).all() and (_np(got[3])[-1] == -1).all()


def test_null_variants():
    shape = (2, 230, 97)
    name = "smooth1.5~smooth3"
    L = GU.R + 1
    prob, labels = GU.pair(name, shape, True)
    want = GU.host_pair(name, shape, True, L)
    assert (want[4][[0, 1, 3, 4, 5, 7]] > 0).all()
    pt, lt = hu.dev_f32(np.array(prob)), _dev(labels)
    for k in range(4):   # each output alone, with and without acc
        only = tuple(i == k for i in range(4))
        got = GU.run_graph(pt, lt, shape, L, want=only)
        assert [g is not None for g in got[:4]] == list(only)
        _same(got, want, "only %s" % NAMES[k])
        _same(GU.run_graph(pt, lt, shape, L, want=only, want_acc=False), want, "only %s, acc = NULL" % NAMES[k])
    _same(GU.run_graph(pt, lt, shape, L, want_acc=False), want, "acc = NULL")
    _same(GU.run_graph(pt, lt, shape, L, want=(True, False, True, False)), want, "the prediction's outputs with labels")
    # labels64 = NULL: every pixel is counted, T is empty
    mixed = TU.mixed_labels(shape)
    for b in (0, L):
        free = hostio.skeleton_graph(prob, GU.THRESHOLD, None, b)
        assert free[1] is None and free[3] is None and not free[4][4:].any() and free[4][0] > 0
        _same(GU.run_graph(pt, None, shape, b, want=(True, False, True, False)), free, "labels64 = NULL")
    with_ignored = hostio.skeleton_graph(prob, GU.THRESHOLD, mixed, L)
    assert not np.array_equal(with_ignored[0], free[0])                     # (the ignored pixels do change the prediction's mask)
    _same(GU.run_graph(pt, _dev(mixed), shape, L), with_ignored, "mixed labels")


def test_in_place_outputs_equal_separate_ones():
    """out_pred == prob and out_true == labels64, as evaluate() calls the entry on rsu_mask_thin's outputs"""
    shape = (2, 230, 97)
    p, labels = CU.float_bank(shape), TU.mixed_labels(shape)
    for L in (0, 3, GU.R + 1, 64):
        want = hostio.skeleton_graph(p, GU.THRESHOLD, labels, L)
        pt, lt = hu.dev_f32(p), _dev(labels)
        got = GU.run_graph(pt, lt, shape, L, in_place=True)
        assert got[0].data_ptr() == pt.data_ptr() and got[1].data_ptr() == lt.data_ptr()
        _same(got, want, ("in place", L))
        again = GU.run_graph(pt, lt, shape, 0)                               # the pruned pair is a pair of masks like any other
        _same(again, hostio.skeleton_graph(want[0], GU.THRESHOLD, want[1], 0), ("in place, again", L))


# ------------------------------------------------------------------------------------------- accumulation
def test_acc_accumulates_and_an_ignored_image_adds_nothing():
    shape = (3, 63, 65)
    L = 3
    p, labels = CU.float_bank(shape), TU.mixed_labels(shape)                # its last image is ignored altogether
    want = hostio.skeleton_graph(p, GU.THRESHOLD, labels, L)[4]
    assert (want[[0, 1, 3, 4, 5, 7]] > 0).all()
    pt, lt = hu.dev_f32(p), _dev(labels)
    acc = GU.run_graph(pt, lt, shape, L)[4]
    assert np.array_equal(_np(acc), want)
    GU.run_graph(pt, lt, shape, L, acc=acc)
    assert np.array_equal(_np(acc), 2 * want)
    head = (2,) + shape[1:]
    assert np.array_equal(_np(GU.run_graph(hu.dev_f32(p[:2]), _dev(labels[:2]), head, L)[4]), want)
    got = GU.run_graph(pt, torch.full(shape, -1, dtype=torch.int64, device=hu.DEV), shape, L, acc=acc)
    assert np.array_equal(_np(acc), 2 * want) and not _np(got[0]).any() and (_np(got[1]) == -1).all() and (_np(got[3]) == -1).all()


def test_two_runs_give_identical_bytes():
    shape = (2, 230, 97)
    p = CU.float_bank(shape)
    lt = _dev(TU.mixed_labels(shape))
    runs = []
    for _ in range(2):
        got = [_np(t) for t in GU.run_graph(hu.dev_f32(p), lt, shape, GU.R + 1)]
        runs.append([a.tobytes() for a in got])
    assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------- the model
ML, MROOT, MP, MB = 3, 16, 20, 2      # the small config of the other model tests


def _model(**kw):
    from road_segmentation_unet_amd.model import ConvolutionalModel, Options
    o = dict(num_layers=ML, root_size=MROOT, patch_size=MP, batch_size=MB, dilated_layers=True, dropout=1.0, lr=0.01, seed=5, logdir=None)
    o.update(kw)
    return ConvolutionalModel(Options(**o), device="cuda:0", params=U.init_params(ML, MROOT, True, seed=13, bias_scale=0.05))


def _patches(n, seed=21):
    """random inputs; labels of smooth blobs, so that the truth has something to thin"""
    S = U.input_size_needed(MP, ML)
    rng = np.random.RandomState(seed)
    return rng.rand(n, S, S, 3).astype(np.float32), TU.masks("smooth1.5", (n, MP, MP)).astype(np.int64)


CL_KEYS = {"cl_hist", "cl_correctness", "cl_completeness", "cl_quality", "cldice_hard", "cl_len_pred", "cl_len_true", "thin_unconverged"}
JN_KEYS = {"jn_hist", "jn_precision", "jn_recall", "jn_f1", "junctions_pred", "junctions_true", "junction_error", "ends_pred", "ends_true",
           "isolated_pred", "isolated_true"}


def _chunks(m, X, y):
    """(net.prob, labels) of every chunk evaluate() runs, the last one padded with zero patches labelled -1"""
    net, B, N = m.net, m.local_batch, len(X)
    out = []
    for t0 in range(0, N, B):
        nb = min(B, N - t0)
        xb, yb = np.zeros((B,) + X.shape[1:], np.float32), np.full((B, MP, MP), -1, np.int64)
        xb[:nb], yb[:nb] = X[t0:t0 + nb], y[t0:t0 + nb]
        net.x.copy_(torch.from_numpy(xb))
        net.labels.copy_(torch.from_numpy(yb))
        net.forward_device(keep=1.0)
        net.evaluate_device()   # (the head writes net.prob)
        out.append((net.prob.cpu().numpy().reshape(B, MP, MP).copy(), yb))
    return out


def _host_composition(chunks, thr, max_iters, min_branch, slack, junctions):
    """mask_thin -> skeleton_graph on its outputs -> distance_hist of the pruned skeletons, and of the junction pixels, and their clusters
    by scipy: what evaluate() must return. Also whether pruning changed every live image"""
    hist, thin_counts, counts = np.zeros((2, 64), np.int64), np.zeros(4, np.int64), np.zeros(8, np.int64)
    jn_hist, jn_counts, changed = np.zeros((2, 64), np.int64), np.zeros(4, np.int64), []
    for prob, yb in chunks:
        sp, st, c, _ = hostio.mask_thin(prob, thr, yb, max_iters)
        op, ot, jp, jt, k = hostio.skeleton_graph(sp, 0.5, st, min_branch)
        hist += hostio.distance_hist(op, 0.5, ot)
        thin_counts += c
        counts += k
        counted = (yb == 0) | (yb == 1)
        for n in range(len(yb)):
            if counted[n].any():
                changed.append(bool((op[n] != sp[n]).any() or (ot[n] != st[n]).any()))
                a, b = CU.scipy_count(jp[n] > 0, 8), CU.scipy_count((jt[n] == 1) & counted[n], 8)
                jn_counts += (a, b, abs(a - b), 1)
        jn_hist += hostio.distance_hist(jp, 0.5, jt)
    want = hostio.centerline_metrics(hist, thin_counts, slack)
    if min_branch > 0:
        want["cl_len_pred"], want["cl_len_true"] = int(counts[0]), int(counts[4])
    want["cl_hist"] = hist
    if junctions:
        want["jn_hist"] = jn_hist
        want.update(hostio.graph_metrics(jn_hist, jn_counts, counts, slack))
    return want, changed, counts


def _check(out, want):
    for k, v in want.items():
        assert np.array_equal(out[k], v) if isinstance(v, np.ndarray) else out[k] == v, (k, out[k], v)


def test_evaluate_with_pruning_and_junctions(monkeypatch):
    from road_segmentation_unet_amd import mask_metrics as M      # (it issues the calls)
    N = 5
    X, y = _patches(N)
    y[1, :3] = -1
    m = _model(validate_centerlines=True, centerline_min_branch=2, validate_junctions=True, relaxed_slack=2)
    chunks = _chunks(m, X, y)
    thr = round(float(np.median(np.concatenate([c[0].reshape(-1) for c in chunks]))) * 256.0) / 256.0
    calls = []
    real = M.call
    monkeypatch.setattr(M, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    out = m.evaluate(X, y, threshold=thr)
    assert calls.count("rsu_mask_thin") == 3 and calls.count("rsu_skeleton_graph") == 3
    assert calls.count("rsu_distance_hist") == 6 and calls.count("rsu_components_pair_count") == 3
    per_chunk = [c for c in calls if c in ("rsu_mask_thin", "rsu_skeleton_graph", "rsu_distance_hist", "rsu_components_pair_count")][:5]
    assert per_chunk == ["rsu_mask_thin", "rsu_skeleton_graph", "rsu_distance_hist", "rsu_distance_hist", "rsu_components_pair_count"]
    want, changed, counts = _host_composition(_chunks(m, X, y), thr, 64, 2, 2, True)
    assert len(changed) == N and all(changed)                         # pruning changes every image
    assert want["junctions_true"] > 0 and counts[5] > 0               # the truth has junctions and ends at this size
    assert CL_KEYS | JN_KEYS <= set(out) and out["jn_hist"].dtype == np.int64 and out["jn_hist"].shape == (2, 64)
    _check(out, want)
    unpruned = _model(validate_centerlines=True, relaxed_slack=2).evaluate(X, y, threshold=thr)
    assert out["cldice_hard"] == unpruned["cldice_hard"]              # it stays on the unpruned skeletons
    assert out["cl_len_pred"] <= unpruned["cl_len_pred"] and out["cl_len_true"] < unpruned["cl_len_true"]
    assert not JN_KEYS & set(unpruned) and set(out) - set(unpruned) == JN_KEYS
    again = m.evaluate(X, y, threshold=thr)
    _check(again, want)
    # _validate logs the scalars and keeps the histogram out of what it returns
    got = m._validate((X, y), 1)
    assert "jn_f1" in got and "junction_error" in got and "jn_hist" not in got and "cl_hist" not in got
    # each flag alone
    del calls[:]
    pruned = _model(validate_centerlines=True, centerline_min_branch=2, relaxed_slack=2)
    got = pruned.evaluate(X, y, threshold=thr)
    assert calls.count("rsu_skeleton_graph") == 3 and calls.count("rsu_distance_hist") == 3 and "rsu_components_pair_count" not in calls
    assert set(got) == set(unpruned) and "junc_pred" not in pruned._mask_metrics.ws
    _check(got, {k: v for k, v in want.items() if k in CL_KEYS})
    del calls[:]
    junc = _model(validate_centerlines=True, validate_junctions=True, relaxed_slack=2)
    got = junc.evaluate(X, y, threshold=thr)
    assert calls.count("rsu_skeleton_graph") == 3 and calls.count("rsu_distance_hist") == 6
    want0, _, _ = _host_composition(_chunks(junc, X, y), thr, 64, 0, 2, True)
    _check(got, want0)
    assert np.array_equal(got["cl_hist"], unpruned["cl_hist"]) and got["cl_len_pred"] == unpruned["cl_len_pred"]
    # with the distances and the components in front: all ride in the one read-back
    both = _model(validate_centerlines=True, centerline_min_branch=2, validate_junctions=True, validate_distances=True,
                  validate_components=True, relaxed_slack=2).evaluate(X, y, threshold=thr)
    _check(both, want)
    assert "b0_error" in both and "relaxed_f1" in both and both["dist_hist"][0].sum() == out["tp"] + out["fp"]
    # the flags off: no call, no buffer, no key
    del calls[:]
    plain_model = _model(validate_centerlines=True, relaxed_slack=2)
    plain = plain_model.evaluate(X, y, threshold=thr)
    assert "rsu_skeleton_graph" not in calls and "rsu_components_pair_count" not in calls and calls.count("rsu_distance_hist") == 3
    mm = plain_model._mask_metrics
    assert "graph" not in mm.lay and not {"graph", "junc_pred", "junc_true", "comp"} & set(mm.ws) and set(plain) == set(unpruned)
    bare = _model()
    assert not (CL_KEYS | JN_KEYS) & set(bare.evaluate(X, y, threshold=thr)) and bare._mask_metrics is None


def test_centerlines_of_predicted_masks_pruned():
    """centerlines() with --centerline_min_branch: the thinned masks pruned in place, every pixel counted"""
    shape = (2, 230, 97)
    prob = np.array(TU.pair("smooth1.5~smooth3", shape)[0])
    skel = hostio.mask_thin(prob, 0.5, None, 64)[0]
    for L in (3, GU.R + 1):
        m = _model(centerline_min_branch=L)
        want = hostio.skeleton_graph(skel, 0.5, None, L)[0]
        got = m.centerlines(prob, threshold=0.5)
        assert got.dtype == np.float32 and got.shape == shape and got.tobytes() == want.tobytes()
        assert 0 < want.sum() < skel.sum()
    assert _model().centerlines(prob, threshold=0.5).tobytes() == skel.tobytes()


def test_cli_save_centerlines_pruned(tmp_path, monkeypatch):
    """the inference branch with --save_centerlines --centerline_min_branch: the PNGs hold the pruned skeletons"""
    from PIL import Image
    from road_segmentation_unet_amd.cli import main
    from road_segmentation_unet_amd.model import ConvolutionalModel
    from road_segmentation_unet_amd import mask_metrics as M      # (it issues the calls)
    rng = np.random.RandomState(4)
    ev = tmp_path / "eval"
    ev.mkdir()
    H, W = 48, 40
    for i in range(2):
        Image.fromarray((rng.rand(H, W, 3) * 255).astype(np.uint8)).save(ev / ("test_%d.png" % i))
    seen, calls = [], []
    real = ConvolutionalModel.centerlines
    monkeypatch.setattr(ConvolutionalModel, "centerlines", lambda self, masks, threshold=0.5: seen.append(
        (np.array(masks), threshold, real(self, masks, threshold))) or seen[-1][2])
    real_call = M.call
    monkeypatch.setattr(M, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    for L in (2, 0):
        del seen[:], calls[:]
        save = tmp_path / ("runs%d" % L)
        argv = ["--num_layers=2", "--root_size=16", "--patch_size=16", "--stride=16", "--batch_size=4", "--num_epoch=0",
                "--eval_data_dir=%s" % ev, "--save_path=%s" % save, "--pred_batch_size=2", "--seed=5", "--logdir=",
                "--save_centerlines", "--centerline_max_iters=32"]
        assert main(argv + (["--centerline_min_branch=%d" % L] if L else [])) == 0
        assert calls.count("rsu_mask_thin") == 1 and calls.count("rsu_skeleton_graph") == (1 if L else 0)
        run = [d for d in os.listdir(save) if os.path.isdir(save / d)]
        files = sorted(f for f in os.listdir(save / run[0]) if f.startswith("centerlines_"))
        assert len(run) == 1 and files == ["centerlines_001.png", "centerlines_002.png"] and len(seen) == 1
        masks, thr, lines = seen[0]
        skel = hostio.mask_thin(masks.reshape(2, H, W), 0.5, None, 32)[0]
        want = hostio.skeleton_graph(skel, 0.5, None, L)[0]
        assert lines.tobytes() == want.tobytes() and (L > 0 or want.tobytes() == skel.tobytes())
        for k, f in enumerate(files):
            png = np.asarray(Image.open(save / run[0] / f).convert("L"))
            assert png.shape == (H, W) and (lines[k].max() == 0 or np.array_equal(png > 127, lines[k] > 0))
