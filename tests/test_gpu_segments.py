"""-m gpu: include/rsu_segments.h against the host restatement hostio.line_segments (which tests/test_segments_host.py holds to hand cases
and to scipy's labelling): rsu_line_segments over the thinned pairs of tests/graph_util.py pruned at L in {0, 8} and over raw, thick
masks, at shapes from one pixel to sixteen labelling tiles; hand masks across tile corners, across sixteen tiles and across a compaction
block's edge; truncation at max_edges; accumulation; two runs byte for byte; the NULL variants; a threshold other than 0.5;
ConvolutionalModel.evaluate() with --validate_segments, road_graph() and the command line's --save_road_graph above it. Every comparison is
equality of the bytes."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import components_util as CU  # noqa: E402
from tests import graph_util as GU  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests import segments_util as SU  # noqa: E402
from tests import thin_util as TU  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402


def _np(t):
    return None if t is None else t.cpu().numpy()


def _dev(labels):
    return torch.from_numpy(np.array(labels)).to(hu.DEV)   # (a copy: the bank's arrays are read-only)


def _check(prob, labels, shape, what, cap=SU.CAP, want=None, **kw):
    want = SU.host(prob, labels, cap, kw.get("threshold", SU.THRESHOLD)) if want is None else want
    got = SU.run_segments(hu.dev_f32(np.array(prob)), None if labels is None else _dev(labels), shape, cap, **kw)
    SU.same(got, want, what)
    return got, want


# ------------------------------------------------------------------------------------------- the bank
@pytest.mark.parametrize("L", SU.PRUNES)
@pytest.mark.parametrize("shape", SU.SHAPES, ids=[SU.shape_id(s) for s in SU.SHAPES])
def test_line_segments_equal_the_host_over_the_thinned_bank(shape, L):
    segments = nodes = diag = 0
    for name in TU.pair_names():
        prob, labels = SU.pair(name, shape, L)
        want = SU.host_pair(name, shape, L)
        assert want[2].max() <= SU.CAP
        _check(prob, labels, shape, (name, shape, L), want=want)
        segments += int(want[2][:, [0, 2]].sum())
        nodes += int(want[2][:, [1, 3]].sum())
        diag += int(want[7][:, 3].sum())
    if min(shape[1:]) > 8:   # the cases are not trivial
        assert segments > 0 and nodes > 0 and diag > 0


@pytest.mark.parametrize("shape", [(3, 63, 65), (2, 230, 97), (1, 129, 200)], ids=SU.shape_id)
def test_raw_unthinned_masks(shape):
    """thick masks: A is mostly zone, the segments are fragments; with mixed labels, the all-ignored image included"""
    labels = TU.mixed_labels(shape)
    for name in ("rand0.45~rand0.55", "smooth3~smooth6", "holed~lone2x2"):
        prob = GU.pair(name, shape, False)[0]
        got, want = _check(prob, labels, shape, (name, shape), cap=4096)
        assert want[2].max() <= 4096
    if shape[0] > 1:   # the padding image of an evaluation chunk: four zero counts, nothing in any map
        assert not want[2][-1].any() and not _np(got[3])[-1].any() and not _np(got[6])[-1].any()


# ------------------------------------------------------------------------------------------- hand masks
def test_hand_masks_across_tiles_and_blocks():
    line, ring = GU.corner_line(), GU.corner_ring()
    _check(*SU.of_masks(line, ring), GU.CORNER_SHAPE, "corner line ~ ring")
    got, want = _check(*SU.of_masks(ring, line), GU.CORNER_SHAPE, "corner ring ~ line")
    assert want[2][0].tolist()[:2] == [1, 0] and want[0][0, 0, 4:].tolist() == [0, 0, 0, 0]      # the ring: one closed segment, no node
    # a plus whose zone lies across the corner of four labelling tiles
    a, b = SU.plus(128, 128, 64, 64, 40)[None], SU.plus(128, 128, 63, 63, 40)[None]
    got, want = _check(*SU.of_masks(a, b), (1, 128, 128), "plus")
    assert want[2][0].tolist() == [4, 1, 4, 1] and (want[0][0, :4, 6:] == 1).all()
    # a diagonal through sixteen labelling tiles: one segment, its root in the first tile, 199 diagonal links
    d = SU.diagonal(200, 200)[None]
    got, want = _check(*SU.of_masks(d, d[:, ::-1].copy()), (1, 200, 200), "diagonal")
    assert want[0][0, 0].tolist() == [1, 200, 0, 199, -40000, -1, 0, 2] and want[1][0, 0, :4].tolist() == [200, 200, 0, 199]
    # two lines whose roots are the last pixel of one compaction block and the first of the next
    m = SU.block_edge_lines()[None]
    got, want = _check(*SU.of_masks(m, m), (1,) + m.shape[1:], "block edge")
    assert want[0][0, :2, 0].tolist() == [SU.BLOCK, SU.BLOCK + 1]


# ------------------------------------------------------------------------------------------- truncation
def test_truncation_keeps_the_first_rows_and_the_true_counts():
    shape, name = (2, 230, 97), "smooth1.5~smooth3"
    prob, labels = SU.pair(name, shape, 0)
    full = SU.host_pair(name, shape, 0)
    count = int(full[2][:, [0, 2]].max())
    assert count > 300
    pt, lt = hu.dev_f32(np.array(prob)), _dev(labels)
    for cap in (1, count - 1, count, count + 1):
        want = SU.host(prob, labels, cap)
        got = SU.run_segments(pt, lt, shape, cap)
        SU.same(got, want, ("truncated", cap))
        for side, (edges, ref) in enumerate(((want[0], full[0]), (want[1], full[1]))):
            for n in range(shape[0]):
                k = min(int(full[2][n, 2 * side]), cap)
                assert np.array_equal(edges[n, :k], ref[n, :k]) and (edges[n, k:] == SU.FILL).all()
        assert np.array_equal(want[2], full[2])                               # the true numbers
        assert want[7][:, 0].tolist() == [int(np.minimum(full[2][:, 2 * s], cap).sum()) for s in (0, 1)]
        assert (cap >= count) == np.array_equal(want[7], full[7])


# ------------------------------------------------------------------------------------------- accumulation, determinism, NULL variants
def test_acc_accumulates_and_two_runs_give_identical_bytes():
    shape = (3, 63, 65)
    prob, labels = GU.pair("smooth1.5~smooth3", shape, True)[0], TU.mixed_labels(shape)
    want = SU.host(prob, labels)
    assert (want[7][:, :4] > 0).all()
    pt, lt = hu.dev_f32(np.array(prob)), _dev(labels)
    first = SU.run_segments(pt, lt, shape)
    SU.same(first, want, "first")
    second = SU.run_segments(pt, lt, shape, acc=first[7])
    assert np.array_equal(_np(first[7]), 2 * want[7])
    for a, b in zip(first[:7], second[:7]):
        assert _np(a).tobytes() == _np(b).tobytes()
    ignored = SU.run_segments(pt, torch.full(shape, -1, dtype=torch.int64, device=hu.DEV), shape, acc=first[7])
    assert np.array_equal(_np(first[7]), 2 * want[7]) and not _np(ignored[2]).any() and (_np(ignored[0]) == SU.FILL).all()


def test_null_variants():
    shape, name = (2, 230, 97), "smooth1.5~smooth3"
    prob, labels = SU.pair(name, shape, 8)
    want = SU.host_pair(name, shape, 8)
    pt, lt = hu.dev_f32(np.array(prob)), _dev(labels)
    for k in range(4):   # each optional map NULL in turn, with and without acc
        asked = tuple(i != k for i in range(4))
        got = SU.run_segments(pt, lt, shape, want=asked)
        assert [g is not None for g in got[3:7]] == list(asked)
        SU.same(got, want, "without %s" % SU.NAMES[3 + k])
    SU.same(SU.run_segments(pt, lt, shape, want=(False,) * 4, want_acc=False), want, "tables and counts alone")
    SU.same(SU.run_segments(pt, lt, shape, want_acc=False), want, "acc = NULL")
    # labels64 = NULL: every pixel is counted, T is empty
    free = SU.host(prob, None)
    assert free[1] is None and free[4] is None and free[6] is None and not free[2][:, 2:].any() and not free[7][1].any()
    got = SU.run_segments(pt, None, shape)
    assert got[1] is None and got[4] is None and got[6] is None
    SU.same(got, free, "labels64 = NULL")
    mixed = TU.mixed_labels(shape)
    _check(prob, mixed, shape, "mixed labels")


@pytest.mark.parametrize("shape", [(2, 230, 97), (3, 63, 65)], ids=SU.shape_id)
def test_float_bank_and_another_threshold(shape):
    """the threshold itself, the float below it, -0.0, NaNs and infinities: one float32 comparison decides; labels -1, 2 and
    (1 << 32) | 1 are not counted and not truth, all 64 bits tested"""
    p, labels = CU.float_bank(shape), TU.mixed_labels(shape)
    for thr in (SU.THRESHOLD, -0.25, 0.625):
        got, want = _check(p, labels, shape, (shape, thr), cap=4096, threshold=thr)
        assert want[2].max() <= 4096 and want[2][:, 0].max() > 0
        ignored = (labels != 0) & (labels != 1)
        assert not _np(got[3])[ignored | np.isnan(p)].any() and not _np(got[5])[ignored | np.isnan(p)].any()


# ------------------------------------------------------------------------------------------- the model
SG_KEYS = {"%s_%s" % (k, s) for k in ("segments", "road_length", "seg_len_mean", "dangling", "free", "rings", "multi", "segments_dropped", "nodes")
           for s in ("pred", "true")} | {"length_ratio"}


def _host_metrics(chunks, thr, max_iters, min_branch, cap):
    acc, counts = np.zeros((2, 8), np.int64), np.zeros(4, np.int64)
    for prob, yb in chunks:
        sp, st, _, _ = hostio.mask_thin(prob, thr, yb, max_iters)
        op, ot = hostio.skeleton_graph(sp, 0.5, st, min_branch)[:2]
        out = hostio.line_segments(op, 0.5, ot, cap)
        acc += out[7]
        counts += out[2].sum(axis=0)
    return hostio.segment_metrics(acc, counts)


def test_evaluate_with_segments_and_road_graph(monkeypatch):
    from road_segmentation_unet_amd import mask_metrics as M      # (it issues the calls)
    from tests import test_gpu_graph as TG
    N = 5
    X, y = TG._patches(N)
    y[1, :3] = -1
    m = TG._model(validate_centerlines=True, centerline_min_branch=2, validate_segments=True, relaxed_slack=2)
    chunks = TG._chunks(m, X, y)
    thr = round(float(np.median(np.concatenate([c[0].reshape(-1) for c in chunks]))) * 256.0) / 256.0
    calls = []
    real = M.call
    monkeypatch.setattr(M, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    out = m.evaluate(X, y, threshold=thr)
    assert calls.count("rsu_line_segments") == 3 and calls.count("rsu_skeleton_graph") == 3
    per_chunk = [c for c in calls if c in ("rsu_mask_thin", "rsu_skeleton_graph", "rsu_distance_hist", "rsu_line_segments")][:4]
    assert per_chunk == ["rsu_mask_thin", "rsu_skeleton_graph", "rsu_distance_hist", "rsu_line_segments"]
    want = _host_metrics(TG._chunks(m, X, y), thr, 64, 2, 4096)
    assert want["segments_true"] > 0 and want["road_length_true"] > 0 and want["segments_dropped_true"] == 0
    assert SG_KEYS <= set(out) and {k: out[k] for k in SG_KEYS} == want
    assert {k: m.evaluate(X, y, threshold=thr)[k] for k in SG_KEYS} == want          # again: the counters are zeroed per pass
    # unpruned, and a table of two rows per patch: the rest is counted as dropped
    small = TG._model(validate_centerlines=True, validate_segments=True, max_segments=2, relaxed_slack=2)
    got = small.evaluate(X, y, threshold=thr)
    want2 = _host_metrics(TG._chunks(small, X, y), thr, 64, 0, 2)
    assert {k: got[k] for k in SG_KEYS} == want2 and want2["segments_dropped_true"] > 0 and want2["segments_true"] <= 2 * N
    # _validate prints and returns the scalars
    got = m._validate((X, y), 1)
    assert SG_KEYS <= set(got) and got["length_ratio"] == m.evaluate(X, y)["length_ratio"]
    # the flags off: no call, no buffer, no key
    del calls[:]
    plain_model = TG._model(validate_centerlines=True, relaxed_slack=2)
    plain = plain_model.evaluate(X, y, threshold=thr)
    mm = plain_model._mask_metrics
    assert "rsu_line_segments" not in calls and "segments" not in mm.lay and not SG_KEYS & set(plain)
    assert not {"segments", "edges_pred", "edges_true", "counts"} & set(mm.ws)
    assert set(out) - set(plain) == SG_KEYS
    # road_graph(): thin, prune, segments; one dict per image, equal to the host chain
    shape = (2, 230, 97)
    prob = np.array(GU.pair("smooth1.5~smooth3", shape, False)[0])
    for L in (0, 8):
        del calls[:]
        g = TG._model(centerline_min_branch=L).road_graph(prob, threshold=0.5)
        assert calls == ["rsu_mask_thin"] + (["rsu_skeleton_graph"] if L else []) + ["rsu_line_segments"]
        skel = hostio.skeleton_graph(hostio.mask_thin(prob, 0.5, None, 64)[0], 0.5, None, L)[0]
        ref = hostio.line_segments(skel, 0.5, None, 4096)
        assert len(g) == 2
        for n in range(2):
            want_g = hostio.road_graph(ref[0][n], int(ref[2][n, 0]), ref[5][n], shape[1], shape[2])
            assert g[n]["segments"] == int(ref[2][n, 0]) > 10 and g[n]["nodes"] == want_g["nodes"] and g[n]["edges"] == want_g["edges"]
            assert {v["kind"] for v in g[n]["nodes"]} >= {"junction", "end"}


def test_cli_save_road_graph(tmp_path, monkeypatch):
    """the inference branch with --save_road_graph: graph_%03d.json beside the overlays hold road_graph() of the cleaned masks"""
    from PIL import Image
    from road_segmentation_unet_amd.cli import main
    from road_segmentation_unet_amd.model import ConvolutionalModel
    rng = np.random.RandomState(4)
    ev = tmp_path / "eval"
    ev.mkdir()
    H, W = 48, 40
    for i in range(2):
        Image.fromarray((rng.rand(H, W, 3) * 255).astype(np.uint8)).save(ev / ("test_%d.png" % i))
    seen = []
    real = ConvolutionalModel.road_graph
    monkeypatch.setattr(ConvolutionalModel, "road_graph", lambda self, masks, threshold=0.5: seen.append(
        (np.array(masks), threshold, real(self, masks, threshold))) or seen[-1][2])
    argv = ["--num_layers=2", "--root_size=16", "--patch_size=16", "--stride=16", "--batch_size=4", "--num_epoch=0", "--eval_data_dir=%s" % ev,
            "--pred_batch_size=2", "--seed=5", "--logdir=", "--centerline_max_iters=32", "--centerline_min_branch=2"]
    save = tmp_path / "runs"
    assert main(argv + ["--save_path=%s" % save, "--save_road_graph", "--max_segments=64"]) == 0
    run = [d for d in os.listdir(save) if os.path.isdir(save / d)]
    files = sorted(f for f in os.listdir(save / run[0]) if f.startswith("graph_"))
    assert len(run) == 1 and files == ["graph_001.json", "graph_002.json"] and len(seen) == 1
    masks, thr, graphs = seen[0]
    assert thr == 0.5 and len(graphs) == 2
    skel = hostio.skeleton_graph(hostio.mask_thin(masks.reshape(2, H, W), 0.5, None, 32)[0], 0.5, None, 2)[0]
    ref = hostio.line_segments(skel, 0.5, None, 64)
    for k, f in enumerate(files):
        want = hostio.road_graph(ref[0][k], int(ref[2][k, 0]), ref[5][k], H, W)
        want["segments"] = int(ref[2][k, 0])
        assert json.load(open(save / run[0] / f)) == want == graphs[k]
    # without the flag: no file, no call
    del seen[:]
    save = tmp_path / "runs_off"
    assert main(argv + ["--save_path=%s" % save]) == 0
    run = [d for d in os.listdir(save) if os.path.isdir(save / d)]
    assert not seen and not [f for f in os.listdir(save / run[0]) if f.startswith("graph_")]
