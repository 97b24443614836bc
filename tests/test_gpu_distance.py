"""-m gpu: include/rsu_distance.h against the host restatements of road_segmentation_unet_amd/hostio.py (which tests/test_distance_host.py
holds to scipy and to a brute-force minimum): both entries over the bank of tests/distance_util.py -- every mask kind against its own
shifted copy, spiral against rings, an all-ones prediction against one true pixel (all 64 bins), empty truth, empty prediction,
neighbouring images -- at shapes from one pixel to the staging limits; the float bank; ignored labels; the NULL variants; accumulation;
two runs byte for byte; ConvolutionalModel.evaluate() with --validate_distances above them. Every comparison is integer equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from tests import components_util as CU  # noqa: E402
from tests import distance_util as DU  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402

BANK_SHAPES = DU.SHAPES + [DU.ALL_BINS_SHAPE]


def _np(t):
    return None if t is None else t.cpu().numpy()


def _dev(labels):
    return torch.from_numpy(np.array(labels)).to(hu.DEV)   # (a copy: the bank's arrays are read-only)


# ------------------------------------------------------------------------------------------- both entries over the bank
@pytest.mark.parametrize("shape", BANK_SHAPES, ids=[DU.shape_id(s) for s in BANK_SHAPES])
def test_both_entries_equal_the_host_over_the_bank(shape):
    for name in DU.pair_names(shape):
        prob, labels = DU.pair(name, shape)
        want_p, want_t, want_h = DU.host_pair(name, shape)
        pt, lt = hu.dev_f32(np.array(prob)), _dev(labels)
        d2p, d2t = DU.run_mask_distance(pt, lt, shape)
        for what, g, w in (("d2_pred", _np(d2p), want_p), ("d2_true", _np(d2t), want_t)):
            assert g.dtype == w.dtype and np.array_equal(g, w), (name, shape, what, int((g != w).sum()))
        acc = _np(DU.run_hist(pt, lt, shape))
        assert acc.dtype == np.int64 and np.array_equal(acc, want_h), (name, shape, acc, want_h)
    if shape[0] > 1:   # images do not see each other: everything lands in the last bin
        h = DU.host_pair("neighbours", shape)[2]
        assert h[0, 63] == 1 and h[1, 63] == 1 and h.sum() == 2
    if shape == DU.ALL_BINS_SHAPE:   # the reference itself fills every bin of acc[0], the saturated one included
        h = DU.host_pair("full~corner", shape)[2]
        assert (h[0] > 0).all() and h[0, 63] == 32844 and h[0].sum() == 39000


# ------------------------------------------------------------------------------------------- floats and labels
@pytest.mark.parametrize("shape", [(2, 130, 67), (3, 63, 65)], ids=DU.shape_id)
def test_float_bank_and_ignored_labels(shape):
    """the threshold itself, the float below it, -0.0, NaNs and infinities: one float32 comparison decides; labels -1, 2 and
    (1 << 32) | 1 are not counted and not truth, all 64 bits tested; distances run across them"""
    p = CU.float_bank(shape)
    labels = DU.mixed_labels(shape)
    assert (labels == ((1 << 32) | 1)).sum() > 100 and (labels == 2).sum() > 100 and (labels == -1).sum() > 100
    P, T = DU.masks_of(p, labels)
    assert P[p == np.float32(0.5)].sum() > 50 and not P[np.isnan(p)].any() and np.isnan(p).sum() > 100 and not T[labels > 1].any()
    for lab in (labels, (labels == 1).astype(np.int64)):
        pt, lt = hu.dev_f32(p), _dev(lab)
        want = hostio.mask_distance(p, DU.THRESHOLD, lab)
        got = DU.run_mask_distance(pt, lt, shape)
        assert np.array_equal(_np(got[0]), want[0]) and np.array_equal(_np(got[1]), want[1])
        assert np.array_equal(_np(DU.run_hist(pt, lt, shape)), hostio.distance_hist(p, DU.THRESHOLD, lab))
    # another threshold, negative: -0.0 and the small positives are inside, the NaNs and -inf stay outside
    want = hostio.mask_distance(p, -0.25, labels)
    got = DU.run_mask_distance(hu.dev_f32(p), _dev(labels), shape, threshold=-0.25)
    assert np.array_equal(_np(got[0]), want[0]) and np.array_equal(_np(got[1]), want[1])


def test_null_variants_of_mask_distance():
    shape = (2, 130, 67)
    prob, labels = DU.pair("rand0.41~shift", shape)
    want_p, want_t, _ = DU.host_pair("rand0.41~shift", shape)
    pt, lt = hu.dev_f32(np.array(prob)), _dev(labels)
    d2p, none = DU.run_mask_distance(pt, lt, shape, want_true=False)
    assert none is None and np.array_equal(_np(d2p), want_p)
    none, d2t = DU.run_mask_distance(pt, lt, shape, want_pred=False)
    assert none is None and np.array_equal(_np(d2t), want_t)
    # labels64 = NULL: every pixel is counted
    mixed = DU.mixed_labels(shape)
    d2p, _ = DU.run_mask_distance(pt, None, shape, want_true=False)
    assert np.array_equal(_np(d2p), hostio.mask_distance(prob, DU.THRESHOLD)[0])
    with_ignored = hostio.mask_distance(prob, DU.THRESHOLD, mixed)[0]
    assert not np.array_equal(with_ignored, _np(d2p))                       # (the ignored pixels do change the prediction's mask)
    assert np.array_equal(_np(DU.run_mask_distance(pt, _dev(mixed), shape, want_true=False)[0]), with_ignored)


# ------------------------------------------------------------------------------------------- accumulation
def test_hist_accumulates_and_padding_adds_nothing():
    shape = (3, 63, 65)
    p = CU.float_bank(shape)
    labels = DU.mixed_labels(shape)                     # its last image is ignored altogether
    want = hostio.distance_hist(p, DU.THRESHOLD, labels)
    pt, lt = hu.dev_f32(p), _dev(labels)
    acc = DU.run_hist(pt, lt, shape)
    assert np.array_equal(_np(acc), want)
    DU.run_hist(pt, lt, shape, acc=acc)
    assert np.array_equal(_np(acc), 2 * want)
    # the head images alone add what the chunk with its ignored tail adds
    head = (2,) + shape[1:]
    assert np.array_equal(_np(DU.run_hist(hu.dev_f32(p[:2]), _dev(labels[:2]), head)), want)
    # nothing counted: exactly nothing is added
    DU.run_hist(pt, torch.full(shape, -1, dtype=torch.int64, device=hu.DEV), shape, acc=acc)
    assert np.array_equal(_np(acc), 2 * want)


def test_two_runs_give_identical_bytes():
    shape = (2, 130, 67)
    p = CU.float_bank(shape)
    lt = _dev(DU.mixed_labels(shape))
    runs = []
    for _ in range(2):
        pt = hu.dev_f32(p)
        got = [_np(t) for t in DU.run_mask_distance(pt, lt, shape)] + [_np(DU.run_hist(pt, lt, shape))]
        runs.append([a.tobytes() for a in got])
    assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------- the model
ML, MROOT, MP, MB = 3, 16, 20, 2      # the small config of the other model tests


def _model(**kw):
    from road_segmentation_unet_amd.model import ConvolutionalModel, Options
    o = dict(num_layers=ML, root_size=MROOT, patch_size=MP, batch_size=MB, dilated_layers=True, dropout=1.0, lr=0.01, seed=5, logdir=None)
    o.update(kw)
    return ConvolutionalModel(Options(**o), device="cuda:0", params=U.init_params(ML, MROOT, True, seed=13, bias_scale=0.05))


def _patches(n, seed=21, p_road=0.3):
    S = U.input_size_needed(MP, ML)
    rng = np.random.RandomState(seed)
    return rng.rand(n, S, S, 3).astype(np.float32), (rng.rand(n, MP, MP) < p_road).astype(np.int64)


KEYS = {"dist_hist", "relaxed_precision", "relaxed_recall", "relaxed_f1", "mean_dist_pred", "mean_dist_true", "far_pred", "far_true"}


def _threshold_inside(m, X, y):
    """a threshold that splits the untrained net's probabilities: the multiple of 1/256 (evaluate() takes no other) nearest their median"""
    return round(float(np.median(np.concatenate([c[0].reshape(-1) for c in _chunks(m, X, y)]))) * 256.0) / 256.0


def _chunks(m, X, y):
    """(net.prob, labels) of every chunk evaluate() runs, the last one padded with zero patches labelled -1: as the components test does"""
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


def test_evaluate_with_validate_distances(monkeypatch):
    """dist_hist equals the sum over the chunks of hostio.distance_hist on the probabilities evaluate produced; the relaxed keys are
    relaxed_metrics of it at --relaxed_slack; without the flag the keys are absent and no rsu_distance_* call is made"""
    from road_segmentation_unet_amd import mask_metrics as M      # (it issues the calls)
    N = 5
    X, y = _patches(N)
    y[1, :3] = -1
    m = _model(validate_distances=True, relaxed_slack=2)
    thr = _threshold_inside(m, X, y)
    calls = []
    real = M.call
    monkeypatch.setattr(M, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    out = m.evaluate(X, y, threshold=thr)
    assert calls.count("rsu_distance_hist") == 3 and not [c for c in calls if c.startswith("rsu_mask_distance")]
    want = np.zeros((2, 64), np.int64)
    for prob, yb in _chunks(m, X, y):
        want += hostio.distance_hist(prob, thr, yb)
    assert want[0].sum() > 100 and want[1].sum() == (y == 1).sum() and want[0, 1:].sum() > 0 and want[1, 1:].sum() > 0
    assert KEYS <= set(out) and out["dist_hist"].dtype == np.int64 and np.array_equal(out["dist_hist"], want)
    rm = hostio.relaxed_metrics(want, 2)
    assert {k: out[k] for k in rm} == rm
    assert out["tp"] == want[0, 0] and out["tp"] + out["fp"] == want[0].sum() and out["tp"] + out["fn"] == want[1].sum()   # the head's own counts
    again = m.evaluate(X, y, threshold=thr)
    assert np.array_equal(again["dist_hist"], want) and again["relaxed_f1"] == out["relaxed_f1"]
    # with the components count in front: both ride in the one read-back
    both = _model(validate_distances=True, validate_components=True, relaxed_slack=2).evaluate(X, y, threshold=thr)
    assert np.array_equal(both["dist_hist"], want) and "b0_error" in both
    # the flag off: no new key, no new call, the same figures
    del calls[:]
    plain_model = _model()
    plain = plain_model.evaluate(X, y, threshold=thr)
    assert not KEYS & set(plain) and not [c for c in calls if c.startswith("rsu_distance") or c.startswith("rsu_mask_distance")]
    assert plain_model._mask_metrics is None
    assert plain["f1"] == out["f1"] and np.array_equal(plain["sums"], out["sums"])


def test_save_best_metric_selects_on_the_relaxed_f1(monkeypatch, tmp_path):
    """_validate compares v[save_best_metric]: with relaxed_f1 a pass whose pixel F1 fell but whose relaxed F1 rose is the new best; with
    the default the same two passes keep the first"""
    X, y = _patches(3)
    passes = [dict(f1=0.5, relaxed_f1=0.6), dict(f1=0.4, relaxed_f1=0.7), dict(f1=0.45, relaxed_f1=0.65)]
    for metric, kw, want_best, want_saves in (("relaxed_f1", dict(validate_distances=True, save_best_metric="relaxed_f1"), 0.7, 2),
                                              ("f1", dict(validate_distances=True), 0.5, 1)):
        m = _model(save_best=True, save_path=str(tmp_path), **kw)
        real = m.evaluate(X, y)
        assert "relaxed_f1" in real
        saves = []
        monkeypatch.setattr(m, "save_as", lambda path: saves.append(path))
        for fake in passes:
            v = dict(real)
            v.update(fake)
            monkeypatch.setattr(m, "evaluate", lambda *a, _v=v, **k: dict(_v))
            got = m._validate((X, y), 1)
            assert got["relaxed_f1"] == fake["relaxed_f1"] and "dist_hist" not in got
        assert m.best_val_score == want_best and len(saves) == want_saves, metric
        assert m.best_val_f1 == 0.5   # the attribute keeps its meaning: the best pixel F1
