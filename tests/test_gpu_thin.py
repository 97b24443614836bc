"""-m gpu: include/rsu_thin.h against the host restatement hostio.mask_thin (which tests/test_thin_host.py holds to the topology of its
input): rsu_mask_thin over the bank of tests/thin_util.py -- every kind as the prediction against the next as the truth -- at shapes from
one pixel to the tiling's limits, truncated (1, K - 1, K, K + 1 iterations) and at the default 64; one solid block across a four-tile
corner; ignored labels kept verbatim; the float bank; the NULL variants; accumulation; two runs byte for byte;
ConvolutionalModel.evaluate() with --validate_centerlines, centerlines() and the command line's --save_centerlines above it. Every comparison is equality of the bytes."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from tests import components_util as CU  # noqa: E402
from tests import thin_util as TU  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402


def _np(t):
    return None if t is None else t.cpu().numpy()


def _dev(labels):
    return torch.from_numpy(np.array(labels)).to(hu.DEV)   # (a copy: the bank's arrays are read-only)


def _same(got, want, what):
    """byte for byte: skel_pred float32, skel_true int64, acc as int64 [4], info as uint32 [N, 2]"""
    sp, st, acc, info = [_np(t) for t in got]
    wp, wt, wc, wi = want
    if sp is not None:
        assert sp.dtype == np.float32 and sp.tobytes() == wp.tobytes(), (what, "skel_pred", int((sp != wp).sum()))
    if st is not None:
        assert st.dtype == np.int64 and st.tobytes() == wt.tobytes(), (what, "skel_true", int((st != wt).sum()))
    if acc is not None:
        assert acc.dtype == np.int64 and acc.tobytes() == wc.tobytes(), (what, "acc", acc, wc)
    if info is not None:
        assert info.view(np.uint32).tobytes() == wi.tobytes(), (what, "info", info, wi)


# ------------------------------------------------------------------------------------------- the bank
@pytest.mark.parametrize("shape", TU.SHAPES, ids=[TU.shape_id(s) for s in TU.SHAPES])
def test_mask_thin_equals_the_host_over_the_bank(shape):
    unconverged = 0
    for name in TU.pair_names():
        prob, labels = TU.pair(name, shape)
        pt, lt = hu.dev_f32(np.array(prob)), _dev(labels)
        for it in TU.ITERS:
            want = TU.host_pair(name, shape, it)
            _same(TU.run_thin(pt, lt, shape, it), want, (name, shape, it))
            unconverged += int((want[3] != 0).sum())
    if min(shape[1:]) > 8:   # info is non-zero exactly where the host says so: the truncated runs of the reference itself are unconverged
        assert unconverged > 0


def test_a_solid_block_across_a_four_tile_corner():
    """100 x 100 pixels over the corner of four tiles: its fixed point lies some 56 iterations and 7 step launches away, every one of them
    passing its rim through the halo; at 64 iterations it has converged, at 32 it has not"""
    shape = TU.BLOCK_SHAPE
    m = TU.block_mask()
    assert m[0, TU.CROWS - 1:TU.CROWS + 1, TU.CORE - 1:TU.CORE + 1].all() and m[0, TU.CROWS, 2 * TU.CORE]
    prob = CU.prob_of(m)
    labels = np.ascontiguousarray(m[:, ::-1, ::-1]).astype(np.int64)
    pt, lt = hu.dev_f32(prob), _dev(labels)
    for it, converged in ((64, True), (32, False)):
        want = hostio.mask_thin(prob, TU.THRESHOLD, labels, it)
        assert (want[3] == 0).all() == converged and (want[3] != 0).all() == (not converged)
        _same(TU.run_thin(pt, lt, shape, it), want, ("block", it))
    assert TU.topology(want[0][0] > 0) == (1, 1)


# ------------------------------------------------------------------------------------------- floats and labels
@pytest.mark.parametrize("shape", [(2, 230, 97), (3, 63, 65)], ids=TU.shape_id)
def test_float_bank_and_ignored_labels(shape):
    """the threshold itself, the float below it, -0.0, NaNs and infinities: one float32 comparison decides; labels -1, 2 and
    (1 << 32) | 1 are not counted and not truth, all 64 bits tested; they are background for the thinning and stay verbatim in skel_true"""
    p = CU.float_bank(shape)
    labels = TU.mixed_labels(shape)
    ignored = (labels != 0) & (labels != 1)
    assert (labels == ((1 << 32) | 1)).sum() > 100 and (labels == 2).sum() > 100 and (labels == -1).sum() > 100
    for thr in (TU.THRESHOLD, -0.25):
        want = hostio.mask_thin(p, thr, labels, 64)
        got = TU.run_thin(hu.dev_f32(p), _dev(labels), shape, 64, threshold=thr)
        _same(got, want, (shape, thr))
        st = _np(got[1])
        assert np.array_equal(st[ignored], labels[ignored]) and set(np.unique(st[~ignored])) <= {0, 1}
        assert not _np(got[0])[ignored | np.isnan(p)].any()
    if shape[0] > 1:   # the padding image of an evaluation chunk: nothing in either skeleton, nothing counted
        alone = hostio.mask_thin(p[:-1], TU.THRESHOLD, labels[:-1], 64)
        assert np.array_equal(alone[2], hostio.mask_thin(p, TU.THRESHOLD, labels, 64)[2])
        assert not _np(got[0])[-1].any() and (st[-1] == -1).all()


def test_null_variants():
    shape = (2, 230, 97)
    name = "smooth3~smooth6"
    prob, labels = TU.pair(name, shape)
    want = TU.host_pair(name, shape, 64)
    pt, lt = hu.dev_f32(np.array(prob)), _dev(labels)
    sp, none, acc, info = TU.run_thin(pt, lt, shape, 64, want_true=False)
    assert none is None and acc is None
    _same((sp, None, None, info), want, "skel_true = NULL")
    none, st, acc, info = TU.run_thin(pt, lt, shape, 64, want_pred=False)
    assert none is None and acc is None
    _same((None, st, None, info), want, "skel_pred = NULL")
    _same(TU.run_thin(pt, lt, shape, 64, want_acc=False, want_info=False), want, "acc = info = NULL")
    # labels64 = NULL: every pixel is counted, T is empty
    mixed = TU.mixed_labels(shape)
    free = hostio.mask_thin(prob, TU.THRESHOLD, None, 64)
    assert free[1] is None and (free[3][:, 1] == 0).all() and free[2][1] == 0 and free[2][2] == 0
    sp, _, _, info = TU.run_thin(pt, None, shape, 64, want_true=False)
    _same((sp, None, None, info), free, "labels64 = NULL")
    with_ignored = hostio.mask_thin(prob, TU.THRESHOLD, mixed, 64)
    assert not np.array_equal(with_ignored[0], free[0])                     # (the ignored pixels do change the prediction's mask)
    _same(TU.run_thin(pt, _dev(mixed), shape, 64), with_ignored, "mixed labels")


# ------------------------------------------------------------------------------------------- accumulation
def test_acc_accumulates_and_an_ignored_image_adds_nothing():
    shape = (3, 63, 65)
    p = CU.float_bank(shape)
    labels = TU.mixed_labels(shape)                     # its last image is ignored altogether
    want = hostio.mask_thin(p, TU.THRESHOLD, labels, 64)[2]
    assert (want > 0).all()
    pt, lt = hu.dev_f32(p), _dev(labels)
    acc = TU.run_thin(pt, lt, shape, 64)[2]
    assert np.array_equal(_np(acc), want)
    TU.run_thin(pt, lt, shape, 64, acc=acc)
    assert np.array_equal(_np(acc), 2 * want)
    head = (2,) + shape[1:]
    assert np.array_equal(_np(TU.run_thin(hu.dev_f32(p[:2]), _dev(labels[:2]), head, 64)[2]), want)
    sp, st, _, info = TU.run_thin(pt, torch.full(shape, -1, dtype=torch.int64, device=hu.DEV), shape, 64, acc=acc)
    assert np.array_equal(_np(acc), 2 * want) and not _np(sp).any() and (_np(st) == -1).all() and not _np(info).any()


def test_two_runs_give_identical_bytes():
    shape = (2, 230, 97)
    p = CU.float_bank(shape)
    lt = _dev(TU.mixed_labels(shape))
    runs = []
    for _ in range(2):
        got = [_np(t) for t in TU.run_thin(hu.dev_f32(p), lt, shape, 5)]
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


KEYS = {"cl_hist", "cl_correctness", "cl_completeness", "cl_quality", "cldice_hard", "cl_len_pred", "cl_len_true", "thin_unconverged"}


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


def _host_composition(chunks, thr, max_iters):
    """mask_thin -> distance_hist of the two skeletons at 0.5 -> the sums evaluate() must return"""
    hist, counts, unconverged = np.zeros((2, 64), np.int64), np.zeros(4, np.int64), 0
    for prob, yb in chunks:
        sp, st, c, info = hostio.mask_thin(prob, thr, yb, max_iters)
        hist += hostio.distance_hist(sp, 0.5, st)
        counts += c
        unconverged += int((info != 0).sum())
    return hist, counts, unconverged


def test_evaluate_with_validate_centerlines(monkeypatch):
    from road_segmentation_unet_amd import mask_metrics as M      # (it issues the calls)
    N = 5
    X, y = _patches(N)
    y[1, :3] = -1
    m = _model(validate_centerlines=True, relaxed_slack=2)
    thr = round(float(np.median(np.concatenate([c[0].reshape(-1) for c in _chunks(m, X, y)]))) * 256.0) / 256.0
    calls = []
    real = M.call
    monkeypatch.setattr(M, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    out = m.evaluate(X, y, threshold=thr)
    assert calls.count("rsu_mask_thin") == 3 and calls.count("rsu_distance_hist") == 3
    hist, counts, unconverged = _host_composition(_chunks(m, X, y), thr, 64)
    assert hist[0].sum() == counts[0] > 20 and hist[1].sum() == counts[2] > 20 and unconverged == 0
    assert KEYS <= set(out) and out["cl_hist"].dtype == np.int64 and np.array_equal(out["cl_hist"], hist)
    assert out["thin_unconverged"] == 0 and (out["cl_len_pred"], out["cl_len_true"]) == (counts[0], counts[2])
    want = hostio.centerline_metrics(hist, counts, 2)
    assert {k: out[k] for k in want} == want and set(want) | {"cl_hist", "thin_unconverged"} == KEYS
    assert "dist_hist" not in out and "relaxed_f1" not in out        # it does not need --validate_distances, and does not switch it on
    again = m.evaluate(X, y, threshold=thr)
    assert np.array_equal(again["cl_hist"], hist) and again["cl_quality"] == out["cl_quality"]
    # one iteration only: the truncated skeletons, and the image sides still moving are counted
    short = _model(validate_centerlines=True, relaxed_slack=2, centerline_max_iters=1)
    got = short.evaluate(X, y, threshold=thr)
    hist1, counts1, unconverged1 = _host_composition(_chunks(short, X, y), thr, 1)
    assert unconverged1 > 0 and got["thin_unconverged"] == unconverged1
    want1 = hostio.centerline_metrics(hist1, counts1, 2)
    assert np.array_equal(got["cl_hist"], hist1) and {k: got[k] for k in want1} == want1
    # with the distances and the components in front: all ride in the one read-back
    both = _model(validate_centerlines=True, validate_distances=True, validate_components=True, relaxed_slack=2).evaluate(X, y, threshold=thr)
    assert np.array_equal(both["cl_hist"], hist) and both["cldice_hard"] == out["cldice_hard"] and "b0_error" in both and "relaxed_f1" in both
    assert both["dist_hist"][0].sum() == out["tp"] + out["fp"]
    # the flag off: the keys of before, no new call, no buffer, the same figures
    del calls[:]
    plain_model = _model()
    plain = plain_model.evaluate(X, y, threshold=thr)
    assert not KEYS & set(plain) and not [c for c in calls if "thin" in c or "distance" in c]
    assert plain_model._mask_metrics is None
    assert plain["f1"] == out["f1"] and np.array_equal(plain["sums"], out["sums"])
    assert set(out) - set(plain) == KEYS


def test_save_best_metric_selects_on_cl_quality(monkeypatch, tmp_path):
    """_validate compares v[save_best_metric]: with cl_quality a pass whose pixel F1 fell but whose centre-line quality rose is the new best"""
    X, y = _patches(3)
    passes = [dict(f1=0.5, cl_quality=0.6), dict(f1=0.4, cl_quality=0.7), dict(f1=0.45, cl_quality=0.65)]
    for metric, kw, want_best, want_saves in (("cl_quality", dict(validate_centerlines=True, save_best_metric="cl_quality"), 0.7, 2),
                                              ("f1", dict(validate_centerlines=True), 0.5, 1)):
        m = _model(save_best=True, save_path=str(tmp_path), **kw)
        real = m.evaluate(X, y)
        assert "cl_quality" in real
        saves = []
        monkeypatch.setattr(m, "save_as", lambda path: saves.append(path))
        for fake in passes:
            v = dict(real)
            v.update(fake)
            monkeypatch.setattr(m, "evaluate", lambda *a, _v=v, **k: dict(_v))
            got = m._validate((X, y), 1)
            assert got["cl_quality"] == fake["cl_quality"] and "cl_hist" not in got
        assert m.best_val_score == want_best and len(saves) == want_saves, metric
        assert m.best_val_f1 == 0.5


def test_centerlines_of_predicted_masks():
    """centerlines(): float masks [n, H, W] (or [n, H, W, 1]) -> the 0 / 1 skeletons of {p >= threshold}, every pixel counted"""
    m = _model()
    shape = (2, 230, 97)
    prob = np.array(TU.pair("smooth3~smooth6", shape)[0])
    want = hostio.mask_thin(prob, 0.5, None, 64)[0]
    got = m.centerlines(prob, threshold=0.5)
    assert got.dtype == np.float32 and got.shape == shape and got.tobytes() == want.tobytes()
    assert m.centerlines(prob[..., None], threshold=0.5).tobytes() == want.tobytes()
    low = m.centerlines(prob, threshold=0.25)
    assert low.tobytes() == hostio.mask_thin(prob, 0.25, None, 64)[0].tobytes() and low.tobytes() != want.tobytes()
    with pytest.raises(ValueError, match="centerlines"):
        m.centerlines(np.zeros((1, 1025, 4), np.float32))
    with pytest.raises(ValueError, match="centerlines"):
        m.centerlines(np.zeros((4, 4), np.float32))


def test_cli_save_centerlines(tmp_path, monkeypatch):
    """the inference branch with --save_centerlines: one greyscale PNG per image beside the overlays, the skeleton of the mask that
    postprocess_masks returned, thinned at 0.5 with every pixel counted; without the flag no such file and no call"""
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
    real = ConvolutionalModel.centerlines
    monkeypatch.setattr(ConvolutionalModel, "centerlines", lambda self, masks, threshold=0.5: seen.append(
        (np.array(masks), threshold, real(self, masks, threshold))) or seen[-1][2])
    for flag in (True, False):
        save = tmp_path / ("runs%d" % flag)
        argv = ["--num_layers=2", "--root_size=16", "--patch_size=16", "--stride=16", "--batch_size=4", "--num_epoch=0",
                "--eval_data_dir=%s" % ev, "--save_path=%s" % save, "--pred_batch_size=2", "--seed=5", "--logdir="]
        assert main(argv + (["--save_centerlines", "--centerline_max_iters=32"] if flag else [])) == 0
        run = [d for d in os.listdir(save) if os.path.isdir(save / d)]
        assert len(run) == 1
        files = sorted(f for f in os.listdir(save / run[0]) if f.startswith("centerlines_"))
        if not flag:
            assert files == [] and len(seen) == 1
            continue
        assert files == ["centerlines_001.png", "centerlines_002.png"] and len(seen) == 1
        masks, thr, lines = seen[0]
        assert thr == 0.5 and masks.shape[:3] == (2, H, W) and lines.shape == (2, H, W) and lines.dtype == np.float32
        want = hostio.mask_thin(masks.reshape(2, H, W), 0.5, None, 32)[0]
        assert lines.tobytes() == want.tobytes()
        for k, f in enumerate(files):
            png = np.asarray(Image.open(save / run[0] / f).convert("L"))
            assert png.shape == (H, W) and (lines[k].max() == 0 or np.array_equal(png > 127, lines[k] > 0))
