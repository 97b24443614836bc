"""CPU-side checks of held-out validation: the rsu_head_eval entry points in header and ctypes table, the three flags, the host
arithmetic of model.metrics_from_eval on hand-built histograms, and hostio's hold-out split and validation tiling."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = 256


# ------------------------------------------------------------------------------------------- symbols
def _header():
    txt = open(os.path.join(ROOT, "include", "rsu.h")).read()
    return txt, re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


@pytest.mark.parametrize("name", ["rsu_head_eval", "rsu_head_eval_ws_floats"])
def test_eval_entry_points_are_declared_and_bound(name):
    from road_segmentation_unet_amd import _lib
    raw, code = _header()
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, code)
    assert m, "%s is not declared in include/rsu.h" % name
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name][1]) == nargs, (name, nargs, len(_lib.SIGNATURES[name][1]))
    assert hasattr(_lib.lib(), name)
    assert re.search(r"#define\s+RSU_EVAL_BINS\s+256\b", raw) and _lib.EVAL_BINS == BINS


def test_eval_ws_query_is_host_code():
    from road_segmentation_unet_amd import _lib
    L = _lib.lib()
    n = L.rsu_head_eval_ws_floats(4 * 388 * 388, 64)
    assert n >= 1024 * (5 + 2 * BINS) and L.rsu_head_eval_ws_floats(100, 12) == 0 and L.rsu_head_eval_ws_floats(0, 64) == 0
    assert L.rsu_head_eval(None, None, None, None, None, None, None, None, None, None, 100, 64, None) == -22


# ------------------------------------------------------------------------------------------- flags
def test_validation_flags_defaults_and_parsing():
    from road_segmentation_unet_amd import cli
    from road_segmentation_unet_amd.model import EXTRA_FLAG_DEFS, FLAG_DEFS, Options
    assert len(FLAG_DEFS) == 30                              # the reference's flags stay as they are
    defs = {n: (t, d) for n, t, d, _ in EXTRA_FLAG_DEFS}
    assert defs["validation_images"] == (int, 0) and defs["validate_every"] == (int, 0) and defs["save_best"] == (bool, False)
    o = Options()
    assert o.validation_images == 0 and o.validate_every == 0 and o.save_best is False
    o = cli.parse_options([])
    assert o.validation_images == 0 and o.validate_every == 0 and o.save_best is False
    o = cli.parse_options(["--validation_images=10", "--validate_every", "250", "--save_best"])
    assert o.validation_images == 10 and o.validate_every == 250 and o.save_best is True
    assert cli.parse_options(["--save_best=false"]).save_best is False and cli.parse_options(["--save_best=true"]).save_best is True
    assert cli.parse_options(["--save_best", "--nosave_best"]).save_best is False
    for bad in (["--validation_images=-1"], ["--validate_every=-5"]):
        with pytest.raises(ValueError):
            cli.parse_options(bad)
    for bad in (["--validation_images=two"], ["--validate_every=1.5"]):
        with pytest.raises(SystemExit):
            cli.parse_options(bad)
    for kw in (dict(validation_images=-1), dict(validation_images=2.5), dict(validate_every="3"), dict(validation_images=True)):
        with pytest.raises(ValueError):
            Options(**kw)


# ------------------------------------------------------------------------------------------- metrics_from_eval
def _hist(entries):
    h = np.zeros((2, BINS), np.int64)
    for label, b, n in entries:
        h[label, b] += n
    return h


def test_metrics_known_counts_at_half():
    from road_segmentation_unet_amd.model import dice_from_sums, metrics_from_eval
    # road: 5 pixels in bin 200, 2 in bin 10, 1 exactly in bin 128 (p = 0.5: predicted road); background: 1 in bin 250, 10 in bin 3, 4 in 127
    h = _hist([(1, 200, 5), (1, 10, 2), (1, 128, 1), (0, 250, 1), (0, 3, 10), (0, 127, 4)])
    sums = [12.5, 20.0, 5.5, 7.25, 8.0]
    m = metrics_from_eval(sums, h, 25, dice_weight=0.5, dice_smooth=1.0, threshold=0.5)
    assert (m["tp"], m["fp"], m["fn"], m["tn"]) == (6, 1, 2, 14)
    assert m["n_counted"] == 23 and m["n_pixels"] == 25
    assert m["loss"] == pytest.approx(12.5 / 25) and m["weighted_mean_loss"] == pytest.approx(12.5 / 20.0)
    D = dice_from_sums(5.5, 7.25, 8.0, 1.0)
    assert m["dice"] == pytest.approx(D) and m["objective"] == pytest.approx(12.5 / 25 + 0.5 * (1 - D))
    p, r = 6 / 7.0, 6 / 8.0
    assert m["precision"] == pytest.approx(p) and m["recall"] == pytest.approx(r) and m["accuracy"] == pytest.approx(20 / 23.0)
    assert m["f1"] == pytest.approx(2 * p * r / (p + r)) and m["iou"] == pytest.approx(6 / 9.0)
    # other thresholds move the counts as the bins say: 0.0 predicts everything road, 1.0 nothing
    m0, m1 = metrics_from_eval(sums, h, 25, threshold=0.0), metrics_from_eval(sums, h, 25, threshold=1.0)
    assert (m0["tp"], m0["fp"], m0["fn"], m0["tn"]) == (8, 15, 0, 0) and (m1["tp"], m1["fp"], m1["fn"], m1["tn"]) == (0, 0, 8, 15)
    assert m1["f1"] == 0.0 and m1["precision"] == 0.0 and m1["iou"] == 0.0
    mq = metrics_from_eval(sums, h, 25, threshold=129 / 256.0)
    assert (mq["tp"], mq["fp"]) == (5, 1)
    # the best interior threshold: anything in (10, 127] keeps all but two road pixels ... the sweep must find the maximum of the 255
    f1s = [metrics_from_eval(sums, h, 25, threshold=k / 256.0)["f1"] for k in range(1, BINS)]
    assert m["best_f1"] == max(f1s) and m["best_threshold"] == (1 + int(np.argmax(f1s))) / 256.0


def test_metrics_empty_classes_and_all_ignored():
    from road_segmentation_unet_amd.model import metrics_from_eval
    m = metrics_from_eval([3.0, 6.0, 0.0, 0.5, 0.0], _hist([(0, 2, 6)]), 6)       # no road pixel at all
    assert (m["tp"], m["fp"], m["fn"], m["tn"]) == (0, 0, 0, 6)
    assert m["recall"] == 0.0 and m["precision"] == 0.0 and m["f1"] == 0.0 and m["iou"] == 0.0 and m["accuracy"] == 1.0
    assert m["best_f1"] == 0.0 and m["best_threshold"] == 1 / 256.0
    m = metrics_from_eval([3.0, 6.0, 2.0, 2.0, 6.0], _hist([(1, 255, 6)]), 6)      # no background pixel
    assert (m["tp"], m["fp"], m["fn"], m["tn"]) == (6, 0, 0, 0) and m["f1"] == 1.0 and m["iou"] == 1.0 and m["accuracy"] == 1.0
    # the all-ignored set: every accumulator is zero
    m = metrics_from_eval(np.zeros(5, np.float32), np.zeros((2, BINS), np.int64), 400)
    assert m["dice"] == 1.0 and m["f1"] == 0.0 and m["loss"] == 0.0 and m["weighted_mean_loss"] == 0.0 and m["objective"] == 0.0
    assert m["accuracy"] == 0.0 and m["n_counted"] == 0 and m["best_f1"] == 0.0
    m = metrics_from_eval(np.zeros(5), np.zeros((2, BINS), np.int64), 0)
    assert m["loss"] == 0.0 and m["dice"] == 1.0


def test_metrics_best_threshold_ties_take_the_lowest():
    from road_segmentation_unet_amd.model import metrics_from_eval
    # road in bin 200, background in bin 40: every threshold k/256 with 40 < k <= 200 separates them perfectly
    m = metrics_from_eval(np.ones(5), _hist([(1, 200, 9), (0, 40, 30)]), 39)
    assert m["best_f1"] == 1.0 and m["best_threshold"] == 41 / 256.0
    m = metrics_from_eval(np.ones(5), _hist([(1, 200, 9), (0, 0, 30)]), 39)
    assert m["best_f1"] == 1.0 and m["best_threshold"] == 1 / 256.0


def test_metrics_threshold_must_be_a_multiple_of_one_256th():
    from road_segmentation_unet_amd.model import metrics_from_eval
    h = _hist([(1, 200, 9), (0, 40, 30)])
    for bad in (0.3, 0.5 + 1e-9, 1.0 / 3.0, -1 / 256.0, 257 / 256.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            metrics_from_eval(np.ones(5), h, 39, threshold=bad)
    for good in (0.0, 0.25, 0.5, 37 / 256.0, 1.0):
        metrics_from_eval(np.ones(5), h, 39, threshold=good)
    with pytest.raises(ValueError):
        metrics_from_eval(np.ones(4), h, 39)
    with pytest.raises(ValueError):
        metrics_from_eval(np.ones(5), h[0], 39)


@pytest.mark.parametrize("threshold", [0.5, 0.25, 200 / 256.0])
def test_metrics_f1_agrees_with_pixel_f1(threshold):
    from road_segmentation_unet_amd.model import metrics_from_eval, pixel_f1
    rng = np.random.RandomState(4)
    n = 5000
    bins = rng.randint(0, BINS, n)
    prob = ((bins + 0.25 + 0.5 * rng.rand(n)) / BINS).astype(np.float32)      # strictly inside their bins: > and >= agree at every k / 256
    truth = (rng.rand(n) < np.where(prob > 0.6, 0.8, 0.15)).astype(np.int64)
    restated = np.minimum(BINS - 1, (prob * np.float32(BINS)).astype(np.int64))
    assert np.array_equal(restated, bins)
    h = np.stack([np.bincount(bins[truth == l], minlength=BINS) for l in (0, 1)])
    m = metrics_from_eval(np.ones(5), h, n, threshold=threshold)
    assert m["f1"] == pytest.approx(pixel_f1(prob, truth, threshold=threshold), rel=1e-12)
    assert m["tp"] == int(((prob > threshold) & (truth == 1)).sum()) and m["tn"] == int(((prob <= threshold) & (truth == 0)).sum())


# ------------------------------------------------------------------------------------------- hold-out split and tiling
def _images(n=3, h=400, seed=0):
    rng = np.random.RandomState(seed)
    return rng.rand(n, h, h, 3).astype(np.float32), rng.rand(n, h, h).astype(np.float32)


@pytest.mark.parametrize("P,S,per_axis", [(388, 572, 1), (128, 312, 3)])
def test_validation_patches_shape_count_and_labels(P, S, per_axis):
    from road_segmentation_unet_amd import hostio
    imgs, gt = _images()
    patches, labels = hostio.validation_patches(imgs, gt, S, P)
    n = 3 * per_axis * per_axis
    assert patches.shape == (n, S, S, 3) and patches.dtype == np.float32
    assert labels.shape == (n, P, P) and labels.dtype == np.int64 and set(np.unique(labels)) == {0, 1}
    off, c0 = (S - P) // 2, (400 - per_axis * P) // 2
    k = 0
    for i in range(3):
        for x in range(per_axis):         # extract_patches' order: x outer, y inner
            for y in range(per_axis):
                y0, x0 = c0 + y * P, c0 + x * P
                assert np.array_equal(labels[k], (gt[i, y0:y0 + P, x0:x0 + P] >= 0.5).astype(np.int64)), (i, x, y)
                # the tile's centre is the image itself, its margin the mirror-expanded image
                assert np.array_equal(patches[k][off:off + P, off:off + P], imgs[i, y0:y0 + P, x0:x0 + P])
                k += 1
    expanded = hostio.mirror_border(imgs, off)
    assert np.array_equal(patches[0], expanded[0, c0:c0 + S, c0:c0 + S])
    with pytest.raises(ValueError):
        hostio.validation_patches(imgs[:, :100, :100], gt[:, :100, :100], S, P)


def test_hold_out_split():
    from road_segmentation_unet_amd import hostio
    from road_segmentation_unet_amd.model import balanced_class_weights
    imgs, gt = _images(n=5, h=32, seed=2)
    gt[3:] = 1.0                                             # the held-out masks are all road: the balanced weights must not see them
    (ti, tg), held = hostio.split_validation(imgs, gt, 2)
    assert np.array_equal(ti, imgs[:3]) and np.array_equal(tg, gt[:3]) and np.array_equal(held[0], imgs[3:]) and np.array_equal(held[1], gt[3:])
    assert balanced_class_weights(tg) == balanced_class_weights(gt[:3]) != balanced_class_weights(gt)
    (ti, tg), held = hostio.split_validation(imgs, gt, 0)
    assert held is None and ti is imgs and tg is gt
    (ti, tg), held = hostio.split_validation(imgs, gt, 4)
    assert len(ti) == 1 and len(held[0]) == 4
    for bad in (5, 6, -1):
        with pytest.raises(ValueError):
            hostio.split_validation(imgs, gt, bad)
