"""-m gpu: include/rsu_components.h against the host restatements of road_segmentation_unet_amd/hostio.py (which tests/test_components_host.py
holds to scipy): labels, areas and edge flags over the bank of tests/components_util.py at both connectivities and for the mask and its
complement; the independence of images; the clean-up bit for bit, in place, with either step alone and on NaN payloads; the pair count
and its accumulation; two runs of every entry byte for byte; ConvolutionalModel.postprocess_masks and evaluate() with
--validate_components above them. Every comparison is integer or bit equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from tests import components_util as CU  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402

SHAPE_IDS = [CU.shape_id(s) for s in CU.SHAPES]


def _np(t):
    return None if t is None else t.cpu().numpy()


# ------------------------------------------------------------------------------------------- rsu_components_label
@pytest.mark.parametrize("connectivity", CU.CONNECTIVITIES)
@pytest.mark.parametrize("shape", CU.SHAPES + [(1, 131, 67)], ids=SHAPE_IDS + ["1x131x67"])
def test_label_equals_the_host_over_the_bank(shape, connectivity):
    for kind in CU.KINDS:
        prob = hu.dev_f32(CU.prob_of(CU.masks(kind, shape)))
        for invert in (False, True):
            want = CU.host_labels(kind, shape, connectivity, invert)
            got = [_np(t) for t in CU.run_label(prob, connectivity, invert, shape)]
            for name, g, w in zip(("labels", "area", "edge"), got, want):
                assert g.dtype == w.dtype and np.array_equal(g, w), (kind, shape, connectivity, invert, name, int((g != w).sum()))
    if shape[1:] == (131, 67):   # the serpentine is one component of 4487 pixels
        lab, area, _ = CU.host_labels("serpentine", shape, 4, False)
        assert set(np.unique(lab)) == {0, 1} and int(area.max()) == 4487


@pytest.mark.parametrize("connectivity", CU.CONNECTIVITIES)
def test_label_with_null_area_and_edge(connectivity):
    shape = (2, 130, 67)
    prob = hu.dev_f32(CU.prob_of(CU.masks("rand0.55", shape)))
    want = CU.host_labels("rand0.55", shape, connectivity, False)
    for want_area, want_edge in ((False, False), (True, False), (False, True)):
        labels, area, edge = CU.run_label(prob, connectivity, False, shape, want_area=want_area, want_edge=want_edge)
        assert np.array_equal(_np(labels), want[0])
        assert area is None or np.array_equal(_np(area), want[1])
        assert edge is None or np.array_equal(_np(edge), want[2])


@pytest.mark.parametrize("connectivity", CU.CONNECTIVITIES)
def test_label_float_bank(connectivity):
    """the threshold itself, the float below it, -0.0, NaNs and infinities: one float32 comparison decides"""
    shape = (2, 130, 67)
    p = CU.float_bank(shape)
    for invert in (False, True):
        want = hostio.label_components(p, CU.THRESHOLD, connectivity, invert)
        got = CU.run_label(hu.dev_f32(p), connectivity, invert, shape)
        for g, w in zip(got, want):
            assert np.array_equal(_np(g), w), (connectivity, invert)
    with np.errstate(invalid="ignore"):
        fg = p >= np.float32(CU.THRESHOLD)
    assert fg[p == np.float32(0.5)].all() and not fg[np.isnan(p)].any() and np.isnan(p).sum() > 100


def test_images_are_independent():
    """the last row of image n and the first row of image n + 1 are both full: neighbours in memory, not in any image"""
    shape = (3, 70, 67)
    m = np.zeros(shape, bool)
    m[:, 0] = m[:, -1] = True
    got = _np(CU.run_label(hu.dev_f32(CU.prob_of(m)), 8, False, shape)[0])
    for n in range(3):
        assert np.all(got[n, 0] == 1) and np.all(got[n, -1] == 69 * 67 + 1) and not got[n, 1:-1].any()
    assert np.array_equal(got, hostio.label_components(CU.prob_of(m), CU.THRESHOLD, 8)[0])


# ------------------------------------------------------------------------------------------- rsu_components_filter
@pytest.mark.parametrize("connectivity", CU.CONNECTIVITIES)
@pytest.mark.parametrize("kind,shape", CU.FILTER_CASES, ids=CU.FILTER_IDS)
def test_filter_equals_the_host(kind, shape, connectivity):
    p = CU.filter_input(kind, shape)
    for min_area, max_hole in CU.FILTER_ARGS:
        want_out, want_stats = hostio.filter_components(p, CU.THRESHOLD, connectivity, min_area, max_hole)
        out, stats = CU.run_filter(hu.dev_f32(p), connectivity, min_area, max_hole, shape)
        what = (kind, shape, connectivity, min_area, max_hole)
        assert np.array_equal(_np(stats), want_stats), (what, _np(stats), want_stats)
        assert np.array_equal(CU.bits(_np(out)), CU.bits(want_out)), what
        # in place, and without stats
        t = hu.dev_f32(p)
        assert CU.bits(_np(t)).tobytes() == CU.bits(p).tobytes()   # (the upload keeps NaN payloads)
        same, none = CU.run_filter(t, connectivity, min_area, max_hole, shape, in_place=True, want_stats=False)
        assert same is t and none is None and np.array_equal(CU.bits(_np(t)), CU.bits(want_out)), what
        # the untouched pixels keep their bits, NaN payloads included
        changed = CU.bits(want_out) != CU.bits(p)
        assert np.array_equal(CU.bits(_np(out))[~changed], CU.bits(p)[~changed])
        if kind == "rand0.55" and shape == (1, 150, 150) and connectivity == 8 and (min_area, max_hole) == (20, 20):
            assert want_stats[0, 1] == 41 and want_stats[0, 4] >= 1000 and changed.sum() > 2000   # the reference itself removes and fills
        if kind == "float_bank" and (min_area, max_hole) == (20, 20):
            assert np.isnan(want_out).sum() > 0 and want_stats[:, 2].sum() > 0 and want_stats[:, 5].sum() > 0


# ------------------------------------------------------------------------------------------- rsu_components_pair_count
@pytest.mark.parametrize("connectivity", CU.CONNECTIVITIES)
@pytest.mark.parametrize("shape", CU.SHAPES, ids=SHAPE_IDS)
def test_pair_count_equals_the_host_and_accumulates(shape, connectivity):
    p = CU.prob_of(CU.masks("rand0.55", shape))
    labels = CU.pair_labels(shape)
    want = hostio.components_pair_count(p, CU.THRESHOLD, labels, connectivity)
    pt, lt = hu.dev_f32(p), torch.from_numpy(labels).to(hu.DEV)
    acc = CU.run_pair_count(pt, lt, connectivity, shape)
    assert np.array_equal(_np(acc), want), (shape, connectivity, _np(acc), want)
    assert want[3] == (shape[0] - 1 if shape[0] > 1 else 1)
    CU.run_pair_count(pt, lt, connectivity, shape, acc=acc)
    assert np.array_equal(_np(acc), 2 * want)
    # nothing counted: exactly nothing is added
    none = torch.full(shape, -1, dtype=torch.int64, device=hu.DEV)
    CU.run_pair_count(pt, none, connectivity, shape, acc=acc)
    assert np.array_equal(_np(acc), 2 * want)


# ------------------------------------------------------------------------------------------- two runs, the same bytes
def test_two_runs_give_identical_bytes():
    shape = (2, 130, 67)
    p = CU.float_bank(shape)
    labels = torch.from_numpy(CU.pair_labels(shape)).to(hu.DEV)
    runs = []
    for _ in range(2):
        pt = hu.dev_f32(p)
        got = [_np(t) for t in CU.run_label(pt, 8, False, shape)] + [_np(t) for t in CU.run_label(pt, 4, True, shape)]
        got += [_np(t) for t in CU.run_filter(pt, 8, 20, 20, shape)] + [_np(CU.run_pair_count(pt, labels, 8, shape))]
        runs.append([a.tobytes() for a in got])
    assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------- the model
ML, MROOT, MP, MB = 3, 16, 20, 2      # the small config of the other model tests


def _model(**kw):
    from road_segmentation_unet_amd.model import ConvolutionalModel, Options
    o = dict(num_layers=ML, root_size=MROOT, patch_size=MP, batch_size=MB, dilated_layers=True, dropout=1.0, lr=0.01, seed=5, logdir=None)
    o.update(kw)
    return ConvolutionalModel(Options(**o), device="cuda:0", params=U.init_params(ML, MROOT, True, seed=13, bias_scale=0.05))


@pytest.mark.parametrize("connectivity", CU.CONNECTIVITIES)
def test_postprocess_masks_equals_the_host(connectivity):
    shape = (2, 130, 67)
    p = CU.float_bank(shape)
    m = _model(min_road_area=20, max_hole_area=20, component_connectivity=connectivity)
    want, stats = hostio.filter_components(p, 0.5, connectivity, 20, 20)
    got = m.postprocess_masks(p[..., None])
    assert got.shape == (2, 130, 67, 1) and got.dtype == np.float32
    assert np.array_equal(CU.bits(got[..., 0]), CU.bits(want))
    assert np.array_equal(m.last_postprocess_stats, stats.sum(axis=0))
    got64 = m.postprocess_masks(np.nan_to_num(p[..., None]).astype(np.float64), threshold=0.5)
    assert got64.dtype == np.float64 and np.array_equal(got64[..., 0].astype(np.float32), hostio.filter_components(np.nan_to_num(p), 0.5, connectivity, 20, 20)[0])
    one = _model(min_road_area=0, max_hole_area=20, component_connectivity=connectivity).postprocess_masks(p[..., None])
    assert np.array_equal(CU.bits(one[..., 0]), CU.bits(hostio.filter_components(p, 0.5, connectivity, 0, 20)[0]))


def _patches(n, seed=21, p_road=0.3):
    S = U.input_size_needed(MP, ML)
    rng = np.random.RandomState(seed)
    return rng.rand(n, S, S, 3).astype(np.float32), (rng.rand(n, MP, MP) < p_road).astype(np.int64)


def test_evaluate_with_validate_components():
    """b0_error and the two counts equal the host's count over net.prob of every chunk (the last one padded with zero patches labelled -1);
    without the flag the result has none of the new keys"""
    N = 5
    X, y = _patches(N)
    y[1, :3] = -1
    m = _model(validate_components=True, component_connectivity=8)
    out = m.evaluate(X, y, threshold=0.5)
    net, B = m.net, m.local_batch
    acc = np.zeros(4, np.int64)
    for t0 in range(0, N, B):
        nb = min(B, N - t0)
        xb, yb = np.zeros((B,) + X.shape[1:], np.float32), np.full((B, MP, MP), -1, np.int64)
        xb[:nb], yb[:nb] = X[t0:t0 + nb], y[t0:t0 + nb]
        net.x.copy_(torch.from_numpy(xb))
        net.labels.copy_(torch.from_numpy(yb))
        net.forward_device(keep=1.0)
        net.evaluate_device()   # (the head writes net.prob)
        acc += hostio.components_pair_count(net.prob.cpu().numpy().reshape(B, MP, MP), 0.5, yb, 8)
    assert acc[3] == N and acc[1] > N
    assert out["components_pred"] == acc[0] and out["components_true"] == acc[1] and out["b0_error"] == acc[2] / N
    again = m.evaluate(X, y, threshold=0.5)
    assert (again["components_pred"], again["components_true"], again["b0_error"]) == (out["components_pred"], out["components_true"], out["b0_error"])
    plain = _model().evaluate(X, y, threshold=0.5)
    assert not {"components_pred", "components_true", "b0_error"} & set(plain)
    assert plain["f1"] == out["f1"] and np.array_equal(plain["sums"], out["sums"])


def test_cli_inference_cleans_up_between_prediction_and_quantisation(tmp_path, capsys, monkeypatch):
    """--min_road_area / --max_hole_area on the command line: postprocess_masks runs on what predict_batchwise returned, its result is
    what quantize_mask gets, and one line reports the summed stats"""
    from PIL import Image
    from road_segmentation_unet_amd import model as M
    from road_segmentation_unet_amd.cli import main
    rng = np.random.RandomState(4)
    ev = tmp_path / "eval"
    ev.mkdir()
    for i in range(2):
        Image.fromarray((rng.rand(48, 48, 3) * 255).astype(np.uint8)).save(ev / ("test_%d.png" % i))
    seen = {}
    post, quant = M.ConvolutionalModel.postprocess_masks, M.ConvolutionalModel.quantize_mask

    def spy_post(self, masks, threshold=0.5):
        seen["in"], seen["threshold"] = np.array(masks), threshold
        seen["out"] = post(self, masks, threshold=threshold)
        return seen["out"]

    def spy_quant(self, masks, threshold, patch_size):
        seen["quantized"] = masks
        return quant(self, masks, threshold, patch_size)

    monkeypatch.setattr(M.ConvolutionalModel, "postprocess_masks", spy_post)
    monkeypatch.setattr(M.ConvolutionalModel, "quantize_mask", spy_quant)
    argv = ["--num_layers=2", "--root_size=16", "--patch_size=16", "--stride=16", "--batch_size=4", "--num_epoch=0", "--eval_data_dir=%s" % ev,
            "--save_path=%s" % (tmp_path / "runs"), "--pred_batch_size=2", "--seed=5", "--min_road_area=6", "--max_hole_area=6",
            "--component_connectivity=4"]
    assert main(argv) == 0
    assert seen["in"].shape == (2, 48, 48, 1) and seen["threshold"] == 0.5 and seen["quantized"] is seen["out"]
    want, stats = hostio.filter_components(seen["in"][..., 0], 0.5, 4, 6, 6)
    assert np.array_equal(CU.bits(seen["out"][..., 0]), CU.bits(want))
    line = "Mask clean-up: {} components, {} removed ({} pixels); {} holes, {} filled ({} pixels)".format(*[int(v) for v in stats.sum(axis=0)])
    assert line in capsys.readouterr().out
