"""-m gpu: ConvolutionalModel.predict on images of any size -- rectangular, a stride that does not cover the image (clamped last tile) --
on both of its paths, the six-way ensemble on H != W, the training loop's periodic prediction and the command line."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd import images as dimages  # noqa: E402
from road_segmentation_unet_amd._lib import call  # noqa: E402
from road_segmentation_unet_amd.model import ConvolutionalModel, Options  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests import rect_util as R  # noqa: E402


def _model(L, P, stride, ensemble, dilated=True, batch=4, seed=3):
    params = U.init_params(L, 16, dilated, seed=seed, bias_scale=0.05)
    opts = Options(num_layers=L, root_size=16, patch_size=P, stride=stride, dilated_layers=dilated, batch_size=batch,
                   ensemble_prediction=ensemble, dropout=1.0)
    return ConvolutionalModel(opts, params=params), params


class _Env:
    """environment variables set for a block and put back behind it"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("ensemble", [False, True])
def test_predict_rectangle_matches_oracle(ensemble):
    """2 images of 47 x 58 at P = 20, stride 12: both axes end in a clamped tile. Per tile the arithmetic is that of a square image and
    averaging does not widen it: the tolerances are test_predict_matches_oracle's."""
    L, P, stride = 3, 20, 12
    imgs = np.random.RandomState(1).rand(2, 47, 58, 3).astype(np.float32)
    m, params = _model(L, P, stride, ensemble, seed=2)
    masks = m.predict(imgs)
    assert masks.shape == (2, 47, 58, 1)
    ref = R.oracle_predict(params, imgs, L, 16, True, P, stride, ensemble)
    err = np.abs(masks - ref).max()
    ref32 = R.oracle_predict(params, imgs, L, 16, True, P, stride, ensemble, emu=False)
    err32 = np.abs(masks - ref32).max()
    print("max error against the bf16-emulating oracle %.3g, against float32 %.3g" % (err, err32))
    assert err <= 4e-3
    assert err32 <= 3e-2
    np.testing.assert_allclose(m.predict_batchwise(imgs, 1), masks, rtol=0, atol=1e-6)


@pytest.mark.parametrize("L,P,H,W,stride,ensemble", [(3, 20, 47, 58, 12, True), (4, 28, 64, 75, 6, False), (3, 20, 44, 44, 7, False)])
def test_shared_window_equals_tilewise_on_any_geometry(L, P, H, W, stride, ensemble):
    """the masks of the two paths add the same tiles in the same order in different launch groupings (fp32 association: the bound of
    test_shared_window_prediction_equals_tilewise); the shared path's tiles are the per-tile forward passes' bit for bit"""
    imgs = np.random.RandomState(L + stride).rand(2, H, W, 3).astype(np.float32)
    m, _ = _model(L, P, stride, ensemble)
    with _Env(RSU_PREDICT_SHARED="0"):
        tilewise = m.predict(imgs)
    with _Env(RSU_PREDICT_SHARED="1"):
        shared = m.predict(imgs)
        with _Env(RSU_PREDICT_MAX_WINDOW=str(m.input_size + 8)):   # runs of one or two tiles per axis
            shared_small = m.predict(imgs)
    assert tilewise.shape == (2, H, W, 1)
    np.testing.assert_allclose(shared, tilewise, rtol=0, atol=5e-7)
    np.testing.assert_allclose(shared_small, tilewise, rtol=0, atol=5e-7)
    x = torch.as_tensor(imgs).to(m.net.device)
    stacks = [x]
    if ensemble:
        stacks = [s.contiguous() for s in dimages.image_augmentation_ensemble_rect(x)] if H != W else [dimages.image_augmentation_ensemble(x).contiguous()]
    m.net.training = False
    B = m.local_batch
    for s in stacks:
        tiles = m._shared_window_tiles(s)
        assert tiles.shape[1:] == (len(hostio.tile_origins(s.shape[2], P, stride)), len(hostio.tile_origins(s.shape[1], P, stride)), P, P)
        flat = tiles.view(-1, P, P)
        for t0 in range(0, flat.shape[0], B):
            nb = min(B, flat.shape[0] - t0)
            dimages.extract_mirrored_patches(s, m.input_size, P, stride, t0=t0, ntiles=nb, out=m.net.x[:nb])
            m.net.forward_device()
            assert torch.equal(m.net.prob[:nb], flat[t0:t0 + nb]), t0


@pytest.mark.parametrize("ensemble", [False, True])
def test_square_covered_input_keeps_its_bits(ensemble):
    """an input the square entries accept: predict() on the default path against a mask assembled here from those entries
    (rsu_extract_tiles, forward_device, ONE rsu_overlap_add of all tiles -- the shared path's grouping --, rsu_overlap_finish)"""
    L, P, H, stride = 3, 20, 44, 12
    imgs = np.random.RandomState(4).rand(2, H, H, 3).astype(np.float32)
    m, _ = _model(L, P, stride, ensemble)
    with _Env(RSU_PREDICT_SHARED="1"):
        masks = m.predict(imgs)
    x = torch.as_tensor(imgs).to(m.net.device)
    if ensemble:
        x = dimages.image_augmentation_ensemble(x).contiguous()
    n, S, B = x.shape[0], m.input_size, m.local_batch
    pps = (H - P) // stride + 1
    nt = n * pps * pps
    probs = torch.zeros((nt, P, P), dtype=torch.float32, device=m.net.device)
    m.net.training = False
    for t0 in range(0, nt, B):
        nb = min(B, nt - t0)
        if nb < B:
            m.net.x.zero_()
        call("rsu_extract_tiles", hu.ptr(x), hu.ptr(m.net.x), n, H, S, P, stride, t0, nb, hu.stream())
        m.net.forward_device()
        probs[t0:t0 + nb] = m.net.prob[:nb]
    acc = torch.zeros((n, H, H), dtype=torch.float32, device=m.net.device)
    hits, out = torch.zeros_like(acc), torch.zeros_like(acc)
    call("rsu_overlap_add", hu.ptr(probs), hu.ptr(acc), hu.ptr(hits), n, H, P, stride, 0, nt, hu.stream())
    call("rsu_overlap_finish", hu.ptr(acc), hu.ptr(hits), hu.ptr(out), acc.numel(), hu.stream())
    want = out.unsqueeze(-1)
    if ensemble:
        want = dimages.invert_image_augmentation_ensemble(want)
    np.testing.assert_array_equal(masks, want.cpu().numpy())


def test_predict_refuses_an_image_smaller_than_the_patch():
    m, _ = _model(3, 20, 12, False)
    with pytest.raises(ValueError, match=r"19 x 58.*--patch_size=20"):
        m.predict(np.zeros((1, 19, 58, 3), np.float32))


def test_training_reaches_its_periodic_prediction_at_any_stride():
    """--patch_size=20 --stride=12 on 46-pixel training images: (46 - 20) % 12 != 0, fine for cutting training patches; the prediction
    every --eval_every steps runs with a clamped last tile instead of asserting"""
    L, P, B = 3, 20, 2
    S = U.input_size_needed(P, L)
    rng = np.random.RandomState(8)
    imgs = rng.rand(2, 46, 46, 3).astype(np.float32)
    truth = (imgs[..., 0] > 0.5) * 1.0
    patches = rng.rand(7, S, S, 3)
    off = (S - P) // 2
    labels = (patches[:, off:off + P, off:off + P, 0] > 0.5) * 1.0
    m = ConvolutionalModel(Options(num_layers=L, root_size=16, patch_size=P, stride=12, batch_size=B, dropout=1.0, lr=0.05, seed=7,
                                   eval_every=2, logdir=None))
    seen = []
    predict = m.predict
    m.predict = lambda x, *a, **kw: seen.append(predict(x, *a, **kw)) or seen[-1]
    stats = m.train(patches, labels, imgs, truth)
    assert stats["patches"] == 6 and m.net.global_step == 3
    assert len(seen) == 1 and seen[0].shape == (2, 46, 46, 1) and np.isfinite(seen[0]).all()


def test_cli_predicts_a_directory_of_rectangles(tmp_path):
    from PIL import Image
    from road_segmentation_unet_amd.cli import main
    rng = np.random.RandomState(4)
    ev, save = tmp_path / "eval", tmp_path / "runs"
    ev.mkdir()
    for i in range(3):
        Image.fromarray((rng.rand(48, 64, 3) * 255).astype(np.uint8)).save(ev / ("test_%d.png" % i))
    argv = ["--num_layers=2", "--root_size=16", "--patch_size=16", "--stride=12", "--batch_size=4", "--num_epoch=0",
            "--eval_data_dir=%s" % ev, "--save_path=%s" % save, "--pred_batch_size=2", "--ensemble_prediction", "--seed=5"]
    assert main(argv) == 0
    runs = [d for d in os.listdir(save) if os.path.isdir(save / d)]
    assert len(runs) == 1
    assert any(f.endswith("-model.chkpt.npz") for f in os.listdir(save))
    files = os.listdir(save / runs[0])
    lines = open(save / runs[0] / "submission.csv").read().strip().split("\n")
    assert lines[0] == "id,prediction" and len(lines) == 3 * 3 * 4 + 1
    assert lines[1].startswith("001_0_0,") and lines[2].startswith("001_0_16,") and lines[-1].startswith("003_48_32,")
    pngs = sorted(f for f in files if f.endswith(".png"))
    assert len(pngs) == 3
    assert Image.open(save / runs[0] / pngs[0]).size == (64, 48)
