"""-m gpu: parity at the sizes and on the data the BASELINE configurations name.
  * real aerial crops from the reference's own training set (tests/golden/real_crops.npz): train on 12, hold 6 out, and require the
    pixel-F1 of the HIP path within 1e-3 of the float32 oracle run with the same trained weights (the north_star tolerance);
  * config 3 (num_layers=6 root_size=64 patch_size=388 --dilated_layers) forward at full size, one patch, against the oracle;
  * config 4's per-GPU share (num_layers=6, four patches): a full-size training step -- properties only (the oracle would need
    hours): finite, repeatable bit for bit, loss falls on a repeated batch;
  * config 5 (604x604, stride 12, 6-way ensemble, 2166 tiles): shared-window masks == tile-by-tile masks, one tile against the
    oracle forward.
The network oracle stays parity-unpinned at the TensorFlow boundary (oracle/unet_oracle.py header); these tests pin the HIP path to
it, not to TensorFlow."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tiler_oracle as T  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402
from road_segmentation_unet_amd.model import ConvolutionalModel, Options, pixel_f1  # noqa: E402
from road_segmentation_unet_amd.unet import UNet  # noqa: E402
from tests import golden_store  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests.parity_record import record  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def _predict_hip(net, xs, B):
    net.training = False
    out = []
    for i in range(0, xs.shape[0], B):
        xb = xs[i:i + B]
        net.x.zero_()
        net.x[:xb.shape[0]].copy_(torch.from_numpy(xb.astype(np.float32)))
        net.forward_device()
        out.append(net.prob[:xb.shape[0]].cpu().numpy().copy())
    return np.concatenate(out)


def test_real_crops_pixel_f1_within_1e3_of_the_float32_oracle():
    """Held-out real crops through a TRAINED network (tests/golden/real_crops_trained_params.part*.npz: the L=3, root=32 net after 90 epochs
    on the 12 training crops, written by tests/golden/make_trained_params.py): pixel-F1 of the HIP path within 1e-3 of the float32
    oracle with the same weights. (Training inside the test made the F1 hinge on the summation order of the weight gradients: 0.38,
    0.15 and 0.0 after 240 steps for three builds that differ in nothing else -- see the next test for the training side.)"""
    z = np.load(os.path.join(HERE, "golden", "real_crops.npz"))
    x = z["x"].astype(np.float64) / 255.0
    y = (z["y"].astype(np.float64) / 255.0 >= 0.5) * 1.0
    P, S = int(z["P"]), int(z["S"])
    L, root, B = 3, 32, 4
    assert S == U.input_size_needed(P, L)
    xte, yte = x[12:], y[12:]
    pz = golden_store.load(os.path.join(HERE, "golden", "real_crops_trained_params"))   # (stored in parts: tests/golden_store.py)
    params = {k.replace("__", "/"): v for k, v in pz.items()}
    net = UNet(L, root, False, B, P, params=params, training=False)
    hip = _predict_hip(net, xte, B)
    ref = U.predict_probs(params, xte.astype(np.float32), L, root, False)                       # float32 oracle
    emu = U.predict_probs(params, xte.astype(np.float32), L, root, False, emulate_bf16=True)   # same rounding points as the HIP path
    f_hip, f_ref, f_emu = pixel_f1(hip, yte), pixel_f1(ref, yte), pixel_f1(emu, yte)
    print("pixel-F1 on 6 held-out real crops: hip %.5f  fp32 oracle %.5f  bf16-emulating oracle %.5f" % (f_hip, f_ref, f_emu))
    assert f_ref > 0.3, f_ref                      # the road class was actually learned on real data
    assert np.abs(hip - emu).max() <= 4e-3
    assert abs(f_hip - f_ref) <= 1e-3, (f_hip, f_ref)


def test_real_crops_training_then_inference_matches_the_rounding_emulating_oracle():
    """The training side on real data: 120 HIP steps from Glorot weights bring the loss down, and the network they produce predicts
    the held-out crops like the bf16-emulating oracle does with the same weights (wherever the chaotic trajectory has led)."""
    z = np.load(os.path.join(HERE, "golden", "real_crops.npz"))
    x = z["x"].astype(np.float64) / 255.0
    y = (z["y"].astype(np.float64) / 255.0 >= 0.5) * 1.0
    P, L, root, B = int(z["P"]), 3, 32, 4
    xtr, ytr, xte = x[:12], y[:12], x[12:]
    m = ConvolutionalModel(Options(num_layers=L, root_size=root, patch_size=P, batch_size=B, dropout=1.0, lr=0.02, seed=21, logdir=None))
    # the reference's loop drops the tail batch: 13 patches -> 3 steps of 4 per epoch (one crop doubled)
    xtr13, ytr13 = np.concatenate([xtr, xtr[:1]]), np.concatenate([ytr, ytr[:1]])
    first = m.train(xtr13, ytr13, None, None)["loss"]
    for _ in range(39):
        st = m.train(xtr13, ytr13, None, None)
    assert np.isfinite(st["loss"]) and st["loss"] < first, (first, st["loss"])
    params = {k: v for k, v in m.net.state_dict().items() if not k.endswith("/Momentum") and k != "global_step"}
    hip = _predict_hip(m.net, xte, B)
    emu = U.predict_probs(params, xte.astype(np.float32), L, root, False, emulate_bf16=True)
    assert np.abs(hip - emu).max() <= 4e-3


def test_config3_full_size_dilated_forward_matches_oracle():
    L, root, P = 6, 64, 388
    S = U.input_size_needed(P, L)
    assert S == 764
    rng = np.random.RandomState(31)
    x = rng.rand(1, S, S, 3).astype(np.float32)
    params = U.init_params(L, root, True, seed=32, bias_scale=0.02)
    net = UNet(L, root, True, 1, P, params=params, training=False)
    net.x.copy_(torch.from_numpy(x))
    net.forward_device()
    hip = net.prob.cpu().numpy().copy()
    emu = U.predict_probs(params, x, L, root, True, emulate_bf16=True)
    assert hip.shape == emu.shape == (1, P, P)
    assert np.isfinite(hip).all()
    record("c3_forward_full_size", d_emu_max=float(np.abs(hip - emu).max()), d_emu_mean=float(np.abs(hip - emu).mean()))
    assert np.abs(hip - emu).max() <= 4e-3, float(np.abs(hip - emu).max())


def test_config3_full_size_dilated_backward_layers_match_oracle():
    """config 3 (L=6, root 64, dilated, 764 -> 388) BACKWARD at full size. A whole-net oracle backward would take the host hours; the
    largest dilated and concat layers are checked one by one instead, each against the oracle's layer operator on the very tensors the
    HIP pass left in its buffers (activations and incoming gradients, bf16): weight gradient + bias gradient, and the backward-data
    launch where its output buffer has a single writer. Covers dil = 2 backward-data / weight-gradient launches at 760-px geometry, the
    3 x 1024-channel concat of conv_6/conv1 and the 3 x 64-channel one of conv_10/conv1."""
    L, root, P = 6, 64, 388
    S = U.input_size_needed(P, L)
    rng = np.random.RandomState(61)
    x = rng.rand(1, S, S, 3).astype(np.float32)
    labels = (rng.rand(1, P, P) < 0.2).astype(np.int64)
    params = U.init_params(L, root, True, seed=62, bias_scale=0.02)
    net = UNet(L, root, True, 1, P, params=params, training=True)
    net.x.copy_(torch.from_numpy(x))
    net.labels.copy_(torch.from_numpy(labels))
    net.forward_device()
    net.backward_device(1.0 / (P * P))
    torch.cuda.synchronize()

    def act(k):
        return net.act[k].float().cpu().numpy()

    def grd(k):
        return net.grad[k].float().cpu().numpy()

    worst = {}

    def check_w(name, xin, dz, dil):
        rdw, rdb = U.conv2d_bwd_weight(xin, dz, dil=dil)
        gw, gb = net.g[name + "/kernel"].cpu().numpy(), net.g[name + "/bias"].cpu().numpy()
        hu.assert_f32_close(gw, rdw, name + " weight gradient", rtol=2e-4, atol_scale=2e-5)
        hu.assert_f32_close(gb, rdb, name + " bias gradient", rtol=2e-4, atol_scale=2e-5)
        worst[name + "/wgrad_rel"] = float(np.linalg.norm(gw - rdw) / np.linalg.norm(rdw))

    def check_dx(name, dz, w, in_hw, dil, got, mask=None, what=""):
        ref = U.conv2d_bwd_data(dz, hu.q(w), in_hw, dil=dil)
        if mask is not None:
            ref = U.relu_bwd(mask, ref)
        hu.assert_bf16_close(got, ref, name + " backward-data" + what)
        worst[name + "/bwd_data_rel" + what] = float(np.linalg.norm(got - hu.q(ref)) / max(np.linalg.norm(ref), 1e-30))

    # conv_dilut_0/atrous_conv2: 64 -> 64, dilation 2, 760 -> 756 px (the largest dilated launch)
    d1, dzd2 = act("d1_0"), grd("d2_0")
    check_w("conv_dilut_0/atrous_conv2", d1, dzd2, 2)
    check_dx("conv_dilut_0/atrous_conv2", dzd2, params["conv_dilut_0/atrous_conv2/kernel"], d1.shape[1:3], 2, grd("d1_0"), mask=d1)
    # conv_dilut_1/atrous_conv1: 64 -> 128, dilation 2 on the pooled level-0 tensor (its backward-data ACCUMULATES into the pool gradient
    # beside conv_1/conv1's: weight gradient only), and atrous_conv2 of the same level with its masked backward-data
    check_w("conv_dilut_1/atrous_conv1", act("pool_0"), grd("d1_1"), 2)
    d1, dzd2 = act("d1_1"), grd("d2_1")
    check_w("conv_dilut_1/atrous_conv2", d1, dzd2, 2)
    check_dx("conv_dilut_1/atrous_conv2", dzd2, params["conv_dilut_1/atrous_conv2/kernel"], d1.shape[1:3], 2, grd("d1_1"), mask=d1)
    # conv_dilut_4/atrous_conv2: 1024 -> 1024, dilation 2, the deepest live dilated pair
    d1, dzd2 = act("d1_4"), grd("d2_4")
    check_w("conv_dilut_4/atrous_conv2", d1, dzd2, 2)
    check_dx("conv_dilut_4/atrous_conv2", dzd2, params["conv_dilut_4/atrous_conv2/kernel"], d1.shape[1:3], 2, grd("d1_4"), mask=d1)
    # conv_6/conv1: concat [skip 1024, dilated skip 1024, up 1024] -> 1024 at 32 px (3072 input channels)
    h = net.act["up_0"].shape[1]
    cat = np.concatenate([U.center_crop(act("c2_4"), h, h), U.center_crop(act("d2_4"), h, h), act("up_0")], axis=3)
    dz1 = grd("c1_6")
    check_w("conv_6/conv1", cat, dz1, 1)
    w6 = params["conv_6/conv1/kernel"]
    check_dx("conv_6/conv1", dz1, w6[:, :, 2048:3072, :], (h, h), 1, grd("up_0"), what=" (up source)")
    check_dx("conv_6/conv1", dz1, w6[:, :, 1024:2048, :], (h, h), 1, grd("skipd_0"), what=" (dilated skip source)")
    # conv_10/conv1: the last decoder stage, concat [64, 64, 64] -> 64 at 392 px
    h = net.act["up_4"].shape[1]
    cat = np.concatenate([U.center_crop(act("c2_0"), h, h), U.center_crop(act("d2_0"), h, h), act("up_4")], axis=3)
    dz1 = grd("c1_10")
    check_w("conv_10/conv1", cat, dz1, 1)
    check_dx("conv_10/conv1", dz1, params["conv_10/conv1/kernel"][:, :, 128:192, :], (h, h), 1, grd("up_4"), what=" (up source)")
    record("c3_backward_layers_full_size", **worst)
    print("c3 backward, layer by layer at full size:", {k: "%.2e" % v for k, v in worst.items()})


@pytest.mark.parametrize("B", [2, 4])
def test_config4_share_full_size_backward_layers_match_oracle(B):
    """config 4's network (L=6, root 64, NOT dilated, 764 -> 388), two patches and the per-GPU share of config 4 itself (FOUR distinct
    patches, the batch `bench.py --workload c4` times: VERDICT r5 item 5), BACKWARD at full size, layer by layer like the config-3
    test above: the deepest block (1024 -> 2048 -> 2048 at 20 -> 16 px), the widest concat (conv_6/conv1: 2 x 1024 -> 1024) and the
    full-resolution decoder stage (conv_10: 128 -> 64 -> 64 at 392 px) -- weight / bias gradients and backward-data against the oracle's
    layer operators on the tensors of the HIP pass"""
    L, root, P = 6, 64, 388
    S = U.input_size_needed(P, L)
    rng = np.random.RandomState(71)
    x = rng.rand(B, S, S, 3).astype(np.float32)
    labels = (rng.rand(B, P, P) < 0.2).astype(np.int64)
    params = U.init_params(L, root, False, seed=72, bias_scale=0.02)
    net = UNet(L, root, False, B, P, params=params, training=True)
    net.x.copy_(torch.from_numpy(x))
    net.labels.copy_(torch.from_numpy(labels))
    net.forward_device()
    net.backward_device(1.0 / (B * P * P))
    torch.cuda.synchronize()

    def act(k):
        return net.act[k].float().cpu().numpy()

    def grd(k):
        return net.grad[k].float().cpu().numpy()

    worst = {}

    def check_w(name, xin, dz):
        rdw, rdb = U.conv2d_bwd_weight(xin, dz)
        gw, gb = net.g[name + "/kernel"].cpu().numpy(), net.g[name + "/bias"].cpu().numpy()
        hu.assert_f32_close(gw, rdw, name + " weight gradient", rtol=2e-4, atol_scale=2e-5)
        hu.assert_f32_close(gb, rdb, name + " bias gradient", rtol=2e-4, atol_scale=2e-5)
        worst[name + "/wgrad_rel"] = float(np.linalg.norm(gw - rdw) / np.linalg.norm(rdw))

    def check_dx(name, dz, w, in_hw, got, mask=None, what=""):
        ref = U.conv2d_bwd_data(dz, hu.q(w), in_hw)
        if mask is not None:
            ref = U.relu_bwd(mask, ref)
        hu.assert_bf16_close(got, ref, name + " backward-data" + what)
        worst[name + "/bwd_data_rel" + what] = float(np.linalg.norm(got - hu.q(ref)) / max(np.linalg.norm(ref), 1e-30))

    # the deepest block: conv_5/conv2 (2048 -> 2048) and conv_5/conv1 (1024 -> 2048 on the pooled level-4 tensor)
    c1, dz2 = act("c1_5"), grd("c2_5")
    check_w("conv_5/conv2", c1, dz2)
    check_dx("conv_5/conv2", dz2, params["conv_5/conv2/kernel"], c1.shape[1:3], grd("c1_5"), mask=c1)
    check_w("conv_5/conv1", act("pool_4"), grd("c1_5"))
    # conv_6/conv1: concat [skip 1024, up 1024] -> 1024
    h = net.act["up_0"].shape[1]
    cat = np.concatenate([U.center_crop(act("c2_4"), h, h), act("up_0")], axis=3)
    dz1 = grd("c1_6")
    check_w("conv_6/conv1", cat, dz1)
    check_dx("conv_6/conv1", dz1, params["conv_6/conv1/kernel"][:, :, 1024:2048, :], (h, h), grd("up_0"), what=" (up source)")
    check_dx("conv_6/conv1", dz1, params["conv_6/conv1/kernel"][:, :, 0:1024, :], (h, h), grd("skip_0"), what=" (skip source)")
    # conv_10: the full-resolution decoder stage
    c1, dz2 = act("c1_10"), grd("c2_10")
    check_w("conv_10/conv2", c1, dz2)
    check_dx("conv_10/conv2", dz2, params["conv_10/conv2/kernel"], c1.shape[1:3], grd("c1_10"), mask=c1)
    h = net.act["up_4"].shape[1]
    cat = np.concatenate([U.center_crop(act("c2_0"), h, h), act("up_4")], axis=3)
    check_w("conv_10/conv1", cat, grd("c1_10"))
    record("c4_backward_layers_full_size" + ("" if B == 2 else "_batch%d" % B), **worst)
    print("c4 (B = %d) backward, layer by layer at full size:" % B, {k: "%.2e" % v for k, v in worst.items()})


def test_real_388_patches_pixel_f1_within_1e3_of_the_float32_oracle():
    """The north_star's F1 claim on 388-px patches: the 16 held-out 388-patches (4 real 400-px images of the reference's training set,
    stride 12: 2.4 M pixels) through an L=5, root=16 U-Net trained on the other 96 images (tests/golden/real388_trained_params.part*.npz,
    written by tests/golden/make_trained_params_388.py on the GPU): pixel-F1 of the HIP path within 1e-3 of the float32 oracle with
    the same weights, and the probabilities within the stated bf16 tolerance of the rounding-emulating oracle."""
    z = golden_store.load(os.path.join(HERE, "golden", "real388_heldout"))
    pz = golden_store.load(os.path.join(HERE, "golden", "real388_trained_params"))
    params = {k.replace("__", "/"): v for k, v in pz.items()}
    L, root, P, S = int(z["L"]), int(z["root"]), int(z["P"]), int(z["S"])
    x = z["x"].astype(np.float32) / 255.0
    y = (z["y"].astype(np.float32) / 255.0 >= 0.5) * 1.0
    off = (S - P) // 2
    xs, ys = [], []
    for i in range(x.shape[0]):
        xp = np.pad(x[i], ((off, off), (off, off), (0, 0)), mode="symmetric")
        for ox in range(0, x.shape[1] - P + 1, 12):
            for oy in range(0, x.shape[1] - P + 1, 12):
                xs.append(xp[oy:oy + S, ox:ox + S])
                ys.append(y[i][oy:oy + P, ox:ox + P])
    xs, ys = np.stack(xs), np.stack(ys)
    assert xs.shape[0] >= 4 and ys.size >= 600000
    B = 4
    net = UNet(L, root, False, B, P, params=params, training=False)
    hip = _predict_hip(net, xs, B)
    ref = U.predict_probs(params, xs, L, root, False)
    emu = U.predict_probs(params, xs, L, root, False, emulate_bf16=True)
    f_hip, f_ref, f_emu = pixel_f1(hip, ys), pixel_f1(ref, ys), pixel_f1(emu, ys)
    record("real_388_patches_f1", f1_hip=f_hip, f1_f32_oracle=f_ref, f1_bf16_oracle=f_emu, pixels=ys.size,
           d_emu_max=float(np.abs(hip - emu).max()), d_emu_mean=float(np.abs(hip - emu).mean()), d_f32_max=float(np.abs(hip - ref).max()),
           d_f32_mean=float(np.abs(hip - ref).mean()))
    print("pixel-F1 on %d held-out 388-patches (%d pixels): hip %.5f  fp32 oracle %.5f  bf16-emulating oracle %.5f" %
          (xs.shape[0], ys.size, f_hip, f_ref, f_emu))
    assert f_ref >= 0.8, f_ref          # a network that actually segments roads
    # trained weights decide sharply: over 2.4 M pixels the worst rounding-boundary flip between two correct bf16 evaluations reaches
    # 4.1e-3 (profiles/r03/parity.json); stated tolerance 8e-3 at the worst pixel, 2e-4 on average, 3e-2 against the float32 oracle
    assert np.abs(hip - emu).max() <= 8e-3 and np.abs(hip - emu).mean() <= 2e-4
    assert np.abs(hip - ref).max() <= 3e-2
    assert abs(f_hip - f_ref) <= 1e-3, (f_hip, f_ref)


def test_config4_share_full_size_training_step_properties():
    L, root, P, B = 6, 64, 388, 4
    S = U.input_size_needed(P, L)
    g = torch.Generator().manual_seed(41)
    x = torch.rand((B, S, S, 3), generator=g)
    labels = (torch.rand((B, P, P), generator=g) < 0.2).to(torch.int64)
    finals, losses = [], []
    for rep in range(2):
        net = UNet(L, root, False, B, P, seed=42, training=True)
        net.x.copy_(x)
        net.labels.copy_(labels)
        ls = []
        for _ in range(3):
            net.forward_device()
            net.backward_device(1.0 / (B * P * P))
            ls.append(float(net.loss_sum.item()) / (B * P * P))
            assert torch.isfinite(net.flat_g[:net.n_live]).all()
            net.apply_momentum(0.01, 0.9)
        torch.cuda.synchronize()
        finals.append(net.flat_w.clone())
        losses.append(ls)
        del net
        torch.cuda.empty_cache()
    assert losses[0] == losses[1], losses                 # bit-repeatable, tile-shape tuning and two streams included
    assert torch.equal(finals[0], finals[1])
    assert all(np.isfinite(losses[0])) and losses[0][2] < losses[0][0], losses[0]
    assert abs(losses[0][0] - np.log(2.0)) < 0.3          # Glorot weights: the first loss sits near ln 2


def test_config5_full_size_sliding_window(monkeypatch):
    # (the tiles of a shared window and of the per-tile pass are the same bits only while every layer sums its reduction in the same
    # order in both: the geometry-dependent split of the deep layers' reductions, rsu.h rsu_conv2d_fwd_k, is switched off for this property
    # test; test_config5_shared_windows_with_split_reductions checks the default path against it by tolerance)
    monkeypatch.setenv("RSU_KSPLIT", "0")
    L, root, P, H, stride = 6, 64, 388, 604, 12
    rng = np.random.RandomState(51)
    img = rng.rand(1, H, H, 3).astype(np.float32)
    params = U.init_params(L, root, True, seed=52, bias_scale=0.02)
    m = ConvolutionalModel(Options(num_layers=L, root_size=root, patch_size=P, stride=stride, dilated_layers=True, batch_size=4,
                                   ensemble_prediction=True, dropout=1.0, logdir=None), params=params)
    old = os.environ.get("RSU_PREDICT_SHARED")
    try:
        os.environ["RSU_PREDICT_SHARED"] = "1"
        shared = m.predict(img)
        os.environ["RSU_PREDICT_SHARED"] = "0"
        tilewise = m.predict(img)
    finally:
        if old is None:
            os.environ.pop("RSU_PREDICT_SHARED", None)
        else:
            os.environ["RSU_PREDICT_SHARED"] = old
    pps = (H - P) // stride + 1
    assert pps == 19 and 6 * pps * pps == 2166
    assert shared.shape == tilewise.shape == (1, H, H, 1)
    assert shared.min() >= 0.0 and shared.max() <= 1.0 and np.isfinite(shared).all()
    np.testing.assert_allclose(shared, tilewise, rtol=0, atol=5e-7)     # same tiles, fp32 association of the overlap sum only
    # one tile of the 2166 against the oracle forward: variant 3 (rot90) of the ensemble, tile (x index 7, y index 11)
    S = m.input_size
    ens = T.image_augmentation_ensemble(img)
    tiles = T.extract_patches(T.mirror_border(ens[3:4], (S - P) // 2), S, stride=stride, predict_patch_size=P)
    t = 7 * pps + 11
    emu = U.predict_probs(params, tiles[t:t + 1].astype(np.float32), L, root, True, emulate_bf16=True)
    m.net.training = False
    m.net.x.zero_()
    m.net.x[0].copy_(torch.from_numpy(tiles[t].astype(np.float32)))
    m.net.forward_device()
    got = m.net.prob[0].cpu().numpy()
    assert np.abs(got - emu[0]).max() <= 4e-3


def test_config5_shared_windows_with_split_reductions(monkeypatch):
    """config 5's default inference path (deep layers with split reductions, rsu_conv2d_fwd_k) against the same path without the split:
    the masks differ by rounding-boundary flips of single bf16 activations only"""
    L, root, P, H, stride = 6, 64, 388, 604, 12
    rng = np.random.RandomState(51)
    img = rng.rand(1, H, H, 3).astype(np.float32)
    params = U.init_params(L, root, True, seed=52, bias_scale=0.02)
    masks = {}
    for ks in ("1", "0"):
        monkeypatch.setenv("RSU_KSPLIT", ks)
        m = ConvolutionalModel(Options(num_layers=L, root_size=root, patch_size=P, stride=stride, dilated_layers=True, batch_size=4,
                                       ensemble_prediction=True, dropout=1.0, logdir=None), params=params)
        masks[ks] = m.predict(img)
        del m
        torch.cuda.empty_cache()
    d = np.abs(masks["1"] - masks["0"])
    assert np.isfinite(masks["1"]).all() and d.max() <= 2e-3 and d.mean() <= 1e-4, (float(d.max()), float(d.mean()))
