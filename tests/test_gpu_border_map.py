"""The border-distance weight map on the GPU (include/rsu.h rsu_border_map): the kernel against the brute-force definition of
tests/border_util.py and, bit for bit, against hostio.border_weight_map; its argument checks; the net, evaluate() and train() with
--border_weight against the same map handed in by the caller."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import unet_oracle as U
from road_segmentation_unet_amd import hostio, pool
from road_segmentation_unet_amd._lib import call, lib
from tests import border_util as bu
from tests import head_util as hd
from tests import hiputil as hu

pytestmark = pytest.mark.gpu
W0, SIGMA = 10.0, 5.0
NAMES = sorted(bu.case_tiles(4, 4))


def _run(labels, mul=None, w0=W0, sigma=SIGMA, want_d2=True):
    """one rsu_border_map call on fresh buffers: (out float32, d2 int32 or None) as numpy"""
    N, H, W = labels.shape
    lab = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int64)).to(hu.DEV)
    m = None if mul is None else torch.from_numpy(np.ascontiguousarray(mul, dtype=np.float32)).to(hu.DEV)
    out = torch.full((N, H, W), -7.0, dtype=torch.float32, device=hu.DEV)
    d2 = torch.full((N, H, W), -7, dtype=torch.int32, device=hu.DEV) if want_d2 else None
    ws = torch.zeros(int(lib().rsu_border_map_ws_bytes(N, H, W)) // 4, dtype=torch.int32, device=hu.DEV)
    call("rsu_border_map", hu.ptr(lab), hu.ptr(m), hu.ptr(out), hu.ptr(d2), hu.ptr(ws), N, H, W, w0, sigma, hu.stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if d2 is None else d2.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(H, W, name):
    """(labels tile, brute-force d2) of one case, computed once per session (the 388 px tiles take seconds each)"""
    tile = bu.case_tiles(H, W)[name]
    return tile, bu.brute_d2(tile)


def _check(labels, rd2, mul, w0, sigma, what):
    """d2 exact against the brute force; out within the derived bound of float64 AND bit-equal to the host mirror; d2 == NULL and a
    second run give the same bits"""
    out, d2 = _run(labels, mul, w0, sigma)
    assert np.array_equal(d2, rd2), what
    valid = (labels == 0) | (labels == 1)
    finite = rd2 < bu.D2_INF
    s = float(np.float32(sigma))
    border = np.where(finite, 1.0 + float(np.float32(w0)) * np.exp(-np.where(finite, rd2, 0).astype(np.float64) / (2.0 * s * s)), 1.0)
    ref = np.where(valid, (1.0 if mul is None else np.where(valid, mul.astype(np.float64), 1.0)) * border, 0.0)
    err = float(np.abs(out.astype(np.float64) - ref).max())
    hout, hd2 = hostio.border_weight_map(labels, w0, sigma, mul=mul)
    differ = int((out.view(np.int32) != hout.view(np.int32)).sum())
    print("%s: max |out - float64| %.3e (bound %.3e); %d of %d values differ from the host mirror's bits"
          % (what, err, bu.tolerance(w0, mul), differ, out.size))
    assert err <= bu.tolerance(w0, mul), what
    assert np.array_equal(hd2, rd2), what
    assert differ == 0, what
    assert not np.any(out[~valid]) and not np.any(np.signbit(out[~valid])) and np.all(d2[~valid] == bu.D2_INF), what   # ignored: +0, INF
    out_nod2, none = _run(labels, mul, w0, sigma, want_d2=False)
    assert none is None and np.array_equal(out_nod2.view(np.int32), out.view(np.int32)), what
    out2, d2b = _run(labels, mul, w0, sigma)
    assert np.array_equal(out2.view(np.int32), out.view(np.int32)) and np.array_equal(d2b, d2), what


@pytest.mark.parametrize("with_mul", [False, True])
@pytest.mark.parametrize("H,W", [(20, 20), (37, 41), (132, 132)])
def test_border_map_against_the_definition(H, W, with_mul):
    """every case, as batches of 1 and of 4 (a case's map must not depend on its neighbours in the batch)"""
    refs = [_reference(H, W, n) for n in NAMES]
    rng = np.random.RandomState(H * W + with_mul)
    for w0, sigma in ((W0, SIGMA), (3.5, 1.25)):
        for i in range(0, len(NAMES), 4):
            group = list(range(i, min(i + 4, len(NAMES))))
            group += group[:4 - len(group)] if len(group) < 4 and len(group) != 1 else []
            labels = np.stack([refs[j][0] for j in group])
            rd2 = np.stack([refs[j][1] for j in group])
            mul = bu.mul_map(rng, labels) if with_mul else None
            _check(labels, rd2, mul, w0, sigma, "%dx%d batch %d %s" % (H, W, len(group), [NAMES[j] for j in group]))
        for j in range(len(NAMES)):
            labels, rd2 = refs[j][0][None], refs[j][1][None]
            _check(labels, rd2, bu.mul_map(rng, labels) if with_mul else None, w0, sigma, "%dx%d batch 1 %s" % (H, W, NAMES[j]))


def test_border_map_at_388():
    """the flagship patch size: a batch of 4 different cases (with a caller map) and batches of 1, against the brute force"""
    H = W = 388
    rng = np.random.RandomState(388)
    batch = ["straight_ignored", "single", "sparse", "all0"]
    labels = np.stack([_reference(H, W, n)[0] for n in batch])
    rd2 = np.stack([_reference(H, W, n)[1] for n in batch])
    _check(labels, rd2, bu.mul_map(rng, labels), W0, SIGMA, "388 batch 4 %s" % batch)
    _check(labels, rd2, None, W0, SIGMA, "388 batch 4 %s no mul" % batch)
    for n in ("diagonal", "only_ignored_other", "all1"):
        tile, d2 = _reference(H, W, n)
        _check(tile[None], d2[None], None, W0, SIGMA, "388 batch 1 %s" % n)


def test_border_map_refuses_bad_arguments_and_touches_nothing():
    N, H, W = 2, 20, 20
    lab = torch.zeros((N, H, W), dtype=torch.int64, device=hu.DEV)
    lab[:, 5] = 1
    out = torch.full((N, H, W), -7.0, dtype=torch.float32, device=hu.DEV)
    d2 = torch.full((N, H, W), -7, dtype=torch.int32, device=hu.DEV)
    ws = torch.full((N * H * W,), -7, dtype=torch.int32, device=hu.DEV)
    ok = dict(labels=hu.ptr(lab), mul=None, out=hu.ptr(out), d2=hu.ptr(d2), ws=hu.ptr(ws), N=N, H=H, W=W, w0=W0, sigma=SIGMA)
    nan, inf = float("nan"), float("inf")
    for b in (dict(labels=None), dict(out=None), dict(ws=None), dict(N=0), dict(H=0), dict(W=0), dict(N=-1), dict(H=-1), dict(W=-1),
              dict(H=1025), dict(W=1025), dict(w0=-0.5), dict(w0=nan), dict(w0=inf), dict(w0=-inf), dict(sigma=0.0), dict(sigma=-1.0),
              dict(sigma=nan), dict(sigma=inf)):
        a = dict(ok, **b)
        rc = lib().rsu_border_map(a["labels"], a["mul"], a["out"], a["d2"], a["ws"], a["N"], a["H"], a["W"], a["w0"], a["sigma"], hu.stream())
        assert rc == hd.RSU_EINVAL, (b, rc)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((d2 == -7).all()) and bool((ws == -7).all())
    call("rsu_border_map", *[ok[k] for k in ("labels", "mul", "out", "d2", "ws", "N", "H", "W", "w0", "sigma")], hu.stream())   # and the good call runs
    torch.cuda.synchronize()
    assert bool((out >= 1.0).all()) and int(d2.min()) == 1


# ------------------------------------------------------------------------------------------- the network
def _abi_map(m, mul=None, w0=W0, sigma=SIGMA):
    """the map of m.labels by the ABI call, on buffers of the test's own"""
    out = torch.zeros((m.B, m.P, m.P), dtype=torch.float32, device=hu.DEV)
    ws = torch.zeros(int(lib().rsu_border_map_ws_bytes(m.B, m.P, m.P)) // 4, dtype=torch.int32, device=hu.DEV)
    call("rsu_border_map", hu.ptr(m.labels), hu.ptr(mul), hu.ptr(out), None, hu.ptr(ws), m.B, m.P, m.P, w0, sigma, hu.stream())
    torch.cuda.synchronize()
    return out


def _same_step(a, b):
    for x, y, what in zip(a, b, ("gradients", "prob", "loss_sum", "weight_sum", "dice_sums")):
        assert torch.equal(hd._bits(x), hd._bits(y)), what


@pytest.mark.parametrize("caller_map", [False, True])
@pytest.mark.parametrize("dice", [0.0, hd.LAM])
@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
@pytest.mark.parametrize("L,root,dilated,P", hd.NETS)
def test_net_step_equals_a_step_on_the_same_map_handed_in(L, root, dilated, P, optimizer, dice, caller_map):
    """a step with border_weight = 10 gives the bits of a step on an identical net without it whose map was computed by the ABI call and
    set through set_pixel_weights -- every gradient, prob, loss_sum, weight_sum, dice_sums; with a caller map on both sides: the mul path"""
    kw = dict(optimizer=optimizer, dice_weight=dice, class_weights=(0.5, 2.0))
    a = hd._net(L, root, dilated, P, border_weight=W0, border_sigma=SIGMA, **kw)
    b = hd._net(L, root, dilated, P, **kw)
    assert a.loss_is_weighted() and a.border_map is not None and tuple(a.border_map.shape) == (a.B, P, P) and b.border_map is None
    for m in (a, b):
        hd._batch(m)
        m.labels[0, :3, :] = -1            # ignored pixels
        m.labels[1, 7, 2] = 2 ** 32 + 1
    mul = None
    if caller_map:
        mul = hu.dev_f32(hd._weight_map(np.random.RandomState(4), a.B * P * P).reshape(a.B, P, P))
        a.set_pixel_weights(mul)
    b.set_pixel_weights(_abi_map(b, mul))
    ra, rb = hd._step(a), hd._step(b)
    _same_step(ra, rb)
    assert torch.equal(hd._bits(a.border_map), hd._bits(b.pixel_weights))
    assert float(ra[3]) > 0.0 and (a.pixel_weights is None) == (not caller_map)
    if optimizer == "adam":
        a.apply_adam(0.01), b.apply_adam(0.01)
    else:
        a.apply_momentum(0.01, 0.9), b.apply_momentum(0.01, 0.9)
    torch.cuda.synchronize()
    assert torch.equal(hd._bits(a.flat_w), hd._bits(b.flat_w))
    # the map follows the labels: new labels, a new map, with nothing set by the caller
    for m in (a, b):
        hd._batch(m, seed=9)
    b.set_pixel_weights(_abi_map(b, mul))
    _same_step(hd._step(a), hd._step(b))


@pytest.mark.parametrize("L,root,dilated,P", hd.NETS)
def test_border_weight_zero_is_the_net_without_it(L, root, dilated, P):
    a = hd._net(L, root, dilated, P, border_weight=0.0)
    b = hd._net(L, root, dilated, P)
    assert a.border_map is None and not a.loss_is_weighted() and not hasattr(a, "_border_ws")
    for m in (a, b):
        hd._batch(m)
    _same_step(hd._step(a), hd._step(b))
    from road_segmentation_unet_amd._lib import RsuError
    from road_segmentation_unet_amd.unet import UNet
    for bad in (dict(border_weight=-1.0), dict(border_weight=float("nan")), dict(border_sigma=0.0), dict(border_sigma=float("inf"))):
        with pytest.raises(RsuError):
            hd._net(L, root, dilated, P, **bad)
    with pytest.raises(RsuError):
        UNet(L, root, dilated, 2, P, training=False, border_weight=1.0)


def test_tune_and_ensure_tuned_keep_working():
    L, root, dilated, P = hd.NETS[0]
    a = hd._net(L, root, dilated, P, border_weight=W0)
    hd._batch(a)
    x0, l0 = a.x.clone(), a.labels.clone()
    a.ensure_tuned(keep=1.0)
    a.ensure_tuned(training=False, keep=1.0)
    assert torch.equal(a.x, x0) and torch.equal(a.labels, l0)
    r1 = hd._step(a)
    a.tune()
    _same_step(r1, hd._step(a))


# ------------------------------------------------------------------------------------------- the model
def _patches(n, seed=21, p_road=0.3, P=20, L=3):
    S = U.input_size_needed(P, L)
    rng = np.random.RandomState(seed)
    return rng.rand(n, S, S, 3).astype(np.float32), (rng.rand(n, P, P) < p_road).astype(np.int64)


@pytest.mark.parametrize("caller_map", [False, True])
def test_model_evaluate_equals_evaluate_on_the_host_map(caller_map):
    """evaluate() of a model with border_weight > 0 has the sums and the histogram of evaluate(weights = the host mirror's map) on a model
    without it, bit for bit -- on a set whose size is not a multiple of the batch: the padded tiles (labels -1) contribute exactly nothing"""
    N = 5
    X, y = _patches(N)
    y[1, :4] = -1
    a = hd._model(class_weights=(0.5, 2.0), dice_weight=0.7, border_weight=W0, border_sigma=SIGMA)
    b = hd._model(class_weights=(0.5, 2.0), dice_weight=0.7)
    assert N % a.local_batch != 0
    wmap = (0.25 + np.random.RandomState(8).rand(N, 20, 20)).astype(np.float32) if caller_map else None
    host_map, _ = hostio.border_weight_map(y, W0, SIGMA, mul=wmap)
    va, vb = a.evaluate(X, y, weights=wmap), b.evaluate(X, y, weights=host_map)
    assert np.array_equal(va["hist"], vb["hist"]) and int(va["hist"].sum()) == N * 400 - 80
    assert np.array_equal(va["sums"], vb["sums"]), (va["sums"], vb["sums"])
    assert va["sums"][1] > (N * 400 - 80) * 0.5 and va["n_pixels"] == N * 400
    for k in ("loss", "objective", "dice", "f1"):
        assert va[k] == vb[k], k
    assert a.net.pixel_weights is None and b.net.pixel_weights is None      # evaluate() leaves the caller's map as it was: none


def test_train_step_with_border_weight_equals_the_host_map_step():
    a = hd._model(border_weight=W0, border_sigma=SIGMA)
    b = hd._model()
    X, y = _patches(2, seed=3)
    la, pa = a.train_step(X, y)
    lb, pb = b.train_step(X, y, weights=hostio.border_weight_map(y, W0, SIGMA)[0])
    torch.cuda.synchronize()
    assert torch.equal(hd._bits(la), hd._bits(lb)) and torch.equal(hd._bits(pa), hd._bits(pb))
    assert torch.equal(hd._bits(a.net.flat_w), hd._bits(b.net.flat_w))
    assert torch.equal(hd._bits(a.net.weight_sum), hd._bits(b.net.weight_sum)) and float(a.net.weight_sum) > 2 * 400


def test_train_with_d4_augmentation_and_border_weight():
    """the end-to-end smoke of the flag: cli.parse_options -> ConvolutionalModel -> train() over a DevicePatchPool with --d4_augmentation;
    the map is computed from the augmented labels in net.labels, and the weights it sums exceed the pixel count"""
    from road_segmentation_unet_amd.cli import parse_options
    from road_segmentation_unet_amd.model import ConvolutionalModel
    L, root, P, B, stride = 2, 16, 12, 3, 8
    S = U.input_size_needed(P, L)
    rng = np.random.RandomState(5)
    off = (S - P) // 2
    ext = rng.rand(2, S + 2 * stride, S + 2 * stride, 3)
    lab = (ext[:, off:-off, off:-off, 1] > 0.5) * 1.0
    opts = parse_options(["--num_layers=%d" % L, "--root_size=%d" % root, "--patch_size=%d" % P, "--batch_size=%d" % B, "--dropout=0.8",
                          "--lr=0.01", "--seed=9", "--d4_augmentation", "--border_weight=10", "--border_sigma=2"])
    opts.logdir = None
    m = ConvolutionalModel(opts)
    assert m.net.border_weight == 10.0 and m.net.border_sigma == 2.0
    np.random.seed(123)
    st = m.train(pool.DevicePatchPool(ext, lab, S, P, stride, device=m.net.device, augment=True, seed=opts.seed), None, None, None)
    torch.cuda.synchronize()
    assert st["patches"] > 0 and np.isfinite(st["loss"]) and st["loss"] > 0
    wsum = float(m.net.weight_sum)
    print("train(): loss %.5f, last batch's weight sum %.1f over %d pixels" % (st["loss"], wsum, B * P * P))
    assert wsum > B * P * P
    # the last batch's map is the host mirror's map of the (augmented) labels still in net.labels
    host_map, _ = hostio.border_weight_map(m.net.labels.cpu().numpy(), 10.0, 2.0)
    assert np.array_equal(m.net.border_map.cpu().numpy().view(np.int32), host_map.view(np.int32))
