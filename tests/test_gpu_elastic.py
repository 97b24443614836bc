"""Elastic deformation in the one-launch batch loader on the GPU (include/rsu.h rsu_elastic_patches): the kernel bit for bit against
hostio.elastic_patches at the smallest shapes at which it can go wrong, against rsu_affine_patches at alpha = 0, the registration of
labels and image without any host restatement, its argument checks, DevicePatchPool's elastic path, and one training epoch with
--elastic_deformation."""
import ctypes

import numpy as np
import pytest
import torch

from road_segmentation_unet_amd import _lib, hostio, pool
from road_segmentation_unet_amd._lib import call, lib
from tests import affine_util as au
from tests import elastic_util as eu
from tests import hiputil as hu

pytestmark = pytest.mark.gpu
SENTINEL = -7


def _run(ext, lab, recs, S, P, entry="rsu_elastic_patches"):
    """one call of the loader on fresh, sentinel-filled buffers: (x float32, labels int64) as numpy"""
    img, lb = hu.dev_f32(ext), torch.from_numpy(np.ascontiguousarray(lab, dtype=np.uint8)).to(hu.DEV)
    n = len(recs)
    x = torch.full((n, S, S, 3), float(SENTINEL), dtype=torch.float32, device=hu.DEV)
    y = torch.full((n, P, P), SENTINEL, dtype=torch.int64, device=hu.DEV)
    recs = np.ascontiguousarray(recs)
    typ = _lib.RsuElastic if entry == "rsu_elastic_patches" else _lib.RsuAffine
    call(entry, hu.ptr(img), hu.ptr(lb), recs.ctypes.data_as(ctypes.POINTER(typ)), n, ext.shape[0], ext.shape[1], lab.shape[1], S, P,
         hu.ptr(x), hu.ptr(y), hu.stream())
    torch.cuda.synchronize()
    return x.cpu().numpy(), y.cpu().numpy()


def _affine_of(recs):
    out = np.zeros(len(recs), dtype=hostio.AFFINE_DTYPE)
    for name in ("image", "cy", "cx", "m00", "m01", "m10", "m11"):
        out[name] = recs[name]
    return out


@pytest.mark.parametrize("Hl,offset,S,P", eu.GEOMS)
def test_kernel_equals_the_host_mirror_bit_for_bit(Hl, offset, S, P):
    ext, lab, recs, hx, hy = eu.case(Hl, offset, S, P)
    N = len(recs)
    assert N == 459 and float(ext.min()) > 0.0                  # positive data: -0.0 never arises
    assert (S * S + 255) // 256 == (2 if S == 20 else 1)         # (28, 4, 20, 12): a full and a ragged workgroup per window
    # the whole bank: 15 launches, the last one of 11 records
    X, Y = _run(ext, lab, recs, S, P)
    assert not np.any(X == SENTINEL) and not np.any(Y == SENTINEL)                        # every element overwritten
    differ = int((X.view(np.int32) != hx.view(np.int32)).sum())
    print("all %d records: %d of %d values differ from the host mirror's bits, %d of %d labels" % (N, differ, X.size, int((Y != hy).sum()), Y.size))
    assert differ == 0 and np.array_equal(Y, hy)
    X2, Y2 = _run(ext, lab, recs, S, P)                                                   # a second run: the same bits
    assert np.array_equal(X2.view(np.int32), X.view(np.int32)) and np.array_equal(Y2, Y)
    # nrec = 1, 4, 33 (crosses the 32-record slice once), at several places of the bank
    for lo, hi in ((0, 1), (N - 1, N), (1, 5), (200, 204), (5, 38), (N - 33, N)):
        x, y = _run(ext, lab, recs[lo:hi], S, P)
        what = "records [%d, %d)" % (lo, hi)
        assert not np.any(x == SENTINEL) and not np.any(y == SENTINEL), what
        assert np.array_equal(x.view(np.int32), hx[lo:hi].view(np.int32)) and np.array_equal(y, hy[lo:hi]), what
    for k in range(N):                                                                    # each sample equals itself run alone
        x, y = _run(ext, lab, recs[k:k + 1], S, P)
        assert np.array_equal(x[0].view(np.int32), X[k].view(np.int32)) and np.array_equal(y[0], Y[k]), k
    assert 0 < int(hy.sum()) < hy.size


@pytest.mark.parametrize("Hl,offset,S,P", eu.GEOMS)
def test_alpha_zero_is_the_affine_loader_and_alpha_above_zero_is_not(Hl, offset, S, P):
    ext, lab, recs, _, _ = eu.case(Hl, offset, S, P)
    X, Y = _run(ext, lab, recs, S, P)
    AX, AY = _run(ext, lab, _affine_of(recs), S, P, entry="rsu_affine_patches")
    zero = recs["alpha"] == 0
    assert int(zero.sum()) == 153 and int((~zero).sum()) == 306
    assert np.array_equal(X[zero].view(np.int32), AX[zero].view(np.int32)) and np.array_equal(Y[zero], AY[zero])
    for k in np.flatnonzero(~zero):
        assert not np.array_equal(X[k], AX[k]), (k, recs[k])


@pytest.mark.parametrize("Hl,offset,S,P", eu.GEOMS)
def test_labels_stay_registered_with_the_image(Hl, offset, S, P):
    """no host restatement involved: channel 0 of the image IS the label mask (0.0 / 1.0), so the centre crop of the deformed input
    window, thresholded, must be the deformed label patch exactly -- labels and image see the same field"""
    _, lab, recs, _, _ = eu.case(Hl, offset, S, P)
    rng = np.random.RandomState(4)
    orig = (0.05 + rng.rand(eu.NIMG, Hl, Hl, 3)).astype(np.float32)
    orig[..., 0] = lab
    ext = hostio.mirror_border(orig, offset).astype(np.float32)
    X, Y = _run(ext, lab, recs, S, P)
    crop = (X[:, offset:offset + P, offset:offset + P, 0] >= np.float32(0.5)).astype(np.int64)
    bad = [k for k in range(len(recs)) if not np.array_equal(crop[k], Y[k])]
    print("%d of %d records: label patch != thresholded centre crop of channel 0" % (len(bad), len(recs)))
    assert not bad, bad[:10]
    assert set(np.unique(Y)) == {0, 1}
    moved = recs["alpha"] == 4
    AY = _run(ext, lab, _affine_of(recs), S, P, entry="rsu_affine_patches")[1]
    assert int((Y[moved] != AY[moved]).sum()) > 0                                         # and the field does move labels


def test_kernel_refuses_bad_arguments_and_touches_nothing():
    Hl, offset, S, P = eu.GEOMS[0]
    ext, lab, recs, hx, hy = eu.case(Hl, offset, S, P)
    img, lb = hu.dev_f32(ext), torch.from_numpy(lab).to(hu.DEV)
    x = torch.full((2, S, S, 3), float(SENTINEL), dtype=torch.float32, device=hu.DEV)
    y = torch.full((2, P, P), SENTINEL, dtype=torch.int64, device=hu.DEV)
    ok = dict(images=hu.ptr(img), labels=hu.ptr(lb), x_out=hu.ptr(x), labels_out=hu.ptr(y), recs=[au.rec(0, 9.5, 9.5, np.eye(2)) + (2.0, 5, 3)],
              nimg=eu.NIMG, He=Hl + 2 * offset, Hl=Hl, S=S, P=P, stream=hu.stream())
    for name, b in eu.abi_cases():
        assert eu.abi_call(lib(), dict(ok, **b)) == -22, name
    torch.cuda.synchronize()
    assert bool((x == SENTINEL).all()) and bool((y == SENTINEL).all())
    assert recs["alpha"][4] > 0 and recs["alpha"][5] > 0
    assert eu.abi_call(lib(), dict(ok, recs=recs[4:6])) == 0                              # and the good call runs
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy().view(np.int32), hx[4:6].view(np.int32)) and np.array_equal(y.cpu().numpy(), hy[4:6])


# ------------------------------------------------------------------------------------------- the pool
def _pool(ext, lab, S, P, **kw):
    return pool.DevicePatchPool(ext, lab, S, P, eu.STRIDE[S], device=hu.DEV, **kw)


def _batches(pl, B, count=3, seed=3):
    """`count` consecutive batches of B patches: [(x, labels, what load_batch returned)]"""
    order = np.random.RandomState(seed).permutation(len(pl))
    out = []
    for i in range(count):
        x = torch.full((B, pl.S, pl.S, 3), float(SENTINEL), dtype=torch.float32, device=hu.DEV)
        y = torch.full((B, pl.P, pl.P), SENTINEL, dtype=torch.int64, device=hu.DEV)
        ret = pl.load_batch([int(k) for k in order[i * B:(i + 1) * B]], x, y)
        torch.cuda.synchronize()
        out.append((x.cpu().numpy(), y.cpu().numpy(), ret))
    return out


@pytest.mark.parametrize("Hl,offset,S,P", [eu.GEOMS[0], eu.GEOMS[2]])
def test_elastic_pool(Hl, offset, S, P):
    ext, lab = au.make_images(eu.NIMG, Hl, offset, seed=10)
    kw = dict(augment=True, rotation=180.0, scale=(0.8, 1.25))
    a, b, c = (_batches(_pool(ext, lab, S, P, seed=s, elastic=(4, 3), **kw), 3) for s in (21, 21, 22))
    plain = _batches(_pool(ext, lab, S, P, seed=21, **kw), 3)
    seen = []
    for (xa, ya, ra), (xb, yb, rb), (xc, yc, rc), (xp, yp, rp) in zip(a, b, c, plain):
        assert ra.dtype == hostio.ELASTIC_DTYPE and len(ra) == 3 and rp.dtype == hostio.AFFINE_DTYPE
        assert np.array_equal(xa.view(np.int32), xb.view(np.int32)) and np.array_equal(ya, yb) and np.array_equal(ra, rb)   # repeats by seed
        assert not np.array_equal(xa, xc) and not np.array_equal(ra["key"], rc["key"])                                     # differs by seed
        assert set(np.unique(ya)) <= {0, 1} and not np.any(xa == SENTINEL) and not np.any(ya == SENTINEL)
        hx, hy = hostio.elastic_patches(ext, lab, ra, S, P)                                                                 # it is the mirror's batch
        assert np.array_equal(xa.view(np.int32), hx.view(np.int32)) and np.array_equal(ya, hy)
        for name in hostio.AFFINE_DTYPE.names[:7]:                               # the geometric stream did not move: the pool without
            assert np.array_equal(ra[name], rp[name]), name                      # `elastic` draws the same patches and matrices
        assert not np.array_equal(xa, xp)
        assert (ra["alpha"] == np.float32(4.0)).all() and (ra["grid"] == 3).all()
        seen += ra["key"].tolist()
    assert len(set(seen)) == 9
    want = pool.elastic_draw(np.random.RandomState((21 + 0xbb67ae85) % 2 ** 32), 9, 4.0, 3)   # the documented generator
    assert seen == want.tolist()
    for bad in ((-1.0, 3), (1.0, 0), (1.0, 17), (65.0, 3), (1.0, 2.5)):
        with pytest.raises(ValueError):
            _pool(ext, lab, S, P, elastic=bad)


def test_pool_issues_one_elastic_launch_per_batch_and_none_with_alpha_zero(monkeypatch):
    Hl, offset, S, P = eu.GEOMS[0]
    ext, lab = au.make_images(eu.NIMG, Hl, offset, seed=9)
    calls = []
    real = _lib.call

    def recorder(name, *args):
        calls.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", recorder)
    on = _pool(ext, lab, S, P, seed=11, elastic=(2.0, 3))                       # alpha > 0 alone turns the one-launch loader on
    assert on.one_launch and on.elastic_on and on.elastic == (2.0, 3)
    res = _batches(on, 4, count=2)
    assert [c[0] for c in calls] == ["rsu_elastic_patches", "rsu_elastic_patches"] and all(r.dtype == hostio.ELASTIC_DTYPE for _, _, r in res)
    del calls[:]
    off = _pool(ext, lab, S, P, seed=11, one_launch=True, elastic=(0.0, 5))
    assert off.one_launch and not off.elastic_on and not hasattr(off, "_elastic_rng")
    (xo, yo, ro), = _batches(off, 4, count=1)
    assert [c[0] for c in calls] == ["rsu_affine_patches"] and ro.dtype == hostio.AFFINE_DTYPE
    del calls[:]
    default = _pool(ext, lab, S, P, seed=11)                                    # the default pool: the loop, no launch of the library
    assert not default.one_launch and not default.elastic_on
    (xd, yd, rd), = _batches(default, 4, count=1)
    assert calls == [] and rd is None
    assert np.array_equal(xd.view(np.int32), xo.view(np.int32)) and np.array_equal(yd, yo)


# ------------------------------------------------------------------------------------------- the model
def test_train_with_elastic_deformation():
    """cli.parse_options -> ConvolutionalModel -> one epoch of train() over a DevicePatchPool built as cli.main builds it: the network and
    the requirements of tests/test_gpu_affine.py test_train_with_random_rotation_scale_and_d4"""
    from oracle import unet_oracle as U
    from road_segmentation_unet_amd.cli import parse_options
    from road_segmentation_unet_amd.model import ConvolutionalModel
    L, root, P, B, stride = 2, 16, 16, 4, 16
    S = U.input_size_needed(P, L)
    off = (S - P) // 2
    rng = np.random.RandomState(5)
    orig = rng.rand(2, P + 2 * stride, P + 2 * stride, 3)
    ext, lab = hostio.mirror_border(orig, off), (orig[..., 1] > 0.5) * 1.0
    argv = ["--num_layers=%d" % L, "--root_size=%d" % root, "--patch_size=%d" % P, "--stride=%d" % stride, "--batch_size=%d" % B, "--lr=0.01",
            "--seed=9", "--elastic_deformation=2,3", "--random_rotation=30", "--random_scale=0.8,1.25", "--d4_augmentation"]
    with pytest.raises(ValueError, match="nodevice_patch_pool"):
        parse_options(argv + ["--nodevice_patch_pool"])
    opts = parse_options(argv)
    opts.logdir = None
    m = ConvolutionalModel(opts)
    pl = pool.DevicePatchPool(ext, lab, S, P, stride, device=m.net.device, augment=opts.d4_augmentation, seed=opts.seed,
                              rotation=opts.random_rotation, scale=opts.random_scale, one_launch=opts.one_launch_loader,
                              jitter=opts.color_jitter, noise=opts.random_noise, elastic=opts.elastic_deformation)
    assert pl.one_launch and pl.elastic_on and pl.elastic == (2.0, 3) and len(pl) == 18
    np.random.seed(123)
    st = m.train(pl, None, None, None)
    torch.cuda.synchronize()
    print("train(): loss %.5f over %d patches" % (st["loss"], st["patches"]))
    assert np.isfinite(st["loss"]) and st["loss"] > 0
    assert st["patches"] == len(range(0, len(pl) - B, B)) * B == 16
    assert set(np.unique(m.net.labels.cpu().numpy())) <= {0, 1}
