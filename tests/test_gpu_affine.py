"""The one-launch batch loader on the GPU (include/rsu.h rsu_affine_patches): the kernel bit for bit against hostio.affine_patches at the
smallest shapes at which it can go wrong, its argument checks, DevicePatchPool's one-launch path against the loop it can replace, and one
training epoch with --random_rotation, --random_scale and --d4_augmentation."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from road_segmentation_unet_amd import _lib, hostio, pool
from road_segmentation_unet_amd._lib import call, lib
from tests import affine_util as au
from tests import hiputil as hu

pytestmark = pytest.mark.gpu
NIMG = 3
SENTINEL = -7


@functools.lru_cache(maxsize=None)
def _case(Hl, offset, S, P):
    """per geometry, computed once and left unchanged: the images, the bank of records and the host mirror's outputs for the whole bank.
    Bank: the identity, the 32 D4 draws' matrices, the dyadic matrices, seeded rotations with zooms from 0.25 (more than one reflection
    period) to 3, and windows centred on the four corners of the image (rotated, zoomed out: taps on both sides of both edges)."""
    ext, lab = au.make_images(NIMG, Hl, offset, seed=7)
    c = offset + (Hl - 1) / 2.0
    I = np.eye(2)
    bank = [au.rec(0, offset + (S - 1) / 2.0, offset + (S - 1) / 2.0 + 1.0, I)]
    bank += [au.rec(k % NIMG, c, c + (k % 3) - 1.0, pool.d4_matrix(op)) for k, op in enumerate(au.D4_OPS)]
    bank += [au.rec(1, c + 0.25, c - 0.75, M) for M in au.DYADIC]
    bank += au.rotation_records(np.random.RandomState(17), 12, NIMG, Hl, offset)
    th = math.radians(33.0)
    R = 0.7 * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    bank += [au.rec(k % NIMG, offset + cy, offset + cx, R if k % 2 else I)
             for k, (cy, cx) in enumerate([(-0.5, -0.5), (-0.5, Hl - 0.5), (Hl - 0.5, -0.5), (Hl - 0.5, Hl - 0.5)])]
    recs = hostio.affine_records(bank)
    hx, hy = hostio.affine_patches(ext, lab, recs, S, P)
    hx.setflags(write=False), hy.setflags(write=False)
    return ext, lab, recs, hx, hy


def _run(ext, lab, recs, S, P):
    """one rsu_affine_patches call on fresh, sentinel-filled buffers: (x float32, labels int64) as numpy"""
    img, lb = hu.dev_f32(ext), torch.from_numpy(np.ascontiguousarray(lab, dtype=np.uint8)).to(hu.DEV)
    n = len(recs)
    x = torch.full((n, S, S, 3), float(SENTINEL), dtype=torch.float32, device=hu.DEV)
    y = torch.full((n, P, P), SENTINEL, dtype=torch.int64, device=hu.DEV)
    recs = np.ascontiguousarray(recs)
    call("rsu_affine_patches", hu.ptr(img), hu.ptr(lb), recs.ctypes.data_as(ctypes.POINTER(_lib.RsuAffine)), n, ext.shape[0], ext.shape[1],
         lab.shape[1], S, P, hu.ptr(x), hu.ptr(y), hu.stream())
    torch.cuda.synchronize()
    return x.cpu().numpy(), y.cpu().numpy()


@pytest.mark.parametrize("Hl,offset,S,P", au.GEOMS)
def test_kernel_equals_the_host_mirror_bit_for_bit(Hl, offset, S, P):
    ext, lab, recs, hx, hy = _case(Hl, offset, S, P)
    assert len(recs) == 51 and float(ext.min()) > 0.0            # positive data: -0.0 never arises
    singles = [_run(ext, lab, recs[k:k + 1], S, P) for k in range(len(recs))]
    # nrec = 1, 4, 33 (crosses the 32-record slice once) and the whole bank (51)
    for lo, hi in ((0, 1), (1, 5), (5, 38), (18, 51), (0, 51)):
        x, y = _run(ext, lab, recs[lo:hi], S, P)
        what = "records [%d, %d)" % (lo, hi)
        assert not np.any(x == SENTINEL) and not np.any(y == SENTINEL), what            # every element overwritten
        differ = int((x.view(np.int32) != hx[lo:hi].view(np.int32)).sum())
        print("%s: %d of %d values differ from the host mirror's bits, %d of %d labels" % (what, differ, x.size, int((y != hy[lo:hi]).sum()), y.size))
        assert differ == 0 and np.array_equal(y, hy[lo:hi]), what
        for k in range(lo, hi):                                                          # each sample equals the same sample run alone
            assert np.array_equal(x[k - lo].view(np.int32), singles[k][0][0].view(np.int32)) and np.array_equal(y[k - lo], singles[k][1][0]), (what, k)
        x2, y2 = _run(ext, lab, recs[lo:hi], S, P)                                       # a second run: the same bits
        assert np.array_equal(x2.view(np.int32), x.view(np.int32)) and np.array_equal(y2, y), what
    assert 0 < int(hy.sum()) < hy.size


def test_kernel_refuses_bad_arguments_and_touches_nothing():
    Hl, offset, S, P = au.GEOMS[0]
    ext, lab, recs, hx, hy = _case(Hl, offset, S, P)
    img, lb = hu.dev_f32(ext), torch.from_numpy(lab).to(hu.DEV)
    x = torch.full((2, S, S, 3), float(SENTINEL), dtype=torch.float32, device=hu.DEV)
    y = torch.full((2, P, P), SENTINEL, dtype=torch.int64, device=hu.DEV)
    ok = dict(images=hu.ptr(img), labels=hu.ptr(lb), x_out=hu.ptr(x), labels_out=hu.ptr(y), recs=[au.rec(0, 9.5, 9.5, np.eye(2))], nimg=NIMG,
              He=Hl + 2 * offset, Hl=Hl, S=S, P=P, stream=hu.stream())
    for name, b in au.abi_cases():
        assert au.abi_call(lib(), dict(ok, **b)) == -22, name
    torch.cuda.synchronize()
    assert bool((x == SENTINEL).all()) and bool((y == SENTINEL).all())
    assert au.abi_call(lib(), dict(ok, recs=recs[:2])) == 0                              # and the good call runs
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy().view(np.int32), hx[:2].view(np.int32)) and np.array_equal(y.cpu().numpy(), hy[:2])


# ------------------------------------------------------------------------------------------- the pool
def _pool(ext, lab, S, P, **kw):
    return pool.DevicePatchPool(ext, lab, S, P, au.STRIDE[S], device=hu.DEV, **kw)


def _batches(pl, B, count=5, seed=3):
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


@pytest.mark.parametrize("augment", [True, False])
@pytest.mark.parametrize("Hl,offset,S,P", au.GEOMS)
def test_one_launch_pool_delivers_the_loops_bits(Hl, offset, S, P, augment):
    """the same seed: a one_launch pool (D4, or plain) and the loop pool deliver bit-equal inputs and equal labels over five batches
    (the images are extended by their own mirror, as the pool's unrotated images are)"""
    ext, lab = au.make_images(NIMG, Hl, offset, seed=9)
    loop = _pool(ext, lab, S, P, augment=augment, seed=11)
    one = _pool(ext, lab, S, P, augment=augment, seed=11, one_launch=True)
    assert not loop.one_launch and one.one_launch
    for (xa, ya, ops), (xb, yb, recs) in zip(_batches(loop, 4), _batches(one, 4)):
        assert np.array_equal(xa.view(np.int32), xb.view(np.int32)) and np.array_equal(ya, yb)
        assert recs.dtype == hostio.AFFINE_DTYPE and len(recs) == 4 and (ops is None) == (not augment)
        if augment:
            for r, op in zip(recs, ops):
                assert [[r["m00"], r["m01"]], [r["m10"], r["m11"]]] == pool.d4_matrix(op).tolist()
    assert loop._rng.random_sample() == one._rng.random_sample()                  # both consumed the stream alike


def test_rotation_and_scale_pool():
    Hl, offset, S, P = au.GEOMS[0]
    ext, lab = au.make_images(NIMG, Hl, offset, seed=10)
    kw = dict(augment=True, rotation=180.0, scale=(0.8, 1.25))
    a, b, c = (_batches(_pool(ext, lab, S, P, seed=s, **kw), 3) for s in (21, 21, 22))
    orig = ext[:, offset:offset + Hl, offset:offset + Hl]
    for (xa, ya, ra), (xb, yb, rb), (xc, yc, rc) in zip(a, b, c):
        assert np.array_equal(xa.view(np.int32), xb.view(np.int32)) and np.array_equal(ya, yb) and np.array_equal(ra, rb)   # repeats by seed
        assert not np.array_equal(xa, xc) and not np.array_equal(ra, rc)                                                   # differs by seed
        assert set(np.unique(ya)) <= {0, 1}
        assert float(xa.min()) >= float(orig.min()) and float(xa.max()) <= float(orig.max())                               # bilinear convexity
        hx, hy = hostio.affine_patches(ext, lab, ra, S, P)                                                                  # and it is the mirror's batch
        assert np.array_equal(xa.view(np.int32), hx.view(np.int32)) and np.array_equal(ya, hy)
    m = np.stack([r for _, _, r in a])
    assert np.abs(m["m01"]).max() > 0.1 and len(np.unique(np.round(m["m00"].astype(np.float64) ** 2 + m["m10"].astype(np.float64) ** 2, 4))) > 3
    with pytest.raises(ValueError):
        _pool(ext, lab, S, P, rotation=-1.0)
    with pytest.raises(ValueError):
        _pool(ext, lab, S, P, scale=(2.0, 1.0))


# ------------------------------------------------------------------------------------------- the model
def test_train_with_random_rotation_scale_and_d4():
    """cli.parse_options -> ConvolutionalModel -> one epoch of train() over a DevicePatchPool built as cli.main builds it"""
    from oracle import unet_oracle as U
    from road_segmentation_unet_amd.cli import parse_options
    from road_segmentation_unet_amd.model import ConvolutionalModel
    L, root, P, B, stride = 2, 16, 16, 4, 16                                   # the geometry of tests/test_gpu_cli.py
    S = U.input_size_needed(P, L)
    off = (S - P) // 2
    rng = np.random.RandomState(5)
    orig = rng.rand(2, P + 2 * stride, P + 2 * stride, 3)
    ext, lab = hostio.mirror_border(orig, off), (orig[..., 1] > 0.5) * 1.0
    argv = ["--num_layers=%d" % L, "--root_size=%d" % root, "--patch_size=%d" % P, "--stride=%d" % stride, "--batch_size=%d" % B, "--lr=0.01",
            "--seed=9", "--random_rotation=30", "--random_scale=0.8,1.25", "--d4_augmentation"]
    with pytest.raises(ValueError, match="nodevice_patch_pool"):
        parse_options(argv + ["--nodevice_patch_pool"])
    opts = parse_options(argv)
    opts.logdir = None
    m = ConvolutionalModel(opts)
    pl = pool.DevicePatchPool(ext, lab, S, P, stride, device=m.net.device, augment=opts.d4_augmentation, seed=opts.seed,
                              rotation=opts.random_rotation, scale=opts.random_scale, one_launch=opts.one_launch_loader)
    assert pl.one_launch and pl.rotation == 30.0 and pl.scale == (0.8, 1.25) and len(pl) == 18
    np.random.seed(123)
    st = m.train(pl, None, None, None)
    torch.cuda.synchronize()
    print("train(): loss %.5f over %d patches" % (st["loss"], st["patches"]))
    assert np.isfinite(st["loss"]) and st["loss"] > 0
    assert st["patches"] == len(range(0, len(pl) - B, B)) * B == 16
    assert set(np.unique(m.net.labels.cpu().numpy())) <= {0, 1}
