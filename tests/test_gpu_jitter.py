"""Per-sample colour jitter and noise on the GPU (include/rsu.h rsu_color_jitter): the two kernels against hostio.color_jitter at the
smallest shapes at which they can go wrong, the argument checks, DevicePatchPool with jitter on against the same pool with jitter off, and a
few training steps with --color_jitter, --random_noise and --random_rotation."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from road_segmentation_unet_amd import _lib, hostio, pool
from road_segmentation_unet_amd._lib import lib
from tests import affine_util as au
from tests import hiputil as hu
from tests import jitter_util as ju

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
MARGIN = 7            # floats in front of and behind x: x itself is then 4-byte aligned only
WS_MARGIN = 3         # int64 words around the workspace
WS_JUNK = 0x7a7a7a7a7a7a7a7a


@functools.lru_cache(maxsize=None)
def _case(S, nrec):
    """per shape, computed once and left unchanged: the batch, its mixed records and the host mirror's output"""
    x = ju.make_batch(nrec, S, seed=100 * S + nrec)
    recs = ju.mixed_records(nrec, seed=S + nrec)
    want = hostio.color_jitter(x, recs)
    x.setflags(write=False), want.setflags(write=False)
    return x, recs, want


def _run(x, recs, with_ws=True):
    """one rsu_color_jitter call on a copy of x inside a sentinel-filled buffer, with a junk-filled workspace inside a sentinel-filled
    buffer of its own: (the result, True if every margin came back untouched)"""
    n, S = x.shape[0], x.shape[1]
    buf = torch.full((2 * MARGIN + x.size,), SENTINEL, dtype=torch.float32, device=hu.DEV)
    buf[MARGIN:MARGIN + x.size] = torch.from_numpy(x.reshape(-1).copy()).to(hu.DEV)
    nws = lib().rsu_color_jitter_ws_bytes(n, S) // 8
    assert nws == min(n, 32) * ((S * S + 4095) // 4096) * 3
    ws = torch.full((2 * WS_MARGIN + nws,), WS_JUNK, dtype=torch.int64, device=hu.DEV)
    recs = np.ascontiguousarray(recs)
    rc = lib().rsu_color_jitter(ctypes.c_void_p(buf.data_ptr() + 4 * MARGIN), recs.ctypes.data_as(ctypes.POINTER(_lib.RsuJitter)), n, S,
                                ctypes.c_void_p(ws.data_ptr() + 8 * WS_MARGIN) if with_ws else None, hu.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    out, w = buf.cpu().numpy(), ws.cpu().numpy()
    clean = bool((out[:MARGIN] == SENTINEL).all() and (out[MARGIN + x.size:] == SENTINEL).all()
                 and (w[:WS_MARGIN] == WS_JUNK).all() and (w[WS_MARGIN + nws:] == WS_JUNK).all())
    return out[MARGIN:MARGIN + x.size].reshape(x.shape), clean


# S: 11 and 12 (odd and even, less than one workgroup), 37 (odd; 1369 pixels do not fill a chunk), 64 (exactly 4096 pixels: one full chunk),
# 91 (odd; 8281 pixels: three chunks, the last partial). nrec 33 crosses the 32-record cut.
@pytest.mark.parametrize("nrec", [1, 3, 33])
@pytest.mark.parametrize("S", [11, 12, 37, 64, 91])
def test_kernels_equal_the_host_mirror(S, nrec):
    x, recs, want = _case(S, nrec)
    got, clean = _run(x, recs)
    differ = int((got != want).sum())
    print("S %d, nrec %d: %d of %d values differ from the host mirror's" % (S, nrec, differ, got.size))
    assert clean, "a margin of x or of the workspace was written"
    assert np.array_equal(got, want)
    assert got.min() >= 0.0 and got.max() <= 1.0
    again, _ = _run(x, recs)                                                  # a second run: the same bits
    assert np.array_equal(again.view(np.int32), got.view(np.int32))
    idt, clean = _run(x, ju.identity(nrec), with_ws=False)          # the identity returns the data bit for bit
    assert clean and np.array_equal(idt.view(np.int32), x.view(np.int32))


@pytest.mark.parametrize("S", [12, 91])
def test_null_workspace_gives_the_same_bits_when_every_k_is_zero(S):
    x, recs, _ = _case(S, 33)
    recs = recs.copy()
    recs["k"] = 0.0                                                           # identity, colour without contrast, noise, colour and noise
    assert (recs["sigma"] > 0).sum() == 16 and np.any(recs["a"] != ju.identity(1)["a"], axis=1).sum() == 16
    a, clean_a = _run(x, recs, with_ws=True)
    b, clean_b = _run(x, recs, with_ws=False)
    assert clean_a and clean_b                                                # (with_ws: the junk in the workspace is not read either)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(a, hostio.color_jitter(x, recs))
    assert not np.array_equal(a, x)


def test_refused_calls_write_nothing():
    S = 12
    x, recs, want = _case(S, 3)
    xd = torch.full((3, S, S, 3), SENTINEL, dtype=torch.float32, device=hu.DEV)
    ws = torch.full((lib().rsu_color_jitter_ws_bytes(3, S) // 8,), WS_JUNK, dtype=torch.int64, device=hu.DEV)
    ok = dict(x=hu.ptr(xd), ws=hu.ptr(ws), recs=[ju.record()], S=S, stream=hu.stream())
    for name, b in ju.abi_cases():
        assert ju.abi_call(lib(), dict(ok, **b)) == -22, name
    torch.cuda.synchronize()
    assert bool((xd == SENTINEL).all()) and bool((ws == WS_JUNK).all())
    xd.copy_(torch.from_numpy(x.copy()))
    assert ju.abi_call(lib(), dict(ok, recs=recs)) == 0                        # and the good call runs
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------- the pool
def _pool(ext, lab, S, P, **kw):
    return pool.DevicePatchPool(ext, lab, S, P, au.STRIDE[S], device=hu.DEV, **kw)


def _batches(pl, B, count=3, seed=3):
    order = np.random.RandomState(seed).permutation(len(pl))
    out = []
    for i in range(count):
        x = torch.full((B, pl.S, pl.S, 3), SENTINEL, dtype=torch.float32, device=hu.DEV)
        y = torch.full((B, pl.P, pl.P), int(SENTINEL), dtype=torch.int64, device=hu.DEV)
        ret = pl.load_batch([int(k) for k in order[i * B:(i + 1) * B]], x, y)
        torch.cuda.synchronize()
        out.append((x.cpu().numpy(), y.cpu().numpy(), ret, None if pl.last_jitter is None else pl.last_jitter.copy()))
    return out


LOADERS = {"loop": dict(augment=True), "one launch": dict(augment=True, one_launch=True),
           "rotation": dict(augment=True, rotation=180.0, scale=(0.8, 1.25))}


@pytest.mark.parametrize("loader", sorted(LOADERS))
@pytest.mark.parametrize("Hl,offset,S,P", au.GEOMS)
def test_pool_with_jitter_is_the_mirror_of_the_pool_without(Hl, offset, S, P, loader):
    """the same seed, jitter on and off: equal labels, equal return values, and the inputs are hostio.color_jitter of the plain inputs
    under the records the pool kept"""
    ext, lab = au.make_images(3, Hl, offset, seed=9)
    ext = (ext / ext.max()).astype(np.float32)                                 # into [0, 1], as the training images are
    kw = LOADERS[loader]
    off = _pool(ext, lab, S, P, seed=11, **kw)
    on = _pool(ext, lab, S, P, seed=11, jitter=(0.3, 0.4, 0.5, 20.0), noise=0.03, **kw)
    assert not off.jitter_on and off.last_jitter is None and off._jitter_ws is None and on.jitter_on
    seen = set()
    for (xa, ya, ra, ja), (xb, yb, rb, jb) in zip(_batches(off, 4), _batches(on, 4)):
        assert ja is None and jb.dtype == hostio.JITTER_DTYPE and len(jb) == 4
        assert np.array_equal(ya, yb) and set(np.unique(yb)) <= {0, 1}
        assert (ra is None and rb is None) or np.array_equal(np.asarray(ra), np.asarray(rb))
        assert np.array_equal(xb, hostio.color_jitter(xa, jb)) and not np.array_equal(xa, xb)
        assert np.any(jb["k"] != 0, axis=1).all() and (jb["sigma"] == np.float32(0.03)).all()
        seen |= set(jb["key"].tolist())
    assert len(seen) == 12
    assert off._rng.random_sample() == on._rng.random_sample()                 # the geometric stream did not move
    want = pool.jitter_draw(np.random.RandomState((11 + 0x6a09e667) % 2 ** 32), 12, 0.3, 0.4, 0.5, 20.0, 0.03)
    assert set(want["key"].tolist()) == seen                                   # and the jitter draws come from the documented generator


def test_pool_without_contrast_passes_no_workspace_and_all_zero_strengths_launch_nothing(monkeypatch):
    Hl, offset, S, P = au.GEOMS[0]
    ext, lab = au.make_images(3, Hl, offset, seed=9)
    ext = (ext / ext.max()).astype(np.float32)
    calls = []
    real = _lib.call

    def recorder(name, *args):
        calls.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", recorder)
    plain = _pool(ext, lab, S, P, seed=11, one_launch=True, jitter=(0.0, 0.0, 0.0, 0.0), noise=0.0)
    (xa, ya, _, ja), = _batches(plain, 4, count=1)
    assert ja is None and not plain.jitter_on and not hasattr(plain, "_jitter_rng") and plain._jitter_ws is None
    assert [c[0] for c in calls] == ["rsu_affine_patches"]
    del calls[:]
    nocon = _pool(ext, lab, S, P, seed=11, one_launch=True, jitter=(0.3, 0.0, 0.5, 20.0), noise=0.03)
    (xb, yb, _, jb), = _batches(nocon, 4, count=1)
    assert [c[0] for c in calls] == ["rsu_affine_patches", "rsu_color_jitter"] and calls[1][1][4] is None and nocon._jitter_ws is None
    assert not jb["k"].any() and np.array_equal(ya, yb) and np.array_equal(xb, hostio.color_jitter(xa, jb))
    with pytest.raises(ValueError):
        _pool(ext, lab, S, P, jitter=(1.0, 0.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        _pool(ext, lab, S, P, noise=-0.5)


# ------------------------------------------------------------------------------------------- the model
def test_train_with_color_jitter_noise_and_rotation():
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
            "--seed=9", "--color_jitter=0.2,0.2,0.2,10", "--random_noise=0.02", "--random_rotation=180"]
    with pytest.raises(ValueError, match="nodevice_patch_pool"):
        parse_options(argv + ["--nodevice_patch_pool"])
    opts = parse_options(argv)
    opts.logdir = None
    m = ConvolutionalModel(opts)
    pl = pool.DevicePatchPool(ext, lab, S, P, stride, device=m.net.device, augment=opts.d4_augmentation, seed=opts.seed,
                              rotation=opts.random_rotation, scale=opts.random_scale, one_launch=opts.one_launch_loader,
                              jitter=opts.color_jitter, noise=opts.random_noise)
    assert pl.one_launch and pl.jitter_on and pl.jitter == (0.2, 0.2, 0.2, 10.0) and pl.noise == 0.02 and len(pl) == 18
    np.random.seed(123)
    st = m.train(pl, None, None, None)
    torch.cuda.synchronize()
    print("train(): loss %.5f over %d patches" % (st["loss"], st["patches"]))
    assert np.isfinite(st["loss"]) and st["loss"] > 0
    assert st["patches"] == len(range(0, len(pl) - B, B)) * B == 16
    assert set(np.unique(m.net.labels.cpu().numpy())) <= {0, 1}
    xin = m.net.x.cpu().numpy()
    assert pl.last_jitter is not None and len(pl.last_jitter) == B and xin.min() >= 0.0 and xin.max() <= 1.0
