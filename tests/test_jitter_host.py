"""Per-sample colour jitter and noise without a GPU: hostio.color_jitter (the numpy float32 statement of include/rsu.h rsu_color_jitter, the
yardstick of tests/test_gpu_jitter.py) against literals and a float64 sequential definition, pool.jitter_draw, the flags and the ABI's
argument checks."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from road_segmentation_unet_amd import _lib, hostio, pool
from road_segmentation_unet_amd.cli import parse_options
from road_segmentation_unet_amd.model import EXTRA_FLAG_DEFS, FLAG_DEFS, Options
from tests import jitter_util as ju

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- the noise
def test_noise_integers_equal_independent_literals():
    assert hostio.jitter_noise_int(0x1234abcd, 6).tolist() == [48286, 90907, 184729, 139881, 143961, 164521]
    assert hostio.jitter_noise_int(0, 3).tolist() == [49624, 89271, 120445]
    assert hostio.JITTER_NOISE_SCALE.dtype == np.float32 and hostio.JITTER_NOISE_SCALE.view(np.uint32) == 0x37ddb3d7
    assert np.float32(1.0 / math.sqrt((65536.0 ** 2 - 1.0) / 3.0)) == hostio.JITTER_NOISE_SCALE


@pytest.mark.parametrize("key", [0x1234abcd, 0])
def test_noise_statistics_within_four_standard_errors(key):
    S = 64
    N = S * S * 3
    assert N == 12288
    g = (hostio.jitter_noise_int(key, N).astype(np.float64) - 131070.0) / math.sqrt((65536.0 ** 2 - 1.0) / 3.0)
    zm, zs = abs(g.mean()) * math.sqrt(N), abs(g.std() - 1.0) * math.sqrt(2 * N)
    print("key %#x: |mean| sqrt(N) = %.2f, |std - 1| sqrt(2N) = %.2f" % (key, zm, zs))
    assert zm <= 4.0 and zs <= 4.0
    # and color_jitter adds exactly sigma * g to a mid-grey sample (no clamp is reached)
    x = np.full((1, S, S, 3), 0.5, np.float32)
    sigma = np.float32(0.03125)
    y = hostio.color_jitter(x, [ju.record(sigma=sigma, key=key)])
    g32 = (hostio.jitter_noise_int(key, N).astype(np.float32) - np.float32(131070.0)) * hostio.JITTER_NOISE_SCALE
    assert np.array_equal(y.reshape(-1), np.float32(0.5) + sigma * g32)
    assert abs(float(y.astype(np.float64).std()) / float(sigma) - 1.0) <= 4.0 / math.sqrt(2 * N) + 1e-6


# ------------------------------------------------------------------------------------------- the colour map
def test_composed_matrices_equal_the_four_steps_in_float64():
    rng = np.random.RandomState(2)
    x = rng.rand(9, 9, 3)
    worst = 0.0
    for b, c, s, th in ju.draw_params(rng, 20, *ju.STRONG):
        A, K = pool.jitter_matrices(b, c, s, th)
        y = x @ A.T + K @ x.mean(axis=(0, 1))
        worst = max(worst, float(np.abs(y - ju.sequential64(x, b, c, s, th, clamp=False)).max()))
        grey = np.full(3, 0.37)
        A1, K1 = pool.jitter_matrices(1.0, 1.0, s, th)                  # saturation and hue alone: grey stays grey
        assert np.abs(A1 @ grey - grey).max() <= 1e-15 and not K1.any()
    print("composed map against the sequence, float64: max difference %.2e" % worst)
    assert worst <= 1e-14          # some twenty float64 roundings of values below 8


def test_mirror_stays_within_the_derived_bound_of_the_float64_definition():
    S = 31
    rng = np.random.RandomState(3)
    x = rng.rand(6, S, S, 3).astype(np.float32)
    params = ju.draw_params(np.random.RandomState(4), 6, *ju.STRONG)
    recs = hostio.jitter_records([ju.record(*pool.jitter_matrices(*p)) for p in params])
    y = hostio.color_jitter(x, recs)
    assert y.dtype == np.float32 and y.shape == x.shape and y.min() >= 0.0 and y.max() <= 1.0
    for j, p in enumerate(params):
        err, bound = float(np.abs(y[j] - ju.sequential64(x[j], *p)).max()), ju.value_bound(recs[j:j + 1])
        print("draw %d (b %.2f c %.2f s %.2f hue %6.1f): max |float32 - float64| %.3e, bound %.3e" % ((j,) + p + (err, bound)))
        assert err <= bound
    assert 0.0 < float((y == 0.0).mean()) < 0.9 and float(np.abs(y - x).max()) > 0.1            # the clamp and the map both act


def test_identity_grey_and_independence_of_the_neighbours():
    rng = np.random.RandomState(5)
    x = ju.make_batch(33, 7, seed=5)
    x.setflags(write=False)
    y = hostio.color_jitter(x, ju.identity(33))
    assert y is not x and np.array_equal(y.view(np.int32), x.view(np.int32))
    # grey input stays grey under saturation and hue alone
    grey = np.repeat(rng.rand(4, 7, 7, 1).astype(np.float32), 3, axis=3)
    recs = pool.jitter_draw(np.random.RandomState(6), 4, 0.0, 0.0, 0.9, 180.0)
    assert not recs["k"].any() and not recs["sigma"].any()
    out = hostio.color_jitter(grey, recs)
    dev = float(np.abs(out - grey).max())
    print("grey under saturation and hue: max deviation %.2e, bound %.2e" % (dev, ju.value_bound(recs)))
    assert dev <= ju.value_bound(recs)
    # a sample's output depends on its own record alone: any cut of a list of 33, and every sample on its own
    recs = ju.mixed_records(33, seed=7)
    assert np.any(recs["k"] != 0, axis=1).sum() == 16 and (recs["sigma"] > 0).sum() == 16
    whole = hostio.color_jitter(x, recs)
    for cut in (1, 16, 32):
        parts = np.concatenate([hostio.color_jitter(x[:cut], recs[:cut]), hostio.color_jitter(x[cut:], recs[cut:])])
        assert np.array_equal(parts.view(np.int32), whole.view(np.int32)), cut
    perm = np.random.RandomState(8).permutation(33)
    assert np.array_equal(hostio.color_jitter(x[perm], recs[perm]).view(np.int32), whole[perm].view(np.int32))
    for j in range(33):
        assert np.array_equal(hostio.color_jitter(x[j:j + 1], recs[j:j + 1])[0].view(np.int32), whole[j].view(np.int32)), j


def test_mirror_refuses_what_the_abi_refuses():
    x = ju.make_batch(2, 5, seed=1)
    hostio.color_jitter(x, [ju.record(), ju.record(np.eye(3), 0.5 * np.eye(3), 1.0, 2 ** 32 - 1)])
    for name, b in ju.abi_cases():
        if "recs" in b and "ws" not in b:
            with pytest.raises(ValueError):
                hostio.color_jitter(x, b["recs"])
    for bad in (x.astype(np.float64), x[..., :2], x[:, :4], x[0], x[:0]):
        with pytest.raises(ValueError):
            hostio.color_jitter(bad, [ju.record()] * len(bad))
    with pytest.raises(ValueError):
        hostio.color_jitter(x, [ju.record()])


# ------------------------------------------------------------------------------------------- draws
def test_jitter_draw_consumes_only_the_draws_that_are_on():
    names = ("brightness", "contrast", "saturation", "hue", "noise")
    values = dict(brightness=0.4, contrast=0.3, saturation=0.5, hue=25.0, noise=0.05)
    for mask in range(32):
        on = [n for i, n in enumerate(names) if mask >> i & 1]
        a, b = np.random.RandomState(40 + mask), np.random.RandomState(40 + mask)
        recs = pool.jitter_draw(a, 3, **{n: values[n] for n in on})
        assert recs.dtype == hostio.JITTER_DTYPE and recs.shape == (3,)
        for j in range(3):
            p = {n: b.random_sample() for n in names[:4] if n in on}                       # in this order, per sample
            key = int(b.randint(0, 2 ** 32)) if "noise" in on else 0
            f = {n: 1.0 + (2.0 * p[n] - 1.0) * values[n] if n in on else 1.0 for n in names[:3]}
            th = (2.0 * p["hue"] - 1.0) * values["hue"] if "hue" in on else 0.0
            A, K = pool.jitter_matrices(f["brightness"], f["contrast"], f["saturation"], th)
            assert np.array_equal(recs["a"][j], A.astype(np.float32).reshape(9)) and np.array_equal(recs["k"][j], K.astype(np.float32).reshape(9)), on
            assert recs["key"][j] == key and recs["sigma"][j] == np.float32(values["noise"] if "noise" in on else 0.0), on
            assert bool(recs["k"][j].any()) == ("contrast" in on)
        assert a.random_sample() == b.random_sample(), on                                  # both consumed the stream alike
    off = pool.jitter_draw(np.random.RandomState(1), 2)
    assert np.array_equal(off, ju.identity(2))
    keys = pool.jitter_draw(np.random.RandomState(2), 64, noise=0.1)["key"]
    assert keys.dtype == np.uint32 and len(set(keys.tolist())) == 64 and int(keys.max()) > 2 ** 31 and len(set((keys >> 16).tolist())) > 60
    for bad in (dict(brightness=1.0), dict(contrast=-0.1), dict(saturation=float("nan")), dict(hue=181.0), dict(hue=-1.0),
                dict(noise=1.5), dict(noise=-0.1), dict(noise=float("inf")), dict(brightness="x")):
        with pytest.raises(ValueError):
            pool.jitter_draw(np.random.RandomState(0), 1, **bad)


def test_jitter_flags_and_command_line():
    assert len(FLAG_DEFS) == 30                                            # the reference's flags stay the reference's
    defs = {d[0]: d for d in EXTRA_FLAG_DEFS}
    assert defs["color_jitter"][1:3] == (str, "0,0,0,0") and defs["random_noise"][1:3] == (float, 0.0)
    o = Options()
    assert o.color_jitter == (0.0, 0.0, 0.0, 0.0) and o.random_noise == 0.0
    o = parse_options(["--color_jitter=0.2,0.3,0.4,10", "--random_noise=0.02", "--random_rotation=180"])
    assert o.color_jitter == (0.2, 0.3, 0.4, 10.0) and o.random_noise == 0.02 and o.random_rotation == 180.0
    assert parse_options(["--color_jitter", "0,0,0,180"]).color_jitter == (0.0, 0.0, 0.0, 180.0)
    assert parse_options(["--random_noise=1"]).random_noise == 1.0
    assert Options(color_jitter=(0.5, 0, 0, 0)).color_jitter == (0.5, 0.0, 0.0, 0.0) and Options(random_noise="0.5").random_noise == 0.5
    nan, inf = float("nan"), float("inf")
    for bad in ("1,0,0,0", "0,1,0,0", "0,0,1,0", "0,0,0,180.5", "-0.1,0,0,0", "0,0,0,-1", "0,0,0", "0,0,0,0,0", "nan,0,0,0", "0,0,0,inf", "a,b,c,d",
                "", None, 0.5, (0.1, 0.1, nan, 0.0), (0.1, 0.1, 0.1), (True, 0, 0, 0)):
        with pytest.raises(ValueError):
            Options(color_jitter=bad)
    for bad in (-0.1, 1.5, nan, inf, -inf, "x", None, True):
        with pytest.raises(ValueError):
            Options(random_noise=bad)
    for argv in (["--color_jitter=1,0,0,0"], ["--color_jitter=0.1,0.1,0.1"], ["--color_jitter=0,0,0,200"], ["--color_jitter=nan,0,0,0"],
                 ["--random_noise=-1"], ["--random_noise=2"], ["--random_noise=nan"]):
        with pytest.raises(ValueError):
            parse_options(argv)
    # with the host pool the flags are refused, not ignored
    for argv in (["--color_jitter=0.1,0,0,0"], ["--color_jitter=0,0,0,5"], ["--random_noise=0.01"]):
        with pytest.raises(ValueError, match="nodevice_patch_pool"):
            parse_options(argv + ["--nodevice_patch_pool"])
    assert parse_options(["--nodevice_patch_pool", "--color_jitter=0,0,0,0", "--random_noise=0"]).device_patch_pool is False


# ------------------------------------------------------------------------------------------- the ABI, on the host
def test_symbol_is_declared_exported_and_bound_with_the_headers_arity():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsu.h")).read(), flags=re.S)
    L = _lib.lib()
    for name, restype in (("rsu_color_jitter", "int"), ("rsu_color_jitter_ws_bytes", "size_t")):
        m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (restype, name), header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(L, name)
    assert re.search(r"#define\s+RSU_JITTER_MAX_LAUNCH\s+32\b", header) and _lib.JITTER_MAX_LAUNCH == 32
    assert ctypes.sizeof(_lib.RsuJitter) == hostio.JITTER_DTYPE.itemsize == 80
    assert [n for n, _ in _lib.RsuJitter._fields_] == list(hostio.JITTER_DTYPE.names)
    assert [getattr(_lib.RsuJitter, n).offset for n in hostio.JITTER_DTYPE.names] == [hostio.JITTER_DTYPE.fields[n][1] for n in hostio.JITTER_DTYPE.names]
    # the partial sums of one launch: three int64 per 4096-pixel share and record, for at most 32 records
    ws = L.rsu_color_jitter_ws_bytes
    assert ws(1, 64) == 24 and ws(1, 65) == 48 and ws(4, 572) == 4 * 80 * 24 and ws(33, 572) == ws(32, 572) == 32 * 80 * 24
    assert ws(0, 64) == ws(-1, 64) == ws(1, 0) == ws(1, -3) == 0


def test_abi_refuses_bad_arguments_on_the_host():
    """every refused call returns from host code before anything is launched (no GPU is needed: the device pointers are never
    dereferenced)"""
    L = _lib.lib()
    p = ctypes.c_void_p(4096)
    ok = dict(x=p, ws=p, recs=[ju.record()], S=12)
    for name, b in ju.abi_cases():
        assert ju.abi_call(L, dict(ok, **b)) == -22, name
    assert ju.abi_call(L, dict(ok, S=6708, recs=[ju.record()] * 4)) == _lib.E2BIG            # x of 2.16 GB
    assert ju.abi_call(L, dict(ok, S=13378, ws=None)) == _lib.E2BIG                          # one sample of 2.15 GB
    assert ju.abi_call(L, dict(ok, S=6708, recs=[ju.record()] * 3 + [ju.record(sigma=2.0)])) == -22   # a bad record comes first
