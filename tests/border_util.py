"""What the border-map tests share (tests/test_border_map_host.py, tests/test_gpu_border_map.py): the brute-force statement of the definition of
include/rsu.h rsu_border_map -- integer distances over all pairs of pixels, float64 weights -- the tolerance derived from float32 rounding,
and the label cases. A plain module, imported by name. Nothing here calls the code under test."""
import numpy as np

D2_INF = 0x7fffffff   # include/rsu.h RSU_BORDER_D2_INF


def brute_d2(tile):
    """D2 of one tile [H, W] by the definition: for every valid pixel the minimum of dy^2 + dx^2 over ALL valid pixels of the other class
    (one |class 0| x |class 1| matrix of integer squared distances, in row chunks); D2_INF where there is none and at ignored pixels."""
    tile = np.asarray(tile)
    d2 = np.full(tile.shape, D2_INF, dtype=np.int64)
    p0, p1 = np.argwhere(tile == 0).astype(np.int32), np.argwhere(tile == 1).astype(np.int32)
    if len(p0) and len(p1):
        best1 = np.full(len(p1), D2_INF, dtype=np.int32)
        chunk = max(1, (1 << 24) // len(p1))
        for i in range(0, len(p0), chunk):
            a = p0[i:i + chunk]
            dd = (a[:, None, 0] - p1[None, :, 0]) ** 2 + (a[:, None, 1] - p1[None, :, 1]) ** 2
            d2[a[:, 0], a[:, 1]] = dd.min(axis=1)
            best1 = np.minimum(best1, dd.min(axis=0))
        d2[p1[:, 0], p1[:, 1]] = best1
    return d2


def brute_map(labels, w0, sigma, mul=None):
    """(out float64, d2 int64) of labels [N, H, W] by the definition, in float64: border = 1 + w0 exp(-D2 / (2 sigma^2)), exactly 1 where D2
    is infinite; out = mul * border at valid pixels (mul taken by selection: an ignored pixel's value is never touched), 0 at ignored ones."""
    labels = np.asarray(labels)
    d2 = np.stack([brute_d2(t) for t in labels])
    valid = (labels == 0) | (labels == 1)
    finite = d2 < D2_INF
    sigma = float(np.float32(sigma))   # (the ABI takes w0 and sigma as float32)
    border = np.where(finite, 1.0 + float(np.float32(w0)) * np.exp(-np.where(finite, d2, 0).astype(np.float64) / (2.0 * sigma * sigma)), 1.0)
    m = np.ones(labels.shape) if mul is None else np.where(valid, np.asarray(mul, dtype=np.float64), 1.0)
    return np.where(valid, m * border, 0.0), d2


def tolerance(w0, mul=None):
    """|out - float64 reference| allowed, from float32 rounding alone: border lies in [1, 1 + w0]; its float32 evaluation rounds the
    exponent's argument, the exponential (a couple of ulp), the product with w0 and the sum with 1 (half an ulp of 1 + w0 each), and the
    product with mul once more: a few ulp of 1 + w0, taken as 8 * 2^-23 * (1 + w0), scaled by the largest |mul| where a map multiplies."""
    scale = 1.0 if mul is None else max(1.0, float(np.nanmax(np.abs(np.asarray(mul, dtype=np.float64)))))
    return 8.0 * 2.0 ** -23 * (1.0 + float(w0)) * scale


def _strips(H, W, diagonal):
    """straight (a row band and a column band per width) or diagonal strips, 1 to 5 px wide"""
    t = np.zeros((H, W), dtype=np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    for k, width in enumerate((1, 2, 3, 4, 5)):
        if diagonal:
            c = (yy + (xx if k % 2 == 0 else -xx)) - (k * (H + W) // 7 - W // 3)
            t[(c >= 0) & (c < width)] = 1
        else:
            y0, x0 = (2 + k * H // 5) % H, (1 + k * W // 5 + W // 9) % W
            t[y0:y0 + width, :] = 1
            if k % 2 == 0:
                t[:, x0:x0 + width] = 1
    return t


def with_ignored(rng, tile):
    """~10 % ignored labels by tests/head_util._with_ignored (-1, a few 255, one 2**32 + 1)"""
    from tests import head_util as hd
    lab, _ = hd._with_ignored(rng, tile.reshape(-1))
    return lab.reshape(tile.shape)


def case_tiles(H, W, seed=0):
    """name -> one label tile [H, W] int64, the cases of the issue: i.i.d. labels, straight and diagonal strips 1 to 5 px wide, a single road
    pixel, all-one-class tiles, ~10 % ignored labels, a tile whose only other-class pixels are ignored"""
    rng = np.random.RandomState(1000 * H + W + seed)
    iid = (rng.rand(H, W) < 0.3).astype(np.int64)
    sparse = (rng.rand(H, W) < 0.03).astype(np.int64)
    single = np.zeros((H, W), dtype=np.int64)
    single[H // 3, (2 * W) // 3] = 1
    only_ignored_other = np.zeros((H, W), dtype=np.int64)       # background everywhere; the "road" is labelled 255 and 2: ignored
    only_ignored_other[H // 2, :] = 255
    only_ignored_other[:, W // 4] = 2
    return {
        "iid": iid,
        "sparse": sparse,
        "straight": _strips(H, W, False),
        "diagonal": _strips(H, W, True),
        "single": single,
        "all0": np.zeros((H, W), dtype=np.int64),
        "all1": np.ones((H, W), dtype=np.int64),
        "iid_ignored": with_ignored(rng, iid),
        "straight_ignored": with_ignored(rng, _strips(H, W, False)),
        "only_ignored_other": only_ignored_other,
    }


def mul_map(rng, labels):
    """a caller map for `labels`: 0.25 .. 1.25, some zeros, and NaN at every ignored pixel (a multiplication there would show)"""
    mul = (0.25 + rng.rand(*labels.shape)).astype(np.float32)
    mul[rng.rand(*labels.shape) < 0.05] = 0.0
    mul[(labels != 0) & (labels != 1)] = np.nan
    return mul
