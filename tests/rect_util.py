"""The tile geometry of prediction on images of any size, restated in numpy from the rule of include/rsu.h rsu_tile_grid (not from the
kernels): along an axis of length L >= P with stride s there are n = ceil((L - P) / s) + 1 tiles, tile i at min(i * s, L - P); tiles run
image-major, then x (column) outer, y (row) inner; the mirror border is np.pad(..., "symmetric") of any width; a pixel's value is the
float64 sum of the tiles that cover it over their number. The six-way ensemble on H != W: the quarter turns are W x H images."""
import numpy as np

from oracle import unet_oracle as U


def origins(L, P, s):
    assert L >= P >= 1 and s >= 1
    n = -(-(L - P) // s) + 1
    return [min(i * s, L - P) for i in range(n)]


def tile_list(nimg, H, W, P, s):
    """[(image, y0, x0)] in tile order"""
    return [(k, y0, x0) for k in range(nimg) for x0 in origins(W, P, s) for y0 in origins(H, P, s)]


def extract(imgs, S, P, s):
    """float tiles [ntiles, S, S, C] of imgs [n, H, W, C]: the dtype of imgs, values copied"""
    off = (S - P) // 2
    padded = np.pad(imgs, ((0, 0), (off, off), (off, off), (0, 0)), "symmetric")
    return np.stack([padded[k, y0:y0 + S, x0:x0 + S] for k, y0, x0 in tile_list(imgs.shape[0], imgs.shape[1], imgs.shape[2], P, s)])


def overlap(prob, nimg, H, W, s):
    """(mean float64 [nimg, H, W], hits int64 [nimg, H, W]) of prob [ntiles, P, P]"""
    P = prob.shape[1]
    acc = np.zeros((nimg, H, W), np.float64)
    hits = np.zeros((nimg, H, W), np.int64)
    for t, (k, y0, x0) in enumerate(tile_list(nimg, H, W, P, s)):
        acc[k, y0:y0 + P, x0:x0 + P] += prob[t].astype(np.float64)
        hits[k, y0:y0 + P, x0:x0 + P] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return acc / hits, hits


def ensemble_variants(imgs):
    """the reference's six variants in its order, as a list: the quarter turns of [n, H, W, ...] are [n, W, H, ...]"""
    return [imgs, imgs[:, :, ::-1], imgs[:, ::-1]] + [np.rot90(imgs, k=k, axes=(1, 2)) for k in (1, 2, 3)]


def invert_ensemble(g):
    """the mean of the six masks, each turned back, added in the reference's order"""
    total = g[0] + g[1][:, :, ::-1] + g[2][:, ::-1]
    for i, k in enumerate((-1, -2, -3)):
        total = total + np.rot90(g[3 + i], k=k, axes=(1, 2))
    return total / 6


def oracle_predict(params, imgs, L, root, dilated, P, s, ensemble, emu=True):
    """ConvolutionalModel.predict with the oracle's network on this module's tiles: float64 [n, H, W, 1]"""
    S = U.input_size_needed(P, L)

    def one(x):
        tiles = extract(np.ascontiguousarray(x), S, P, s).astype(np.float32)
        probs = np.concatenate([U.predict_probs(params, tiles[i:i + 4], L, root, dilated, emulate_bf16=emu) for i in range(0, tiles.shape[0], 4)])
        return overlap(probs.reshape(-1, P, P), x.shape[0], x.shape[1], x.shape[2], s)[0][..., None]
    if not ensemble:
        return one(imgs)
    return invert_ensemble([one(v) for v in ensemble_variants(imgs)])
