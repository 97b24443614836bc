"""Device-side patch/stride tiler and prediction ensemble, mirroring the hot-path subset of the reference's
src/images.py (same function names, argument meaning, ordering conventions and assertions).

Everything here runs on the GPU through librsu_hip.so (rsu_extract_tiles / rsu_overlap_add / rsu_overlap_finish, and their _rect
forms for what the reference asserts against: H != W, a stride that does not cover the image, a border wider than the image) or is
pure index plumbing on torch tensors (flips / rot90). Inputs may be numpy arrays or torch tensors; results are torch
tensors on the device (call .cpu().numpy() for the reference's numpy convention).
"""
import ctypes

import numpy as np
import torch

from ._lib import call

DEV = "cuda:0"


def _dev(a, device=None):
    t = torch.as_tensor(a)
    return t.to(device or DEV, torch.float32).contiguous()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def tile_grid(H, W, patch_size, stride):
    """(ny, nx): the tile grid of an H x W image (include/rsu.h rsu_tile_grid; hostio.tile_origins is the same rule per axis).
    ValueError for an image smaller than the patch."""
    H, W, patch_size, stride = int(H), int(W), int(patch_size), int(stride)
    if patch_size < 1 or stride < 1:
        raise ValueError("--patch_size=%d and --stride=%d must be at least 1" % (patch_size, stride))
    if H < patch_size or W < patch_size:
        raise ValueError("an image of %d x %d pixels is smaller than --patch_size=%d: predict with a smaller --patch_size (the weights do "
                         "not depend on it)" % (H, W, patch_size))
    ny, nx = ctypes.c_int(0), ctypes.c_int(0)
    call("rsu_tile_grid", H, W, patch_size, stride, ctypes.byref(ny), ctypes.byref(nx))
    return ny.value, nx.value


def _reference_geometry(H, W, S, P, stride):
    """whether rsu_extract_tiles / rsu_overlap_add accept this input: a square image, the stride covering it exactly, a mirror border
    (S is None: no border) no wider than the image. Such inputs stay on those entries; the rect entries give them the same bits."""
    return H == W and (H - P) % stride == 0 and (S is None or (S - P) // 2 <= H)


def extract_mirrored_patches(images, patch_size, predict_patch_size, stride, t0=0, ntiles=None, out=None):
    """images.mirror_border(images, (patch_size - predict_patch_size) / 2) followed by
    images.extract_patches(..., patch_size, stride, predict_patch_size) (tf_aerial_images.py:288-293), fused on device.

    images: [n, H, W, 3] float, H and W at least predict_patch_size, any stride: the grid of hostio.tile_origins per axis, the last tile
    clamped to the image's edge where the stride does not cover it. Returns float32 [ntiles, S, S, 3] for tile indices [t0, t0+ntiles)
    of the reference's ordering: image-major, then x (column) outer, y (row) inner (images.py:75-77). The padded image is never built."""
    images = _dev(images)
    n, H, W, C = images.shape
    assert C == 3
    assert (patch_size - predict_patch_size) % 2 == 0 and predict_patch_size <= patch_size
    ny, nx = tile_grid(H, W, predict_patch_size, stride)
    total = n * nx * ny
    if ntiles is None:
        ntiles = total - t0
    if out is None:
        out = torch.empty((ntiles, patch_size, patch_size, 3), dtype=torch.float32, device=images.device)
    if _reference_geometry(H, W, patch_size, predict_patch_size, stride):
        call("rsu_extract_tiles", _ptr(images), _ptr(out), n, H, patch_size, predict_patch_size, stride, t0, ntiles, _stream(images))
    else:
        call("rsu_extract_tiles_rect", _ptr(images), _ptr(out), n, H, W, patch_size, predict_patch_size, stride, t0, ntiles, _stream(images))
    return out


class OverlapAccumulator:
    """images.images_from_patches (images.py:131-164) as an accumulator: add() tile ranges in any split, finish() divides
    by the hit count. Deterministic (gather form, no atomics); partial accumulators of different ranks can be summed.
    image_size: an int (square) or an (H, W) pair; any stride (the tile grid of extract_mirrored_patches)."""

    def __init__(self, num_images, image_size, patch_size, stride, device=DEV):
        H, W = (image_size, image_size) if isinstance(image_size, (int, np.integer)) else image_size
        self.n, self.H, self.W, self.P, self.stride = num_images, int(H), int(W), patch_size, stride
        self.ny, self.nx = tile_grid(self.H, self.W, patch_size, stride)
        self.acc = torch.zeros((num_images, self.H, self.W), dtype=torch.float32, device=device)
        self.hits = torch.zeros_like(self.acc)

    def add(self, probs, t0):
        """probs: [ntiles, P, P] float32 device tensor holding tiles t0 .. t0+ntiles-1"""
        probs = probs.contiguous()
        if _reference_geometry(self.H, self.W, None, self.P, self.stride):
            call("rsu_overlap_add", _ptr(probs), _ptr(self.acc), _ptr(self.hits), self.n, self.H, self.P, self.stride, t0, probs.shape[0],
                 _stream(probs))
        else:
            call("rsu_overlap_add_rect", _ptr(probs), _ptr(self.acc), _ptr(self.hits), self.n, self.H, self.W, self.P, self.stride, t0,
                 probs.shape[0], _stream(probs))

    def finish(self):
        out = torch.empty_like(self.acc)
        call("rsu_overlap_finish", _ptr(self.acc), _ptr(self.hits), _ptr(out), self.acc.numel(), _stream(out))
        return out.unsqueeze(-1)  # [n, H, W, 1] like the reference


def images_from_patches(patches, stride=None):
    """images.py:131-164 for [num_images, num_patches, p, p, 1] device/numpy input (single channel, the mask case)."""
    patches = _dev(patches)
    n, npatch, p, _, c = patches.shape
    assert c == 1
    if stride is None:
        stride = p
    side = int(round(np.sqrt(npatch)))
    assert side * side == npatch, "Square image assumption broken"
    acc = OverlapAccumulator(n, (side - 1) * stride + p, p, stride, device=patches.device)
    acc.add(patches.reshape(n * npatch, p, p), 0)
    return acc.finish()


def image_augmentation_ensemble(imgs):
    """images.py:376-396: [id, flip W, flip H, rot90 k=1,2,3 over axes (1,2)], grouped by transform."""
    imgs = torch.as_tensor(imgs)
    parts = [imgs, torch.flip(imgs, dims=(2,)), torch.flip(imgs, dims=(1,))] + [torch.rot90(imgs, k=k, dims=(1, 2)) for k in (1, 2, 3)]
    return torch.cat(parts, dim=0)


def invert_image_augmentation_ensemble(masks):
    """images.py:399-417: inverse transforms, mean of the 6 variants (returns a new tensor; the reference mutates its input)."""
    masks = torch.as_tensor(masks)
    assert masks.shape[0] % 6 == 0
    n = masks.shape[0] // 6
    g = [masks[i * n:(i + 1) * n] for i in range(6)]
    total = g[0] + torch.flip(g[1], dims=(2,)) + torch.flip(g[2], dims=(1,))
    for i, k in enumerate((-1, -2, -3)):
        total = total + torch.rot90(g[3 + i], k=k, dims=(1, 2))
    return total / 6


def image_augmentation_ensemble_rect(imgs):
    """image_augmentation_ensemble for [n, H, W, ...] with H != W, where the quarter turns have another shape and the six variants no
    longer stack: ([id, flip W, flip H, rot90 k=2] at H x W, [rot90 k=1, rot90 k=3] at W x H)"""
    imgs = torch.as_tensor(imgs)
    upright = [imgs, torch.flip(imgs, dims=(2,)), torch.flip(imgs, dims=(1,)), torch.rot90(imgs, k=2, dims=(1, 2))]
    turned = [torch.rot90(imgs, k=1, dims=(1, 2)), torch.rot90(imgs, k=3, dims=(1, 2))]
    return torch.cat(upright, dim=0), torch.cat(turned, dim=0)


def invert_image_augmentation_ensemble_rect(upright, turned):
    """invert_image_augmentation_ensemble for the two stacks of image_augmentation_ensemble_rect: the same six terms added in the same
    order, g0 + flip(g1) + flip(g2) + rot(g3) + rot(g4) + rot(g5), then / 6"""
    assert upright.shape[0] % 4 == 0 and turned.shape[0] * 2 == upright.shape[0]
    n = upright.shape[0] // 4
    g0, g1, g2, g4 = (upright[i * n:(i + 1) * n] for i in range(4))
    g3, g5 = turned[:n], turned[n:]
    total = g0 + torch.flip(g1, dims=(2,)) + torch.flip(g2, dims=(1,))
    for g, k in ((g3, -1), (g4, -2), (g5, -3)):
        total = total + torch.rot90(g, k=k, dims=(1, 2))
    return total / 6
