"""What the connected-component tests share (tests/test_components_host.py, test_gpu_components.py, test_gpu_components_fenced.py): the
bank of masks and of float inputs, scipy's labelling brought to the header's labels (1 + the smallest row-major index) as the
independent check of the host restatements, and the launch helpers of include/rsu_components.h. A plain module, imported by name."""
import functools

import numpy as np

f32 = np.float32
TILE = 64                 # components.h CC_TILE
THRESHOLD = 0.5
# (N, H, W) with 64-pixel tiles: one pixel; one row and one column of two tiles; a tile less / more than a pixel; three by two tiles, both
# axes partial; three by three tiles: two merge levels
SHAPES = [(1, 1, 1), (2, 1, 70), (2, 70, 1), (3, 63, 65), (2, 130, 67), (1, 150, 150)]
CONNECTIVITIES = (4, 8)


def shape_id(s):
    return "%dx%dx%d" % tuple(s)


# ------------------------------------------------------------------------------------------- masks [H, W]
def serpentine(H, W):
    """every second row full, joined alternately at the right and the left end: ONE component whose smallest index is reached only along
    a path that crosses every tile border many times"""
    m = np.zeros((H, W), bool)
    m[::2] = True
    for k, y in enumerate(range(1, H - 1, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = True
    return m


def spiral(H, W):
    """a one-pixel-wide rectangular spiral from the top left corner inwards, one pixel of background between its turns"""
    m = np.zeros((H, W), bool)
    y = x = d = turns = 0
    m[0, 0] = True
    while turns < 2:
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        ok = 0 <= ny < H and 0 <= nx < W and not m[ny, nx] and not (0 <= ay < H and 0 <= ax < W and m[ay, ax])
        if ok:
            y, x, turns = ny, nx, 0
            m[y, x] = True
        else:
            d, turns = (d + 1) % 4, turns + 1
    return m


def rings(H, W):
    """concentric one-pixel rectangular rings two pixels apart and a speck at the centre: holes nest, and a hole holds a speck"""
    m = np.zeros((H, W), bool)
    k = 1
    while 2 * k < min(H, W) - 1:
        m[k, k:W - k] = m[H - 1 - k, k:W - k] = True
        m[k:H - k, k] = m[k:H - k, W - 1 - k] = True
        k += 3
    m[H // 2, W // 2] = True
    return m


def _rand(d):
    return lambda H, W: np.random.RandomState(7).random_sample((H, W)) < d


MASKS = {
    "empty": lambda H, W: np.zeros((H, W), bool),
    "full": lambda H, W: np.ones((H, W), bool),
    "rand0.41": _rand(0.41),
    "rand0.55": _rand(0.55),
    "rand0.62": _rand(0.62),
    "checker": lambda H, W: (np.add.outer(np.arange(H), np.arange(W)) % 2) == 0,
    "serpentine": serpentine,
    "serpentine_t": lambda H, W: np.ascontiguousarray(serpentine(W, H).T),
    "spiral": spiral,
    "rings": rings,
}
KINDS = sorted(MASKS)


@functools.lru_cache(maxsize=None)
def _masks_cached(kind, shape):
    N, H, W = shape
    m = MASKS[kind](H, W)
    out = np.stack([m if n % 2 == 0 else m[::-1, ::-1] for n in range(N)])   # the odd images turned by 180 degrees: images differ
    out.setflags(write=False)
    return out


def masks(kind, shape):
    """bool [N, H, W] (read-only, shared between the tests)"""
    return _masks_cached(kind, tuple(shape))


def prob_of(mask, seed=11):
    """float32 probabilities whose mask at THRESHOLD is `mask`: foreground in [0.5, 1), background in [0, 0.5), the threshold itself and
    the float below it among them"""
    rng = np.random.RandomState(seed)
    u = rng.random_sample(mask.shape).astype(f32) * f32(0.49)
    p = np.where(mask, f32(0.5) + u, u).astype(f32)
    flat, mflat = p.reshape(-1), mask.reshape(-1)
    fg, bg = np.nonzero(mflat)[0], np.nonzero(~mflat)[0]
    if fg.size:
        flat[fg[0]] = f32(THRESHOLD)
    if bg.size:
        flat[bg[0]] = np.nextafter(f32(THRESHOLD), f32(0))
    return p


def float_bank(shape, seed=13):
    """float32 [N, H, W]: rand0.55 as probabilities with every fifth pixel replaced, in turn, by the threshold, the float below it, -0.0,
    a NaN with a payload, +inf, -inf and a negative NaN"""
    p = prob_of(masks("rand0.55", shape), seed).copy()
    flat = p.reshape(-1)
    special = np.array([0x3f000000, 0x3effffff, 0x80000000, 0x7fc12345, 0x7f800000, 0xff800000, 0xffc00001], np.uint32).view(f32)
    pos = np.arange(0, flat.size, 5)
    flat[pos] = special[np.arange(pos.size) % special.size]
    return p


# ------------------------------------------------------------------------------------------- scipy, brought to the header's labels
def scipy_labels(mask, connectivity):
    """int32 [H, W]: scipy.ndimage.label with the 4- or 8-neighbourhood, every label replaced by 1 + the smallest row-major index"""
    from scipy import ndimage
    lab, k = ndimage.label(mask, structure=np.ones((3, 3), int) if connectivity == 8 else None)
    if k == 0:
        return np.zeros(mask.shape, np.int32)
    idx = np.arange(mask.size).reshape(mask.shape)
    smallest = np.asarray(ndimage.minimum(idx, lab, index=np.arange(1, k + 1)), np.int64)
    return np.concatenate([[0], smallest + 1])[lab].astype(np.int32)


def scipy_area_edge(lab):
    counts = np.bincount(lab.reshape(-1))
    area = np.where(lab > 0, counts[lab], 0).astype(np.int32)
    border = np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))
    edge = (np.isin(lab, border[border > 0])).astype(np.uint8)
    return area, edge


def scipy_filter(p, threshold, connectivity, min_area, max_hole):
    """the four steps of rsu_components_filter composed from scipy calls, one image [H, W]: (out, stats[6])"""
    with np.errstate(invalid="ignore"):
        f0 = p >= f32(threshold)
    stats = np.zeros(6, np.int64)
    removed, filled = np.zeros(p.shape, bool), np.zeros(p.shape, bool)
    if min_area > 1:
        lab = scipy_labels(f0, connectivity)
        area, _ = scipy_area_edge(lab)
        removed = (lab > 0) & (area < min_area)
        stats[0] = len(np.unique(lab[lab > 0]))
        stats[1] = len(np.unique(lab[removed]))
        stats[2] = removed.sum()
    if max_hole > 0:
        lab = scipy_labels(~(f0 & ~removed), 4 if connectivity == 8 else 8)
        area, edge = scipy_area_edge(lab)
        hole = (lab > 0) & (edge == 0)
        filled = hole & (area <= max_hole)
        stats[3] = len(np.unique(lab[hole]))
        stats[4] = len(np.unique(lab[filled]))
        stats[5] = filled.sum()
    out = p.copy()
    out[removed] = f32(0)
    out[filled] = f32(1)
    return out, stats


def scipy_count(mask, connectivity):
    from scipy import ndimage
    return int(ndimage.label(mask, structure=np.ones((3, 3), int) if connectivity == 8 else None)[1])


# (kind, shape) of the clean-up tests, "float_bank" beside the masks; and the (min_area, max_hole) pairs: both steps, either alone, none,
# the smallest that do anything, and ones no component survives
FILTER_CASES = [("rand0.55", (1, 150, 150)), ("rand0.55", (2, 130, 67)), ("rand0.41", (3, 63, 65)), ("rings", (2, 130, 67)),
                ("checker", (2, 70, 70)), ("rand0.62", (2, 1, 70)), ("full", (1, 1, 1)), ("float_bank", (2, 130, 67))]
FILTER_IDS = ["%s-%s" % (k, shape_id(s)) for k, s in FILTER_CASES]
FILTER_ARGS = ((20, 20), (20, 0), (0, 20), (1, 0), (2, 1), (1 << 24, 1 << 24))


def filter_input(kind, shape):
    return float_bank(shape) if kind == "float_bank" else prob_of(masks(kind, shape))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ------------------------------------------------------------------------------------------- the host reference, once per case
@functools.lru_cache(maxsize=None)
def host_labels(kind, shape, connectivity, invert):
    """hostio.label_components of prob_of(masks(kind, shape)): computed once, shared, read-only"""
    from road_segmentation_unet_amd import hostio
    out = hostio.label_components(prob_of(masks(kind, shape)), THRESHOLD, connectivity, invert)
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------- launches (GPU tests)
def ws_bytes(shape):
    from road_segmentation_unet_amd._lib import lib
    return int(lib().rsu_components_ws_bytes(*shape))


def new_ws(shape):
    """a workspace of the advertised size, filled with a pattern: the entries must not count on its contents"""
    import torch
    from tests import hiputil as hu
    return torch.full((ws_bytes(shape) // 4,), 0x7FA57FA5, dtype=torch.int32, device=hu.DEV)


def run_label(prob_t, connectivity, invert, shape, want_area=True, want_edge=True, ws=None, threshold=THRESHOLD):
    """(labels, area or None, edge or None) as device tensors"""
    import torch
    from road_segmentation_unet_amd._lib import call
    from tests import hiputil as hu
    ws = new_ws(shape) if ws is None else ws
    labels = torch.full(shape, -7, dtype=torch.int32, device=hu.DEV)
    area = torch.full(shape, -7, dtype=torch.int32, device=hu.DEV) if want_area else None
    edge = torch.full(shape, 77, dtype=torch.uint8, device=hu.DEV) if want_edge else None
    call("rsu_components_label", hu.ptr(prob_t), float(threshold), connectivity, int(invert), hu.ptr(labels), hu.ptr(area), hu.ptr(edge),
         hu.ptr(ws), shape[0], shape[1], shape[2], hu.stream())
    return labels, area, edge


def run_filter(prob_t, connectivity, min_area, max_hole, shape, in_place=False, want_stats=True, ws=None, threshold=THRESHOLD):
    """(out, stats or None) as device tensors; in_place: out is prob_t itself"""
    import torch
    from road_segmentation_unet_amd._lib import call
    from tests import hiputil as hu
    ws = new_ws(shape) if ws is None else ws
    out = prob_t if in_place else torch.full(shape, float("nan"), dtype=torch.float32, device=hu.DEV)
    stats = torch.full((shape[0], 6), -7, dtype=torch.int64, device=hu.DEV) if want_stats else None
    call("rsu_components_filter", hu.ptr(prob_t), float(threshold), connectivity, int(min_area), int(max_hole), hu.ptr(out), hu.ptr(stats),
         hu.ptr(ws), shape[0], shape[1], shape[2], hu.stream())
    return out, stats


def run_pair_count(prob_t, labels_t, connectivity, shape, acc=None, ws=None, threshold=THRESHOLD):
    """acc (int64 [4] on the device; a new zeroed one when not given) after one more rsu_components_pair_count"""
    import torch
    from road_segmentation_unet_amd._lib import call
    from tests import hiputil as hu
    ws = new_ws(shape) if ws is None else ws
    acc = torch.zeros(4, dtype=torch.int64, device=hu.DEV) if acc is None else acc
    call("rsu_components_pair_count", hu.ptr(prob_t), float(threshold), hu.ptr(labels_t), connectivity, hu.ptr(acc), hu.ptr(ws), shape[0],
         shape[1], shape[2], hu.stream())
    return acc


def pair_labels(shape, seed=17):
    """int64 labels [N, H, W]: blobs of road, about 8 % ignored (-1, 2 and 1 << 32, whose low 32 bits are a valid label) and, with more
    than one image, the last image ignored altogether (the padding of an evaluation chunk)"""
    rng = np.random.RandomState(seed)
    lab = (rng.random_sample(shape) < 0.5).astype(np.int64)
    r = rng.random_sample(shape)
    lab[r < 0.08] = -1
    lab[r < 0.05] = 2
    lab[r < 0.02] = 1 << 32
    if shape[0] > 1:
        lab[-1] = -1
    return lab
