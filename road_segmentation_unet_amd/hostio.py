"""Host-side data formats either side of the hot path (SURVEY.md section 8(f) "next" rows 2 and 3): PNG loading, the
offline rotation augmentation, mask quantisation and the Kaggle submission CSV. Plain numpy/scipy/PIL, off the timed path;
each function cites the reference lines it mirrors (/root/reference/src/images.py)."""
import glob
import os

import numpy as np

FOREGROUND_THRESHOLD = .25  # src/constants.py:1
IMG_PATCH_SIZE = 16         # src/constants.py:2
PIXEL_DEPTH = 255           # src/constants.py:5


def img_float_to_uint8(img):
    """images.py:19-21"""
    return (np.asarray(img) * PIXEL_DEPTH).round().astype(np.uint8)


def load(directory):
    """images.py:24-32: every *.png of `directory`, sorted, as float32 in [0,1]: [n, H, W(, C)]"""
    from PIL import Image
    out = []
    for path in sorted(glob.glob(os.path.join(directory, '*.png'))):
        a = np.asarray(Image.open(path))
        out.append(a.astype(np.float32) / (65535.0 if a.dtype == np.uint16 else 255.0))
    print("Loaded {} images from {}".format(len(out), directory))
    shapes = sorted({a.shape for a in out})
    if len(shapes) > 1:
        raise ValueError("the images of {} differ in shape ({}): one call handles images of one common shape, put each shape into a "
                         "directory of its own".format(directory, ", ".join("x".join(str(d) for d in sh) for sh in shapes)))
    return np.asarray(out)


def load_train_data(directory):
    """images.py:240-253"""
    return load(os.path.abspath(os.path.join(directory, 'images/'))), load(os.path.abspath(os.path.join(directory, 'groundtruth/')))


def mirror_border(images, n):
    """images.py:269-281 (numpy 'symmetric' pad)"""
    pad = ((0, 0), (n, n), (n, n)) + (((0, 0),) if images.ndim == 4 else ())
    return np.pad(images, pad, "symmetric")


def tile_origins(length, patch_size, stride):
    """The prediction tiles' origins along one axis (include/rsu.h rsu_tile_grid): 0, stride, 2 stride, ... while origin + patch_size <=
    length and, where (length - patch_size) % stride != 0, one more tile at length - patch_size: the clamped last tile. An axis with
    (length - patch_size) % stride == 0 has the reference's grid, range(0, length - patch_size + 1, stride)."""
    length, patch_size, stride = int(length), int(patch_size), int(stride)
    if patch_size < 1 or stride < 1:
        raise ValueError("tile_origins: patch_size %d and stride %d must be at least 1" % (patch_size, stride))
    if length < patch_size:
        raise ValueError("tile_origins: a side of %d pixels is shorter than --patch_size=%d" % (length, patch_size))
    origins = list(range(0, length - patch_size + 1, stride))
    if origins[-1] != length - patch_size:
        origins.append(length - patch_size)
    return origins


def extract_patches(images, patch_size, stride=None, predict_patch_size=None):
    """images.py:35-85 (host version for the training pool; the prediction path uses the fused device kernel)"""
    if not predict_patch_size:
        predict_patch_size = patch_size
    assert (patch_size - predict_patch_size) % 2 == 0 and predict_patch_size <= patch_size
    if not stride:
        stride = patch_size
    n, h, w = images.shape[:3]
    assert h == w, "Assume square images"
    assert (h - patch_size) % stride == 0, "Stride sliding should cover the whole image"
    starts = range(0, h - patch_size + 1, stride)
    out = np.zeros((n * len(starts) ** 2, patch_size, patch_size) + images.shape[3:])
    k = 0
    for i in range(n):
        for x in starts:          # x outer
            for y in starts:      # y inner
                out[k] = images[i, y:y + patch_size, x:x + patch_size]
                k += 1
    return out


def expand_and_rotate(imgs, angles, offset=0):
    """images.py:320-351: mirror-pad by ceil(h(sqrt2-1)/2) + ceil(offset/sqrt2), rotate every image by each angle with
    nearest-neighbour resampling (scipy.ndimage.rotate order=0, angle 0 skipped), centre-crop to h + 2*offset."""
    from scipy.ndimage import rotate
    has_channels = imgs.ndim == 4
    if not has_channels:
        imgs = imgs[..., None]
    b, h, w, c = imgs.shape
    assert h == w
    out_size = h + 2 * offset
    assert out_size % 2 == 0
    padding = int(np.ceil(h * (np.sqrt(2) - 1) / 2)) + int(np.ceil(offset / np.sqrt(2)))
    print("Applying rotations: {} degrees... ".format(", ".join(str(a) for a in angles)))
    padded = mirror_border(imgs, padding)
    res = np.zeros((b * len(angles), out_size, out_size, c))
    for i, angle in enumerate(angles):
        r = padded if angle == 0 else rotate(padded, angle=angle, axes=(1, 2), order=0)
        ctr, half = r.shape[1] // 2, out_size // 2
        res[i * b:(i + 1) * b] = r[:, ctr - half:ctr + half, ctr - half:ctr + half]
    return res if has_channels else res[..., 0]


def quantize_mask(masks, threshold, patch_size):
    """images.py:256-266: per patch_size block, label = mean(mask >= 0.5) > threshold"""
    out = masks.copy()
    n, height, width = masks.shape[:3]
    for y in range(0, height, patch_size):
        for x in range(0, width, patch_size):
            lab = (masks[:, y:y + patch_size, x:x + patch_size, 0] >= 0.5).reshape(n, -1).mean(axis=1) > threshold
            out[:, y:y + patch_size, x:x + patch_size, 0] = lab[:, None, None]
    return out


def labels_for_patches(patches):
    """images.py:88-99"""
    return (patches.mean(axis=(1, 2)) > FOREGROUND_THRESHOLD).astype(np.int64)


def submission_rows(masks, patch_size=IMG_PATCH_SIZE):
    """body of images.save_submission_csv (images.py:206-237): '{img:03d}_{x}_{y},{label}' with x the outer index. masks [n, H, W(, 1)]
    with H and W multiples of patch_size (ValueError otherwise); H != W gives (W / patch_size) x (H / patch_size) rows per image."""
    if masks.ndim == 4:
        masks = masks.squeeze(-1)
    n, h, w = masks.shape
    if h < patch_size or w < patch_size or h % patch_size or w % patch_size:
        raise ValueError("submission rows need masks whose sides are multiples of %d, not %d x %d" % (patch_size, h, w))
    nx, ny = w // patch_size, h // patch_size
    if h == w:
        patches = extract_patches(masks, patch_size)
    else:   # extract_patches' order and float64 patches on a rectangle
        patches = np.zeros((n * nx * ny, patch_size, patch_size))
        for k in range(n):
            for j in range(nx):
                for i in range(ny):
                    patches[(k * nx + j) * ny + i] = masks[k, i * patch_size:(i + 1) * patch_size, j * patch_size:(j + 1) * patch_size]
    labels = labels_for_patches(patches).reshape(n, nx, ny)
    return ["{:03d}_{}_{},{}".format(k + 1, patch_size * j, patch_size * i, labels[k, j, i])
            for k in range(n) for j in range(nx) for i in range(ny)]


def save_submission_csv(masks, path, patch_size=IMG_PATCH_SIZE):
    os.makedirs(path, exist_ok=True)
    filename = os.path.abspath(os.path.join(path, "submission.csv"))
    with open(filename, "w") as f:
        print("Saving predictions in {}".format(filename))
        f.write("id,prediction\n")
        for r in submission_rows(masks, patch_size):
            f.write(r + "\n")
    return filename


def overlays(imgs, masks, fade=0.95):
    """Road masks painted in red over the aerial images (the reference's images.overlays, images.py:102-128): per image one
    PIL alpha-composite of an RGBA layer (red, alpha = 255 * mask * fade, truncated to uint8) onto the RGB image made opaque.
    imgs [n, H, W, 3] float in [0, 1], masks [n, H, W(, 1)] -> uint8 [n, H, W, 4]."""
    from PIL import Image
    pictures = img_float_to_uint8(np.asarray(imgs))
    if pictures.ndim != 4 or pictures.shape[-1] != 3:
        raise AssertionError('Predict image should be colored')
    n, height, width = pictures.shape[:3]
    alpha = (img_float_to_uint8(np.asarray(masks).reshape(n, height, width)) * fade).astype(np.uint8)

    def painted(k):
        layer = np.zeros((height, width, 4), dtype=np.uint8)
        layer[..., 0] = 255
        layer[..., 3] = alpha[k]
        base = Image.fromarray(pictures[k]).convert("RGBA")
        return np.asarray(Image.alpha_composite(base, Image.fromarray(layer)))

    return np.stack([painted(k) for k in range(n)]) if n else np.zeros((0, height, width, 4), dtype=np.uint8)


def overlap_pred_true(pred, true):
    """images.py:282-293: prediction in the red, ground truth in the green channel"""
    pred, true = np.asarray(pred), np.asarray(true)
    num_images, im_height, im_width = pred.shape
    out = np.zeros((num_images, im_height, im_width, 3), dtype=np.uint8)
    out[:, :, :, 0] = img_float_to_uint8(pred)
    out[:, :, :, 1] = img_float_to_uint8(true)
    return out


def overlapp_error(pred, true):
    """images.py:296-309: white where prediction and ground truth agree"""
    pred, true = np.asarray(pred), np.asarray(true)
    num_images, im_height, im_width = pred.shape
    agree = np.logical_not(np.logical_xor(img_float_to_uint8(true).astype(bool), img_float_to_uint8(pred).astype(bool)))
    err = img_float_to_uint8(agree * 1)
    return np.repeat(err[..., None], 3, axis=-1)


def save_all(images, directory, format_="images_{:03d}.png", greyscale=False):
    """images.py:185-205 (matplotlib.image.imsave: 2-D arrays go through the colour map, normalised to their own range)"""
    import matplotlib as mpl
    import matplotlib.image as mpimg
    images = np.asarray(images)
    os.makedirs(directory, exist_ok=True)
    if images.ndim == 4 and images.shape[-1] == 1:
        images = images.squeeze(-1)
    cmap = "gray" if greyscale else mpl.rcParams.get("image.cmap")
    for n in range(images.shape[0]):
        mpimg.imsave(os.path.join(directory, format_.format(n + 1)), images[n], cmap=cmap)


def img_to_label_patches(img, patch_size=IMG_PATCH_SIZE):
    """summary.py:134-139 on the host, quirk included: the [n] label vector resized in place to [n, ps, ps] (zero filled)"""
    lab = labels_for_patches(extract_patches(np.asarray(img), patch_size))
    out = np.zeros(lab.shape[0] * patch_size * patch_size, dtype=lab.dtype)
    out[:lab.shape[0]] = lab
    return out.reshape(lab.shape[0], patch_size, patch_size)


def split_validation(images, groundtruth, k):
    """Hold out the LAST k training images, whole: ((train images, train ground truth), (held-out images, held-out ground truth)).
    Whole images, because the training patches of one image overlap at --stride: a patch held out on its own shares most of its
    pixels with patches that stay. k == 0 holds out nothing (the second pair is None); k must leave at least one training image."""
    k, n = int(k), len(images)
    if len(groundtruth) != n:
        raise ValueError("%d images but %d ground-truth masks" % (n, len(groundtruth)))
    if k < 0 or (k > 0 and k >= n):
        raise ValueError("--validation_images=%d must be >= 0 and leave at least one of the %d training images" % (k, n))
    if k == 0:
        return (images, groundtruth), None
    return (images[:n - k], groundtruth[:n - k]), (images[n - k:], groundtruth[n - k:])


def validation_patches(images, groundtruth, input_size, patch_size):
    """The validation set of held-out images: the images mirror-expanded like the training images (expand_and_rotate at angle 0 is
    mirror_border by (input_size - patch_size) / 2) but not rotated, tiled WITHOUT overlap (stride = patch_size, extract_patches and
    its x-outer order). H // patch_size tiles per axis, centred; the H % patch_size border pixels belong to no tile (they still feed
    the tiles' context). Returns (patches float32 [n, input_size, input_size, 3], labels int64 [n, patch_size, patch_size] binarised
    at 0.5); label tile k is groundtruth[i, y:y + patch_size, x:x + patch_size] of the tile's own (i, x, y)."""
    images, groundtruth = np.asarray(images), np.asarray(groundtruth)
    assert (input_size - patch_size) % 2 == 0 and patch_size <= input_size
    n, h = images.shape[0], images.shape[1]
    if groundtruth.shape[:3] != images.shape[:3]:
        raise ValueError("images %s and ground truth %s differ in shape" % (images.shape[:3], groundtruth.shape[:3]))
    per_axis = h // patch_size
    if n < 1 or per_axis < 1:
        raise ValueError("validation needs at least one image of at least patch_size = %d pixels (got %d of %d)" % (patch_size, n, h))
    offset, span = (input_size - patch_size) // 2, per_axis * patch_size
    c0 = (h - span) // 2
    expanded = mirror_border(images, offset)[:, c0:c0 + span + 2 * offset, c0:c0 + span + 2 * offset]
    patches = extract_patches(expanded, patch_size=input_size, predict_patch_size=patch_size, stride=patch_size)
    labels = extract_patches(groundtruth[:, c0:c0 + span, c0:c0 + span], patch_size=patch_size, stride=patch_size)
    return patches.astype(np.float32), (labels >= 0.5).astype(np.int64)


BORDER_D2_INF = 0x7fffffff   # include/rsu.h RSU_BORDER_D2_INF


def _f32_bits(u):
    return np.array(u, dtype=np.uint32).view(np.float32)[()]


def _border_exp(t):
    """exp(t) for a float32 array t <= 0, by the sequence of float32 operations rsu_border_map's kernel runs (csrc/border_map.hip bm_exp;
    numpy rounds every float32 operation on its own, as that file is compiled to do): bit for bit the device's values."""
    t = np.asarray(t, dtype=np.float32)
    tt = np.maximum(t, np.float32(-87.0))
    k = np.rint(tt * _f32_bits(0x3fb8aa3b))                      # log2(e)
    r = tt - k * _f32_bits(0x3f317200)                           # ln2, high part
    r = r - k * _f32_bits(0x35bfbe8e)                            # ln2, low part
    p = np.full_like(r, _f32_bits(0x39500d01))                   # 1/5040
    for c in (_f32_bits(0x3ab60b61), _f32_bits(0x3c088889), _f32_bits(0x3d2aaaab), _f32_bits(0x3e2aaaab), np.float32(0.5),
              np.float32(1.0), np.float32(1.0)):                 # 1/720, 1/120, 1/24, 1/6, 1/2, 1, 1
        p = p * r + c
    scale = ((k.astype(np.int32) + 127) << 23).astype(np.uint32).view(np.float32)
    return np.where(t < np.float32(-87.0), np.float32(0.0), p * scale).astype(np.float32)


def border_weight_map(labels, w0, sigma, mul=None):
    """The border-distance weight map of the loss, on the host: the CPU statement of include/rsu.h rsu_border_map (what --border_weight
    computes on the device per batch). labels: integer [N, H, W] (or [H, W]); per tile, PATCH-LOCAL:
      a label is valid if it is 0 or 1; D2(p) = the exact squared Euclidean distance of a valid pixel to the nearest valid pixel of the
      other class in its tile (BORDER_D2_INF where the tile has none); border(p) = 1 + w0 exp(-D2(p) / (2 sigma^2)) in float32, exactly 1
      where D2 is infinite; out = (mul if given else 1) * border for a valid pixel; an ignored pixel (any other label) has out = +0 and
      d2 = BORDER_D2_INF, is nobody's other class, and its `mul` is never used (it may be NaN).
    Returns (out float32, d2 int32), shaped like labels. Separable: nearest valid pixel of each class per column (running maxima down and
    up), then per row min over x' of (x - x')^2 + g(x')^2. The float32 arithmetic is the device kernel's, operation for operation: out
    equals rsu_border_map's bit for bit."""
    lab = np.asarray(labels)
    shape = lab.shape
    if lab.ndim == 2:
        lab = lab[None]
    if lab.ndim != 3 or lab.dtype.kind not in "iu":
        raise ValueError("border_weight_map: labels must be an integer array [N, H, W] or [H, W], not %s %s" % (lab.dtype, shape))
    w0f, sf = np.float32(w0), np.float32(sigma)
    if not (np.isfinite(w0f) and w0f >= 0 and np.isfinite(sf) and sf > 0):
        raise ValueError("border_weight_map: w0 must be finite and >= 0, sigma finite and > 0 (got %r, %r)" % (w0, sigma))
    N, H, W = lab.shape
    big = np.int64(1) << 40
    ys = np.arange(H, dtype=np.int64)[None, :, None]
    sq = []   # per class: squared vertical distance to the nearest valid pixel of that class in the column (big where none)
    for c in (0, 1):
        m = lab == c
        above = np.maximum.accumulate(np.where(m, ys, -big), axis=1)                      # the down sweep
        below = np.minimum.accumulate(np.where(m, ys, big)[:, ::-1], axis=1)[:, ::-1]     # the up sweep
        g = np.minimum(ys - above, below - ys)
        sq.append(np.where(g < big // 2, g * g, big))
    xs = np.arange(W, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2                                                # [x][x']
    d2 = np.full((N, H, W), BORDER_D2_INF, dtype=np.int64)
    rows = max(1, (1 << 22) // max(1, W * W))
    for n in range(N):
        for y0 in range(0, H, rows):
            sl = slice(y0, min(H, y0 + rows))
            for c in (0, 1):   # pixels of class c look at the other class's column distances
                best = (sq[1 - c][n, sl][:, None, :] + dx2[None]).min(axis=2)
                d2[n, sl] = np.where((lab[n, sl] == c) & (best < big), best, d2[n, sl])
    valid = (lab == 0) | (lab == 1)
    finite = d2 < BORDER_D2_INF
    c = np.float32(-1.0 / (2.0 * float(sf) * float(sf)))
    e = _border_exp(np.where(finite, d2, 0).astype(np.float32) * c)
    border = np.where(finite, np.float32(1.0) + w0f * e, np.float32(1.0)).astype(np.float32)
    if mul is not None:
        mulf = np.asarray(mul, dtype=np.float32).reshape(lab.shape)
        with np.errstate(invalid="ignore"):
            border = np.where(valid, mulf, np.float32(1.0)) * border
    out = np.where(valid, border, np.float32(0.0)).astype(np.float32)
    return out.reshape(shape), d2.astype(np.int32).reshape(shape)


# include/rsu.h rsu_affine_t as a numpy record (32 bytes) and the bounds rsu_affine_patches checks
AFFINE_DTYPE = np.dtype([("image", "<i4"), ("cy", "<f4"), ("cx", "<f4"), ("m00", "<f4"), ("m01", "<f4"), ("m10", "<f4"), ("m11", "<f4"),
                         ("pad_", "<i4")])
AFFINE_MAX_M, AFFINE_MAX_CENTRE = 64.0, float(1 << 22)


def affine_records(recs):
    """recs as an AFFINE_DTYPE array [n]: such an array itself, or a sequence of (image, cy, cx, m00, m01, m10, m11)"""
    if isinstance(recs, np.ndarray) and recs.dtype == AFFINE_DTYPE:
        return np.ascontiguousarray(recs.reshape(-1))
    out = np.zeros(len(recs), dtype=AFFINE_DTYPE)
    for k, r in enumerate(recs):
        out[k] = tuple(r)[:7] + (0,)
    return out


def _affine_offsets(n):
    """the output offsets from the centre of an [n][n] output, (n - 1) / 2: (di [n][1], dj [1][n]) float32"""
    d = np.arange(n, dtype=np.float32) - np.float32(n - 1) * np.float32(0.5)
    return d[:, None], d[None, :]


def _affine_source(rec, n, offset, Hl):
    """per pixel of an [n][n] output centred at (n - 1) / 2: the reflected tap rows y0, y1 and columns x0, x1 ([n][n] int64) and the
    fractions fy, fx ([n][n] float32), by the float32 operations of csrc/affine_patches.hip ap_source, one numpy operation each"""
    return _affine_source_tail(rec, *_affine_offsets(n), offset, Hl)


def _affine_source_tail(rec, di, dj, offset, Hl):
    """_affine_source from the output offsets (di, dj) on (csrc/affine_patches.hip ap_source_tail): the rule of rsu_affine_patches from
    "sy =" on, which rsu_elastic_patches enters with displaced offsets"""
    f = np.float32
    off = f(offset)
    sy = (f(rec["cy"]) - off) + (f(rec["m00"]) * di + f(rec["m01"]) * dj)
    sx = (f(rec["cx"]) - off) + (f(rec["m10"]) * di + f(rec["m11"]) * dj)
    ty, tx = np.floor(sy), np.floor(sx)
    fy, fx = sy - ty, sx - tx

    def reflect(t):
        m = np.mod(t, 2 * Hl)   # (numpy's mod is the floored one: ((t % 2Hl) + 2Hl) % 2Hl of C)
        return np.where(m < Hl, m, 2 * Hl - 1 - m)
    ty, tx = ty.astype(np.int64), tx.astype(np.int64)
    return reflect(ty), reflect(ty + 1), reflect(tx), reflect(tx + 1), fy.astype(np.float32), fx.astype(np.float32)


def _affine_lerp(v00, v01, v10, v11, fy, fx):
    gy, gx = np.float32(1.0) - fy, np.float32(1.0) - fx
    return (v00 * gx + v01 * fx) * gy + (v10 * gx + v11 * fx) * fy


def _affine_check(what, images, labels, recs, S, P):
    """what rsu_affine_patches refuses, for the mirror `what` (recs: a record array with AFFINE_DTYPE's fields): ValueError, or
    (images, labels as arrays, offset)"""
    img = np.asarray(images)
    lab = np.asarray(labels)
    if img.ndim != 4 or img.shape[3] != 3 or img.shape[1] != img.shape[2] or lab.ndim != 3 or lab.shape[1] != lab.shape[2] \
            or lab.shape[0] != img.shape[0] or img.dtype != np.float32:
        raise ValueError("%s: images must be float32 [n, He, He, 3] and labels [n, Hl, Hl], not %s %s and %s"
                         % (what, img.dtype, img.shape, lab.shape))
    nimg, He, Hl = img.shape[0], img.shape[1], lab.shape[1]
    if P < 1 or S < P or He < Hl or (He - Hl) % 2 or (S - P) % 2 or He - Hl != S - P:
        raise ValueError("%s: He - Hl = %d and S - P = %d must be even and equal, with S >= P >= 1" % (what, He - Hl, S - P))
    if recs.size < 1:
        raise ValueError("%s: no records" % what)
    vals = np.stack([recs[k] for k in ("cy", "cx", "m00", "m01", "m10", "m11")], axis=1)
    if not np.all(np.isfinite(vals)) or np.abs(vals[:, 2:]).max() > AFFINE_MAX_M or np.abs(vals[:, :2]).max() > AFFINE_MAX_CENTRE \
            or recs["image"].min() < 0 or recs["image"].max() >= nimg:
        raise ValueError("%s: every record needs an image in [0, %d), finite fields, |m| <= 64 and a centre within 2^22" % (what, nimg))
    return img, lab, (He - Hl) // 2


def affine_patches(images, labels, recs, S, P):
    """The one-launch batch loader on the host: the numpy float32 statement of include/rsu.h rsu_affine_patches, operation for operation
    (numpy rounds every float32 operation on its own, as csrc/affine_patches.hip is compiled to do): x and labels equal the device's bit
    for bit. images: float32 [nimg, He, He, 3], the mirror-extended images; labels: [nimg, Hl, Hl] in {0, 1}; recs: an AFFINE_DTYPE array
    or a sequence of (image, cy, cx, m00, m01, m10, m11), with (cy, cx) the window's centre in the extended image (row, column) and
    M = [[m00, m01], [m10, m11]] mapping an output offset to a source offset. Every tap is reflected about the ORIGINAL image's edges
    (symmetric padding, repeated). Returns (x float32 [n, S, S, 3], labels int64 [n, P, P]). ValueError for what the ABI refuses."""
    S, P = int(S), int(P)
    recs = affine_records(recs)
    img, lab, offset = _affine_check("affine_patches", images, labels, recs, S, P)
    Hl = lab.shape[1]
    labf = lab.astype(np.float32)
    x = np.empty((recs.size, S, S, 3), np.float32)
    y = np.empty((recs.size, P, P), np.int64)
    for k, rec in enumerate(recs):
        n = int(rec["image"])
        y0, y1, x0, x1, fy, fx = _affine_source(rec, S, offset, Hl)
        im = img[n, offset:offset + Hl, offset:offset + Hl]   # (index + offset) of the extended image
        x[k] = _affine_lerp(im[y0, x0], im[y0, x1], im[y1, x0], im[y1, x1], fy[..., None], fx[..., None])
        y0, y1, x0, x1, fy, fx = _affine_source(rec, P, offset, Hl)
        lf = labf[n]
        y[k] = _affine_lerp(lf[y0, x0], lf[y0, x1], lf[y1, x0], lf[y1, x1], fy, fx) >= np.float32(0.5)
    return x, y


# include/rsu.h rsu_jitter_t as a numpy record (80 bytes) and the bounds rsu_color_jitter checks
JITTER_DTYPE = np.dtype([("a", "<f4", (9,)), ("k", "<f4", (9,)), ("sigma", "<f4"), ("key", "<u4")])
JITTER_MAX_AK = 64.0
JITTER_NOISE_SCALE = np.uint32(0x37ddb3d7).view(np.float32)   # 1 / sqrt((65536^2 - 1) / 3), the Irwin-Hall sum's standard deviation


def jitter_records(recs):
    """recs as a JITTER_DTYPE array [n]: such an array itself, or a sequence of (A [3][3] or [9], K likewise, sigma, key)"""
    if isinstance(recs, np.ndarray) and recs.dtype == JITTER_DTYPE:
        return np.ascontiguousarray(recs.reshape(-1))
    out = np.zeros(len(recs), dtype=JITTER_DTYPE)
    for j, (a, k, sigma, key) in enumerate(recs):
        out[j] = (np.asarray(a, dtype=np.float32).reshape(9), np.asarray(k, dtype=np.float32).reshape(9), sigma, int(key) & 0xffffffff)
    return out


def _jitter_mix(v):
    """the murmur3 finaliser on a uint32 array (csrc/color_jitter.hip cj_mix; products wrap modulo 2^32)"""
    v = v ^ (v >> np.uint32(16))
    v = v * np.uint32(0x85ebca6b)
    v = v ^ (v >> np.uint32(13))
    v = v * np.uint32(0xc2b2ae35)
    return v ^ (v >> np.uint32(16))


def jitter_noise_int(key, count):
    """n of include/rsu.h rsu_color_jitter for the elements e = 0 .. count - 1 under `key`: uint32 [count], the sum of the four 16-bit
    halves of h1 = mix(e ^ key) and h2 = mix(h1 ^ 0x9e3779b9)"""
    e = np.arange(count, dtype=np.uint32)
    h1 = _jitter_mix(e ^ np.uint32(int(key) & 0xffffffff))
    h2 = _jitter_mix(h1 ^ np.uint32(0x9e3779b9))
    m = np.uint32(0xffff)
    return (h1 & m) + (h1 >> np.uint32(16)) + (h2 & m) + (h2 >> np.uint32(16))


def color_jitter(x, recs):
    """Per-sample colour jitter and noise on the host: the numpy float32 statement of include/rsu.h rsu_color_jitter, operation for
    operation (numpy rounds every float32 operation on its own, as csrc/color_jitter.hip is compiled to do; the means come from exact
    int64 sums): the result equals the device's bit for bit. x: float32 [n, S, S, 3]; recs: a JITTER_DTYPE array or a sequence of
    (A, K, sigma, key), one per sample. Returns a new float32 array; x is left as it is. ValueError for what the ABI refuses."""
    xs = np.asarray(x)
    if xs.ndim != 4 or xs.shape[3] != 3 or xs.shape[1] != xs.shape[2] or xs.dtype != np.float32 or xs.shape[0] < 1 or xs.shape[1] < 1:
        raise ValueError("color_jitter: x must be float32 [n, S, S, 3] with n, S >= 1, not %s %s" % (xs.dtype, xs.shape))
    recs = jitter_records(recs)
    if recs.size != xs.shape[0]:
        raise ValueError("color_jitter: %d records for %d samples" % (recs.size, xs.shape[0]))
    ak = np.concatenate([recs["a"], recs["k"]], axis=1)
    if not np.all(np.isfinite(ak)) or np.abs(ak).max() > JITTER_MAX_AK or not np.all(np.isfinite(recs["sigma"])) \
            or recs["sigma"].min() < 0.0 or recs["sigma"].max() > 1.0:
        raise ValueError("color_jitter: every record needs finite fields, |a| and |k| <= 64 and sigma in [0, 1]")
    if xs.size * 4 >= 0x7ffffff0:
        raise ValueError("color_jitter: x reaches 2 GiB")
    f = np.float32
    n, S = xs.shape[0], xs.shape[1]
    out = np.empty_like(xs)
    for j, rec in enumerate(recs):
        a, k, sigma = rec["a"], rec["k"], f(rec["sigma"])
        px = xs[j].reshape(S * S, 3)
        x0, x1, x2 = px[:, 0], px[:, 1], px[:, 2]
        m = np.zeros(3, np.float32)
        if np.any(k != 0):
            q = np.rint(np.fmin(np.fmax(px, f(-256.0)), f(256.0)) * f(16777216.0)).astype(np.int64)
            sums = q.sum(axis=0, dtype=np.int64)
            m = (sums.astype(np.float64) / (np.float64(S * S) * 16777216.0)).astype(np.float32)
        g = None
        if sigma > 0:
            g = ((jitter_noise_int(rec["key"], S * S * 3).astype(np.float32) - f(131070.0)) * JITTER_NOISE_SCALE).reshape(S * S, 3)
        y = np.empty((S * S, 3), np.float32)
        for r in range(3):
            d = (k[3 * r] * m[0] + k[3 * r + 1] * m[1]) + k[3 * r + 2] * m[2]
            yr = ((a[3 * r] * x0 + a[3 * r + 1] * x1) + a[3 * r + 2] * x2) + d
            if g is not None:
                yr = yr + sigma * g[:, r]
            y[:, r] = np.fmin(np.fmax(yr, f(0.0)), f(1.0))
        out[j] = y.reshape(S, S, 3)
    return out


# include/rsu.h rsu_elastic_t as a numpy record (48 bytes) and the bounds rsu_elastic_patches checks
ELASTIC_DTYPE = np.dtype([("image", "<i4"), ("cy", "<f4"), ("cx", "<f4"), ("m00", "<f4"), ("m01", "<f4"), ("m10", "<f4"), ("m11", "<f4"),
                          ("alpha", "<f4"), ("key", "<u4"), ("grid", "<i4"), ("pad_", "<i4", (2,))])
ELASTIC_MAX_ALPHA, ELASTIC_MAX_GRID = 64.0, 16
ELASTIC_SIXTH = np.uint32(0x3e2aaaab).view(np.float32)   # 1 / 6 rounded: the spline's weights are products, not quotients


def elastic_records(recs):
    """recs as an ELASTIC_DTYPE array [n]: such an array itself, or a sequence of (image, cy, cx, m00, m01, m10, m11, alpha, key, grid)"""
    if isinstance(recs, np.ndarray) and recs.dtype == ELASTIC_DTYPE:
        return np.ascontiguousarray(recs.reshape(-1))
    out = np.zeros(len(recs), dtype=ELASTIC_DTYPE)
    for k, r in enumerate(recs):
        r = tuple(r)
        out[k] = r[:8] + (int(r[8]) & 0xffffffff, r[9], (0, 0))
    return out


def elastic_lattice(key, alpha, G):
    """The control lattice of include/rsu.h rsu_elastic_patches: float32 [G + 3][G + 3][2], component `axis` of point (a, b) = alpha * g
    with g the noise value of rsu_color_jitter for the element index (a * 32 + b) * 2 + axis under `key`"""
    G = int(G)
    a, b, axis = np.meshgrid(np.arange(G + 3, dtype=np.uint32), np.arange(G + 3, dtype=np.uint32), np.arange(2, dtype=np.uint32), indexing="ij")
    e = (a * np.uint32(32) + b) * np.uint32(2) + axis
    h1 = _jitter_mix(e ^ np.uint32(int(key) & 0xffffffff))
    h2 = _jitter_mix(h1 ^ np.uint32(0x9e3779b9))
    m = np.uint32(0xffff)
    n = (h1 & m) + (h1 >> np.uint32(16)) + (h2 & m) + (h2 >> np.uint32(16))
    g = (n.astype(np.float32) - np.float32(131070.0)) * JITTER_NOISE_SCALE
    return (np.float32(alpha) * g).astype(np.float32)


def elastic_weights(f):
    """the four cubic B-spline weights of the fractions f (float32 array): float32 [4] + f.shape, in the order of operations rsu.h states"""
    f = np.asarray(f, dtype=np.float32)
    one, three = np.float32(1.0), np.float32(3.0)
    g1, f2 = one - f, f * f
    f3 = f2 * f
    return np.stack([((g1 * g1) * g1) * ELASTIC_SIXTH,
                     ((three * f3 - np.float32(6.0) * f2) + np.float32(4.0)) * ELASTIC_SIXTH,
                     (((three * f2 - three * f3) + three * f) + one) * ELASTIC_SIXTH,
                     f3 * ELASTIC_SIXTH]).astype(np.float32)


def _elastic_axis(S, G):
    """per window pixel index 0 .. S - 1 of one axis: (cell k int64 [S] in [0, G - 1], weights float32 [4][S])"""
    q = np.float32(np.float64(G) / np.float64(S))
    t = (np.arange(S, dtype=np.float32) + np.float32(0.5)) * q
    k = np.clip(np.floor(t).astype(np.int64), 0, G - 1)
    return k, elastic_weights(t - k.astype(np.float32))


def elastic_field(lattice, S):
    """The displacement field of include/rsu.h rsu_elastic_patches over an input window of S pixels: float32 [2][S][S], [axis][iw][jw], the
    uniform cubic B-spline over `lattice` (float32 [G + 3][G + 3][2], elastic_lattice) with both sums in index order, one numpy operation
    per float32 operation of the kernel"""
    lat = np.asarray(lattice, dtype=np.float32)
    if lat.ndim != 3 or lat.shape[0] != lat.shape[1] or lat.shape[2] != 2 or not 1 <= lat.shape[0] - 3 <= ELASTIC_MAX_GRID or int(S) < 1:
        raise ValueError("elastic_field: lattice must be [G + 3, G + 3, 2] with G in [1, 16] and S >= 1, not %s and %r" % (lat.shape, S))
    S, G = int(S), lat.shape[0] - 3
    k, w = _elastic_axis(S, G)
    ky, kx = k[:, None], k[None, :]
    wy, wx = w[:, :, None], w[:, None, :]
    u = np.empty((2, S, S), np.float32)
    for axis in range(2):
        c = lat[:, :, axis]
        row = [((wx[0] * c[ky + a, kx] + wx[1] * c[ky + a, kx + 1]) + wx[2] * c[ky + a, kx + 2]) + wx[3] * c[ky + a, kx + 3] for a in range(4)]
        u[axis] = ((wy[0] * row[0] + wy[1] * row[1]) + wy[2] * row[2]) + wy[3] * row[3]
    return u


def elastic_patches(images, labels, recs, S, P):
    """The one-launch batch loader with elastic deformation on the host: the numpy float32 statement of include/rsu.h rsu_elastic_patches,
    operation for operation: x and labels equal the device's bit for bit. images, labels, S, P as affine_patches; recs: an ELASTIC_DTYPE
    array or a sequence of (image, cy, cx, m00, m01, m10, m11, alpha, key, grid). Input pixel (i, j) is displaced by the field at (i, j),
    label pixel (i, j) by the field at (i + offset, j + offset): the centre crop of the same field. Returns (x float32 [n, S, S, 3],
    labels int64 [n, P, P]). ValueError for what the ABI refuses."""
    S, P = int(S), int(P)
    recs = elastic_records(recs)
    img, lab, offset = _affine_check("elastic_patches", images, labels, recs, S, P)
    if not np.all(np.isfinite(recs["alpha"])) or recs["alpha"].min() < 0.0 or recs["alpha"].max() > ELASTIC_MAX_ALPHA \
            or recs["grid"].min() < 1 or recs["grid"].max() > ELASTIC_MAX_GRID:
        raise ValueError("elastic_patches: every record needs a finite alpha in [0, 64] and a grid in [1, 16]")
    Hl = lab.shape[1]
    labf = lab.astype(np.float32)
    x = np.empty((recs.size, S, S, 3), np.float32)
    y = np.empty((recs.size, P, P), np.int64)
    for k, rec in enumerate(recs):
        n = int(rec["image"])
        u = elastic_field(elastic_lattice(rec["key"], rec["alpha"], rec["grid"]), S)
        di, dj = _affine_offsets(S)
        y0, y1, x0, x1, fy, fx = _affine_source_tail(rec, di + u[0], dj + u[1], offset, Hl)
        im = img[n, offset:offset + Hl, offset:offset + Hl]   # (index + offset) of the extended image
        x[k] = _affine_lerp(im[y0, x0], im[y0, x1], im[y1, x0], im[y1, x1], fy[..., None], fx[..., None])
        ul = u[:, offset:offset + P, offset:offset + P]
        di, dj = _affine_offsets(P)
        y0, y1, x0, x1, fy, fx = _affine_source_tail(rec, di + ul[0], dj + ul[1], offset, Hl)
        lf = labf[n]
        y[k] = _affine_lerp(lf[y0, x0], lf[y0, x1], lf[y1, x0], lf[y1, x1], fy, fx) >= np.float32(0.5)
    return x, y


# ---- clDice: the soft skeleton and the centre-line Dice term on the host (include/rsu_cldice.h)
CLDICE_MAX_ITERS = 16   # rsu_cldice.h RSU_CLDICE_MAX_ITERS
_CLDICE_CROSS = ((-1, 0), (0, -1), (0, 0), (0, 1), (1, 0))                       # up, left, centre, right, down
_CLDICE_BOX = tuple((dr, dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1))          # row-major


def _cldice_pick(x, offsets, fill, arg):
    """min (arg = np.argmin) or max (np.argmax) of x [B, H, W] over the window `offsets`; positions outside the image hold `fill`
    and never win. Returns (values, index of the winner in `offsets`): the FIRST of equal candidates, as the kernels decide."""
    B, H, W = x.shape
    pad = np.full((B, H + 2, W + 2), fill, x.dtype)
    pad[:, 1:-1, 1:-1] = x
    win = np.stack([pad[:, 1 + dr:1 + dr + H, 1 + dc:1 + dc + W] for dr, dc in offsets])
    code = arg(win, axis=0)
    return np.take_along_axis(win, code[None], axis=0)[0], code


def _cldice_chain(x, iters):
    """E_0..E_{k+1}, the erosions' and dilations' winners, d_j, S_j and the second ReLU's masks of skel(x), in x's own precision, every
    operation rounded once: E_{j+1} = erode(E_j), O_j = dilate(E_{j+1}), d_j = relu(E_j - O_j), S_j = S_{j-1} + relu(d_j - S_{j-1} d_j)."""
    E, amin, amax, d, S, r = [x], [], [], [], [], []
    zero = x.dtype.type(0)
    for j in range(iters + 1):
        e, c = _cldice_pick(E[j], _CLDICE_CROSS, np.inf, np.argmin)
        E.append(e)
        amin.append(c)
        o, c = _cldice_pick(e, _CLDICE_BOX, -np.inf, np.argmax)
        amax.append(c)
        t = E[j] - o
        d.append(np.where(t > 0, t, zero))
        if j == 0:
            S.append(d[0])
            r.append(None)
        else:
            u = d[j] - S[j - 1] * d[j]
            r.append(u > 0)
            S.append(S[j - 1] + np.where(u > 0, u, zero))
    return E, amin, amax, d, S, r


def _cldice_check_iters(iters):
    if isinstance(iters, bool) or int(iters) != iters or not 0 <= int(iters) <= CLDICE_MAX_ITERS:
        raise ValueError("cldice iterations must be an int in [0, %d], not %r" % (CLDICE_MAX_ITERS, iters))
    return int(iters)


def soft_skeleton(x, iters):
    """The soft skeleton of include/rsu_cldice.h (Shit et al. 2021, soft_skel) of maps x [B, H, W] in numpy float32, the kernels'
    operations in their order with one rounding each: equal to rsu_cldice_fwd's skel_p / skel_y bit for bit. Erosion is the min over the
    cross, dilation the max over the 3 x 3 box; positions outside an image do not exist."""
    x = np.ascontiguousarray(x, np.float32)
    if x.ndim != 3:
        raise ValueError("soft_skeleton: maps [B, H, W], not shape %r" % (x.shape,))
    return _cldice_chain(x, _cldice_check_iters(iters))[4][-1]


def _cldice_route(val, code, offsets):
    """the transpose of a window pick: out[n + offsets[code[n]]] += val[n]"""
    B, H, W = val.shape
    out = np.zeros_like(val)
    for o, (dr, dc) in enumerate(offsets):
        v = np.where(code == o, val, 0.0)
        out[:, max(0, dr):H + min(0, dr), max(0, dc):W + min(0, dc)] += v[:, max(0, -dr):H - max(0, dr), max(0, -dc):W - max(0, dc)]
    return out


def cldice_gradient(prob, labels, iters, scale, smooth, sums=None):
    """The clDice term scale * (1 - clD) of include/rsu_cldice.h in numpy float64 from float32 probabilities [B, H, W] and int64 labels:
    returns (skel_p, skel_y, sums, gprob) with sums = {A, Bp, Cc, Dy} and gprob = d term / d prob, the sub-gradient pinned as the
    kernels pin it: among equal candidates of a window the first in row-major order wins (cross: up, left, centre, right, down),
    relu'(0) = 0. Pixels whose label is neither 0 nor 1 are constants of the skeleton: they take part in the pooling, add nothing to
    the sums and get gprob = 0. sums: None, or four numbers the gradient's factors are formed from in place of the maps' own sums, as
    rsu_cldice_bwd forms them from what it finds in memory (the returned sums stay the maps' own)."""
    k = _cldice_check_iters(iters)
    p = np.ascontiguousarray(prob, np.float64)
    labels = np.asarray(labels)
    if p.ndim != 3 or labels.shape != p.shape:
        raise ValueError("cldice_gradient: prob and labels [B, H, W], not %r and %r" % (p.shape, labels.shape))
    scale, s = float(scale), float(smooth)
    if not (np.isfinite(s) and s > 0.0 and np.isfinite(scale) and scale >= 0.0):
        raise ValueError("cldice_gradient: smooth must be finite and > 0, scale finite and >= 0")
    y = (labels == 1).astype(np.float64)
    m = (labels == 0) | (labels == 1)
    E, amin, amax, d, S, r = _cldice_chain(p, k)
    skel_p, skel_y = S[k], _cldice_chain(y, k)[4][-1]
    A, Bp = float(np.sum(np.where(m, skel_p * y, 0.0))), float(np.sum(np.where(m, skel_p, 0.0)))
    Cc, Dy = float(np.sum(np.where(m, skel_y * p, 0.0))), float(np.sum(np.where(m, skel_y, 0.0)))
    own = np.array([A, Bp, Cc, Dy])
    if sums is not None:
        A, Bp, Cc, Dy = (float(v) for v in sums)
    Tp, Ts = (A + s) / (Bp + s), (Cc + s) / (Dy + s)
    dTp, dTs = 2.0 * Ts * Ts / (Tp + Ts) ** 2, 2.0 * Tp * Tp / (Tp + Ts) ** 2
    gS = np.where(m, -scale * dTp * (y * (Bp + s) - (A + s)) / (Bp + s) ** 2, 0.0)
    a = [None] * (k + 1)              # a_j: the gradient that reaches E_j - O_j through d_j
    for j in range(k, 0, -1):
        a[j] = np.where(r[j] & (d[j] > 0), gS * (1.0 - S[j - 1]), 0.0)
        gS = np.where(r[j], gS * (1.0 - d[j]), gS)
    a[0] = np.where(d[0] > 0, gS, 0.0)
    gE = -_cldice_route(a[k], amax[k], _CLDICE_BOX)                    # wrt E_{k+1}
    for j in range(k, -1, -1):
        gE = a[j] + _cldice_route(gE, amin[j], _CLDICE_CROSS)
        if j > 0:
            gE = gE - _cldice_route(a[j - 1], amax[j - 1], _CLDICE_BOX)
    gprob = np.where(m, gE - scale * dTs * skel_y / (Dy + s), 0.0)
    return skel_p, skel_y, own, gprob


# ---- Lovasz: the Jaccard surrogate on the host (include/rsu_lovasz.h)
LOVASZ_MAX_PIXELS = 1 << 24   # rsu_lovasz.h: H * W


def _lovasz_image(p, lab):
    """one image, flat: (loss float32, g float32 per pixel with its sign and 0 at ignored pixels) -- the operations of rsu_lovasz.h, one
    float32 rounding each"""
    f32 = np.float32
    counted = (lab == 0) | (lab == 1)
    idx = np.nonzero(counted)[0]
    g_pix = np.zeros(p.shape, f32)
    n = idx.size
    if n == 0:
        return f32(0), g_pix
    y = lab[idx].astype(np.int64)
    with np.errstate(invalid="ignore"):
        e = np.abs(y.astype(f32) - p[idx])
    # descending by the unsigned pattern, ties by ascending pixel index: a stable ascending sort of the complemented pattern
    order = np.argsort(~e.view(np.uint32), kind="stable")
    ys = y[order]
    G = int(ys.sum())
    c = np.cumsum(ys)
    k = np.arange(1, n + 1, dtype=np.int64)
    J = f32(1) - (G - c).astype(f32) / (G + k - c).astype(f32)
    g = J - np.concatenate([np.zeros(1, f32), J[:-1]])
    with np.errstate(invalid="ignore", over="ignore"):
        loss = np.sum(e[order] * g, dtype=f32)
    g_pix[idx[order]] = np.where(ys == 1, -g, g)
    return f32(loss), g_pix


def _lovasz_args(prob, labels):
    p = np.ascontiguousarray(prob, np.float32)
    labels = np.asarray(labels)
    if p.ndim != 3 or labels.shape != p.shape:
        raise ValueError("lovasz: prob and labels [B, H, W], not %r and %r" % (p.shape, labels.shape))
    if p.shape[1] * p.shape[2] > LOVASZ_MAX_PIXELS or min(p.shape) < 1:
        raise ValueError("lovasz: 1 <= H * W <= 2^24 and B >= 1, not shape %r" % (p.shape,))
    return p, labels.astype(np.int64)


def lovasz_loss(prob, labels):
    """The per-image Lovasz losses L_b of include/rsu_lovasz.h, float32 [B], from float32 probabilities [B, H, W] and int64 labels: the
    errors |y - p| of the pixels whose label is 0 or 1, ranked by their unsigned bit pattern descending (ties: ascending pixel index),
    times the differences of the Jaccard loss along the ranks. The products are summed by numpy's float32 pairwise sum; the kernels'
    order differs (rsu_lovasz.h), so the two agree within the bound of a float32 sum, not in bits."""
    p, labels = _lovasz_args(prob, labels)
    return np.array([_lovasz_image(p[b].reshape(-1), labels[b].reshape(-1))[0] for b in range(p.shape[0])], np.float32)


def lovasz_gradient(prob, labels, scale, into=None):
    """d (scale / B sum_b L_b) / d prob of include/rsu_lovasz.h in numpy float32, equal to rsu_lovasz_fwd_bwd's gprob bit for bit:
    c = f32(scale) / f32(B), c * g_{r(i)} negated where y = 1, +0 at pixels whose label is neither 0 nor 1 (their p is not looked at).
    into: None, or a float32 array [B, H, W] the gradient is added to (one rounding), as accumulate != 0 does; it is not modified."""
    p, labels = _lovasz_args(prob, labels)
    scale = np.float32(scale)
    if not (np.isfinite(scale) and scale >= 0):
        raise ValueError("lovasz_gradient: scale must be finite and >= 0")
    c = scale / np.float32(p.shape[0])
    out = np.empty(p.shape, np.float32)
    for b in range(p.shape[0]):
        out[b] = (c * _lovasz_image(p[b].reshape(-1), labels[b].reshape(-1))[1]).reshape(p.shape[1:])
    if into is not None:
        into = np.asarray(into, np.float32)
        if into.shape != p.shape:
            raise ValueError("lovasz_gradient: into must have prob's shape")
        out = into + out
    return out


# ---- connected components on the host (include/rsu_components.h)
COMPONENTS_MAX_PIXELS = 1 << 24   # rsu_components.h: H * W
COMPONENTS_TILE = 64              # components.h CC_TILE


def _cc_check(prob, threshold, connectivity):
    p = np.ascontiguousarray(prob, np.float32)
    if p.ndim != 3 or min(p.shape) < 1 or p.shape[1] * p.shape[2] > COMPONENTS_MAX_PIXELS or p.size >= 1 << 31:
        raise ValueError("components: prob [N, H, W] with N, H, W >= 1, H * W <= 2^24 and N * H * W < 2^31, not shape %r" % (p.shape,))
    t = np.float32(threshold)
    if not np.isfinite(t):
        raise ValueError("components: threshold must be finite, not %r" % (threshold,))
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError("components: connectivity must be 4 or 8, not %r" % (connectivity,))
    return p, t


def _cc_foreground(p, t):
    """p >= threshold as one float32 comparison: NaN is background, p == threshold is foreground"""
    with np.errstate(invalid="ignore"):
        return p >= t


def _cc_offsets(connectivity):
    return [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])


def _cc_labels(fg, connectivity):
    """labels int32 [H, W] of one mask: 1 + the smallest row-major index of the pixel's component, 0 at background. A union-find on
    whole arrays: every pixel takes the smallest parent among itself and its neighbours (union), hangs its root under it (link by smaller
    index, np.minimum.at: the order of the updates is immaterial), then every pixel jumps to its root (find / flatten); parents only
    decrease, and the loop ends when a round changes nothing -- then neighbours share a root, and a root is the smallest index it can
    reach."""
    H, W = fg.shape
    n = H * W
    flat = fg.reshape(-1)
    idx = np.nonzero(flat)[0]
    par = np.full(n + 1, n, np.int64)       # background, and the sentinel n, point at n
    par[idx] = idx
    pad = np.full((H + 2, W + 2), n, np.int64)
    nb = [(dy, dx) for dy, dx in _cc_offsets(connectivity)] + [(-dy, -dx) for dy, dx in _cc_offsets(connectivity)]
    while idx.size:
        pad[1:-1, 1:-1] = par[:n].reshape(H, W)
        m = pad[1:-1, 1:-1].copy()
        for dy, dx in nb:
            np.minimum(m, pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W], out=m)
        m = m.reshape(-1)[idx]
        new = par.copy()
        np.minimum.at(new, par[idx], m)
        new[idx] = np.minimum(new[idx], m)
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, par):
            break
        par = new
    return np.where(flat, par[:n] + 1, 0).astype(np.int32).reshape(H, W)


def _cc_area_edge(labels):
    """(area int32, edge uint8) per pixel from the labels of one image"""
    H, W = labels.shape
    flat = labels.reshape(-1)
    counts = np.bincount(flat, minlength=H * W + 1)
    counts[0] = 0
    touches = np.zeros(H * W + 1, bool)
    for line in (labels[0], labels[-1], labels[:, 0], labels[:, -1]):
        touches[line] = True
    touches[0] = False
    return counts[flat].astype(np.int32).reshape(H, W), touches[flat].astype(np.uint8).reshape(H, W)


def label_components(prob, threshold, connectivity, invert=False):
    """rsu_components_label on the host: (labels int32, area int32, edge uint8), each [N, H, W], of the mask p >= threshold (invert: of
    its complement, NaN included) at connectivity 4 or 8; every image on its own."""
    p, t = _cc_check(prob, threshold, connectivity)
    fg = _cc_foreground(p, t)
    if invert:
        fg = ~fg
    labels = np.stack([_cc_labels(fg[n], connectivity) for n in range(p.shape[0])])
    ae = [_cc_area_edge(labels[n]) for n in range(p.shape[0])]
    return labels, np.stack([a for a, _ in ae]), np.stack([e for _, e in ae])


def filter_components(prob, threshold, connectivity, min_area, max_hole):
    """rsu_components_filter on the host: (out float32 [N, H, W], stats int64 [N, 6]) -- components of fewer than min_area pixels removed
    (+0), then the holes (components of the complement at the dual connectivity that touch no image edge) of at most max_hole pixels
    filled (1), every other pixel with the bits it had; stats = {components, components removed, pixels removed, holes, holes filled,
    pixels filled} per image, a skipped step's three fields 0."""
    p, t = _cc_check(prob, threshold, connectivity)
    for name, v in (("min_area", min_area), ("max_hole", max_hole)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError("components: %s must be an integer >= 0, not %r" % (name, v))
    N = p.shape[0]
    f1 = _cc_foreground(p, t)
    removed, filled = np.zeros(p.shape, bool), np.zeros(p.shape, bool)
    stats = np.zeros((N, 6), np.int64)
    for n in range(N):
        if min_area > 1:
            lab = _cc_labels(f1[n], connectivity)
            area, _ = _cc_area_edge(lab)
            removed[n] = (lab > 0) & (area < min_area)
            roots = lab.reshape(-1) == np.arange(1, lab.size + 1)
            stats[n, 0:3] = roots.sum(), (roots & removed[n].reshape(-1)).sum(), removed[n].sum()
        if max_hole > 0:
            lab = _cc_labels(~(f1[n] & ~removed[n]), 4 if connectivity == 8 else 8)
            area, edge = _cc_area_edge(lab)
            hole = (lab > 0) & (edge == 0)
            filled[n] = hole & (area <= max_hole)
            roots = lab.reshape(-1) == np.arange(1, lab.size + 1)
            stats[n, 3:6] = (roots & hole.reshape(-1)).sum(), (roots & filled[n].reshape(-1)).sum(), filled[n].sum()
    bits = p.view(np.uint32).copy()
    bits[removed] = 0
    bits[filled] = 0x3f800000
    return bits.view(np.float32), stats


def components_pair_count(prob, threshold, labels, connectivity):
    """rsu_components_pair_count on the host: int64 [4] = {sum cp, sum cy, sum |cp - cy|, images with a counted pixel}; cp the components of
    {label in {0, 1} and p >= threshold}, cy those of {label == 1}, per image."""
    p, t = _cc_check(prob, threshold, connectivity)
    labels = np.asarray(labels).astype(np.int64)
    if labels.shape != p.shape:
        raise ValueError("components: labels must have prob's shape")
    counted = (labels == 0) | (labels == 1)
    pred = counted & _cc_foreground(p, t)
    acc = np.zeros(4, np.int64)
    for n in range(p.shape[0]):
        cp = len(np.unique(_cc_labels(pred[n], connectivity))) - (0 if pred[n].all() else 1)
        cy = len(np.unique(_cc_labels(labels[n] == 1, connectivity))) - (0 if (labels[n] == 1).all() else 1)
        acc += (cp, cy, abs(cp - cy), int(counted[n].any()))
    return acc


def label_components_tiled(mask, connectivity, tile=COMPONENTS_TILE):
    """The steps of csrc/components.hip on one boolean mask [H, W], serially and in plain Python (slow: for tests): per tile every pixel
    starts at its horizontal run's first pixel and the runs are united with the row above, leaving out the pairs a neighbour of the same
    run makes; the tile roots become image indices with a tile area and edge flag each; at level m the pairs across the two new inner
    borders of every 2^m x 2^m group of tiles are united (link the larger root under the smaller); then every pixel walks to its root
    and the tile roots add their area and edge flag to it. Returns (labels, area, edge, levels)."""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    T = int(tile)
    par = np.zeros(H * W, np.int64)          # parent index + 1, 0 = background
    ta = np.zeros(H * W, np.int64)
    tedge = np.zeros(H * W, bool)

    def find(p, i, off):
        while p[i] - off != i:
            i = p[i] - off
        return i

    def union(p, a, b, off):
        a, b = find(p, a, off), find(p, b, off)
        if a != b:
            p[max(a, b)] = min(a, b) + off

    ty_n, tx_n = -(-H // T), -(-W // T)
    for ty in range(ty_n):
        for tx in range(tx_n):
            y0, x0 = ty * T, tx * T
            f = np.zeros((T, T), bool)
            sub = mask[y0:y0 + T, x0:x0 + T]
            f[:sub.shape[0], :sub.shape[1]] = sub
            lp = np.full(T * T, -1, np.int64)
            for r in range(T):
                start = 0
                for c in range(T):
                    if not f[r, c]:
                        start = c + 1
                    else:
                        lp[r * T + c] = r * T + start
            for r in range(1, T):
                for c in range(T):
                    if not f[r, c]:
                        continue
                    u, l, ul = f[r - 1, c], c > 0 and f[r, c - 1], c > 0 and f[r - 1, c - 1]
                    rt, ur = c < T - 1 and f[r, c + 1], c < T - 1 and f[r - 1, c + 1]
                    i = r * T + c
                    if u:
                        if not (l and ul):
                            union(lp, i, i - T, 0)
                    elif connectivity == 8:
                        if ul and not l:
                            union(lp, i, i - T - 1, 0)
                        if ur and not rt:
                            union(lp, i, i - T + 1, 0)
            for r in range(sub.shape[0]):
                for c in range(sub.shape[1]):
                    if f[r, c]:
                        root = find(lp, r * T + c, 0)
                        g = (y0 + root // T) * W + x0 + root % T
                        par[(y0 + r) * W + x0 + c] = g + 1
                        ta[g] += 1
                        y, x = y0 + r, x0 + c
                        tedge[g] |= y == 0 or y == H - 1 or x == 0 or x == W - 1
    levels = 0
    while (1 << levels) < max(ty_n, tx_n):
        levels += 1
    for m in range(1, levels + 1):
        size = T << m
        for gy in range(-(-ty_n // (1 << m))):
            for gx in range(-(-tx_n // (1 << m))):
                x0, y0 = gx * size, gy * size
                x1, y1 = min(x0 + size, W), min(y0 + size, H)
                xb, yb = x0 + size // 2, y0 + size // 2
                if xb < W:
                    for y in range(y0, y1):
                        a = y * W + xb - 1
                        b = a + 1
                        if not par[a]:
                            continue
                        if par[b]:
                            union(par, a, b, 1)
                        if connectivity == 8:
                            if y + 1 < y1 and par[b + W]:
                                union(par, a, b + W, 1)
                            if y - 1 >= y0 and par[b - W]:
                                union(par, a, b - W, 1)
                if yb < H:
                    for x in range(x0, x1):
                        a = (yb - 1) * W + x
                        b = a + W
                        if not par[a]:
                            continue
                        if par[b]:
                            union(par, a, b, 1)
                        if connectivity == 8:
                            if x + 1 < x1 and par[b + 1]:
                                union(par, a, b + 1, 1)
                            if x - 1 >= x0 and par[b - 1]:
                                union(par, a, b - 1, 1)
    labels = np.zeros(H * W, np.int32)
    tot = np.zeros(H * W, np.int64)
    tot_edge = np.zeros(H * W, bool)
    for g in range(H * W):
        if par[g]:
            r = find(par, g, 1)
            labels[g] = r + 1
            if ta[g]:
                tot[r] += ta[g]
                tot_edge[r] |= tedge[g]
    lab0 = np.maximum(labels.astype(np.int64) - 1, 0)
    area = np.where(labels > 0, tot[lab0], 0).astype(np.int32)
    edge = np.where(labels > 0, tot_edge[lab0], False).astype(np.uint8)
    return labels.reshape(H, W), area.reshape(H, W), edge.reshape(H, W), levels


# ---- mask distances on the host (include/rsu_distance.h)
DIST_BINS, DIST_NONE, DIST_MAX_SIDE = 64, 0x7fffffff, 1024   # rsu_distance.h RSU_DIST_BINS, RSU_DIST_NONE, RSU_DIST_MAX_SIDE


def _dist_check(prob, threshold, labels, need_labels):
    p = np.ascontiguousarray(prob, np.float32)
    if p.ndim != 3 or min(p.shape) < 1 or max(p.shape[1:]) > DIST_MAX_SIDE:
        raise ValueError("distance: prob [N, H, W] with N, H, W >= 1 and H, W <= %d, not shape %r" % (DIST_MAX_SIDE, p.shape))
    t = np.float32(threshold)
    if not np.isfinite(t):
        raise ValueError("distance: threshold must be finite, not %r" % (threshold,))
    if labels is None:
        if need_labels:
            raise ValueError("distance: labels are required")
        return p, t, None
    lab = np.asarray(labels)
    if lab.shape != p.shape or lab.dtype.kind not in "iu":
        raise ValueError("distance: labels must be an integer array of prob's shape %r, not %s %r" % (p.shape, lab.dtype, lab.shape))
    return p, t, lab.astype(np.int64)


def _dist_masks(p, t, lab):
    """(P, T): P = {counted and p >= threshold} (one float32 comparison: NaN outside, p == threshold inside), T = {label == 1}; without
    labels every pixel is counted and T is empty"""
    with np.errstate(invalid="ignore"):
        pred = p >= t
    if lab is None:
        return pred, np.zeros(p.shape, bool)
    return pred & ((lab == 0) | (lab == 1)), lab == 1


def _dist_transform(mask):
    """int32 [N, H, W]: the exact squared Euclidean distance of every pixel to the nearest True pixel of its own image, DIST_NONE in an
    image without one. Separable, in integers: the nearest mask pixel per column (running maxima down and up), then per row the min
    over x' of (x - x')^2 + g(x')^2, taken offset by offset until the offset's square alone reaches the largest minimum so far."""
    N, H, W = mask.shape
    out = np.full((N, H, W), DIST_NONE, np.int64)
    live = np.nonzero(mask.reshape(N, -1).any(axis=1))[0]
    if live.size == 0:
        return out.astype(np.int32)
    m = mask[live]
    big = np.int64(1) << 40
    ys = np.arange(H, dtype=np.int64)[None, :, None]
    above = np.maximum.accumulate(np.where(m, ys, -big), axis=1)
    below = np.minimum.accumulate(np.where(m, ys, big)[:, ::-1], axis=1)[:, ::-1]
    g = np.minimum(ys - above, below - ys)
    sq = np.where(g < big // 2, g * g, big)
    best = sq.copy()
    d = 1
    while d < W and d * d < int(best.max()):
        np.minimum(best[:, :, d:], sq[:, :, :-d] + d * d, out=best[:, :, d:])
        np.minimum(best[:, :, :-d], sq[:, :, d:] + d * d, out=best[:, :, :-d])
        d += 1
    out[live] = best
    return out.astype(np.int32)


def mask_distance(prob, threshold, labels=None):
    """rsu_mask_distance on the host: (d2_pred, d2_true), int32 [N, H, W] each -- the exact squared Euclidean distance of EVERY pixel to
    P = {label in {0, 1} and p >= threshold} and to T = {label == 1} of its own image, DIST_NONE where the image has no such pixel.
    Ignored pixels are plain geometry. labels=None: every pixel is counted and T is empty (d2_true is DIST_NONE everywhere)."""
    p, t, lab = _dist_check(prob, threshold, labels, False)
    pred, true = _dist_masks(p, t, lab)
    return _dist_transform(pred), _dist_transform(true)


_DIST_SQUARES = np.arange(DIST_BINS, dtype=np.int64) ** 2


def distance_bin(d2):
    """bin(d2) of rsu_distance.h: min(r, DIST_BINS - 1) with r the smallest integer such that r * r >= d2, in integers (a search in the
    table of squares); DIST_NONE lands in the last bin"""
    return np.minimum(np.searchsorted(_DIST_SQUARES, np.asarray(d2, np.int64), side="left"), DIST_BINS - 1).astype(np.int64)


def distance_hist(prob, threshold, labels):
    """rsu_distance_hist on the host: int64 [2, DIST_BINS]; hist[0][b] = the pixels of P whose distance to T falls into bin b, hist[1][b] =
    the pixels of T by their distance to P, summed over the images. An image without a counted pixel adds nothing."""
    p, t, lab = _dist_check(prob, threshold, labels, True)
    pred, true = _dist_masks(p, t, lab)
    d2_pred, d2_true = _dist_transform(pred), _dist_transform(true)
    hist = np.zeros((2, DIST_BINS), np.int64)
    hist[0] = np.bincount(distance_bin(d2_true[pred]), minlength=DIST_BINS)
    hist[1] = np.bincount(distance_bin(d2_pred[true]), minlength=DIST_BINS)
    return hist


def relaxed_metrics(hist, slack):
    """The buffer-relaxed scores of Mnih & Hinton from a distance histogram (int [2, DIST_BINS], distance_hist / rsu_distance_hist) at
    `slack` = rho pixels, an int in [0, DIST_BINS - 2]:
      relaxed_precision = the share of predicted road pixels with a true road pixel within rho (sum(hist[0][:rho + 1]) / max(sum(hist[0]), 1)),
      relaxed_recall    = the share of true road pixels with a predicted one within rho, likewise from hist[1],
      relaxed_f1        = their harmonic mean, 0 when both are 0,
      mean_dist_pred / mean_dist_true = the mean BIN INDEX of the predicted / true pixels: the distance rounded up to whole pixels and
                          SATURATING at DIST_BINS - 1 = 63 (a pixel farther than 62 pixels away, or without any pixel of the other mask in
                          its image, counts as 63), 0 without pixels,
      far_pred / far_true = the share of them in that last bin.
    At slack 0 the first two are the plain pixel precision and recall. Distances are per image: a road just outside a patch is not seen."""
    h = np.asarray(hist)
    if h.shape != (2, DIST_BINS) or h.dtype.kind not in "iu":
        raise ValueError("relaxed_metrics: hist must be an integer array [2, %d], not %s %r" % (DIST_BINS, h.dtype, h.shape))
    if isinstance(slack, bool) or not isinstance(slack, (int, np.integer)) or not 0 <= slack <= DIST_BINS - 2:
        raise ValueError("relaxed_metrics: slack must be an integer in [0, %d], not %r" % (DIST_BINS - 2, slack))
    h = h.astype(np.int64)
    tot = [int(h[0].sum()), int(h[1].sum())]
    precision, recall = [float(int(h[s][:int(slack) + 1].sum())) / max(tot[s], 1) for s in (0, 1)]
    idx = np.arange(DIST_BINS, dtype=np.int64)
    mean = [float(int((h[s] * idx).sum())) / max(tot[s], 1) for s in (0, 1)]
    far = [float(int(h[s][-1])) / max(tot[s], 1) for s in (0, 1)]
    f1 = 2.0 * precision * recall / (precision + recall) if precision + recall > 0.0 else 0.0
    return {"relaxed_precision": precision, "relaxed_recall": recall, "relaxed_f1": f1, "mean_dist_pred": mean[0], "mean_dist_true": mean[1],
            "far_pred": far[0], "far_true": far[1]}


# ---- centre-lines on the host (include/rsu_thin.h)
THIN_MAX_SIDE, THIN_MAX_ITERS = 1024, 512   # rsu_thin.h RSU_THIN_MAX_SIDE, RSU_THIN_MAX_ITERS


def _thin_iters(max_iters):
    if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)) or not 1 <= max_iters <= THIN_MAX_ITERS:
        raise ValueError("thin: max_iters must be an integer in [1, %d], not %r" % (THIN_MAX_ITERS, max_iters))
    return int(max_iters)


def _thin_deleted(m, sub):
    """the pixels of bool [N, H, W] that sub-iteration `sub` of Guo & Hall's rule deletes (everything outside an image is background)"""
    q = np.pad(m, ((0, 0), (1, 1), (1, 1)))
    H, W = m.shape[1:]

    def at(dy, dx):
        return q[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    p2, p3, p4, p5, p6, p7, p8, p9 = at(-1, 0), at(-1, 1), at(0, 1), at(1, 1), at(1, 0), at(1, -1), at(0, -1), at(-1, -1)
    i8 = np.int8
    C = (~p2 & (p3 | p4)).astype(i8) + (~p4 & (p5 | p6)).astype(i8) + (~p6 & (p7 | p8)).astype(i8) + (~p8 & (p9 | p2)).astype(i8)
    N1 = (p9 | p2).astype(i8) + (p3 | p4).astype(i8) + (p5 | p6).astype(i8) + (p7 | p8).astype(i8)
    N2 = (p2 | p3).astype(i8) + (p4 | p5).astype(i8) + (p6 | p7).astype(i8) + (p8 | p9).astype(i8)
    Nn = np.minimum(N1, N2)
    mm = ((p6 | p7 | ~p9) & p8) if sub == 0 else ((p2 | p3 | ~p5) & p4)
    return m & (C == 1) & (Nn >= 2) & (Nn <= 3) & ~mm


def thin_mask(mask, max_iters):
    """Guo & Hall's two-sub-iteration parallel thinning (CACM 1989, algorithm A1; the rule of include/rsu_thin.h) of a bool [N, H, W],
    image by image: (skeleton bool [N, H, W], deleted int64 [N]). An iteration is sub-iteration 0 then 1, each deleting all its pixels at
    once from the state before it; the loop ends after max_iters iterations or with the first iteration that deletes nothing anywhere.
    deleted[n] = the pixels the LAST executed iteration took from image n: 0 means image n reached its fixed point within max_iters."""
    m = np.asarray(mask)
    if m.ndim != 3 or m.dtype != np.bool_ or min(m.shape) < 1:
        raise ValueError("thin_mask: mask must be a bool array [N, H, W] with N, H, W >= 1, not %s %r" % (m.dtype, m.shape))
    m = m.copy()
    deleted = np.zeros(m.shape[0], np.int64)
    for _ in range(_thin_iters(max_iters)):
        deleted[:] = 0
        for sub in (0, 1):
            d = _thin_deleted(m, sub)
            deleted += d.reshape(d.shape[0], -1).sum(axis=1)
            m &= ~d
        if not deleted.any():
            break
    return m, deleted


def mask_thin(prob, threshold, labels, max_iters):
    """rsu_mask_thin on the host, in its output formats: (skel_pred float32 [N, H, W] with 1.0 on the skeleton of P = {label in {0, 1} and
    p >= threshold}, skel_true int64 [N, H, W] with 1 on the skeleton of T = {label == 1}, 0 on every other counted pixel and the label
    itself on an ignored one, counts int64 [4] = {|S_P|, |S_P and T|, |S_T|, |S_T and P|}, info uint32 [N, 2] = the pixels the last
    executed iteration deleted from P / from T per image). labels=None: every pixel is counted, T is empty and skel_true is None."""
    p, t, lab = _dist_check(prob, threshold, labels, False)
    if max(p.shape[1:]) > THIN_MAX_SIDE:
        raise ValueError("thin: H, W <= %d, not shape %r" % (THIN_MAX_SIDE, p.shape))
    pred, true = _dist_masks(p, t, lab)
    sp, dp = thin_mask(pred, max_iters)
    st, dt = thin_mask(true, max_iters)
    counts = np.array([sp.sum(), (sp & true).sum(), st.sum(), (st & pred).sum()], np.int64)
    skel_true = None if lab is None else np.where((lab == 0) | (lab == 1), st.astype(np.int64), lab)
    return sp.astype(np.float32), skel_true, counts, np.stack([dp, dt], axis=1).astype(np.uint32)


def centerline_metrics(cl_hist, counts, slack):
    """The centre-line scores of the road-extraction literature (Wiedemann 1998, Heipke 1997) and the clDice METRIC on hard skeletons
    (Shit et al. 2021) from cl_hist = the distance histogram of the two SKELETONS (int [2, DIST_BINS]: distance_hist / rsu_distance_hist
    of mask_thin's two outputs at threshold 0.5) and counts = mask_thin's four integers {|S_P|, |S_P and T|, |S_T|, |S_T and P|}, at
    `slack` = the buffer width in pixels, an int in [0, DIST_BINS - 2]:
      cl_correctness  = the share of the predicted centre-line within slack of the true one (sum(cl_hist[0][:slack + 1]) / max(sum(cl_hist[0]), 1)),
      cl_completeness = the share of the true centre-line within slack of the predicted one, likewise from cl_hist[1],
      cl_quality      = comp * corr / (comp - comp * corr + corr), 0 when both are 0,
      cldice_hard     = the harmonic mean of tprec = |S_P and T| / max(|S_P|, 1) and tsens = |S_T and P| / max(|S_T|, 1), 0 when both are 0,
      cl_len_pred / cl_len_true = |S_P| / |S_T|: the skeletons' PIXEL COUNTS, a proxy of the centre-line length (a diagonal step counts
                        like a straight one), not a length in pixels."""
    h = np.asarray(cl_hist)
    if h.shape != (2, DIST_BINS) or h.dtype.kind not in "iu":
        raise ValueError("centerline_metrics: cl_hist must be an integer array [2, %d], not %s %r" % (DIST_BINS, h.dtype, h.shape))
    c = np.asarray(counts)
    if c.shape != (4,) or c.dtype.kind not in "iu" or (c < 0).any():
        raise ValueError("centerline_metrics: counts must be four integers >= 0, not %s %r" % (c.dtype, counts))
    if isinstance(slack, bool) or not isinstance(slack, (int, np.integer)) or not 0 <= slack <= DIST_BINS - 2:
        raise ValueError("centerline_metrics: slack must be an integer in [0, %d], not %r" % (DIST_BINS - 2, slack))
    h = h.astype(np.int64)
    tot = [int(h[0].sum()), int(h[1].sum())]
    corr, comp = [float(int(h[s][:int(slack) + 1].sum())) / max(tot[s], 1) for s in (0, 1)]
    quality = comp * corr / (comp - comp * corr + corr) if comp + corr > 0.0 else 0.0
    sp, spt, st, stp = (int(v) for v in c)
    tprec, tsens = float(spt) / max(sp, 1), float(stp) / max(st, 1)
    hard = 2.0 * tprec * tsens / (tprec + tsens) if tprec + tsens > 0.0 else 0.0
    return {"cl_correctness": corr, "cl_completeness": comp, "cl_quality": quality, "cldice_hard": hard, "cl_len_pred": sp, "cl_len_true": st}


# ---- centre-line pruning and nodes on the host (include/rsu_graph.h)
GRAPH_MAX_SIDE, GRAPH_MAX_BRANCH = 1024, 64   # rsu_graph.h RSU_GRAPH_MAX_SIDE, RSU_GRAPH_MAX_BRANCH


def _graph_branch(min_branch):
    if isinstance(min_branch, bool) or not isinstance(min_branch, (int, np.integer)) or not 0 <= min_branch <= GRAPH_MAX_BRANCH:
        raise ValueError("graph: min_branch must be an integer in [0, %d], not %r" % (GRAPH_MAX_BRANCH, min_branch))
    return int(min_branch)


def _graph_mask(mask, what):
    m = np.asarray(mask)
    if m.ndim != 3 or m.dtype != np.bool_ or min(m.shape) < 1:
        raise ValueError("%s: mask must be a bool array [N, H, W] with N, H, W >= 1, not %s %r" % (what, m.dtype, m.shape))
    return m


def _graph_counts(m):
    """(n8, X) of bool [N, H, W], int8 each: the number of set neighbours and the number of 0 -> 1 steps around the eight neighbours
    p2 .. p9, clockwise from north and cyclic (everything outside an image is background)"""
    q = np.pad(m, ((0, 0), (1, 1), (1, 1)))
    H, W = m.shape[1:]
    ring = [q[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))]
    n8 = np.zeros(m.shape, np.int8)
    X = np.zeros(m.shape, np.int8)
    for i in range(8):
        n8 += ring[i]
        X += ~ring[i] & ring[(i + 1) % 8]
    return n8, X


def _graph_end(m):
    n8, X = _graph_counts(m)
    return m & (X <= 1) & (n8 <= 3)


def prune_mask(mask, min_branch):
    """Morphological pruning (Gonzalez & Woods; the rule of include/rsu_graph.h) of a bool [N, H, W], image by image, L = min_branch:
    X1 = A, L times X1 &= ~END(X1); E = END(X1), L times E = A & dilate8(E); B = X1 | E, with END(A) = A and X <= 1 and n8 <= 3. A
    branch of at most L pixels goes, a longer one stays whole; a free curve of at most 2 L pixels vanishes; a loop is untouched. Known
    artefact: a spur within L pixels (geodesic) of a true line end grows back with that end."""
    a = _graph_mask(mask, "prune_mask")
    L = _graph_branch(min_branch)
    x1 = a.copy()
    for _ in range(L):
        x1 &= ~_graph_end(x1)
    e = _graph_end(x1)
    H, W = a.shape[1:]
    for _ in range(L):
        q = np.pad(e, ((0, 0), (1, 1), (1, 1)))
        d = np.zeros_like(e)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                d |= q[:, dy:dy + H, dx:dx + W]
        e = a & d
    return x1 | e if L else x1


def skeleton_nodes(mask):
    """(ends, isolated, junctions), bool [N, H, W] each, of a bool [N, H, W]: an end is a pixel of END(mask) with a neighbour, an
    isolated pixel one without, a junction pixel a pixel of the mask whose crossing number X is 3 or more (include/rsu_graph.h).
    Adjacent junction pixels are one junction."""
    m = _graph_mask(mask, "skeleton_nodes")
    n8, X = _graph_counts(m)
    end = m & (X <= 1) & (n8 <= 3)
    return end & (n8 >= 1), end & (n8 == 0), m & (X >= 3)


def skeleton_graph(prob, threshold, labels, min_branch):
    """rsu_skeleton_graph on the host, in its output formats: (out_pred float32, out_true int64, junc_pred float32, junc_true int64,
    counts int64 [8]). out_* hold the pruned B of P = {label in {0, 1} and p >= threshold} and of T = {label == 1}, junc_* the junction
    pixels of the two B; on the truth side an ignored pixel keeps its label. counts = {|B|, ends, isolated, junction pixels} of P, then
    of T. labels=None: every pixel is counted, T is empty and the two *_true outputs are None."""
    p, t, lab = _dist_check(prob, threshold, labels, False)
    if max(p.shape[1:]) > GRAPH_MAX_SIDE:
        raise ValueError("graph: H, W <= %d, not shape %r" % (GRAPH_MAX_SIDE, p.shape))
    L = _graph_branch(min_branch)
    pred, true = _dist_masks(p, t, lab)
    counts = np.zeros(8, np.int64)
    outs = []
    for side, a in enumerate((pred, true)):
        b = prune_mask(a, L)
        ends, iso, junc = skeleton_nodes(b)
        counts[4 * side:4 * side + 4] = (b.sum(), ends.sum(), iso.sum(), junc.sum())
        outs.append((b, junc))
    if lab is None:
        out_true = junc_true = None
    else:
        counted = (lab == 0) | (lab == 1)
        out_true, junc_true = (np.where(counted, m.astype(np.int64), lab) for m in outs[1])
    return outs[0][0].astype(np.float32), out_true, outs[0][1].astype(np.float32), junc_true, counts


def graph_metrics(jn_hist, jn_counts, counts, slack):
    """The junction and end scores of a validation pass from jn_hist = the distance histogram of the two JUNCTION-PIXEL masks (int
    [2, DIST_BINS]: distance_hist / rsu_distance_hist of skeleton_graph's junc_pred at threshold 0.5 and junc_true), jn_counts = four
    integers {junction clusters of the prediction, of the truth (8-connected components of the junction pixels), the sum over the
    patches of |pred - true| clusters, the patches with a counted pixel}, counts = skeleton_graph's eight integers, at `slack` pixels:
      jn_precision   = the share of predicted junction pixels within slack of a true one (read as relaxed_metrics reads its histogram),
      jn_recall      = the share of true junction pixels within slack of a predicted one,
      jn_f1          = their harmonic mean, 0 when both are 0,
      junctions_pred / junctions_true = the cluster counts,
      junction_error = the mean |pred - true| clusters per patch that has a counted pixel, 0 without one,
      ends_pred / ends_true / isolated_pred / isolated_true = pixel counts.
    A road that leaves its patch ends there and counts as an end, on both sides alike: the comparison is the figure, not the count."""
    h = np.asarray(jn_hist)
    if h.shape != (2, DIST_BINS) or h.dtype.kind not in "iu":
        raise ValueError("graph_metrics: jn_hist must be an integer array [2, %d], not %s %r" % (DIST_BINS, h.dtype, h.shape))
    j = np.asarray(jn_counts)
    if j.shape != (4,) or j.dtype.kind not in "iu" or (j < 0).any():
        raise ValueError("graph_metrics: jn_counts must be four integers >= 0, not %s %r" % (j.dtype, jn_counts))
    c = np.asarray(counts)
    if c.shape != (8,) or c.dtype.kind not in "iu" or (c < 0).any():
        raise ValueError("graph_metrics: counts must be eight integers >= 0, not %s %r" % (c.dtype, counts))
    if isinstance(slack, bool) or not isinstance(slack, (int, np.integer)) or not 0 <= slack <= DIST_BINS - 2:
        raise ValueError("graph_metrics: slack must be an integer in [0, %d], not %r" % (DIST_BINS - 2, slack))
    h = h.astype(np.int64)
    tot = [int(h[0].sum()), int(h[1].sum())]
    prec, rec = [float(int(h[s][:int(slack) + 1].sum())) / max(tot[s], 1) for s in (0, 1)]
    f1 = 2.0 * prec * rec / (prec + rec) if prec + rec > 0.0 else 0.0
    jp, jt, err, patches = (int(v) for v in j)
    return {"jn_precision": prec, "jn_recall": rec, "jn_f1": f1, "junctions_pred": jp, "junctions_true": jt,
            "junction_error": float(err) / patches if patches else 0.0, "ends_pred": int(c[1]), "ends_true": int(c[5]),
            "isolated_pred": int(c[2]), "isolated_true": int(c[6])}


# ---- road segments on the host (include/rsu_segments.h)
SEGMENTS_MAX_SIDE, SEGMENTS_MAX_EDGES = 1024, 65536   # rsu_segments.h RSU_SEGMENTS_MAX_SIDE, RSU_SEGMENTS_MAX_EDGES
SEGMENTS_BLOCK, SEGMENTS_TILE = 256, (64, 16)         # csrc/segments.hip SG_BLOCK; SG_TW, SG_TH
_SEG_RING = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))   # p2 .. p9: clockwise from north


def _segments_edges(max_edges):
    if isinstance(max_edges, bool) or not isinstance(max_edges, (int, np.integer)) or not 1 <= max_edges <= SEGMENTS_MAX_EDGES:
        raise ValueError("segments: max_edges must be an integer in [1, %d], not %r" % (SEGMENTS_MAX_EDGES, max_edges))
    return int(max_edges)


def segment_zones(mask):
    """(S, Z), bool [N, H, W] each, of a bool [N, H, W]: J = the pixels with crossing number X >= 3, the node zones Z = mask and
    dilate8(J), the segment pixels S = mask and not Z (include/rsu_segments.h)"""
    a = _graph_mask(mask, "segment_zones")
    junc = skeleton_nodes(a)[2]
    H, W = a.shape[1:]
    q = np.pad(junc, ((0, 0), (1, 1), (1, 1)))
    d = np.zeros_like(a)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            d |= q[:, dy:dy + H, dx:dx + W]
    z = a & d
    return a & ~z, z


def _segments_image(a, max_edges, fill):
    """(rows int32 [max_edges, 8], segments, nodes, seg int32 [H, W], node int32 [H, W]) of one bool [H, W]"""
    H, W = a.shape
    s, z = (m[0] for m in segment_zones(a[None]))
    ends, iso, _ = skeleton_nodes(a[None])
    end = (ends[0] | iso[0]) & s
    seg, zone = _cc_labels(s, 8), _cc_labels(z, 8)
    index = np.arange(H * W, dtype=np.int64).reshape(H, W)
    node = np.where(end, -(index + 1), zone).astype(np.int32)
    pad = lambda m: np.pad(m, 1)   # noqa: E731
    at = lambda m, k: m[1 + _SEG_RING[k][0]:1 + _SEG_RING[k][0] + H, 1 + _SEG_RING[k][1]:1 + _SEG_RING[k][1] + W]   # noqa: E731
    sq, zq, aq = pad(s), pad(zone), pad(a)
    sn = [at(sq, k) for k in range(8)]
    zn = [at(zq, k).astype(np.int64) for k in range(8)]
    an = [at(aq, k) for k in range(8)]
    # links towards E (2), SE (3), S (4), SW (5): every pair once; a diagonal one only if neither pixel 4-adjacent to both is in A
    ortho = sn[2].astype(np.int64) + sn[4]
    diag = (sn[3] & ~an[2] & ~an[4]).astype(np.int64) + (sn[5] & ~an[6] & ~an[4])
    # contacts: the distinct zone labels among the eight neighbours; orthogonal if the label is among N, E, S, W
    contacts = np.zeros((H, W), np.int64)
    big = np.int64(1) << 40
    lo, hi = np.full((H, W), big), np.full((H, W), -big)
    for k in range(8):
        first = zn[k] != 0
        for m in range(k):
            first &= zn[m] != zn[k]
        edge = (zn[0] == zn[k]) | (zn[2] == zn[k]) | (zn[4] == zn[k]) | (zn[6] == zn[k])
        contacts += first
        ortho += first & edge
        diag += first & ~edge
        lo = np.where(first, np.minimum(lo, zn[k]), lo)
        hi = np.where(first, np.maximum(hi, zn[k]), hi)
    lo = np.where(end, np.minimum(lo, -(index + 1)), lo)
    hi = np.where(end, np.maximum(hi, -(index + 1)), hi)
    where = np.nonzero(s.reshape(-1))[0]
    owner = seg.reshape(-1)[where].astype(np.int64)
    labels = np.unique(owner)                          # ascending: the row order
    row_of = np.searchsorted(labels, owner)
    k = labels.size
    table = np.zeros((k, 8), np.int64)
    table[:, 0] = labels
    table[:, 4], table[:, 5] = big, -big
    for col, src in ((1, np.ones((H, W), np.int64)), (2, ortho), (3, diag), (6, contacts), (7, end.astype(np.int64))):
        np.add.at(table[:, col], row_of, src.reshape(-1)[where])
    np.minimum.at(table[:, 4], row_of, lo.reshape(-1)[where])
    np.maximum.at(table[:, 5], row_of, hi.reshape(-1)[where])
    none = table[:, 4] == big
    table[none, 4] = table[none, 5] = 0
    rows = np.full((max_edges, 8), fill, np.int32)
    rows[:min(k, max_edges)] = table[:max_edges]
    return rows, k, int(np.unique(zone[z]).size), seg, node


def segments_acc(rows, stored):
    """the eight integers rsu_line_segments adds to acc[side] for the first `stored` rows of one image: {rows stored, pixels, ortho,
    diag, dangling, free, rings, multi}"""
    r = np.asarray(rows)[:stored].astype(np.int64)
    c, e = r[:, 6], r[:, 7]
    return np.array([stored, r[:, 1].sum(), r[:, 2].sum(), r[:, 3].sum(), ((c == 1) & (e == 1)).sum(), ((c == 0) & (e >= 1)).sum(),
                     (c + e == 0).sum(), (c + e > 2).sum()], np.int64)


def line_segments(prob, threshold, labels, max_edges, fill=0):
    """rsu_line_segments on the host, in its output formats: (edges_pred, edges_true int32 [N, max_edges, 8], counts int32 [N, 4],
    seg_pred, seg_true, node_pred, node_true int32 [N, H, W], acc int64 [2, 8]) of P = {label in {0, 1} and p >= threshold} and of
    T = {label == 1}. A row is {label, pixels, ortho, diag, node_a, node_b, contacts, ends}, in ascending label order; rows at and past
    min(count, max_edges) keep `fill`; counts = {segments of P, nodes of P, segments of T, nodes of T}, the true numbers. labels=None:
    every pixel is counted, T is empty and the three *_true outputs are None."""
    p, t, lab = _dist_check(prob, threshold, labels, False)
    if max(p.shape[1:]) > SEGMENTS_MAX_SIDE:
        raise ValueError("segments: H, W <= %d, not shape %r" % (SEGMENTS_MAX_SIDE, p.shape))
    cap = _segments_edges(max_edges)
    N = p.shape[0]
    counts = np.zeros((N, 4), np.int32)
    acc = np.zeros((2, 8), np.int64)
    outs = []
    for side, a in enumerate(_dist_masks(p, t, lab)):
        if side == 1 and lab is None:
            outs.append((None, None, None))
            continue
        per = [_segments_image(a[n], cap, fill) for n in range(N)]
        for n, (rows, k, nodes, _, _) in enumerate(per):
            counts[n, 2 * side:2 * side + 2] = (k, nodes)
            acc[side] += segments_acc(rows, min(k, cap))
        outs.append((np.stack([r[0] for r in per]), np.stack([r[3] for r in per]), np.stack([r[4] for r in per])))
    return outs[0][0], outs[1][0], counts, outs[0][1], outs[1][1], outs[0][2], outs[1][2], acc


def segment_metrics(acc, counts_sum):
    """The road-network figures of a validation pass from acc = rsu_line_segments' sixteen integers ([2, 8]: {rows stored, pixels, ortho,
    diag, dangling, free, rings, multi} of the prediction, then of the truth) and counts_sum = the sum of its counts over the patches
    ({segments of P, nodes of P, segments of T, nodes of T}), per side * in (pred, true):
      segments_*          = the stored rows,
      road_length_*       = ortho + sqrt(2) diag over them (float64),
      seg_len_mean_*      = road_length / segments, 0 without one,
      dangling_*, free_*, rings_*, multi_* = the rows of each kind,
      segments_dropped_*  = the true segment count minus the stored rows (rows past --max_segments),
      nodes_*             = the node zones,
    and length_ratio = road_length_pred / road_length_true, 0 without truth."""
    a = np.asarray(acc)
    if a.shape != (2, 8) or a.dtype.kind not in "iu" or (a.astype(np.int64) < 0).any():
        raise ValueError("segment_metrics: acc must be sixteen integers >= 0 as [2, 8], not %s %r" % (a.dtype, a.shape))
    c = np.asarray(counts_sum)
    if c.shape != (4,) or c.dtype.kind not in "iu" or (c.astype(np.int64) < 0).any():
        raise ValueError("segment_metrics: counts_sum must be four integers >= 0, not %s %r" % (c.dtype, counts_sum))
    out, length = {}, []
    for side, name in enumerate(("pred", "true")):
        rows, _, ortho, diag, dangling, free, rings, multi = (int(v) for v in a[side])
        total = float(ortho) + float(np.sqrt(np.float64(2.0))) * float(diag)
        length.append(total)
        if int(c[2 * side]) < rows:
            raise ValueError("segment_metrics: more stored rows (%d) than segments (%d)" % (rows, int(c[2 * side])))
        out.update({"segments_" + name: rows, "road_length_" + name: total, "seg_len_mean_" + name: total / rows if rows else 0.0,
                    "dangling_" + name: dangling, "free_" + name: free, "rings_" + name: rings, "multi_" + name: multi,
                    "segments_dropped_" + name: int(c[2 * side]) - rows, "nodes_" + name: int(c[2 * side + 1])})
    out["length_ratio"] = length[0] / length[1] if length[1] > 0.0 else 0.0
    return out


# ---- ordered polylines on the host (include/rsu_paths.h)
PATHS_MAX_SIDE, PATHS_MAX_EDGES, PATHS_MAX_LEN = 1024, 65536, 1 << 20   # rsu_paths.h RSU_PATHS_MAX_SIDE, RSU_PATHS_MAX_EDGES, RSU_PATHS_MAX_LEN
PATHS_BLOCK, PATHS_TILE = 256, (64, 16)                                 # csrc/paths.hip PT_BLOCK; PT_TW, PT_TH
PATH_KINDS = ("open", "ring", "branched", "long")                       # the kind of a stored row: 0, 1, 2, 3
_PATH_DIRS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))   # ascending row-major offset: NW N NE W E SW S SE


def path_rounds(max_len):
    """R = ceil(log2(max_len)): the doublings (jump launches) of one rsu_segment_paths call"""
    return (int(max_len) - 1).bit_length()


def path_link_mask(s):
    """int32 [H, W] of a bool [H, W]: bit d set where the pixel and its neighbour in direction d (_PATH_DIRS) are path-linked: both in S
    and 4-adjacent, or diagonal neighbours with neither of the two pixels 4-adjacent to both in S (include/rsu_paths.h); 0 outside S"""
    H, W = s.shape
    q = np.pad(s, 1)
    at = [q[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in _PATH_DIRS]
    n, w, e, so = at[1], at[3], at[4], at[6]
    link = [at[0] & ~n & ~w, n, at[2] & ~n & ~e, w, e, at[5] & ~so & ~w, so, at[7] & ~so & ~e]
    mask = np.zeros((H, W), np.int32)
    for d in range(8):
        mask |= (s & link[d]).astype(np.int32) << d
    return mask


def _paths_check(seg, edges, counts, side, max_len, max_points):
    sg, e, c = np.asarray(seg), np.asarray(edges), np.asarray(counts)
    if sg.ndim != 3 or sg.dtype.kind not in "iu" or min(sg.shape) < 1:
        raise ValueError("segment_paths: seg must be an integer array [N, H, W] with N, H, W >= 1, not %s %r" % (sg.dtype, sg.shape))
    N, H, W = sg.shape
    if max(H, W) > PATHS_MAX_SIDE:
        raise ValueError("segment_paths: H, W <= %d, not shape %r" % (PATHS_MAX_SIDE, sg.shape))
    if isinstance(side, bool) or not isinstance(side, (int, np.integer)) or side not in (0, 1):
        raise ValueError("segment_paths: side must be 0 or 1, not %r" % (side,))
    if e.ndim != 3 or e.shape[0] != N or e.shape[2] != 8 or e.dtype.kind not in "iu" or not 1 <= e.shape[1] <= PATHS_MAX_EDGES:
        raise ValueError("segment_paths: edges must be an integer array [%d, max_edges, 8] with max_edges in [1, %d], not %s %r"
                         % (N, PATHS_MAX_EDGES, e.dtype, e.shape))
    if c.shape != (N, 4) or c.dtype.kind not in "iu":
        raise ValueError("segment_paths: counts must be an integer array [%d, 4], not %s %r" % (N, c.dtype, c.shape))
    if isinstance(max_len, bool) or not isinstance(max_len, (int, np.integer)) or not 1 <= max_len <= PATHS_MAX_LEN:
        raise ValueError("segment_paths: max_len must be an integer in [1, %d], not %r" % (PATHS_MAX_LEN, max_len))
    if isinstance(max_points, bool) or not isinstance(max_points, (int, np.integer)) or not 1 <= max_points <= H * W:
        raise ValueError("segment_paths: max_points must be an integer in [1, H W = %d], not %r" % (H * W, max_points))
    if N * H * W * 16 >= 0x7ffffff0:
        raise ValueError("segment_paths: an arc buffer of %d x %d x %d pixels (16 bytes each) reaches 2 GiB" % (N, H, W))
    return sg, e, c


def _paths_walk(mask, start, ring, limit):
    """the pixels of one segment from `start` along the links: mask = the flat link masks, ring: leave the start towards its smaller
    neighbour and stop in front of it again; at most `limit` pixels"""
    W = mask[1]
    m = mask[0]
    out, prev, cur = [start], -1, start
    while len(out) < limit:
        nxt = -1
        for d in range(8):
            if m[cur] >> d & 1:
                w = cur + _PATH_DIRS[d][0] * W + _PATH_DIRS[d][1]
                if w != prev:
                    nxt = w
                    break
        if nxt < 0 or nxt == start:
            break
        out.append(nxt)
        prev, cur = cur, nxt
    return out


def segment_paths(seg, edges, counts, side, max_len, max_points, fill=0):
    """rsu_segment_paths on the host, by a sequential walk, in its output formats: (paths int32 [N, max_points], offsets int32
    [N, max_edges + 1], kind int32 [N, max_edges], pos int32 [N, H, W], info int32 [N, 4]) of seg int32 [N, H, W], edges int32
    [N, max_edges, 8] and counts int32 [N, 4] of one rsu_line_segments call, for side 0 (counts[:, 0]) or 1 (counts[:, 2]). The first
    stored = min(count, max_edges) rows are read; a stored row is open (kind 0), a ring (1), branched (2: a pixel of link degree >= 3) or
    too long (3: pixels > max_len, tested first); the pixels of an open row run from its smaller-indexed terminal, those of a ring from
    its smallest pixel towards the smaller-indexed of that pixel's two neighbours; offsets = the exclusive sums of the ordered rows'
    pixel counts (the true numbers, also past max_points), paths[n, offsets[n, r] + p] = the row-major index of position p of row r,
    pos = 1 + position at ordered pixels and 0 elsewhere, info = {points, open rows, ring rows, rows of kind 2 or 3}. Elements the entry
    does not touch keep `fill`: rows at and past stored, offsets past stored, path elements no ordered row owns. Bad arguments raise
    ValueError by the header's rules."""
    sg, e, c = _paths_check(seg, edges, counts, side, max_len, max_points)
    N, H, W = sg.shape
    cap = e.shape[1]
    paths = np.full((N, int(max_points)), fill, np.int32)
    offsets = np.full((N, cap + 1), fill, np.int32)
    kind = np.full((N, cap), fill, np.int32)
    pos = np.zeros((N, H, W), np.int32)
    info = np.zeros((N, 4), np.int32)
    for n in range(N):
        stored = min(max(int(c[n, 2 * side]), 0), cap)
        rows = e[n, :stored].astype(np.int64)
        flat = sg[n].reshape(-1).astype(np.int64)
        mask = path_link_mask(sg[n] != 0).reshape(-1)
        where = np.nonzero(flat)[0]
        row_of = np.searchsorted(rows[:, 0], flat[where])
        hit = row_of < stored
        hit[hit] = rows[row_of[hit], 0] == flat[where[hit]]
        where, row_of = where[hit], row_of[hit]                     # the pixels of stored rows, ascending index; their rows
        deg = np.array([bin(int(v)).count("1") for v in mask[where]], np.int64) if where.size else np.zeros(0, np.int64)
        branched = np.zeros(stored, bool)
        np.logical_or.at(branched, row_of, deg >= 3)
        big = np.int64(1) << 40
        minterm = np.full(stored, big)
        np.minimum.at(minterm, row_of[deg <= 1], where[deg <= 1])
        found = np.bincount(row_of, minlength=stored) if stored else np.zeros(0, np.int64)
        k = np.where(rows[:, 1] > max_len, 3, np.where(branched, 2, np.where(minterm != big, 0, 1)))
        length = np.where(k <= 1, rows[:, 1], 0)
        off = np.concatenate([[0], np.cumsum(length)])
        kind[n, :stored] = k
        offsets[n, :stored + 1] = off.astype(np.int32)
        info[n] = (off[-1], (k == 0).sum(), (k == 1).sum(), (k >= 2).sum())
        m = (mask.tolist(), W)
        for r in range(stored):
            if k[r] > 1 or not found[r]:
                continue
            ring = k[r] == 1
            start = int(rows[r, 0]) - 1 if ring else int(minterm[r])
            if not 0 <= start < H * W or not mask[start] and ring:
                continue
            for p, v in enumerate(_paths_walk(m, start, ring, int(found[r]))):
                pos[n].reshape(-1)[v] = p + 1
                if 0 <= off[r] + p < max_points:
                    paths[n, off[r] + p] = v
    return paths, offsets, kind, pos, info


def simplify_path(points, eps):
    """Ramer-Douglas-Peucker on a chain of points, integer [n, 2]: the first and the last point stay, and between two kept points every
    point within eps of the straight line between them goes (the distance to the line through them; to the point where the two
    coincide). eps = 0 returns the input. A ring is a chain that is cut at its first point: it is treated as open, from position 0 to
    its last pixel. Host only."""
    pts = np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] != 2 or pts.dtype.kind not in "iu":
        raise ValueError("simplify_path: points must be an integer array [n, 2], not %s %r" % (pts.dtype, pts.shape))
    if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)) or not eps >= 0 or not np.isfinite(eps):
        raise ValueError("simplify_path: eps must be a finite number >= 0, not %r" % (eps,))
    n = pts.shape[0]
    if eps == 0 or n <= 2:
        return pts.copy()
    p = pts.astype(np.float64)
    keep = np.zeros(n, bool)
    keep[0] = keep[-1] = True
    stack = [(0, n - 1)]
    while stack:
        a, b = stack.pop()
        if b - a < 2:
            continue
        d, q = p[b] - p[a], p[a + 1:b] - p[a]
        norm = float(np.hypot(d[0], d[1]))
        dist = np.abs(d[0] * q[:, 1] - d[1] * q[:, 0]) / norm if norm > 0.0 else np.hypot(q[:, 0], q[:, 1])
        i = int(np.argmax(dist))
        if dist[i] > eps:
            keep[a + 1 + i] = True
            stack += [(a, a + 1 + i), (a + 1 + i, b)]
    return pts[keep]


def _node_touches(m, node, y, x):
    """node id `node` touches pixel (y, x) of node map m: the pixel's own negative id, or a positive zone id among its eight neighbours"""
    if node < 0:
        return int(m[y, x]) == node
    return node > 0 and bool((m[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] == node).any())


def road_graph(edges, count, node_map, H, W, paths=None):
    """One image's network as a plain dict from rsu_line_segments' outputs: edges int32 [max_edges, 8], count = its segment count (the
    first min(count, max_edges) rows are read), node_map = node_* of the image, int32 [H, W] (sparse: node ids at zone pixels, negative
    ids at line ends).
      nodes: [{id, kind: junction | end | isolated, y, x}]: a junction's position is the centroid of its zone, an end's its pixel; an
             isolated pixel is an end whose segment has one pixel. Ascending id.
      edges: [{id, a, b, pixels, length, contacts, ends}], length = ortho + sqrt(2) diag, in row order.
    paths = (paths int32 [max_points], offsets int32 [max_edges + 1], kind int32 [max_edges]) of the image from rsu_segment_paths: every
    edge also gets "kind" (open | ring | branched | long) and "path", a list of [y, x] (empty for the unordered kinds; cut where the
    points passed max_points). An open path is reversed when node a touches its last pixel and not its first (the pixel's own negative id
    in node_map, or a positive zone id among its eight neighbours), so it runs from a to b where that is decidable; otherwise the
    device order stays."""
    e = np.asarray(edges)
    m = np.asarray(node_map)
    if e.ndim != 2 or e.shape[1] != 8 or e.dtype.kind not in "iu":
        raise ValueError("road_graph: edges must be an integer array [max_edges, 8], not %s %r" % (e.dtype, e.shape))
    if m.shape != (H, W) or m.dtype.kind not in "iu":
        raise ValueError("road_graph: node_map must be an integer array [%d, %d], not %s %r" % (H, W, m.dtype, m.shape))
    if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or count < 0:
        raise ValueError("road_graph: count must be an integer >= 0, not %r" % (count,))
    rows = e[:min(int(count), e.shape[0])].astype(np.int64)
    lone = set(int(-r[4]) for r in rows if r[1] == 1 and r[6] == 0 and r[7] == 1)   # one-pixel segments without a contact
    nodes = []
    ys, xs = np.nonzero(m)
    ids = m[ys, xs].astype(np.int64)
    for i in np.unique(ids):
        sel = ids == i
        if i > 0:
            nodes.append({"id": int(i), "kind": "junction", "y": float(ys[sel].mean()), "x": float(xs[sel].mean())})
        else:
            nodes.append({"id": int(i), "kind": "isolated" if int(-i) in lone else "end", "y": float(ys[sel][0]), "x": float(xs[sel][0])})
    root2 = float(np.sqrt(np.float64(2.0)))
    out = [{"id": int(r[0]), "a": int(r[4]), "b": int(r[5]), "pixels": int(r[1]), "length": float(r[2]) + root2 * float(r[3]),
            "contacts": int(r[6]), "ends": int(r[7])} for r in rows]
    if paths is not None:
        pts, off, kind = (np.asarray(a) for a in paths)
        if pts.ndim != 1 or off.shape != (e.shape[0] + 1,) or kind.shape != (e.shape[0],) or any(a.dtype.kind not in "iu" for a in (pts, off, kind)):
            raise ValueError("road_graph: paths must be integer arrays ([max_points], [%d], [%d]), not %r, %r, %r"
                             % (e.shape[0] + 1, e.shape[0], pts.shape, off.shape, kind.shape))
        for i, (r, edge) in enumerate(zip(rows, out)):
            k = int(kind[i])
            if not 0 <= k <= 3:
                raise ValueError("road_graph: kind[%d] = %d is none of 0 .. 3" % (i, k))
            chain = []
            if k <= 1:
                lo = min(max(int(off[i]), 0), pts.shape[0])
                hi = min(max(int(off[i]) + int(r[1]), lo), pts.shape[0])
                chain = [[int(v) // W, int(v) % W] for v in pts[lo:hi]]
                if k == 0 and len(chain) > 1 and _node_touches(m, int(r[4]), *chain[-1]) and not _node_touches(m, int(r[4]), *chain[0]):
                    chain.reverse()
            edge["kind"], edge["path"] = PATH_KINDS[k], chain
    return {"nodes": nodes, "edges": out}


# ---- network distances and the path-length score on the host (include/rsu_routes.h)
ROUTES_MAX_SIDE, ROUTES_MAX_NODES, ROUTES_MAX_EDGES = 1024, 1024, 65536   # rsu_routes.h RSU_ROUTES_MAX_SIDE, RSU_ROUTES_MAX_NODES; max_edges
ROUTES_INF, ROUTES_Q = 0x3fffffff, 65536                                  # rsu_routes.h RSU_ROUTES_INF (no path), RSU_ROUTES_Q (the unit of q)
ROUTES_ORTHO, ROUTES_DIAG = 70, 99                                        # a weight is 70 ortho + 99 diag: 99 / 70 is a convergent of sqrt(2)
ROUTES_BLOCK, ROUTES_TILE = 256, 64                                       # csrc/routes.hip RT_BLOCK, RT_TILE


def _routes_int(what, name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError("%s: %s must be an integer in [%d, %d], not %r" % (what, name, lo, hi, v))
    return int(v)


def _routes_check(node_map, edges, counts, side, max_nodes):
    m, e, c = np.asarray(node_map), np.asarray(edges), np.asarray(counts)
    if m.ndim != 3 or m.dtype.kind not in "iu" or min(m.shape) < 1:
        raise ValueError("graph_routes: node_map must be an integer array [N, H, W] with N, H, W >= 1, not %s %r" % (m.dtype, m.shape))
    N, H, W = m.shape
    if max(H, W) > ROUTES_MAX_SIDE:
        raise ValueError("graph_routes: H, W <= %d, not shape %r" % (ROUTES_MAX_SIDE, m.shape))
    if isinstance(side, bool) or not isinstance(side, (int, np.integer)) or side not in (0, 1):
        raise ValueError("graph_routes: side must be 0 or 1, not %r" % (side,))
    if e.ndim != 3 or e.shape[0] != N or e.shape[2] != 8 or e.dtype.kind not in "iu" or not 1 <= e.shape[1] <= ROUTES_MAX_EDGES:
        raise ValueError("graph_routes: edges must be an integer array [%d, max_edges, 8] with max_edges in [1, %d], not %s %r"
                         % (N, ROUTES_MAX_EDGES, e.dtype, e.shape))
    if c.shape != (N, 4) or c.dtype.kind not in "iu":
        raise ValueError("graph_routes: counts must be an integer array [%d, 4], not %s %r" % (N, c.dtype, c.shape))
    cap = _routes_int("graph_routes", "max_nodes", max_nodes, 1, ROUTES_MAX_NODES)
    if N * H * W * 4 >= 0x7ffffff0 or N * cap * cap * 4 >= 0x7ffffff0:
        raise ValueError("graph_routes: node_map (%d x %d x %d) or dist (%d x %d x %d) reaches 2 GiB" % (N, H, W, N, cap, cap))
    return m, e, c, cap


def _routes_find(ids, v):
    """the rows of the node ids `v` in a table whose ids ascend in absolute value: the first row whose |id| is not below |v|, taken where
    its id is v; -1 elsewhere"""
    v = np.asarray(v, np.int64)
    r = np.searchsorted(np.abs(ids), np.abs(v))
    hit = r < ids.size
    hit[hit] = ids[r[hit]] == v[hit]
    return np.where(hit, r, -1)


def graph_routes(node_map, edges, counts, side, max_nodes, fill=0, solver=None):
    """rsu_graph_routes on the host, in its output formats: (nodes int32 [N, max_nodes, 4], dist int32 [N, max_nodes, max_nodes], info int32
    [N, 4]) of node_map int32 [N, H, W], edges int32 [N, max_edges, 8] and counts int32 [N, 4] of one side of rsu_line_segments (side 0
    reads counts[:, 0], side 1 counts[:, 2]). A node is a root pixel p of node_map (node_map[p] == p + 1: a zone's smallest pixel, or
    node_map[p] < 0: a line end), numbered in ascending p; its row is {id, y, x, pixels}: an end's pixel and 1, a zone's rounded centroid
    (2 sum + pixels) // (2 pixels) and its pixel count. A stored row of edges with node_a != node_b is an edge of weight
    min(70 ortho + 99 diag, ROUTES_INF) between its two nodes; parallel edges keep the minimum; a row with a negative ortho or diag or a
    node that is not in the stored table is skipped and counted. dist[n, i, j] is the length of the shortest path (Floyd-Warshall in
    integer min-plus, sums cut at ROUTES_INF), ROUTES_INF without one, 0 on the diagonal. info = {nodes, nodes stored, edges used, rows
    skipped}. Rows and columns at and past the stored nodes keep `fill`. Bad arguments raise ValueError by the header's rules.
    solver: a function that takes the int32 matrix of the direct edges' weights (ROUTES_INF: none, 0 on the diagonal) and returns the
    distances in its place, instead of the Floyd-Warshall loop here (tools/bench_routes.py times scipy's this way)."""
    m, e, c, cap = _routes_check(node_map, edges, counts, side, max_nodes)
    N, H, W = m.shape
    nodes = np.full((N, cap, 4), fill, np.int32)
    dist = np.full((N, cap, cap), fill, np.int32)
    info = np.zeros((N, 4), np.int32)
    index = np.arange(H * W, dtype=np.int64)
    for n in range(N):
        flat = m[n].reshape(-1).astype(np.int64)
        roots = np.nonzero((flat == index + 1) | (flat < 0))[0]
        total, stored = roots.size, min(roots.size, cap)
        roots = roots[:stored]
        ids = flat[roots]
        table = np.stack([ids, roots // W, roots % W, np.ones(stored, np.int64)], axis=1)
        zone = np.nonzero(flat > 0)[0]                      # the zones' pixels add to their node's sums
        row = _routes_find(ids, flat[zone])
        zone, row = zone[row >= 0], row[row >= 0]
        pixels, sy, sx = (np.zeros(stored, np.int64) for _ in range(3))
        np.add.at(pixels, row, 1)
        np.add.at(sy, row, zone // W)
        np.add.at(sx, row, zone % W)
        z = (ids > 0) & (pixels > 0)
        table[z, 1] = (2 * sy[z] + pixels[z]) // (2 * pixels[z])
        table[z, 2] = (2 * sx[z] + pixels[z]) // (2 * pixels[z])
        table[z, 3] = pixels[z]
        nodes[n, :stored] = table
        rows = e[n, :min(max(int(c[n, 2 * side]), 0), e.shape[1])].astype(np.int64)
        rows = rows[rows[:, 4] != rows[:, 5]]               # rings and loops through one node are no edges
        ia, ib = _routes_find(ids, rows[:, 4]), _routes_find(ids, rows[:, 5])
        good = (rows[:, 2] >= 0) & (rows[:, 3] >= 0) & (ia >= 0) & (ib >= 0)
        w = np.minimum(ROUTES_ORTHO * rows[good, 2] + ROUTES_DIAG * rows[good, 3], ROUTES_INF).astype(np.int32)
        D = np.full((stored, stored), ROUTES_INF, np.int32)
        D[np.arange(stored), np.arange(stored)] = 0
        np.minimum.at(D, (ia[good], ib[good]), w)
        np.minimum.at(D, (ib[good], ia[good]), w)
        for k in range(stored if solver is None else 0):    # (the sum of two entries stays inside int32)
            D = np.minimum(D, np.minimum(D[:, k, None] + D[None, k, :], ROUTES_INF))
        if solver is not None:
            D = solver(D)
        dist[n, :stored, :stored] = D
        info[n] = (total, stored, int(good.sum()), int((~good).sum()))
    return nodes, dist, info


def _score_check(nodes_a, dist_a, info_a, nodes_b, dist_b, info_b, slack):
    arrays = [np.asarray(a) for a in (nodes_a, dist_a, info_a, nodes_b, dist_b, info_b)]
    na = arrays[0]
    if na.ndim != 3 or na.shape[2] != 4 or not 1 <= na.shape[1] <= ROUTES_MAX_NODES or na.shape[0] < 1:
        raise ValueError("route_score: nodes_a must be an integer array [N, max_nodes, 4] with max_nodes in [1, %d], not %r"
                         % (ROUTES_MAX_NODES, na.shape))
    N, cap = na.shape[:2]
    for name, a, shape in zip(("nodes_a", "dist_a", "info_a", "nodes_b", "dist_b", "info_b"), arrays,
                              ((N, cap, 4), (N, cap, cap), (N, 4)) * 2):
        if a.shape != shape or a.dtype.kind not in "iu":
            raise ValueError("route_score: %s must be an integer array %r, not %s %r" % (name, shape, a.dtype, a.shape))
    _routes_int("route_score", "slack", slack, 0, 1023)
    return arrays, N, cap


def route_score(nodes_a, dist_a, info_a, nodes_b, dist_b, info_b, slack, fill=0):
    """rsu_route_score on the host: (match int32 [N, max_nodes], acc int64 [4]) of two graphs in graph_routes' formats with one
    max_nodes. match[n, i], for every stored node i of a, is the stored node j of b with the smallest (dy)^2 + (dx)^2 (ties: the smaller
    j) where that is at most slack^2, else -1; rows at and past the stored count keep `fill`. Every pair i < k of a with
    0 < d = dist_a[i, k] < ROUTES_INF adds to acc = {pairs, sum q, unmatched, broken}: q = ROUTES_Q where either node is unmatched
    (unmatched) or e = dist_b[match i, match k] is ROUTES_INF (broken), else min(ROUTES_Q, ROUTES_Q |d - e| // d). The direction's score is
    1 - sum q / (ROUTES_Q pairs) (route_metrics)."""
    (na, da, fa, nb, db, fb), N, cap = _score_check(nodes_a, dist_a, info_a, nodes_b, dist_b, info_b, slack)
    match = np.full((N, cap), fill, np.int32)
    acc = np.zeros(4, np.int64)
    for n in range(N):
        sa, sb = (min(max(int(f[n, 1]), 0), cap) for f in (fa, fb))
        pa, pb = na[n, :sa, 1:3].astype(np.int64), nb[n, :sb, 1:3].astype(np.int64)
        if sb:
            d2 = ((pa[:, None, :] - pb[None, :, :]) ** 2).sum(axis=2)
            best = np.argmin(d2, axis=1)                     # (the first of equal minima: the smaller j)
            m = np.where(d2[np.arange(sa), best] <= int(slack) ** 2, best, -1)
        else:
            m = np.full(sa, -1, np.int64)
        match[n, :sa] = m
        i, k = np.triu_indices(sa, 1)
        d = da[n, i, k].astype(np.int64)
        pair = (d > 0) & (d < ROUTES_INF)
        i, k, d = i[pair], k[pair], d[pair]
        lost = (m[i] < 0) | (m[k] < 0)
        e = np.where(lost, ROUTES_INF, db[n, np.maximum(m[i], 0), np.maximum(m[k], 0)].astype(np.int64)) if sb else np.full(d.size, ROUTES_INF, np.int64)
        broken = ~lost & (e >= ROUTES_INF)
        q = np.where(lost | broken, ROUTES_Q, np.minimum(ROUTES_Q, ROUTES_Q * np.abs(d - e) // np.maximum(d, 1)))
        acc += np.array([d.size, q.sum(), lost.sum(), broken.sum()], np.int64)
    return match, acc


def route_metrics(acc_true_to_pred, acc_pred_to_true, info_sums):
    """The path-length figures of a validation pass from the two directions' rsu_route_score counters ({pairs, sum q, unmatched, broken}
    each) and info_sums = rsu_graph_routes' info summed over the patches, of the prediction then of the truth ({nodes, nodes stored, edges
    used, rows skipped} each), per direction * in (true_to_pred, pred_to_true) and side + in (pred, true):
      apls_*               = 1 - sum q / (ROUTES_Q pairs), 0 without a pair,
      route_pairs_*, route_unmatched_*, route_broken_* = the pairs, those with an unmatched node, those whose counterparts no path joins,
      graph_nodes_+        = the nodes, graph_nodes_dropped_+ = those past --max_graph_nodes,
    and apls = the harmonic mean of the two directions, 0 where either has no pairs. The control points are the graphs' own nodes: no
    points are injected along the edges (include/rsu_routes.h)."""
    out, score = {}, []
    s = np.asarray(info_sums)
    if s.shape != (8,) or s.dtype.kind not in "iu" or (s.astype(np.int64) < 0).any():
        raise ValueError("route_metrics: info_sums must be eight integers >= 0, not %s %r" % (s.dtype, s.shape))
    for name, acc in (("true_to_pred", acc_true_to_pred), ("pred_to_true", acc_pred_to_true)):
        a = np.asarray(acc)
        if a.shape != (4,) or a.dtype.kind not in "iu" or (a.astype(np.int64) < 0).any():
            raise ValueError("route_metrics: acc_%s must be four integers >= 0, not %s %r" % (name, a.dtype, a.shape))
        pairs, q, unmatched, broken = (int(v) for v in a)
        if q > ROUTES_Q * pairs or unmatched + broken > pairs:
            raise ValueError("route_metrics: acc_%s = %r is no sum over %d pairs" % (name, a.tolist(), pairs))
        score.append(1.0 - q / float(ROUTES_Q * pairs) if pairs else 0.0)
        out.update({"apls_" + name: score[-1], "route_pairs_" + name: pairs, "route_unmatched_" + name: unmatched, "route_broken_" + name: broken})
    t, p = score
    out["apls"] = 2.0 * t * p / (t + p) if int(np.asarray(acc_true_to_pred)[0]) and int(np.asarray(acc_pred_to_true)[0]) and t + p > 0.0 else 0.0
    for side, name in enumerate(("pred", "true")):
        if int(s[4 * side + 1]) > int(s[4 * side]):
            raise ValueError("route_metrics: more stored nodes (%d) than nodes (%d)" % (int(s[4 * side + 1]), int(s[4 * side])))
        out["graph_nodes_" + name], out["graph_nodes_dropped_" + name] = int(s[4 * side]), int(s[4 * side]) - int(s[4 * side + 1])
    return out
