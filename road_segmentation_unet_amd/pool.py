"""The training-patch pool and the input path of the train loop.

The reference cuts EVERY training patch out of the rotated, mirror-extended images up front (tf_aerial_images.py:404-418 ->
images.extract_patches, images.py:35-85): a float64 array of 28-34 GB at the README configuration, from which each step feeds
`patches[batch_indices]` (tf_aerial_images.py:233-239). Here the pool is an index: patch k of the reference's array is a window of
extended image k // pps^2 at (x, y) = ((r // pps) * stride, (r % pps) * stride), r = k % pps^2 (x outer, y inner) -- the same
patches in the same order, cut when a batch asks for them.

  PatchPool        host float32 images; gather() returns numpy batches (what ConvolutionalModel.train accepts next to the
                   reference's plain arrays); BatchUploader moves them through pinned memory on a copy stream, one batch ahead.
  DevicePatchPool  the extended images live in HBM (a few GB of 288); load_batch() cuts the windows on the GPU straight into the
                   network's input buffers: no host work, no PCIe traffic per step. Optionally applies the stochastic D4
                   augmentation the reference intended but never ran (stochastic_images_augmentation, tf_aerial_images.py:173-210:
                   the graph feeds the augmented tensor itself, so the subgraph is bypassed): per sample,
                   flip up-down / flip left-right / transpose with probability 1/2 each, then rot90 by a uniform k in 0..3, applied
                   alike to the input window and its label patch. Off by default (parity with the reference's actual behaviour).
                   With rotation > 0, scale != (1, 1) or one_launch, load_batch() is ONE rsu_affine_patches call (include/rsu.h) for the
                   whole batch instead: every sample goes through a 2x2 matrix of its own, M = (1 / s) R(theta) D -- a random zoom s,
                   a random rotation theta, the sample's D4 draw D -- with bilinear taps reflected about the original image's edges.
                   Continuous rotation and zoom then cost no further copy of the training set; the plain window (M = 1) and D4 (M = D)
                   are the same launch and deliver the loop's bits.
                   With jitter = (B, C, S, H) or noise above zero, load_batch() then makes ONE rsu_color_jitter call on the finished input
                   windows: brightness, contrast about the sample's own mean, saturation, hue and noise, drawn per sample from a
                   generator of their own (the geometric draws, and with them the labels, do not move).
                   With elastic = (alpha, grid) and alpha > 0, the batch goes through ONE rsu_elastic_patches call instead of
                   rsu_affine_patches: the same launch shape with a smooth random displacement of every output pixel in front of the
                   sample's matrix -- the U-Net paper's elastic deformation: control points on a lattice of `grid` cells per axis
                   across the input window, interpolated by a cubic B-spline, formed per pixel inside the kernel from one 32-bit key
                   per sample. alpha is the standard deviation of the CONTROL POINTS in output pixels; the interpolated field's
                   deviation is smaller (the spline averages 16 neighbours). A large alpha on a fine grid (above about S / (3 grid)) can
                   fold the field: nothing prevents it, the choice is the user's. The keys come from a generator of their own: the
                   geometric and the jitter draws do not move. Labels are displaced by exactly the field their window pixel sees. The
                   effect on F1 is not measured.
"""
import ctypes
import math

import numpy as np
import torch


class PatchPool:
    def __init__(self, extended_images, extended_labels, input_size, patch_size, stride):
        ei, el = np.asarray(extended_images), np.asarray(extended_labels)
        assert ei.ndim == 4 and el.ndim == 3 and ei.shape[0] == el.shape[0]
        assert ei.shape[1] == ei.shape[2] and el.shape[1] == el.shape[2], "Assume square images"
        self.S, self.P, self.stride = int(input_size), int(patch_size), int(stride)
        assert (ei.shape[1] - self.S) % self.stride == 0 and (el.shape[1] - self.P) % self.stride == 0, \
            "Stride sliding should cover the whole image"
        self.pps = (ei.shape[1] - self.S) // self.stride + 1
        assert self.pps == (el.shape[1] - self.P) // self.stride + 1, "image and label pools must tile alike"
        self.images = np.ascontiguousarray(ei, dtype=np.float32)
        self.labels = np.ascontiguousarray(el >= 0.5, dtype=np.uint8)  # tf_aerial_images.py:220 binarises at 0.5
        self.shape = (self.images.shape[0] * self.pps * self.pps, self.S, self.S, self.images.shape[-1])

    def __len__(self):
        return self.shape[0]

    def locate(self, k):
        """(image, x, y) of patch k in the reference's extract_patches order"""
        n, r = divmod(int(k), self.pps * self.pps)
        return n, (r // self.pps) * self.stride, (r % self.pps) * self.stride

    def gather(self, indices):
        """patches float32 [b, S, S, C] and labels float32 [b, P, P] in {0, 1} == patches[indices], labels_patches[indices]"""
        b = len(indices)
        x = np.empty((b, self.S, self.S, self.images.shape[-1]), np.float32)
        y = np.empty((b, self.P, self.P), np.float32)
        for j, k in enumerate(indices):
            n, x0, y0 = self.locate(k)
            x[j] = self.images[n, y0:y0 + self.S, x0:x0 + self.S]
            y[j] = self.labels[n, y0:y0 + self.P, x0:x0 + self.P]
        return x, y


def d4_draw(rng, count):
    """per sample (flip_ud, flip_lr, transpose, k): the draws of tf_aerial_images.py:183-201 (proba > 0.5; floor(U * 4))"""
    u = rng.random_sample((count, 4))
    return [(bool(a > 0.5), bool(b > 0.5), bool(c > 0.5), int(np.floor(d * 4))) for a, b, c, d in u]


def d4_apply(t, op):
    """t: [H, W(, C)] tensor (square); tf.image.flip_up_down / flip_left_right / transpose_image / rot90 (counter-clockwise)"""
    ud, lr, tr, k = op
    if ud:
        t = torch.flip(t, (0,))
    if lr:
        t = torch.flip(t, (1,))
    if tr:
        t = t.transpose(0, 1)
    if k:
        t = torch.rot90(t, k, (0, 1))
    return t


def d4_matrix(op):
    """The 2x2 integer matrix D with d4_apply(t, op)[p] = t[D p] for pixel offsets p = (row, column) from the centre of the square: the
    flips negate a coordinate, the transpose swaps them, one rot90 (counter-clockwise) reads (row, column) at (column, -row); d4_apply
    runs them in that order, so the source offset of an output offset is U L T R^k p."""
    ud, lr, tr, k = op
    D = np.eye(2, dtype=np.int64)
    if ud:
        D = D @ np.array([[-1, 0], [0, 1]])
    if lr:
        D = D @ np.array([[1, 0], [0, -1]])
    if tr:
        D = D @ np.array([[0, 1], [1, 0]])
    for _ in range(int(k) % 4):
        D = D @ np.array([[0, 1], [-1, 0]])
    return D


def check_rotation_scale(rotation, scale):
    """(rotation in degrees, (lo, hi)) as floats; ValueError unless rotation is finite and >= 0 and 1/64 < lo <= hi <= 64"""
    try:
        rot = float(rotation)
        lo, hi = (float(v) for v in scale)
    except (TypeError, ValueError):
        rot = lo = hi = float("nan")
    if not (math.isfinite(rot) and rot >= 0.0):
        raise ValueError("rotation must be a finite number of degrees >= 0, not %r" % (rotation,))
    if not (math.isfinite(lo) and math.isfinite(hi) and 1.0 / 64 < lo <= hi <= 64.0):
        raise ValueError("scale must be (lo, hi) with 1/64 < lo <= hi <= 64, not %r" % (scale,))
    return rot, (lo, hi)


def affine_draw(rng, count, rotation=0.0, scale=(1.0, 1.0), d4=False):
    """Per sample, in this order from `rng`: the four D4 uniforms of d4_draw (only with d4, so a D4-only draw consumes the stream exactly
    as d4_draw does), u for the angle theta = (2u - 1) * rotation degrees (only with rotation > 0), u for the zoom s = exp(U(log lo,
    log hi)) (only with scale != (1, 1)). Returns float32 [count, 2, 2]: M = (1 / s) R(theta) D, R(theta) = [[cos, -sin], [sin, cos]] on
    (row, column) offsets, D = d4_matrix of the sample's draw; float64 arithmetic, rounded once. M maps an output offset to a source offset:
    the sample shows its source zoomed IN by s."""
    rot, (lo, hi) = check_rotation_scale(rotation, scale)
    zoom = (lo, hi) != (1.0, 1.0)
    ncol = (4 if d4 else 0) + (1 if rot > 0.0 else 0) + (1 if zoom else 0)
    M = np.empty((count, 2, 2), np.float32)
    u = rng.random_sample((count, ncol)) if ncol else np.zeros((count, 0))
    for j in range(count):
        col = 0
        D = np.eye(2)
        if d4:
            a, b, c, d = u[j, :4]
            D = d4_matrix((bool(a > 0.5), bool(b > 0.5), bool(c > 0.5), int(np.floor(d * 4)))).astype(np.float64)
            col = 4
        theta, s = 0.0, 1.0
        if rot > 0.0:
            theta = math.radians((2.0 * u[j, col] - 1.0) * rot)
            col += 1
        if zoom:
            s = math.exp(math.log(lo) + u[j, col] * (math.log(hi) - math.log(lo)))
        R = np.array([[math.cos(theta), -math.sin(theta)], [math.sin(theta), math.cos(theta)]])
        M[j] = ((1.0 / s) * R) @ D
    return M


def check_elastic(elastic):
    """(alpha, grid) as (float, int); ValueError unless alpha is finite and in [0, 64] and grid is an integer in [1, 16]"""
    try:
        alpha, grid = elastic
        a = float(alpha)
    except (TypeError, ValueError):
        alpha, a, grid = None, float("nan"), 0
    if isinstance(alpha, bool) or isinstance(grid, bool) or not isinstance(grid, (int, np.integer)) \
            or not (math.isfinite(a) and 0.0 <= a <= 64.0) or not 1 <= grid <= 16:
        raise ValueError("elastic must be (alpha, grid) with alpha in [0, 64] pixels and an integer grid in [1, 16], not %r" % (elastic,))
    return a, int(grid)


def elastic_draw(rng, count, alpha, grid):
    """Per sample from `rng`, only with alpha > 0: key = rng.randint(0, 2**32). Uniform 32-bit keys: the lattice's hash XORs the key in, so
    keys that differ in low bits only would give permuted copies of one lattice. Returns uint32 [count] (zeros, nothing drawn, with
    alpha == 0)."""
    a, _ = check_elastic((alpha, grid))
    keys = np.zeros(count, dtype=np.uint32)
    if a > 0.0:
        for j in range(count):
            keys[j] = rng.randint(0, 2 ** 32)
    return keys


LUMA = (0.299, 0.587, 0.114)   # the weights saturation mixes towards (ITU-R BT.601, tf.image.rgb_to_grayscale)


def check_jitter(jitter, noise):
    """((B, C, S, H), sigma) as floats; ValueError unless B, C, S are finite and in [0, 1), H is in [0, 180] and sigma in [0, 1]"""
    try:
        jit = tuple(float(v) for v in jitter)
    except (TypeError, ValueError):
        jit = ()
    if len(jit) != 4 or any(isinstance(v, bool) for v in jitter) or not all(math.isfinite(v) for v in jit) \
            or not all(0.0 <= v < 1.0 for v in jit[:3]) or not 0.0 <= jit[3] <= 180.0:
        raise ValueError("jitter must be (B, C, S, H) with B, C, S in [0, 1) and H in [0, 180] degrees, not %r" % (jitter,))
    try:
        sigma = float(noise)
    except (TypeError, ValueError):
        sigma = float("nan")
    if isinstance(noise, bool) or not (math.isfinite(sigma) and 0.0 <= sigma <= 1.0):
        raise ValueError("noise must be a float in [0, 1], not %r" % (noise,))
    return jit, sigma


_I3 = np.eye(3)
_LUMA_ROWS = np.outer(np.ones(3), np.array(LUMA))                                                  # 1 w^T
_THIRDS = np.full((3, 3), 1.0 / 3.0)                                                               # u u^T, u = (1, 1, 1) / sqrt 3
_CROSS = np.array([[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]]) / math.sqrt(3.0)         # [u]x


def _jitter_matrices(b, c, s, cos_t, sin_t):
    """jitter_matrices from the angle's cosine and sine; scalars, or arrays [n] for (A, K) [n][3][3]. Products and sums of float64 only,
    in one order: a sample's matrices are the same bits whether formed alone or in a batch."""
    b, c, s, cos_t, sin_t = (np.asarray(v, dtype=np.float64)[..., None, None] for v in (b, c, s, cos_t, sin_t))
    sat = s * _I3 + (1.0 - s) * _LUMA_ROWS
    hue = cos_t * _I3 + (1.0 - cos_t) * _THIRDS + sin_t * _CROSS
    hs = (hue[..., :, 0:1] * sat[..., 0:1, :] + hue[..., :, 1:2] * sat[..., 1:2, :]) + hue[..., :, 2:3] * sat[..., 2:3, :]
    return (c * b) * hs, ((1.0 - c) * b) * hs


def jitter_matrices(b, c, s, theta):
    """(A, K) float64 [3][3] of include/rsu.h rsu_color_jitter for brightness b, contrast c, saturation s and a hue angle theta in degrees:
    A = c b Hue Sat, K = (1 - c) b Hue Sat with Sat = s I + (1 - s) 1 w^T (w = LUMA) and Hue the rotation by theta about (1, 1, 1) / sqrt 3
    (Rodrigues: cos I + (1 - cos) u u^T + sin [u]x). x -> A x + K mean(x) is brightness, then contrast about the per-channel mean
    (tf.image.adjust_contrast), then saturation towards luma, then hue, without clamps in between; grey stays grey under Sat and Hue."""
    t = math.radians(theta)
    return _jitter_matrices(b, c, s, math.cos(t), math.sin(t))


def jitter_draw(rng, count, brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0, noise=0.0):
    """Per sample, in this order from `rng`, each only when its strength is above zero: u for b = 1 + (2u - 1) brightness, u for
    c = 1 + (2u - 1) contrast, u for s = 1 + (2u - 1) saturation, u for theta = (2u - 1) hue degrees, key = rng.randint(0, 2**32) (with
    noise). Uniform 32-bit keys: the noise hash XORs the key in, so keys that differ in low bits only would give locally permuted copies
    of one field. Returns hostio.JITTER_DTYPE records [count]: jitter_matrices formed in float64 and rounded once, sigma = noise."""
    from .hostio import JITTER_DTYPE
    (B, C, S, H), sigma = check_jitter((brightness, contrast, saturation, hue), noise)
    recs = np.zeros(count, dtype=JITTER_DTYPE)
    p = np.empty((5, count))
    for j in range(count):
        p[0, j] = 1.0 + (2.0 * rng.random_sample() - 1.0) * B if B > 0.0 else 1.0
        p[1, j] = 1.0 + (2.0 * rng.random_sample() - 1.0) * C if C > 0.0 else 1.0
        p[2, j] = 1.0 + (2.0 * rng.random_sample() - 1.0) * S if S > 0.0 else 1.0
        t = math.radians((2.0 * rng.random_sample() - 1.0) * H) if H > 0.0 else 0.0
        p[3, j], p[4, j] = math.cos(t), math.sin(t)
        if sigma > 0.0:
            recs["key"][j] = rng.randint(0, 2 ** 32)
    A, K = _jitter_matrices(*p)
    recs["a"], recs["k"], recs["sigma"] = A.reshape(count, 9), K.reshape(count, 9), sigma
    return recs


class DevicePatchPool(PatchPool):
    def __init__(self, extended_images, extended_labels, input_size, patch_size, stride, device, augment=False, seed=2017,
                 rotation=0.0, scale=(1.0, 1.0), one_launch=False, jitter=(0.0, 0.0, 0.0, 0.0), noise=0.0, elastic=(0.0, 3)):
        """elastic: (alpha, grid), the standard deviation of the elastic deformation's control points in output pixels (0 = off: nothing is
        drawn and rsu_affine_patches runs as without it) and the lattice's cells per axis across the input window; alpha > 0 turns
        one_launch on. The keys come from RandomState((seed + 0xbb67ae85) % 2**32), not from the geometric or the jitter stream.
        jitter: (B, C, S, H), the strengths of brightness, contrast, saturation (each in [0, 1): a factor uniform in [1 - v, 1 + v]) and
        hue (degrees, a uniform angle in [-H, H]); noise: sigma in [0, 1] of the per-element noise. All zero = off: nothing is drawn,
        allocated or launched. The draws come from RandomState((seed + 0x6a09e667) % 2**32), not from the geometric stream.
        rotation: degrees; a sample is rotated by a uniform angle in [-rotation, rotation] (0 = off). scale: (lo, hi); a sample is
        zoomed by a log-uniform factor in [lo, hi] ((1, 1) = off). one_launch: send plain and D4-only batches through the kernel too."""
        super().__init__(extended_images, extended_labels, input_size, patch_size, stride)
        self.device = torch.device(device)
        self.dev_images = torch.from_numpy(self.images).to(self.device)
        self.dev_labels = torch.from_numpy(self.labels).to(self.device)
        self.augment = bool(augment)
        self._rng = np.random.RandomState(seed)
        self.rotation, self.scale = check_rotation_scale(rotation, scale)
        self.elastic = check_elastic(elastic)
        self.elastic_on = self.elastic[0] > 0.0
        self.one_launch = bool(one_launch) or self.rotation > 0.0 or self.scale != (1.0, 1.0) or self.elastic_on
        if self.elastic_on:
            self._elastic_rng = np.random.RandomState((int(seed) + 0xbb67ae85) % 2 ** 32)
        if self.one_launch and self.images.shape[-1] != 3:
            raise ValueError("the one-launch loader cuts 3-channel images, not %d channels" % self.images.shape[-1])
        self.jitter, self.noise = check_jitter(jitter, noise)
        self.jitter_on = any(v > 0.0 for v in self.jitter) or self.noise > 0.0
        self.last_jitter = None   # the rsu_jitter_t records (hostio.JITTER_DTYPE) of the last batch
        self._jitter_ws = None
        if self.jitter_on:
            from . import _lib
            if self.images.shape[-1] != 3:
                raise ValueError("colour jitter and noise need 3-channel images, not %d channels" % self.images.shape[-1])
            self._jitter_rng = np.random.RandomState((int(seed) + 0x6a09e667) % 2 ** 32)
            if self.jitter[1] > 0.0:   # only contrast needs the means: the partial sums of one launch, whatever the batch size
                nbytes = _lib.lib().rsu_color_jitter_ws_bytes(_lib.JITTER_MAX_LAUNCH, self.S)
                self._jitter_ws = torch.empty(nbytes // 8, dtype=torch.int64, device=self.device)

    def affine_records(self, indices, matrices):
        """the rsu_affine_t records (hostio.AFFINE_DTYPE) of patches `indices` under float32 `matrices` [b, 2, 2]"""
        from .hostio import AFFINE_DTYPE
        recs = np.zeros(len(indices), dtype=AFFINE_DTYPE)
        half = (self.S - 1) / 2.0
        for j, k in enumerate(indices):
            n, x0, y0 = self.locate(k)
            recs[j] = (n, y0 + half, x0 + half, matrices[j, 0, 0], matrices[j, 0, 1], matrices[j, 1, 0], matrices[j, 1, 1], 0)
        return recs

    def elastic_records(self, indices, matrices, keys):
        """the rsu_elastic_t records (hostio.ELASTIC_DTYPE) of patches `indices` under float32 `matrices` [b, 2, 2] and lattice `keys` [b],
        with the pool's (alpha, grid)"""
        from .hostio import ELASTIC_DTYPE
        aff = self.affine_records(indices, matrices)
        recs = np.zeros(len(indices), dtype=ELASTIC_DTYPE)
        for name in ("image", "cy", "cx", "m00", "m01", "m10", "m11"):
            recs[name] = aff[name]
        recs["alpha"], recs["key"], recs["grid"] = self.elastic[0], keys, self.elastic[1]
        return recs

    def _load_batch_one_launch(self, indices, x_out, labels_out):
        from . import _lib
        b = len(indices)
        if tuple(x_out.shape) != (b, self.S, self.S, 3) or x_out.dtype != torch.float32 or not x_out.is_contiguous() \
                or tuple(labels_out.shape) != (b, self.P, self.P) or labels_out.dtype != torch.int64 or not labels_out.is_contiguous() \
                or x_out.device != self.dev_images.device or labels_out.device != self.dev_images.device:
            raise ValueError("load_batch: x_out must be a contiguous float32 [%d, %d, %d, 3] and labels_out a contiguous int64 [%d, %d, %d] "
                             "on %s" % (b, self.S, self.S, b, self.P, self.P, self.dev_images.device))
        matrices = affine_draw(self._rng, b, self.rotation, self.scale, self.augment)
        st = ctypes.c_void_p(torch.cuda.current_stream(self.dev_images.device).cuda_stream)
        if self.elastic_on:
            recs = self.elastic_records(indices, matrices, elastic_draw(self._elastic_rng, b, *self.elastic))
            name, rp = "rsu_elastic_patches", recs.ctypes.data_as(ctypes.POINTER(_lib.RsuElastic))
        else:
            recs = self.affine_records(indices, matrices)
            name, rp = "rsu_affine_patches", recs.ctypes.data_as(ctypes.POINTER(_lib.RsuAffine))
        _lib.call(name, self.dev_images.data_ptr(), self.dev_labels.data_ptr(), rp, b, self.images.shape[0], self.images.shape[1],
                  self.labels.shape[1], self.S, self.P, x_out.data_ptr(), labels_out.data_ptr(), st)
        return recs

    def _jitter_batch(self, x_out):
        """one rsu_color_jitter call on the finished input windows of a batch; its records stay in self.last_jitter"""
        from . import _lib
        b = x_out.shape[0]
        if tuple(x_out.shape) != (b, self.S, self.S, 3) or x_out.dtype != torch.float32 or not x_out.is_contiguous() \
                or x_out.device != self.dev_images.device:
            raise ValueError("load_batch: colour jitter needs x_out as a contiguous float32 [b, %d, %d, 3] on %s"
                             % (self.S, self.S, self.dev_images.device))
        recs = jitter_draw(self._jitter_rng, b, *self.jitter, noise=self.noise)
        st = ctypes.c_void_p(torch.cuda.current_stream(self.dev_images.device).cuda_stream)
        ws = self._jitter_ws.data_ptr() if self._jitter_ws is not None else None
        _lib.call("rsu_color_jitter", x_out.data_ptr(), recs.ctypes.data_as(ctypes.POINTER(_lib.RsuJitter)), b, self.S, ws, st)
        self.last_jitter = recs

    def load_batch(self, indices, x_out, labels_out):
        """x_out f32 [b, S, S, C], labels_out int64 [b, P, P] (device tensors: the network's input buffers). Returns the D4 draws (None
        without augmentation), or the batch's records where the batch went through the one-launch loader (hostio.AFFINE_DTYPE, or
        hostio.ELASTIC_DTYPE with elastic deformation on). With jitter or noise on, the
        input windows are then transformed in place (self.last_jitter: the records)."""
        ret = self._load_batch(indices, x_out, labels_out)
        if self.jitter_on:
            self._jitter_batch(x_out)
        return ret

    def _load_batch(self, indices, x_out, labels_out):
        if self.one_launch:
            return self._load_batch_one_launch(indices, x_out, labels_out)
        ops = d4_draw(self._rng, len(indices)) if self.augment else None
        for j, k in enumerate(indices):
            n, x0, y0 = self.locate(k)
            xi = self.dev_images[n, y0:y0 + self.S, x0:x0 + self.S]
            li = self.dev_labels[n, y0:y0 + self.P, x0:x0 + self.P]
            if ops is not None:
                xi, li = d4_apply(xi, ops[j]), d4_apply(li, ops[j])
            x_out[j].copy_(xi)
            labels_out[j].copy_(li)
        return ops


class BatchUploader:
    """Host batches -> HBM through two pinned buffers and a copy stream, one batch ahead of the step that consumes it: while
    step i runs, batch i+1 is converted to float32 into pinned memory and copied (20.5 MB at config 2: ~0.35 ms of PCIe Gen5)."""

    def __init__(self, net):
        self.net = net
        dev = net.device
        self.stream = torch.cuda.Stream(device=dev)
        self.pin_x = [torch.empty(net.x.shape, dtype=torch.float32).pin_memory() for _ in range(2)]
        self.pin_l = [torch.empty(net.labels.shape, dtype=torch.int64).pin_memory() for _ in range(2)]
        self.dev_x = [torch.empty_like(net.x) for _ in range(2)]
        self.dev_l = [torch.empty_like(net.labels) for _ in range(2)]
        self.ready = [torch.cuda.Event() for _ in range(2)]
        self.consumed = [torch.cuda.Event() for _ in range(2)]
        self._used = [False, False]

    def stage(self, slot, patches, labels):
        """start the upload of one batch (numpy or tensors; float64 inputs are narrowed here, on the host, once)"""
        if self._used[slot]:
            self.consumed[slot].synchronize()  # the step that read this slot's device copy has taken it
        np.copyto(self.pin_x[slot].numpy(), np.asarray(patches), casting="same_kind")
        np.copyto(self.pin_l[slot].numpy(), np.asarray(labels), casting="unsafe")
        with torch.cuda.stream(self.stream):
            self.dev_x[slot].copy_(self.pin_x[slot], non_blocking=True)
            self.dev_l[slot].copy_(self.pin_l[slot], non_blocking=True)
            self.ready[slot].record(self.stream)

    def commit(self, slot):
        """make the staged batch the network's input (device-to-device, on the compute stream)"""
        cur = torch.cuda.current_stream(self.net.device)
        cur.wait_event(self.ready[slot])
        self.net.x.copy_(self.dev_x[slot])
        self.net.labels.copy_(self.dev_l[slot])
        self.consumed[slot].record(cur)
        self._used[slot] = True
