"""Host-side mirror of the reference's network definition (/root/reference/src/unet.py) over the HIP C ABI.

`input_size_needed` and `forward` keep the reference's names, argument meaning and error behaviour
(unet.py:12, unet.py:100); `UNet` owns what the TF graph + session owned: the variables (TF names, TF
layouts, float32), their Momentum slots, the activation buffers and the backward pass
(tf_aerial_images.py:103-122). PyTorch is only the device-memory / stream / collective plumbing: every
arithmetic kernel on the path is a hand-written HIP kernel reached through librsu_hip.so.
"""
import ctypes
import math
import os
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import RsuSrc, RsuWgradJob, call
from .optim import (DECAY_MODES, DEFAULT_LR_SCHEDULE, EMA_SUFFIX, LR_SCHEDULES, OPTIMIZERS, OptimizerStep,  # noqa: F401  (the optimizer step's
                    _PACK_CONV_BWD, _PACK_CONV_FIRST, _PACK_CONV_FWD, _PACK_CONVT_BWD, _PACK_CONVT_FWD, _accumulate_arg, _clip_arg,  # names stay
                    _decay_args, _ema_arg, _int_arg, _ptr, adam_scalars, clip_scale, ema_decay_at, lr_at)   # importable from here as before)
from .schedule import BackwardSchedule, cu_shares  # noqa: F401  (cu_shares: importable from here as before)

NUM_CHANNELS = 3  # src/constants.py:3
NUM_LABELS = 2    # src/constants.py:4


def input_size_needed(output_size, num_layers):
    """Utility function to compute image size for a given U-Net output (reference: unet.py:100-115).

    Same arithmetic, same AssertionError text as the reference."""
    for i in range(num_layers - 1):
        assert output_size % 2 == 0, 'expand layer {} has size {} not divisible by 2' \
            .format(num_layers - i, output_size)
        output_size = (output_size + 4) / 2
    for i in range(num_layers - 1):
        output_size = (output_size + 4) * 2
    return int(output_size + 4)


def param_shapes(num_layers, root_size, dilated_layers):
    """(name, shape) of every variable unet.forward creates, in creation order (unet.py:23,34-45,67,88-91,95)."""
    shapes = [("color_space_adjust/kernel", (1, 1, 3, 3)), ("color_space_adjust/bias", (3,))]
    nf, cin = root_size, NUM_CHANNELS
    for i in range(num_layers):
        if dilated_layers:
            shapes += [("conv_dilut_%d/atrous_conv1/kernel" % i, (3, 3, cin, nf)), ("conv_dilut_%d/atrous_conv1/bias" % i, (nf,)),
                       ("conv_dilut_%d/atrous_conv2/kernel" % i, (3, 3, nf, nf)), ("conv_dilut_%d/atrous_conv2/bias" % i, (nf,))]
        shapes += [("conv_%d/conv1/kernel" % i, (3, 3, cin, nf)), ("conv_%d/conv1/bias" % i, (nf,)),
                   ("conv_%d/conv2/kernel" % i, (3, 3, nf, nf)), ("conv_%d/conv2/bias" % i, (nf,))]
        cin = nf
        nf *= 2
    nf //= 2
    for i in range(num_layers - 1):
        nf //= 2
        shapes += [("up_conv_%d/kernel" % i, (2, 2, nf, 2 * nf)), ("up_conv_%d/bias" % i, (nf,))]
        ccat = (3 if dilated_layers else 2) * nf
        j = num_layers + i
        shapes += [("conv_%d/conv1/kernel" % j, (3, 3, ccat, nf)), ("conv_%d/conv1/bias" % j, (nf,)),
                   ("conv_%d/conv2/kernel" % j, (3, 3, nf, nf)), ("conv_%d/conv2/bias" % j, (nf,))]
    shapes += [("weight_output/kernel", (1, 1, nf, NUM_LABELS)), ("weight_output/bias", (NUM_LABELS,))]
    return shapes


def _is_dead(name, num_layers):
    """The level L-1 dilated pair is built but never consumed (unet.py:57-59): no gradient, never updated."""
    return name.startswith("conv_dilut_%d/" % (num_layers - 1))


def glorot_uniform_params(num_layers, root_size, dilated_layers, seed):
    """tf.layers defaults: glorot_uniform kernels, zero biases. (TF's own seeds are op-id derived and not
    reproducible outside TF; parity tests inject identical weights instead.)"""
    rng = np.random.RandomState(seed)
    out = {}
    for name, shp in param_shapes(num_layers, root_size, dilated_layers):
        if name.endswith("kernel"):
            recept = shp[0] * shp[1]
            limit = math.sqrt(6.0 / (recept * shp[2] + recept * shp[3]))
            out[name] = rng.uniform(-limit, limit, size=shp).astype(np.float32)
        else:
            out[name] = np.zeros(shp, np.float32)
    return out


def dropout_key_value(seed, site, global_step, micro_step=0):
    """The 32-bit dropout key of (seed, dropout site, optimizer step, micro-batch of that step): a sum of the four, each times an odd
    32-bit constant of its own, modulo 2^32. micro_step 0 adds nothing: a net that does not accumulate keeps the keys it always had."""
    return (seed * 0x9E3779B9 + site * 0x85EBCA6B + global_step * 0xC2B2AE35 + micro_step * 0x27D4EB2F) & 0xFFFFFFFF


def _src(t, h, w):
    """window (h, w) centred in NHWC tensor t (crop offset floor((H-h)/2), unet.py:70-83)"""
    H, W, C = t.shape[1], t.shape[2], t.shape[3]
    return RsuSrc(t.data_ptr(), H, W, C, (H - h) // 2, (W - w) // 2)


class UNet(OptimizerStep):
    """Variables + buffers + forward/backward of the U-Net for a FIXED (batch, patch_size) -- the reference's graph is
    static in exactly the same way (tf_aerial_images.py:133-138). The optimizer step is the base class's (optim.py)."""

    def __init__(self, num_layers, root_size, dilated_layers, batch_size, patch_size, device="cuda:0", params=None, seed=2017,
                 training=True, optimizer="momentum", class_weights=None, dice_weight=0.0, dice_smooth=1.0, border_weight=0.0, border_sigma=5.0,
                 clip_grad_norm=None, ema_decay=None, ema_warmup=True, accumulate_steps=None, weight_decay=None, weight_decay_mode="decoupled",
                 focal_gamma=0.0, cldice_weight=0.0, cldice_iters=10, cldice_smooth=1.0, lovasz_weight=0.0):
        """optimizer: "momentum" (the reference's MomentumOptimizer: apply_momentum) or "adam" (tf.train.AdamOptimizer: apply_adam; a
        second fp32 slot per variable, flat_v).
        class_weights: None or a pair (w0, w1) of finite floats >= 0, not both 0: the weighted cross-entropy of rsu.h
        rsu_head_fwd_bwd_w (see backward_device). None and (1, 1) are the reference's unweighted loss.
        dice_weight: lambda >= 0 of the soft-Dice term, loss = cross-entropy + lambda (1 - Dice) (rsu.h rsu_head_fwd_bwd_dice); 0.0: no such
        term, the step issues the launches it always did. dice_smooth: the term's smoothing constant, > 0.
        border_weight: w0 >= 0 of the border-distance weight map (rsu.h rsu_border_map): with w0 > 0 every backward_device and
        evaluate_device first turns self.labels into the map (1 + w0 exp(-D2 / (2 border_sigma^2)), D2 the squared distance to the other
        class inside the patch) times the map of set_pixel_weights, if any, and hands it to the head as its pixel weights; 0.0: no
        buffer, no launch, the passes are what they always were. border_sigma: > 0, in pixels. Training nets only.
        clip_grad_norm: None, or c > 0 (finite): apply_momentum / apply_adam first take the global norm of the live gradient on the
        device (rsu.h rsu_grad_norm) and step with the gradient scaled by min(1, c / norm); a step whose gradient holds an inf or a nan, or
        whose sum of squares overflows, changes nothing (see apply_momentum). No host synchronisation; clip_stats() reads the counters.
        A huge c only measures and guards. None: no buffer, no launch, the step is what it always was.
        ema_decay: None (or 0), or d in (0, 1): apply_momentum / apply_adam end with one rsu_ema_step launch (rsu.h) that moves flat_ema,
        a float32 shadow of flat_w initialised to the initial weights, by tf.train.ExponentialMovingAverage's rule at the decay
        ema_decay_at(d, global_step, ema_warmup); averaged_weights() evaluates with it; state_dict() carries it as
        `<var>/ExponentialMovingAverage`. ema_warmup: TensorFlow's num_updates rule, min(d, (1 + t) / (10 + t)). Training nets only.
        None: no buffer, no launch, the step is what it always was.
        accumulate_steps: None (or 1), or an int K > 1: one optimizer step takes K backward passes over K micro-batches of batch_size
        patches each, with accumulate_gradients() behind every backward_device(); the K-th call leaves the float32 sum of the K
        gradients, ((g_0 + g_1) + ...) + g_{K-1}, in flat_g, where the exchange, the norm and the update pass read it, and
        apply_momentum / apply_adam refuse to step before it. backward_device's inv_count stays 1 / (pixel count of the WHOLE effective
        batch). One more float32 buffer, flat_gsum (4 B per weight), and one rsu_grad_accumulate launch per micro-batch (rsu.h).
        micro_step (0..K-1) enters the dropout keys. Training nets only. None: no buffer, no launch, the step is what it always was.
        weight_decay: None, or lambda > 0 (finite): apply_momentum / apply_adam run the decaying update pass (rsu_optim.h
        rsu_update_table_run_decay / rsu_update_table_run_adam_decay) in place of the plain or clipping one -- one launch, the same grid,
        the same bytes. The packed kernels decay (3x3 convs, the first conv, transposed convs: decaying_parameters() of them); biases, the
        colour-adjust matrix and the 1x1 head do not. weight_decay_mode: "decoupled" (AdamW; under Momentum the same step in front of
        the rule): w -= f32(lr_t) * f32(lambda) * w at the scheduled rate lr_t = learning_rate(lr0), then the rule; or "l2": lambda * w
        joins the gradient behind gscale and the clipping factor (the penalty lambda / 2 |w|^2; loss_sum never includes it). No buffer,
        nothing in state_dict(). The moving average, gradient accumulation and the data-parallel exchange sit in front of or behind
        the update pass and are what they were. Training nets only (ValueError otherwise; bad values raise ValueError too). None: the
        step is what it always was.
        focal_gamma: gamma >= 0 (finite) of the focal cross-entropy (rsu_loss.h): with gamma > 0 every counted pixel's cross-entropy is
        scaled by (1 - p_t)^gamma in backward_device (rsu_head_fwd_bwd_focal) and in evaluate_device (rsu_head_eval_focal): loss_sum and
        eval_sums[0] are then sum omega F CE. It multiplies the class weights, the weight map and the border map; the Dice term is added
        to it unchanged; inv_count stays 1 / pixel count, so the gradient shrinks. Labels other than 0 / 1 are ignored, as in every
        weighted pass. 0.0: the passes issue exactly the launches they always did.
        cldice_weight: lambda >= 0 of the clDice (centre-line Dice) term, objective += lambda (1 - clD) (rsu_cldice.h): the soft skeletons of
        prob and of the label map by cldice_iters (0 .. 16) erosions, cldice_smooth > 0 the term's smoothing constant. With lambda > 0
        backward_device runs the head as pass A, rsu_cldice_fwd, rsu_cldice_bwd and rsu_head_fwd_bwd_aux (see there), evaluate_device adds
        one rsu_cldice_fwd into eval_cldice_sums, and the net owns cldice_sums (f32[4] {A, Bp, Cc, Dy}), eval_cldice_sums, the two
        skeleton maps, gprob and the term's workspace. Class weights, the weight map, the border map and the focal factor do not enter
        the term. 0.0: no buffer, no launch, the passes are what they always were. Training nets only.
        lovasz_weight: lambda >= 0 of the Lovasz (Jaccard surrogate) term, objective += lambda * the mean over the batch's images of the
        per-image Lovasz loss (rsu_lovasz.h). With lambda > 0 backward_device runs the head as pass A, rsu_lovasz_fwd_bwd and
        rsu_head_fwd_bwd_aux (see there), evaluate_device adds one rsu_lovasz_fwd into eval_lovasz_sum, and the net owns lovasz_sum
        (f32[2] {sum_b L_b, images}), eval_lovasz_sum, gprob (shared with the clDice term) and the sort's workspace. Weights and the focal
        factor do not enter the term. 0.0: no buffer, no launch. Training nets only.
        The learning-rate curve is set_lr_schedule()'s; the default is the reference's staircase."""
        self._init_optimizer(training, optimizer, clip_grad_norm, ema_decay, ema_warmup, accumulate_steps, weight_decay, weight_decay_mode)
        assert root_size % 8 == 0 and (root_size // 8) & (root_size // 8 - 1) == 0, "root_size must be 8 * 2^k for the HIP path"
        self.L, self.root, self.dilated = num_layers, root_size, bool(dilated_layers)
        self.B, self.P = batch_size, patch_size
        self.S = input_size_needed(patch_size, num_layers)
        self.device = torch.device(device)
        if self.device.type == "cuda":
            torch.cuda.set_device(self.device)  # the library works on the HIP current device (rsu.h "devices")
        self.training = training
        self.class_weights = class_weights   # (a property: validated, mirrored to the device as f32[2])
        self.pixel_weights = None            # the weight map [B, P, P] float32 on the device, or None (set_pixel_weights)
        self.dice_weight, self.dice_smooth = dice_weight, dice_smooth   # (properties: validated)
        self.focal_gamma = focal_gamma       # (a property: validated)
        self.cldice_weight, self.cldice_iters, self.cldice_smooth = cldice_weight, cldice_iters, cldice_smooth   # (properties: validated)
        if self._cldice_weight > 0.0 and not training:
            raise _lib.RsuError("a forward-only net has no loss to add a clDice term to")
        self.cldice_sums = self.eval_cldice_sums = self.skel_p = self.skel_y = self.gprob = self._cldice_ws = None
        self.lovasz_weight = lovasz_weight   # (a property: validated)
        if self._lovasz_weight > 0.0 and not training:
            raise _lib.RsuError("a forward-only net has no loss to add a Lovasz term to")
        self.lovasz_sum = self.eval_lovasz_sum = self._lovasz_ws = None
        self.border_weight, self.border_sigma = self._border_args(border_weight, border_sigma)
        self.border_map = None               # the generated weight map [B, P, P] float32 (derived from labels per pass), with border_weight > 0
        self.keep = 1.0        # dropout keep probability of the forward pass in flight (set by forward_device)
        self.dropout_seed = int(seed) if seed is not None else 0
        self.backward_cu_budget = None   # CUs the backward launches may plan for in total (None: the library's default)
        self._tuned = set()    # (training?, backward_cu_budget, dropout?) combinations the tuning pass has run for (tune / ensure_tuned)
        # which stream, CU share, weight-gradient group and workspace every launch gets; its side streams are `wstreams`
        # (the schedule reaches _timed through a weak reference: net -> sched -> bound method -> net would be a cycle, and a dropped net would
        # hold its device buffers until Python's next FULL collection, which a long-running process with many objects rarely runs)
        me = weakref.ref(self)
        self.sched = BackwardSchedule(self.device, batch_size, training, lambda *args: me()._timed(*args))
        self.wstream = self.wstreams[0] if self.wstreams else None   # the first side stream
        self.pool_code = {}
        self.prof = None       # list collecting (tag, algorithmic flops, start event, end event, CU share) when profiling
        self.on_grads = None   # callback(lo): every gradient at flat position >= lo is final (see dist.GradBucketer)
        _lib.lib()  # fail loudly now if the HIP extension is missing
        self._check_tensor_sizes()
        self._alloc_params(params if params is not None else glorot_uniform_params(num_layers, root_size, dilated_layers, seed))
        self._alloc_buffers()
        self.repack()

    @property
    def class_weights(self):
        """None or the pair (w0, w1) that scales the loss of the pixels labelled 0 / 1 (backward_device)"""
        return self._class_weights

    @class_weights.setter
    def class_weights(self, cw):
        if cw is not None:
            cw = tuple(float(v) for v in cw)
            if len(cw) != 2 or not all(math.isfinite(v) and v >= 0.0 for v in cw) or cw == (0.0, 0.0):
                raise _lib.RsuError("class_weights must be None or two finite floats >= 0, not both 0; got %r" % (cw,))
        self._class_weights = cw
        self._class_w_dev = torch.tensor(cw, dtype=torch.float32, device=self.device) if cw is not None else None

    @property
    def dice_weight(self):
        """lambda of the soft-Dice term: the default dice_scale of backward_device (0.0: the cross-entropy alone)"""
        return self._dice_weight

    @dice_weight.setter
    def dice_weight(self, v):
        try:
            v = float(v)
        except (TypeError, ValueError):
            v = float("nan")
        if not (math.isfinite(v) and v >= 0.0):
            raise _lib.RsuError("dice_weight must be a finite float >= 0")
        self._dice_weight = v

    @property
    def focal_gamma(self):
        """gamma of the focal cross-entropy (rsu_loss.h): > 0 sends backward_device and evaluate_device to the focal heads; 0.0: no
        modulation, the launches of a net without it"""
        return self._focal_gamma

    @focal_gamma.setter
    def focal_gamma(self, v):
        try:
            v = float(v)
        except (TypeError, ValueError):
            v = float("nan")
        if not (math.isfinite(v) and v >= 0.0):
            raise _lib.RsuError("focal_gamma must be a finite float >= 0")
        self._focal_gamma = v

    @property
    def cldice_weight(self):
        """lambda of the clDice term: the default cldice_scale of backward_device (0.0: no such term)"""
        return self._cldice_weight

    @cldice_weight.setter
    def cldice_weight(self, v):
        try:
            v = float(v)
        except (TypeError, ValueError):
            v = float("nan")
        if not (math.isfinite(v) and v >= 0.0):
            raise _lib.RsuError("cldice_weight must be a finite float >= 0")
        self._cldice_weight = v

    @property
    def cldice_iters(self):
        """k: the erosions of the soft skeleton (rsu_cldice.h), an int in [0, 16]"""
        return self._cldice_iters

    @cldice_iters.setter
    def cldice_iters(self, v):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= _lib.CLDICE_MAX_ITERS:
            raise _lib.RsuError("cldice_iters must be an int in [0, %d]" % _lib.CLDICE_MAX_ITERS)
        self._cldice_iters = int(v)

    @property
    def cldice_smooth(self):
        """the smoothing constant s of Tp = (A + s) / (Bp + s), Ts = (Cc + s) / (Dy + s)"""
        return self._cldice_smooth

    @cldice_smooth.setter
    def cldice_smooth(self, v):
        try:
            v = float(v)
        except (TypeError, ValueError):
            v = float("nan")
        if not (math.isfinite(v) and v > 0.0):
            raise _lib.RsuError("cldice_smooth must be a finite float > 0")
        self._cldice_smooth = v

    def _cldice_buffers(self):
        """the term's device buffers, made when a pass first needs them (in __init__ with cldice_weight > 0): the sums of the training
        and of the evaluation pass, the skeletons of prob and of the labels, gprob = d term / d prob, and the workspace the forward
        leaves for the backward (rsu_cldice_ws_floats; it grows with cldice_iters)"""
        need = int(_lib.lib().rsu_cldice_ws_floats(self.B, self.P, self.P, self._cldice_iters))
        if self.cldice_sums is None:
            dev = self.device
            self.cldice_sums = torch.zeros(4, dtype=torch.float32, device=dev)
            self.eval_cldice_sums = torch.zeros(4, dtype=torch.float32, device=dev)
            self.skel_p, self.skel_y = (torch.zeros((self.B, self.P, self.P), dtype=torch.float32, device=dev) for _ in range(2))
        if self.gprob is None:
            self.gprob = torch.zeros((self.B, self.P, self.P), dtype=torch.float32, device=self.device)
        if self._cldice_ws is None or self._cldice_ws.numel() < need:
            self._cldice_ws = torch.zeros(need, dtype=torch.float32, device=self.device)

    def _cldice_fwd(self, sums):
        """rsu_cldice_fwd of self.prob / self.labels on the current stream: the skeletons, and sums += {A, Bp, Cc, Dy}"""
        call("rsu_cldice_fwd", _ptr(self.prob), _ptr(self.labels), self._cldice_iters, _ptr(self.skel_p), _ptr(self.skel_y), _ptr(sums),
             _ptr(self._cldice_ws), self.B, self.P, self.P, self._stream())

    @property
    def lovasz_weight(self):
        """lambda of the Lovasz term: the default lovasz_scale of backward_device (0.0: no such term)"""
        return self._lovasz_weight

    @lovasz_weight.setter
    def lovasz_weight(self, v):
        try:
            v = float(v)
        except (TypeError, ValueError):
            v = float("nan")
        if not (math.isfinite(v) and v >= 0.0):
            raise _lib.RsuError("lovasz_weight must be a finite float >= 0")
        self._lovasz_weight = v

    def _lovasz_buffers(self):
        """the term's device buffers, made when a pass first needs them (in __init__ with lovasz_weight > 0): {sum_b L_b, images} of the
        training and of the evaluation pass, gprob (the clDice term's, if that made it first) and the sort's workspace"""
        if self.lovasz_sum is None:
            dev = self.device
            self.lovasz_sum = torch.zeros(2, dtype=torch.float32, device=dev)
            self.eval_lovasz_sum = torch.zeros(2, dtype=torch.float32, device=dev)
            need = int(_lib.lib().rsu_lovasz_ws_bytes(self.B, self.P, self.P))
            if need == 0:
                raise _lib.RsuError("the Lovasz term takes patches of at most 2^24 pixels")
            self._lovasz_ws = torch.zeros(need // 4, dtype=torch.int32, device=dev)
        if self.gprob is None:
            self.gprob = torch.zeros((self.B, self.P, self.P), dtype=torch.float32, device=self.device)

    @property
    def dice_smooth(self):
        """the smoothing constant s of D = (2 I + s) / (P + Y + s)"""
        return self._dice_smooth

    @dice_smooth.setter
    def dice_smooth(self, v):
        try:
            v = float(v)
        except (TypeError, ValueError):
            v = float("nan")
        if not (math.isfinite(v) and v > 0.0):
            raise _lib.RsuError("dice_smooth must be a finite float > 0")
        self._dice_smooth = v

    def _border_args(self, w0, sigma):
        try:
            w0, sigma = float(w0), float(sigma)
        except (TypeError, ValueError):
            w0 = sigma = float("nan")
        if not (math.isfinite(w0) and w0 >= 0.0 and math.isfinite(sigma) and sigma > 0.0):
            raise _lib.RsuError("border_weight must be a finite float >= 0 and border_sigma a finite float > 0")
        if w0 > 0.0 and not self.training:
            raise _lib.RsuError("a forward-only net has no loss to weight")
        if w0 > 0.0 and self.P > _lib.BORDER_MAX_SIDE:
            raise _lib.RsuError("border_weight needs patch_size <= %d (rsu.h rsu_border_map), not %d" % (_lib.BORDER_MAX_SIDE, self.P))
        return w0, sigma

    def set_pixel_weights(self, t):
        """The per-pixel weight map of the loss (backward_device): `t` [B, P, P] (tensor or array, any float type) is copied into the
        device tensor `pixel_weights` (float32, allocated on first use; later calls reuse it, so a captured or queued step keeps reading
        the same memory); None removes the map. Training nets only."""
        if t is None:
            self.pixel_weights = None
            return
        if not self.training:
            raise _lib.RsuError("a forward-only net has no loss to weight")
        if self.__dict__.get("_pixel_w_buf") is None:
            self._pixel_w_buf = torch.ones((self.B, self.P, self.P), dtype=torch.float32, device=self.device)
        src = torch.as_tensor(t)
        if tuple(src.shape) != tuple(self._pixel_w_buf.shape):
            raise _lib.RsuError("pixel weights must have shape %s, not %s" % (tuple(self._pixel_w_buf.shape), tuple(src.shape)))
        self._pixel_w_buf.copy_(src)
        self.pixel_weights = self._pixel_w_buf

    def loss_is_weighted(self):
        """whether the next backward pass takes the weighted head (rsu_head_fwd_bwd_w): class weights other than (1, 1), a weight map, or
        the generated border map (border_weight > 0)"""
        return ((self._class_weights is not None and self._class_weights != (1.0, 1.0)) or self.pixel_weights is not None
                or self.border_weight > 0.0)

    def _head_pixel_weights(self):
        """The head's pixel weights for the pass being issued: the caller's map (or None), or -- border_weight > 0 -- the border map of
        self.labels times it, computed here, on the current stream, in front of the head launch (rsu.h rsu_border_map: two short launches,
        no synchronisation; measured beside the head in profiles/r07/border_map.txt)."""
        if self.border_weight <= 0.0:
            return self.pixel_weights
        call("rsu_border_map", _ptr(self.labels), _ptr(self.pixel_weights), _ptr(self.border_map), None, _ptr(self._border_ws), self.B, self.P,
             self.P, self.border_weight, self.border_sigma, self._stream())
        return self.border_map

    @property
    def wstreams(self):
        """the side streams of the backward schedule: a host may assign [] for single-stream passes and assign the list back"""
        return self.sched.streams

    @wstreams.setter
    def wstreams(self, streams):
        self.sched.streams = streams

    # ------------------------------------------------------------------ parameters
    def _alloc_params(self, init):
        shapes = param_shapes(self.L, self.root, self.dilated)
        live = [(n, s) for n, s in shapes if not _is_dead(n, self.L)]
        dead = [(n, s) for n, s in shapes if _is_dead(n, self.L)]
        self.names = [n for n, _ in shapes]
        off, self._slices = 0, {}
        for n, s in live + dead:
            if n == (dead[0][0] if dead else None):
                self.n_live = off
            cnt = int(np.prod(s))
            self._slices[n] = (off, cnt, s)
            off += (cnt + 3) // 4 * 4  # 16-byte aligned starts
        if not dead:
            self.n_live = off
        self.n_flat = off
        dev = self.device
        self.flat_w = torch.zeros(off, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(off, dtype=torch.float32, device=dev)
        self.w, self.g = {}, {}
        for n, (o, cnt, s) in self._slices.items():
            self.w[n] = self.flat_w[o:o + cnt].view(s)
            self.g[n] = self.flat_g[o:o + cnt].view(s)
            self.w[n].copy_(torch.from_numpy(np.ascontiguousarray(init[n], dtype=np.float32)))
        self._alloc_optimizer_state()

    def state_dict(self):
        """TF variable names, TF layouts (HWIO / [kh,kw,out,in]) + Momentum slots + global_step. An Adam net: the slots are
        `<var>/Adam` (m) and `<var>/Adam_1` (v), plus the float32 scalars `beta1_power` and `beta2_power` once a step has set them.
        An averaging net (ema_decay): `<var>/ExponentialMovingAverage`, TensorFlow's shadow-variable name, for every variable."""
        self._not_averaged("state_dict")
        d = {n: self.w[n].detach().cpu().numpy().copy() for n in self.names}
        d.update(self._optimizer_state_dict())
        return d

    def load_state_dict(self, d):
        """Weights, slots and global_step from a state_dict() (or a TensorFlow checkpoint renamed to it). A Momentum net reads the
        `/Momentum` slots present and ignores Adam keys. An Adam net reads `/Adam`, `/Adam_1`, `beta1_power`, `beta2_power`; a checkpoint
        without Adam slots (a Momentum run's) loads the weights and global_step, zeroes m and v and resets the powers: the next
        apply_adam starts them at its (beta1, beta2), as a fresh AdamOptimizer does. An averaging net reads
        `<var>/ExponentialMovingAverage`; a variable whose key is missing gets the loaded weights as its average (a shadow starts at its
        variable's value). A net without averaging ignores those keys."""
        self._not_averaged("load_state_dict")
        self._load_count = getattr(self, "_load_count", 0) + 1
        for n in self.names:
            self.w[n].copy_(torch.from_numpy(np.ascontiguousarray(d[n], dtype=np.float32)))
        self._load_optimizer_state(d)
        self.repack()

    def _check_tensor_sizes(self):
        """The kernels address a tensor through 32-bit byte offsets: every activation must stay below 2 GiB (the entry points
        return RSU_E2BIG otherwise). Checked here, where the batch is chosen, with the largest batch that fits."""
        h0 = self.S - 2                                    # level-0 conv1 output, `root` channels: the largest tensor of a level
        per_patch = max(self.S * self.S * 16, h0 * h0 * self.root) * 2
        limit = 0x7ffffff0
        if self.B * per_patch >= limit:
            raise _lib.RsuError("batch_size %d is too large for num_layers=%d patch_size=%d: the level-0 activations (%d bytes per patch) "
                                "must stay below 2 GiB per tensor; the largest per-GPU batch is %d"
                                % (self.B, self.L, self.P, per_patch, (limit - 1) // per_patch))

    # ------------------------------------------------------------------ buffers
    def _bf(self, *shape):
        return torch.zeros(shape, dtype=torch.bfloat16, device=self.device)

    def _alloc_buffers(self):
        B, L, S = self.B, self.L, self.S
        dev = self.device
        self.x = torch.zeros((B, S, S, 3), dtype=torch.float32, device=dev)
        self.in16 = self._bf(B, S, S, 16)
        self.act, self.grad = {}, {}
        h, nf = S, self.root
        self.level_in = {}
        for i in range(L):
            self.level_in[i] = h
            if self.dilated and i < L - 1:
                self.act["d1_%d" % i] = self._bf(B, h - 4, h - 4, nf)
                self.act["d2_%d" % i] = self._bf(B, h - 8, h - 8, nf)
            self.act["c1_%d" % i] = self._bf(B, h - 2, h - 2, nf)
            self.act["c2_%d" % i] = self._bf(B, h - 4, h - 4, nf)
            if i < L - 1:
                assert (h - 4) % 2 == 0
                self.act["pool_%d" % i] = self._bf(B, (h - 4) // 2, (h - 4) // 2, nf)
                h = (h - 4) // 2
                nf *= 2
        h = h - 4
        for i in range(L - 1):
            nf //= 2
            j = L + i
            self.act["up_%d" % i] = self._bf(B, 2 * h, 2 * h, nf)
            h = 2 * h
            self.act["c1_%d" % j] = self._bf(B, h - 2, h - 2, nf)
            self.act["c2_%d" % j] = self._bf(B, h - 4, h - 4, nf)
            h -= 4
        assert h == self.P, (h, self.P)
        self.last_name = "c2_%d" % (2 * L - 2) if L > 1 else "c2_0"
        self.prob = torch.zeros((B, self.P, self.P), dtype=torch.float32, device=dev)
        self.logits = torch.zeros((B, self.P, self.P, 2), dtype=torch.float32, device=dev)
        self.labels = torch.zeros((B, self.P, self.P), dtype=torch.int64, device=dev)
        # loss_sum and, next to it, weight_sum (the sum of the pixels' loss weights; written by the weighted head only): one buffer, zeroed
        # by one launch in front of the head
        self._loss_acc = torch.zeros(2, dtype=torch.float32, device=dev)
        self.loss_sum, self.weight_sum = self._loss_acc[0:1], self._loss_acc[1:2]
        # {I, P, Y} of the soft-Dice term: overwritten by the first of the Dice head's two launches, read by the second (rsu.h
        # rsu_head_dice_sums); all zero (D = 1) until a pass with dice_scale > 0 has run
        self.dice_sums = torch.zeros(3, dtype=torch.float32, device=dev)
        # accumulators of held-out validation (rsu.h rsu_head_eval; evaluate_device adds to them, reset_eval zeroes them): the sums
        # {sum omega CE, sum omega, I, P, Y} and the per-class histogram of the probabilities. Not part of state_dict
        self.eval_sums = torch.zeros(5, dtype=torch.float32, device=dev)
        self.eval_hist = torch.zeros((2, _lib.EVAL_BINS), dtype=torch.int64, device=dev)
        # workspace of the conv launches that cut their reduction into slices (rsu.h rsu_conv2d_fwd_k: the deep levels at small batches);
        # one per stream that issues conv launches -- the main stream, and the side stream of the dilated twin blocks in the forward pass
        nk = int(_lib.lib().rsu_conv_splitk_ws_floats()) if os.environ.get("RSU_KSPLIT", "1") != "0" else 0
        self.sched.kws = torch.zeros(nk, dtype=torch.float32, device=dev) if nk else None
        # (one per side stream: whether a layer splits must never depend on which stream its launch went to)
        self.sched.kws_side = [torch.zeros(nk, dtype=torch.float32, device=dev) for _ in self.wstreams] if (nk and self.dilated) else []
        if self.training:
            for k, t in self.act.items():
                if k.startswith("up_") or k.startswith("c") or k.startswith("d") or k.startswith("pool_"):
                    self.grad[k] = torch.zeros_like(t)
            # cropped skip gradients (decoder conv1 bwd-data outputs for the skip sources)
            for i in range(L - 1):
                up = self.act["up_%d" % i]
                self.grad["skip_%d" % i] = torch.zeros_like(up)
                if self.dilated:
                    self.grad["skipd_%d" % i] = torch.zeros_like(up)
            lib = _lib.lib()
            ws = [lib.rsu_head_ws_floats(B * self.P * self.P, self.root), lib.rsu_head_w_ws_floats(B * self.P * self.P, self.root),
                  lib.rsu_head_dice_ws_floats(B * self.P * self.P, self.root), lib.rsu_head_eval_ws_floats(B * self.P * self.P, self.root),
                  lib.rsu_conv_first_bwd_ws_floats(self.root)]
            for kind, n, s, segs in self._packed_kernels():   # (the dead level L-1 dilated pair has the shapes of the level's live block)
                if kind == _PACK_CONV_FWD:
                    for c in segs:
                        ws.append(lib.rsu_conv2d_bwd_weight_ws_floats(s[2], c, s[3]))
                    ws.append(lib.rsu_bias_grad_ws_floats(B * S * S, s[3]))
                elif kind == _PACK_CONVT_FWD:
                    ws.append(lib.rsu_convT2x2_bwd_weight_ws_floats(s[3], s[2]))
            ws.append(lib.rsu_wgrad_group_ws_floats())
            self.ws = torch.zeros(int(max(ws)) + 64, dtype=torch.float32, device=dev)
            # (one workspace per stream that launches weight gradients: their slabs are live at the same time)
            self.sched.ws_side = [self.ws] + [torch.zeros_like(self.ws) for _ in self.wstreams[1:]]
            self.gfirst = torch.zeros((2, 9, 12, self.root), dtype=torch.float32, device=dev)  # gx of conv1 / atrous_conv1 (rsu.h)
            if self._cldice_weight > 0.0:
                self._cldice_buffers()
            if self._lovasz_weight > 0.0:
                self._lovasz_buffers()
            if self.border_weight > 0.0:   # the generated weight map and the column distances between its two launches (rsu.h rsu_border_map)
                self.border_map = torch.zeros((B, self.P, self.P), dtype=torch.float32, device=dev)
                self._border_ws = torch.zeros(int(lib.rsu_border_map_ws_bytes(B, self.P, self.P)) // 4, dtype=torch.int32, device=dev)
            # code bytes of the max-pools (argmax + ReLU bits per pooled element, rsu_maxpool2x2_fwd_code): the gradient junction of a
            # level reads them instead of the level's conv2 activation. RSU_POOL_CODE=0: it reads the activation (same bits)
            if os.environ.get("RSU_POOL_CODE", "1") == "1":
                for i in range(L - 1):
                    self.pool_code[i] = torch.zeros(self.act["pool_%d" % i].shape, dtype=torch.uint8, device=dev)

    def _conv_sources_c(self, name, shape):
        """channel counts of the concat sources feeding conv `name` (decoder conv1: [skip,(dil skip),up], unet.py:79/85)"""
        cin, cout = shape[2], shape[3]
        blk = int(name.split("/")[0].split("_")[-1]) if name.startswith("conv_") and not name.startswith("conv_dilut") else -1
        if name.endswith("conv1/kernel") and blk >= self.L:
            return [cout] * (3 if self.dilated else 2)
        return [cin]

    def _packed_kernels(self):
        """(RSU_PACK_* kind of the forward pack, name, shape, concat segments or None) of every live variable that has bf16 MFMA copies,
        in flat order: what repack(), _build_update_table() and the weight-gradient workspace sizing walk"""
        for n, (_, _, s) in self._slices.items():
            if not n.endswith("kernel") or _is_dead(n, self.L):
                continue
            if n.startswith("up_conv"):
                yield _PACK_CONVT_FWD, n, s, None
            elif s[0] == 3 and s[2] == NUM_CHANNELS:  # level-0 conv1 / atrous_conv1 over the 16-channel input tensor
                yield _PACK_CONV_FIRST, n, s, None
            elif s[0] == 3:
                yield _PACK_CONV_FWD, n, s, self._conv_sources_c(n, s)

    # ------------------------------------------------------------------ packed bf16 weights
    def repack(self):
        """float32 master weights -> bf16 MFMA fragment order (after init / load / every optimizer step): ONE kernel launch
        over a device-resident job table (rsu_pack_table_*) built on first use."""
        lib = _lib.lib()
        st = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream) if self.device.type == "cuda" else None
        if not hasattr(self, "pk"):
            self.pk = {}
            jobs = []  # (kind, weight name, packed tensor, k, Cin_total, ci_off, ci_cnt, Cout, segs)

            def buf(nbytes):
                return torch.zeros(nbytes // 2, dtype=torch.bfloat16, device=self.device)
            for kind, n, s, segs in self._packed_kernels():
                if kind == _PACK_CONVT_FWD:
                    cout, cin = s[2], s[3]
                    self.pk[n, "fwd"] = buf(4 * lib.rsu_packed_bytes(1, cout, (ctypes.c_int * 1)(cin), 1))
                    self.pk[n, "bwd"] = buf(lib.rsu_packed_bytes(4, cin, (ctypes.c_int * 1)(cout), 1))
                    jobs.append((kind, n, self.pk[n, "fwd"], 2, cin, 0, cin, cout, None))
                    if self.training:
                        jobs.append((_PACK_CONVT_BWD, n, self.pk[n, "bwd"], 2, cin, 0, cin, cout, None))
                elif kind == _PACK_CONV_FIRST:
                    self.pk[n, "fwd"] = buf(lib.rsu_packed_first_bytes(s[3]))
                    jobs.append((kind, n, self.pk[n, "fwd"], 3, 3, 0, 3, s[3], None))
                else:
                    cin, cout = s[2], s[3]
                    self.pk[n, "fwd"] = buf(lib.rsu_packed_bytes(9, cout, (ctypes.c_int * len(segs))(*segs), len(segs)))
                    jobs.append((kind, n, self.pk[n, "fwd"], 3, cin, 0, cin, cout, segs))
                    off = 0
                    for si, c in enumerate(segs):  # one backward-data pack per concat source
                        self.pk[n, "bwd", si] = buf(lib.rsu_packed_bytes(9, c, (ctypes.c_int * 1)(cout), 1))
                        if self.training:
                            jobs.append((_PACK_CONV_BWD, n, self.pk[n, "bwd", si], 3, cin, off, c, cout, None))
                        off += c
            esz = lib.rsu_pack_table_entry_bytes()
            host = ctypes.create_string_buffer(esz * (len(jobs) + 3 * sum(1 for j in jobs if j[0] == _PACK_CONVT_FWD)))
            idx = 0
            for kind, n, packed, k, cin, off, cnt, cout, segs in jobs:
                seg = (ctypes.c_int * len(segs))(*segs) if segs else None
                used = lib.rsu_pack_table_add(host, idx, kind, _ptr(self.w[n]), _ptr(packed), k, cin, off, cnt, cout, seg, len(segs) if segs else 0)
                if used < 1:
                    raise _lib.RsuError("rsu_pack_table_add(%s) failed: %d" % (n, used))
                idx += used
            nb = ctypes.c_int(0)
            _lib.check(lib.rsu_pack_table_finish(host, idx, ctypes.byref(nb)), "rsu_pack_table_finish")
            self._pack_n, self._pack_blocks = idx, nb.value
            self._pack_table = torch.frombuffer(bytearray(host.raw[:esz * idx]), dtype=torch.uint8).to(self.device)
        call("rsu_pack_table_run", _ptr(self._pack_table), self._pack_n, self._pack_blocks, st)

    # ------------------------------------------------------------------ forward
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _timed(self, tag, flops, fn, *args):
        """call an ABI entry point; when profiling, bracket it with events on the launch stream"""
        if self.prof is None:
            call(fn, *args)
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call(fn, *args)
        e1.record()
        # (the share of the chip this launch plans for: bench.py prices a launch's duration by it -- two half-chip launches side by side)
        self.prof.append((tag, flops, e0, e1, (self.sched.ncu() or _lib.lib().rsu_get_cu_budget()) / 256.0))

    def _grads_ready(self, name):
        if self.on_grads is not None:  # (dist.GradBucketer waits for the weight-gradient stream itself: extra_streams)
            self.sched.flush()         # queued weight gradients must be ON the side stream before the exchange may wait for it
            self.on_grads(self._slices[name][0])

    def _conv(self, name, srcs, hin, out, dil=1):
        arr = (RsuSrc * len(srcs))(*srcs)
        cout = out.shape[3]
        cin = sum(s.C for s in srcs)
        ho = hin - 2 * dil
        kws = self.sched.kws_here()
        nb = out.shape[0]   # (the batch of the tensors at hand: forward_device may run the two halves of a batch as two chains)
        self._timed("conv3x3_fwd", 2.0 * nb * ho * ho * cout * cin * 9, "rsu_conv2d_fwd_k", arr, len(srcs),
                    _ptr(self.pk[name + "/kernel", "fwd"]), _ptr(self.w[name + "/bias"]), _ptr(out), nb, hin, hin, cout, dil, 1,
                    self.sched.ncu(), _ptr(kws), kws.numel() if kws is not None else 0, self._stream())

    def _conv_first(self, name, out, h, dil, st, in16=None, x=None):
        if x is not None:
            # colour adjust + first conv in one launch, straight from the f32 input (rsu.h rsu_color_conv_first_fwd; same bits, no dropout)
            call("rsu_color_conv_first_fwd", _ptr(x), _ptr(self.w["color_space_adjust/kernel"]), _ptr(self.w["color_space_adjust/bias"]),
                 _ptr(self.pk[name + "/kernel", "fwd"]), _ptr(self.w[name + "/bias"]), _ptr(out), out.shape[0], h, h, self.root, dil,
                 self.sched.ncu(), st)
            return
        call("rsu_conv_first_fwd", _ptr(self.in16 if in16 is None else in16), _ptr(self.pk[name + "/kernel", "fwd"]), _ptr(self.w[name + "/bias"]),
             _ptr(out), out.shape[0], h, h, self.root, dil, self.sched.ncu(), st)

    def dropout_key(self, site):
        """32-bit key of dropout site `site` (encoder level i -> i, decoder stage i -> L + i: the 2L-1 tf.nn.dropout calls of
        unet.py:29-30,64-65) for the current global step -- and, on an accumulating net, the current micro-batch of it, so that the
        micro-batches of one step draw different masks; the hash of (key, element index) replaces TF's Philox stream"""
        return dropout_key_value(self.dropout_seed, site, self.global_step, self.micro_step)

    @property
    def micro_step(self):
        """which micro-batch of the current optimizer step the next forward / backward pass belongs to: 0..accumulate_steps-1, the count
        of accumulate_gradients() calls since the last step; always 0 on a net that does not accumulate"""
        return min(self._accum_calls, self.accumulate_steps - 1)

    def forward_device(self, want_logits=False, keep=1.0):
        """unet.forward (unet.py:12-97) on self.x (already on device); keep = dropout_keep (1.0: none); fills self.prob."""
        keep = float(keep)
        assert 0.0 < keep <= 1.0, "dropout keep probability must be in (0, 1]"
        self.keep = keep
        for f in self._forward_steps(0, self.B, want_logits, keep):
            f()
        return self.act[self.last_name]

    def _forward_steps(self, b0, nb, want_logits, keep):
        """the launches of a forward pass over images [b0, b0 + nb) as a list of closures (one ABI call each, issued on the stream that is
        current when the closure runs). (Two chains over the halves of a batch on two streams were measured: -2..-4 % on the step,
        profiles/r04/fwd_halves_probe.txt.)"""
        L, S = self.L, self.S
        a = {k: t[b0:b0 + nb] for k, t in self.act.items()}
        x, in16, prob, logits = self.x[b0:b0 + nb], self.in16[b0:b0 + nb], self.prob[b0:b0 + nb], self.logits[b0:b0 + nb]
        code = {k: t[b0:b0 + nb] for k, t in self.pool_code.items()}
        steps = []

        def add(f):
            steps.append(f)
        # A forward-only net without dropout reads the f32 input in the level-0 convs themselves (rsu_color_conv_first_fwd: one launch, the
        # 16-channel tensor is never built, same bits). A training step needs that tensor for the first conv's weight gradient anyway, and the
        # first conv reads it back hot from the Infinity Cache: measured (profiles/r06/kernel_stats_fused_first.md), the fused launch beside a
        # colour-adjust launch on the side stream takes 66 us against 14.5 + 48 us of the two launches in a row -- training keeps the two.
        fused_first = keep == 1.0 and not self.training
        xin = x if fused_first else None
        if not fused_first:
            add(lambda: call("rsu_color_adjust_fwd", _ptr(x), _ptr(self.w["color_space_adjust/kernel"]), _ptr(self.w["color_space_adjust/bias"]),
                             _ptr(in16), nb * S * S, keep, self.dropout_key(0), self._stream()))
        cur, h = None, S
        for i in range(L):
            last = i == L - 1
            if self.dilated and not last:
                # the dilated twin block (unet.py:32-39) reads the level's input and feeds only a decoder skip: it runs on the second
                # stream beside the main block (joined in front of the decoder)
                def twin(i=i, cur=cur, h=h):
                    with self.sched.side():
                        if i == 0:
                            self._conv_first("conv_dilut_0/atrous_conv1", a["d1_0"], h, 2, self._stream(), in16, xin)
                        else:
                            self._conv("conv_dilut_%d/atrous_conv1" % i, [_src(cur, h, h)], h, a["d1_%d" % i], dil=2)
                        self._conv("conv_dilut_%d/atrous_conv2" % i, [_src(a["d1_%d" % i], h - 4, h - 4)], h - 4, a["d2_%d" % i], dil=2)
                add(twin)
            if i == 0:
                add(lambda h=h: self._conv_first("conv_0/conv1", a["c1_0"], h, 1, self._stream(), in16, xin))
            else:
                add(lambda i=i, cur=cur, h=h: self._conv("conv_%d/conv1" % i, [_src(cur, h, h)], h, a["c1_%d" % i]))
            if last:
                add(lambda i=i, h=h: self._conv("conv_%d/conv2" % i, [_src(a["c1_%d" % i], h - 2, h - 2)], h - 2, a["c2_%d" % i]))
            else:
                # conv2 + ReLU + the level's 2x2 max-pool (+ the next level's dropout, + the code bytes of the gradient junction): one
                # call, one launch where the pool folds into the conv's epilogue (rsu.h rsu_conv2d_fwd_pool)
                def conv2_pool(i=i, h=h):
                    c1, c2 = a["c1_%d" % i], a["c2_%d" % i]
                    nf_ = c2.shape[3]
                    src = (RsuSrc * 1)(_src(c1, h - 2, h - 2))
                    kws = self.sched.kws_here()
                    self._timed("conv3x3_fwd", 2.0 * nb * (h - 4) * (h - 4) * nf_ * c1.shape[3] * 9, "rsu_conv2d_fwd_pool_k", src, 1,
                                _ptr(self.pk["conv_%d/conv2/kernel" % i, "fwd"]), _ptr(self.w["conv_%d/conv2/bias" % i]), _ptr(c2),
                                _ptr(a["pool_%d" % i]), _ptr(code.get(i)), nb, h - 2, h - 2, nf_, keep, self.dropout_key(i + 1), self.sched.ncu(),
                                _ptr(kws), kws.numel() if kws is not None else 0, self._stream())
                add(conv2_pool)
                cur, h = a["pool_%d" % i], (h - 4) // 2
        net, h = a["c2_%d" % (L - 1)], h - 4
        if self.dilated:
            add(self.sched.join)
        for i in range(L - 1):
            j, lvl = L + i, L - 2 - i
            up = a["up_%d" % i]
            if keep < 1.0:  # unet.py:64-65
                if self.act.get("drop_%d" % i) is None:
                    self.act["drop_%d" % i] = torch.zeros_like(self.act["c2_%d" % (j - 1)] if i > 0 else self.act["c2_%d" % (L - 1)])
                drop = self.act["drop_%d" % i][b0:b0 + nb]
                add(lambda net=net, drop=drop, i=i: call("rsu_dropout_fwd", _ptr(net), _ptr(drop), net.numel(), keep, self.dropout_key(L + i), self._stream()))
                net = drop
            add(lambda net=net, up=up, i=i, h=h: call("rsu_convT2x2_fwd", _ptr(net), _ptr(self.pk["up_conv_%d/kernel" % i, "fwd"]),
                                                     _ptr(self.w["up_conv_%d/bias" % i]), _ptr(up), nb, h, h, net.shape[3], up.shape[3], self.sched.ncu(), self._stream()))
            h = 2 * h

            def dec(j=j, lvl=lvl, up=up, h=h):
                srcs = [_src(a["c2_%d" % lvl], h, h)]
                if self.dilated:
                    srcs.append(_src(a["d2_%d" % lvl], h, h))
                srcs.append(_src(up, h, h))
                self._conv("conv_%d/conv1" % j, srcs, h, a["c1_%d" % j])
            add(dec)
            add(lambda j=j, h=h: self._conv("conv_%d/conv2" % j, [_src(a["c1_%d" % j], h - 2, h - 2)], h - 2, a["c2_%d" % j]))
            net, h = a["c2_%d" % j], h - 4
        if not self.training or want_logits:
            add(lambda net=net: call("rsu_head_fwd", _ptr(net), _ptr(self.w["weight_output/kernel"]), _ptr(self.w["weight_output/bias"]), _ptr(prob),
                                     _ptr(logits) if want_logits else None, nb * self.P * self.P, self.root, self._stream()))
        return steps

    # ------------------------------------------------------------------ held-out validation
    def reset_eval(self):
        """zero the validation accumulators eval_sums / eval_hist (on the current stream)"""
        self.eval_sums.zero_()
        self.eval_hist.zero_()
        if self.eval_cldice_sums is not None:
            self.eval_cldice_sums.zero_()
        if self.eval_lovasz_sum is not None:
            self.eval_lovasz_sum.zero_()

    def evaluate_device(self):
        """The forward-only loss and metric counts of self.x / self.labels, for data the optimizer does not see: ONE rsu_head_eval launch
        (rsu.h) behind a forward_device(keep=1.0) of a training net, which itself runs no head. It fills self.prob and ADDS to
        eval_sums (f32[5]) += {sum omega CE, sum omega, I, P, Y} -- omega and the sums as backward_device defines them, with this net's
        class weights and weight map -- and to eval_hist (int64 [2, 256]): hist[label][min(255, int(p * 256))] += 1 for every pixel whose
        label is 0 or 1; any other label ignores its pixel. No gradient buffer, loss_sum, weight_sum or dice_sums is written, and nothing
        is read back: a caller sums a whole set on the device (reset_eval first) and synchronises once. With cldice_weight > 0 one
        rsu_cldice_fwd (rsu_cldice.h) follows the head: eval_cldice_sums (f32[4]) += {A, Bp, Cc, Dy} of this batch; with
        lovasz_weight > 0 one rsu_lovasz_fwd (rsu_lovasz.h): eval_lovasz_sum (f32[2]) += {sum_b L_b, images}. ensure_tuned(training=False)
        belongs in front of the first such forward pass: at keep == 1 the encoder takes the fused conv + pool launches, whose tuning
        keys differ from a dropout step's."""
        if not self.training:
            raise _lib.RsuError("evaluate_device needs a training net (labels and the head's workspace); a forward-only net has no loss")
        if self.keep != 1.0:
            raise _lib.RsuError("evaluate_device follows forward_device(keep=1.0): the activations in flight were made with dropout")
        if self._focal_gamma > 0.0:   # the objective the net is trained on: sums[0] += sum omega F CE (rsu_loss.h)
            call("rsu_head_eval_focal", _ptr(self.act[self.last_name]), _ptr(self.w["weight_output/kernel"]), _ptr(self.w["weight_output/bias"]),
                 _ptr(self.labels), _ptr(self._class_w_dev), _ptr(self._head_pixel_weights()), self._focal_gamma, _ptr(self.prob),
                 _ptr(self.eval_sums), _ptr(self.eval_hist), _ptr(self.ws), self.B * self.P * self.P, self.root, self._stream())
        else:
            call("rsu_head_eval", _ptr(self.act[self.last_name]), _ptr(self.w["weight_output/kernel"]), _ptr(self.w["weight_output/bias"]),
                 _ptr(self.labels), _ptr(self._class_w_dev), _ptr(self._head_pixel_weights()), _ptr(self.prob), _ptr(self.eval_sums),
                 _ptr(self.eval_hist), _ptr(self.ws), self.B * self.P * self.P, self.root, self._stream())
        if self._cldice_weight > 0.0:
            self._cldice_buffers()
            self._cldice_fwd(self.eval_cldice_sums)
        if self._lovasz_weight > 0.0:
            self._lovasz_buffers()
            call("rsu_lovasz_fwd", _ptr(self.prob), _ptr(self.labels), _ptr(self.eval_lovasz_sum), _ptr(self._lovasz_ws), self.B, self.P,
                 self.P, self._stream())

    # ------------------------------------------------------------------ backward
    def _wgrad(self, name, srcs_t, dz, hout, dil=1, block_done=False):
        """dW (HWIO rows per source) + db of conv `name`; srcs_t = list of (tensor, window size). With grouping on (RSU_WG_GROUP) the
        launches are only queued here; the schedule sends a whole group to the side stream as one launch. block_done: this is a
        block's conv2 gradient, behind which a group may close (BackwardSchedule.block_done)."""
        cout = dz.shape[3]
        cin_total = self.w[name + "/kernel"].shape[2]
        off = 0
        if self.sched.grouped:
            for t, win in srcs_t:
                db = self.g[name + "/bias"] if off == 0 else None  # BiasAddGrad rides along with the first source's launch
                job = RsuWgradJob(_lib.WGRAD_CONV3X3, _src(t, win, win), dz.data_ptr(), self.g[name + "/kernel"].data_ptr(),
                                  db.data_ptr() if db is not None else None, hout, hout, cin_total, off, cout, dil)
                self.sched.queue(job, 2.0 * self.B * hout * hout * cout * t.shape[3] * 9, (name, off))
                off += t.shape[3]
            if block_done:
                self.sched.block_done()
            return
        with self.sched.side() as ws:
            st = self._stream()
            for t, win in srcs_t:
                s = _src(t, win, win)
                db = _ptr(self.g[name + "/bias"]) if off == 0 else None  # BiasAddGrad rides along with the first source's launch
                fl = 2.0 * self.B * hout * hout * cout * t.shape[3] * 9
                self._timed("conv3x3_bwd_weight", fl, "rsu_conv2d_bwd_weight", ctypes.byref(s), _ptr(dz), _ptr(self.g[name + "/kernel"]), db,
                            _ptr(ws), self.B, hout, hout, cin_total, off, cout, dil, self.sched.ncu(), st)
                off += t.shape[3]

    def _wgradT(self, i, upin, dup, hh, nf):
        """dK + db of up_conv_i (queued like _wgrad when grouping is on)"""
        if self.sched.grouped:
            job = RsuWgradJob(_lib.WGRAD_CONVT2X2, RsuSrc(upin.data_ptr(), hh, hh, upin.shape[3], 0, 0), dup.data_ptr(),
                              self.g["up_conv_%d/kernel" % i].data_ptr(), self.g["up_conv_%d/bias" % i].data_ptr(), 0, 0, 0, 0, nf, 1)
            self.sched.queue(job, 0.0, ("up_conv_%d" % i, upin.data_ptr()), transposed=True)
            return
        with self.sched.side() as ws:
            call("rsu_convT2x2_bwd_weight", _ptr(upin), _ptr(dup), _ptr(self.g["up_conv_%d/kernel" % i]), _ptr(self.g["up_conv_%d/bias" % i]),
                 _ptr(ws), self.B, hh, hh, upin.shape[3], nf, self.sched.ncu(), self._stream())

    def _wgrad_first(self, name, dz, h, dil, where):
        """dW + db + gx (gfirst[0]; the dilated twin, dil 2: gfirst[1]) of a level-0 first conv: a launch of its own inside `where`,
        the schedule's context that gives it a stream, a CU share and a workspace"""
        with where as ws:
            call("rsu_conv_first_bwd_weight", _ptr(self.in16), _ptr(dz), _ptr(self.g[name + "/kernel"]), _ptr(self.gfirst[dil - 1]),
                 _ptr(self.g[name + "/bias"]), _ptr(ws), self.B, h, h, self.root, dil, self.sched.ncu(), self._stream())

    def _bwd_data(self, name, dz, dx, hin, relu_src=None, accumulate=0, src_index=0, dil=1):
        """Conv2DBackpropInput towards concat source `src_index` of conv `name` (its own weight pack)"""
        cout = self.w[name + "/kernel"].shape[3]
        cnt = dx.shape[3]
        ho = hin - 2 * dil
        kws = self.sched.kws_here()
        self._timed("conv3x3_bwd_data", 2.0 * self.B * ho * ho * cout * cnt * 9, "rsu_conv2d_bwd_data_k", _ptr(dz),
                    _ptr(self.pk[name + "/kernel", "bwd", src_index]), _ptr(dx), _ptr(relu_src), accumulate, self.B, hin, hin, cnt, 0, cnt,
                    cout, dil, self.sched.ncu(), _ptr(kws), kws.numel() if kws is not None else 0, self._stream())

    def backward_device(self, inv_count, update=None, dice_scale=None, cldice_scale=None, lovasz_scale=None):
        """loss + all gradients for self.x / self.labels; forward_device() must have run. inv_count = 1 / (global pixel count).
        The loss is the reference's mean softmax cross-entropy unless class weights other than (1, 1) or a weight map are set
        (class_weights, set_pixel_weights): then pixel p counts omega_p = class_weights[label_p] * pixel_weights[p] times in loss_sum and
        in the gradients, weight_sum receives sum omega, and inv_count STAYS 1 / pixel count (rsu.h rsu_head_fwd_bwd_w;
        loss_sum / weight_sum is the weighted mean, for reporting). A label in self.labels other than 0 and 1 IGNORES its pixel in that
        weighted pass: no loss, no gradient, no weight (prob is still written). The unweighted pass expects labels in {0, 1}; to ignore
        pixels without weighting the others, set a map of ones. After an unweighted pass weight_sum is 0.
        dice_scale (None: self.dice_weight) > 0 adds dice_scale * (1 - D) to the objective, D the soft Dice of THIS net's batch (rsu.h
        rsu_head_fwd_bwd_dice): the head then runs as two launches with the device buffer dice_sums = {I, P, Y} between them (no host
        synchronisation), labels other than 0 / 1 are ignored, the weight map enters D and the class weights do not. loss_sum and weight_sum
        stay the cross-entropy's; the term's value is dice_scale * (1 - D) with D from dice_sums. A data-parallel host passes
        dice_weight / world. With dice_scale == 0 the pass is exactly the one described above.
        focal_gamma > 0 takes the focal head instead (rsu_loss.h rsu_head_fwd_bwd_focal): omega F CE per counted pixel in loss_sum and its
        gradient, F = (1 - p_t)^gamma; weight_sum, the Dice term and inv_count as above.
        cldice_scale (None: self.cldice_weight) > 0 adds cldice_scale * (1 - clD) of THIS net's batch (rsu_cldice.h). The head then runs as:
        pass A, which writes prob (rsu_head_dice_sums when the Dice term is on too, otherwise rsu_head_fwd); cldice_sums zeroed on the stream;
        rsu_cldice_fwd (skel_p, skel_y, cldice_sums); rsu_cldice_bwd (gprob = d term / d prob); rsu_head_fwd_bwd_aux with this net's gamma, Dice
        term and weights, which carries gprob to the logits. No host synchronisation; loss_sum and weight_sum stay the cross-entropy part,
        the term's value is cldice_scale * (1 - clD) with clD from cldice_sums. A data-parallel host passes cldice_weight / world. With
        cldice_scale == 0 the pass issues exactly the launches described above.
        lovasz_scale (None: self.lovasz_weight) > 0 adds lovasz_scale * (1 / B) sum_b L_b, L_b the Lovasz loss of image b of THIS net's
        batch (rsu_lovasz.h). The head then runs as: pass A as above; the clDice launches, if that term is on, which write gprob; lovasz_sum
        zeroed on the stream; rsu_lovasz_fwd_bwd (lovasz_sum += {sum_b L_b, B}; gprob accumulated if clDice wrote it, otherwise
        overwritten); rsu_head_fwd_bwd_aux. No host synchronisation; the term's value is lovasz_scale * lovasz_sum[0] / lovasz_sum[1]. A
        mean of per-image losses: a data-parallel or accumulating host passes lovasz_weight / (world * micro-batches) and gets the
        objective of one large batch. With lovasz_scale == 0 the pass issues exactly the launches described above.
        update = (lr0, momentum): accepted from callers that name the Momentum step they will take; it changes nothing here -- the step
        is apply_momentum's -- but a net built with another optimizer refuses it."""
        self._not_averaged("backward_device")
        if update is not None and self.optimizer != "momentum":
            raise _lib.RsuError("backward_device(update=...) is the Momentum step; an %s net steps with apply_%s after the pass"
                                % (self.optimizer, self.optimizer))
        dice_scale = self._dice_weight if dice_scale is None else float(dice_scale)
        if not (math.isfinite(dice_scale) and dice_scale >= 0.0):
            raise _lib.RsuError("dice_scale must be a finite float >= 0, not %r" % (dice_scale,))
        cldice_scale = self._cldice_weight if cldice_scale is None else float(cldice_scale)
        if not (math.isfinite(cldice_scale) and cldice_scale >= 0.0):
            raise _lib.RsuError("cldice_scale must be a finite float >= 0, not %r" % (cldice_scale,))
        lovasz_scale = self._lovasz_weight if lovasz_scale is None else float(lovasz_scale)
        if not (math.isfinite(lovasz_scale) and lovasz_scale >= 0.0):
            raise _lib.RsuError("lovasz_scale must be a finite float >= 0, not %r" % (lovasz_scale,))
        st = self._stream()
        self.sched.begin(self.backward_cu_budget)
        try:
            self._backward_body(inv_count, dice_scale, cldice_scale, lovasz_scale)
        finally:
            self.sched.end()   # (an exception inside must not leave later launches planned for a share of the chip)
        # ---- color_space_adjust (unet.py:22-23): its input gradient is never materialised (include/rsu.h, rsu_conv_first_bwd_weight):
        #   dW0[ci][cj] = 1/keep * sum_{t,co} W1[t][cj][co] * gxc[t][ci][cj][co];  db0[cj] = 1/keep * sum_{t,co} W1[t][cj][co] * gm[t][cj][co]
        inv_keep = float(np.float32(1.0) / np.float32(self.keep))
        gk, gb = self.g["color_space_adjust/kernel"], self.g["color_space_adjust/bias"]
        call("rsu_color_adjust_bwd", _ptr(self.gfirst[0]), _ptr(self.w["conv_0/conv1/kernel"]), _ptr(gk), _ptr(gb), self.root, inv_keep, 0, st)
        if self.dilated and self.L > 1:
            call("rsu_color_adjust_bwd", _ptr(self.gfirst[1]), _ptr(self.w["conv_dilut_0/atrous_conv1/kernel"]), _ptr(gk), _ptr(gb), self.root,
                 inv_keep, 1, st)

    def _backward_body(self, inv_count, dice_scale=0.0, cldice_scale=0.0, lovasz_scale=0.0):
        B, L, st, a, g = self.B, self.L, self._stream(), self.act, self.grad
        keep = self.keep
        last = a[self.last_name]
        self._loss_acc.zero_()
        pixel_w = self._head_pixel_weights()
        if cldice_scale > 0.0 or lovasz_scale > 0.0:
            # the terms with a gradient wrt prob: pass A writes prob; the clDice term (rsu_cldice.h: the fused skeleton forward and backward)
            # and the Lovasz term (rsu_lovasz.h: the sort and the Jaccard differences) turn it into gprob, the second adding to the first;
            # the aux head carries gprob to the logits next to the cross-entropy (focal with gamma > 0) and the Dice term
            head = (_ptr(last), _ptr(self.w["weight_output/kernel"]), _ptr(self.w["weight_output/bias"]))
            npix = B * self.P * self.P
            if cldice_scale > 0.0:
                self._cldice_buffers()
            if lovasz_scale > 0.0:
                self._lovasz_buffers()
            if dice_scale > 0.0:
                call("rsu_head_dice_sums", *head, _ptr(self.labels), _ptr(pixel_w), _ptr(self.prob), _ptr(self.dice_sums), _ptr(self.ws), npix,
                     self.root, st)
            else:
                call("rsu_head_fwd", *head, _ptr(self.prob), None, npix, self.root, st)
            if cldice_scale > 0.0:
                self.cldice_sums.zero_()
                self._cldice_fwd(self.cldice_sums)
                call("rsu_cldice_bwd", _ptr(self.prob), _ptr(self.labels), _ptr(self.skel_p), _ptr(self.skel_y), _ptr(self.cldice_sums),
                     self._cldice_iters, cldice_scale, self._cldice_smooth, _ptr(self.gprob), _ptr(self._cldice_ws), B, self.P, self.P, st)
            if lovasz_scale > 0.0:
                self.lovasz_sum.zero_()
                call("rsu_lovasz_fwd_bwd", _ptr(self.prob), _ptr(self.labels), lovasz_scale, 1 if cldice_scale > 0.0 else 0, _ptr(self.gprob),
                     _ptr(self.lovasz_sum), _ptr(self._lovasz_ws), B, self.P, self.P, st)
            call("rsu_head_fwd_bwd_aux", *head, _ptr(self.labels), _ptr(self._class_w_dev), _ptr(pixel_w), self._focal_gamma,
                 _ptr(self.dice_sums) if dice_scale > 0.0 else None, dice_scale, self._dice_smooth, _ptr(self.prob), _ptr(self.loss_sum),
                 _ptr(self.weight_sum), _ptr(g[self.last_name]), _ptr(self.g["weight_output/kernel"]), _ptr(self.g["weight_output/bias"]),
                 _ptr(self.ws), npix, self.root, inv_count, _ptr(self.gprob), st)
        elif self._focal_gamma > 0.0:
            # the focal head (rsu_loss.h): the weighted head's arguments and gamma; with a Dice term pass B behind an unchanged pass A
            head = (_ptr(last), _ptr(self.w["weight_output/kernel"]), _ptr(self.w["weight_output/bias"]), _ptr(self.labels))
            npix = B * self.P * self.P
            if dice_scale > 0.0:
                call("rsu_head_dice_sums", *head, _ptr(pixel_w), _ptr(self.prob), _ptr(self.dice_sums), _ptr(self.ws), npix, self.root, st)
            call("rsu_head_fwd_bwd_focal", *head, _ptr(self._class_w_dev), _ptr(pixel_w), self._focal_gamma,
                 _ptr(self.dice_sums) if dice_scale > 0.0 else None, dice_scale, self._dice_smooth, _ptr(self.prob), _ptr(self.loss_sum),
                 _ptr(self.weight_sum), _ptr(g[self.last_name]), _ptr(self.g["weight_output/kernel"]), _ptr(self.g["weight_output/bias"]),
                 _ptr(self.ws), npix, self.root, inv_count, st)
        elif dice_scale > 0.0:
            head = (_ptr(last), _ptr(self.w["weight_output/kernel"]), _ptr(self.w["weight_output/bias"]), _ptr(self.labels))
            npix = B * self.P * self.P
            call("rsu_head_dice_sums", *head, _ptr(pixel_w), _ptr(self.prob), _ptr(self.dice_sums), _ptr(self.ws), npix, self.root, st)
            call("rsu_head_fwd_bwd_dice", *head, _ptr(self._class_w_dev), _ptr(pixel_w), _ptr(self.dice_sums), dice_scale,
                 self._dice_smooth, _ptr(self.prob), _ptr(self.loss_sum), _ptr(self.weight_sum), _ptr(g[self.last_name]),
                 _ptr(self.g["weight_output/kernel"]), _ptr(self.g["weight_output/bias"]), _ptr(self.ws), npix, self.root, inv_count, st)
        elif self.loss_is_weighted():
            call("rsu_head_fwd_bwd_w", _ptr(last), _ptr(self.w["weight_output/kernel"]), _ptr(self.w["weight_output/bias"]), _ptr(self.labels),
                 _ptr(self._class_w_dev), _ptr(pixel_w), _ptr(self.prob),
                 _ptr(self.loss_sum), _ptr(self.weight_sum), _ptr(g[self.last_name]), _ptr(self.g["weight_output/kernel"]),
                 _ptr(self.g["weight_output/bias"]), _ptr(self.ws), B * self.P * self.P, self.root, inv_count, st)
        else:
            call("rsu_head_fwd_bwd", _ptr(last), _ptr(self.w["weight_output/kernel"]), _ptr(self.w["weight_output/bias"]), _ptr(self.labels),
                 _ptr(self.prob), _ptr(self.loss_sum), _ptr(g[self.last_name]), _ptr(self.g["weight_output/kernel"]),
                 _ptr(self.g["weight_output/bias"]), _ptr(self.ws), B * self.P * self.P, self.root, inv_count, st)
        # ---- decoder, stage L-2 .. 0
        for i in reversed(range(L - 1)):
            j, lvl = L + i, L - 2 - i
            c1, c2, up = a["c1_%d" % j], a["c2_%d" % j], a["up_%d" % i]
            h = up.shape[1]
            nf = c2.shape[3]
            dz2, dz1 = g["c2_%d" % j], g["c1_%d" % j]
            self._wgrad("conv_%d/conv2" % j, [(c1, h - 2)], dz2, h - 4, block_done=True)
            self._bwd_data("conv_%d/conv2" % j, dz2, dz1, h - 2, relu_src=c1)
            srcs = [(a["c2_%d" % lvl], h)] + ([(a["d2_%d" % lvl], h)] if self.dilated else []) + [(up, h)]
            self._wgrad("conv_%d/conv1" % j, srcs, dz1, h - 2)
            self._bwd_data("conv_%d/conv1" % j, dz1, g["skip_%d" % i], h, src_index=0)
            if self.dilated:
                self._bwd_data("conv_%d/conv1" % j, dz1, g["skipd_%d" % i], h, src_index=1)
            dup = g["up_%d" % i]
            self._bwd_data("conv_%d/conv1" % j, dz1, dup, h, src_index=2 if self.dilated else 1)
            # transposed conv
            upin = a["c2_%d" % (j - 1)] if i > 0 else a["c2_%d" % (L - 1)]
            gin = g["c2_%d" % (j - 1)] if i > 0 else g["c2_%d" % (L - 1)]
            if keep < 1.0:  # the transposed conv read the dropped tensor; (dropped > 0) = ReLU mask AND keep mask
                upin = a["drop_%d" % i]
            hh = h // 2
            self._wgradT(i, upin, dup, hh, nf)
            call("rsu_convT2x2_bwd_data", _ptr(dup), _ptr(self.pk["up_conv_%d/kernel" % i, "bwd"]), _ptr(gin), _ptr(upin), float(np.float32(1.0) / np.float32(keep)), B, hh, hh,
                 upin.shape[3], nf, self.sched.ncu(), st)
            self._grads_ready("up_conv_%d/kernel" % i)  # up_conv_i, conv_{L+i} and everything created later are final
        # ---- encoder, level L-1 .. 0
        for i in reversed(range(L)):
            c1, c2 = a["c1_%d" % i], a["c2_%d" % i]
            h = self.level_in[i]
            nf = c2.shape[3]
            dz2, dz1 = g["c2_%d" % i], g["c1_%d" % i]
            if i < L - 1:
                dec = L - 2 - i
                hs = a["up_%d" % dec].shape[1]
                call("rsu_pool_skip_relu_bwd_code", _ptr(c2), _ptr(self.pool_code.get(i)), _ptr(g["pool_%d" % i]), _ptr(g["skip_%d" % dec]), _ptr(dz2), B, h - 4, h - 4, nf, hs, hs,
                     keep, self.dropout_key(i + 1), st)
            # (level 0 of a net without dilated twins: its conv2 gradient joins the pass's last group, flushed below)
            self._wgrad("conv_%d/conv2" % i, [(c1, h - 2)], dz2, h - 4, block_done=i > 0 or self.dilated)
            self._bwd_data("conv_%d/conv2" % i, dz2, dz1, h - 2, relu_src=c1)
            if i > 0:
                pin = a["pool_%d" % (i - 1)]
                self._wgrad("conv_%d/conv1" % i, [(pin, h)], dz1, h - 2)
                self._bwd_data("conv_%d/conv1" % i, dz1, g["pool_%d" % (i - 1)], h)
            else:
                # the last group: nothing is left to run beside it on the main stream (unless the dilated twin of level 0 follows), so
                # it plans for the whole chip; the level-0 conv1 gradient below is a launch of its own
                alone = not (self.dilated and L > 1)
                self.sched.flush(alone=alone)
                self._wgrad_first("conv_0/conv1", dz1, h, 1, self.sched.tail(alone))
            if self.dilated and i < L - 1:
                d1, d2 = a["d1_%d" % i], a["d2_%d" % i]
                dzd2, dzd1 = g["d2_%d" % i], g["d1_%d" % i]
                dec = L - 2 - i
                hs = a["up_%d" % dec].shape[1]
                call("rsu_pool_skip_relu_bwd", _ptr(d2), None, _ptr(g["skipd_%d" % dec]), _ptr(dzd2), B, h - 8, h - 8, nf, hs, hs, 1.0, 0, st)
                self._wgrad("conv_dilut_%d/atrous_conv2" % i, [(d1, h - 4)], dzd2, h - 8, dil=2, block_done=True)
                self._bwd_data("conv_dilut_%d/atrous_conv2" % i, dzd2, dzd1, h - 4, relu_src=d1, dil=2)
                if i > 0:
                    pin = a["pool_%d" % (i - 1)]
                    self._wgrad("conv_dilut_%d/atrous_conv1" % i, [(pin, h)], dzd1, h - 4, dil=2)
                    self._bwd_data("conv_dilut_%d/atrous_conv1" % i, dzd1, g["pool_%d" % (i - 1)], h, accumulate=1, dil=2)
                else:
                    self._wgrad_first("conv_dilut_0/atrous_conv1", dzd1, h, 2, self.sched.side(alone=True))
            if i > 0:
                # first LIVE variable of the level in creation order: the dilated pair of level L-1 is dead and sits behind n_live
                # (marking it ready launched nothing, and the largest block waited for level L-2)
                first_name = ("conv_dilut_%d/atrous_conv1/kernel" if (self.dilated and i < L - 1) else "conv_%d/conv1/kernel") % i
                self._grads_ready(first_name)
        self.sched.flush(alone=True)
        self.sched.join()

    def tune(self, training=None, keep=1.0):
        """The explicit tile-shape tuning pass (rsu.h rsu_set_autotune): ONE untimed forward (+ backward) over random data with the
        library in RSU_TUNE_MEASURE mode -- every conv geometry of this network at the CU shares its launches use is timed once on an
        idle device -- then back to RSU_TUNE_LOOKUP, in which the launch entry points never measure nor synchronise. Weights, Momentum
        slots and the step counter are untouched; x / labels are restored; class weights, the weight map and dice_weight stay as
        set (the pass takes the head they select). All shapes give the same bits: this only moves time. Under
        data parallelism call it before the first collective is in flight (and again after changing backward_cu_budget).
        `keep` is the dropout keep probability of the steps that follow: with keep < 1 the encoder's conv2 launches take the unfused
        conv + max-pool pair (rsu.h rsu_conv2d_fwd_pool folds the pool only at keep == 1), whose tuning keys differ from the fused
        launch's -- the pass must measure the keys the steps will look up."""
        lib = _lib.lib()
        training = self.training if training is None else (training and self.training)
        keep = float(keep)
        self._tuned.add((bool(training), self.backward_cu_budget, keep < 1.0))
        if lib.rsu_get_autotune() == _lib.TUNE_OFF or os.environ.get("RSU_AUTOTUNE", "1") == "0":
            return
        x0, l0 = self.x.clone(), self.labels.clone()
        g = torch.Generator(device="cpu").manual_seed(12345)
        self.x.copy_(torch.rand(tuple(self.x.shape), generator=g))
        self.labels.copy_((torch.rand(tuple(self.labels.shape), generator=g) < 0.2).to(torch.int64))
        on_grads, self.on_grads = self.on_grads, None   # no gradient exchange from inside the tuning pass
        prof, self.prof = self.prof, None
        call("rsu_set_autotune", _lib.TUNE_MEASURE)
        try:
            self.forward_device(keep=keep)
            if training:
                self.backward_device(1.0 / (self.B * self.P * self.P))
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
        finally:
            call("rsu_set_autotune", _lib.TUNE_LOOKUP)
            self.on_grads, self.prof = on_grads, prof
            self.x.copy_(x0)
            self.labels.copy_(l0)

    def ensure_tuned(self, training=None, keep=1.0):
        """tune() once per (forward-only / training, backward CU budget, dropout on / off): what the hosts call in front of their
        first step"""
        training = self.training if training is None else (training and self.training)
        drop = float(keep) < 1.0
        if (bool(training), self.backward_cu_budget, drop) not in self._tuned and ((True, self.backward_cu_budget, drop) not in self._tuned):
            self.tune(training, keep=keep)


_DEFAULT_MODELS = {}


def forward(X, num_layers, root_size, dilated_layers, dropout_keep=None, params=None):
    """Drop-in for the reference's unet.forward (unet.py:12): X [B,S,S,3] float32 in [0,1] -> logits [B,P,P,2].

    The reference builds a TF graph and creates its variables on first use; here the variables live in a cached UNet
    keyed by the static shapes (pass `params` -- a dict of TF-named numpy arrays -- to set them). dropout_keep = None or
    1.0: no dropout (unet.py:29: `if dropout_keep is not None`); < 1: tf.nn.dropout at the 2L-1 sites with counter-based
    masks."""
    keep = 1.0 if dropout_keep is None else float(dropout_keep)
    X = torch.as_tensor(X)
    B, S = X.shape[0], X.shape[1]
    assert X.shape[2] == S and X.shape[3] == NUM_CHANNELS
    P = S - 12 * 2 ** (num_layers - 1) + 8
    assert input_size_needed(P, num_layers) == S, "input size {} is not a valid U-Net input for {} layers".format(S, num_layers)
    key = (num_layers, root_size, bool(dilated_layers), B, P)
    m = _DEFAULT_MODELS.get(key)
    if m is None:
        m = _DEFAULT_MODELS[key] = UNet(num_layers, root_size, dilated_layers, B, P, params=params, training=False)
    elif params is not None:
        m.load_state_dict(params)
    m.x.copy_(X.to(m.device, torch.float32))
    m.forward_device(want_logits=True, keep=keep)
    return m.logits
