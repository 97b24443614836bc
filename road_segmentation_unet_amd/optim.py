"""The optimizer step of the U-Net in one place: the float32 host arithmetic of its rules, the validators of UNet's optimizer arguments and
OptimizerStep, the base class of unet.UNet that owns the optimizer's state and apply_momentum / apply_adam (kernels: csrc/optim.hip)."""
import contextlib
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import call

_PACK_CONV_FWD, _PACK_CONV_BWD, _PACK_CONVT_FWD, _PACK_CONVT_BWD, _PACK_CONV_FIRST = range(5)   # rsu.h RSU_PACK_*


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def adam_scalars(lr_t, beta1_power, beta2_power, beta1, beta2):
    """The host side of one tf.train.AdamOptimizer step, float32 as TensorFlow computes it: alpha = lr_t * sqrt(1 - beta2^t) / (1 - beta1^t)
    (ApplyAdam's step size, from the powers BEFORE the step) and the powers after it (AdamOptimizer._finish: beta1_power * beta1,
    beta2_power * beta2). Returns (alpha, next beta1_power, next beta2_power) as numpy float32 scalars."""
    f = np.float32
    b1p, b2p = f(beta1_power), f(beta2_power)
    alpha = f(lr_t) * np.sqrt(f(1) - b2p) / (f(1) - b1p)
    return f(alpha), f(b1p * f(beta1)), f(b2p * f(beta2))


def clip_scale(sumsq, max_norm):
    """The host mirror of the record rsu.h rsu_grad_norm writes: from the float32 sum of squares and max_norm (rounded to float32, as the
    ABI takes it) the pair (norm, scale) as numpy float32 scalars, norm = (float)sqrt((double)sumsq) and scale = norm > max_norm ?
    (float)((double)max_norm / (double)norm) : 1 -- exactly 1 at norm == max_norm. A sumsq that is not finite (an overflow included) is
    the skipped step: scale 0."""
    f = np.float32
    s, c = f(sumsq), np.float64(f(max_norm))
    with np.errstate(invalid="ignore"):
        norm = f(np.sqrt(np.float64(s)))
    if not np.isfinite(s):
        return norm, f(0.0)
    return norm, (f(c / np.float64(norm)) if np.float64(norm) > c else f(1.0))


def _clip_arg(value):
    """UNet's clip_grad_norm: None (no clipping), or a finite float > 0"""
    if value is None:
        return None
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not (math.isfinite(v) and v > 0.0):
        raise _lib.RsuError("clip_grad_norm must be None or a finite float > 0, not %r" % (value,))
    return v


def _ema_arg(value):
    """UNet's ema_decay: None or 0 (no averaging), or a float in (0, 1)"""
    if value is None:
        return None
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not (0.0 <= v and np.float32(v) < np.float32(1.0)):   # (below 1 as the float32 the kernel's scalar comes from)
        raise _lib.RsuError("ema_decay must be None or a float in [0, 1), not %r" % (value,))
    return v if v > 0.0 else None


def ema_decay_at(decay, t, warmup=True):
    """The decay of the moving average's update number t (t = 1 for the first: the global_step the optimizer step has just produced),
    float32 as tf.train.ExponentialMovingAverage computes it: with warm-up (its num_updates rule) min(f32(decay), f32(1 + t) / f32(10 + t)),
    else f32(decay). Returns a numpy float32; the kernel gets f32(1) - it."""
    f = np.float32
    d = f(decay)
    if warmup:
        d = min(d, f(1 + int(t)) / f(10 + int(t)))
    return f(d)


LR_SCHEDULES = ("staircase", "constant", "cosine", "linear")
DECAY_MODES = ("decoupled", "l2")
DEFAULT_LR_SCHEDULE = ("staircase", 0, 0, 0.0)   # lr_at's defaults: the reference's curve


def _int_arg(value, what, lowest=0):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < lowest:
        raise ValueError("%s must be an integer >= %d, not %r" % (what, lowest, value))
    return int(value)


def lr_at(step, lr0, schedule="staircase", warmup_steps=0, total_steps=0, final=0.0):
    """The learning rate of the optimizer step taken after `step` steps (t = step, the global_step in front of the step), as the
    float the update pass receives: float(np.float32(base * warm)), base and warm in float64, rounded once.
    base, by schedule:
      staircase  the reference's tf.train.exponential_decay(lr0, t, 1000, 0.95, staircase=True) (tf_aerial_images.py:116-117), the
                 float32 expression f32(lr0) * f32(0.95) ** f32(t // 1000)
      constant   lr0
      cosine     lr0 * (F + (1 - F) * 0.5 * (1 + cos(pi * min(t, T) / T)))
      linear     lr0 * (F + (1 - F) * (1 - min(t, T) / T))
    with T = total_steps >= 1 (cosine and linear; the other two ignore it) and F = final in [0, 1], the fraction of lr0 the two end at.
    warm = min(1, (t + 1) / W) for W = warmup_steps > 0, else 1: a linear ramp over the first W steps, on top of any schedule.
    The defaults (staircase, no warm-up) return the bits the reference's expression has. Bad arguments raise ValueError."""
    t = _int_arg(step, "step")
    W, T = _int_arg(warmup_steps, "warmup_steps"), _int_arg(total_steps, "total_steps")
    try:
        lr0f, F = float(lr0), float(final)
    except (TypeError, ValueError):
        lr0f = F = float("nan")
    if isinstance(lr0, bool) or isinstance(final, bool) or not (math.isfinite(lr0f) and lr0f >= 0.0):
        raise ValueError("lr0 must be a finite float >= 0, not %r" % (lr0,))
    if not (0.0 <= F <= 1.0):
        raise ValueError("final must be a float in [0, 1], not %r" % (final,))
    if schedule not in LR_SCHEDULES:
        raise ValueError("schedule must be one of %s, not %r" % ("|".join(LR_SCHEDULES), schedule))
    if schedule in ("cosine", "linear") and T < 1:
        raise ValueError("the %s schedule needs total_steps >= 1, not %r" % (schedule, total_steps))
    if schedule == "staircase":
        base = float(np.float32(lr0f) * np.float32(0.95) ** np.float32(t // 1000))
    elif schedule == "constant":
        base = lr0f
    elif schedule == "cosine":
        base = lr0f * (F + (1.0 - F) * 0.5 * (1.0 + math.cos(math.pi * min(t, T) / T)))
    else:
        base = lr0f * (F + (1.0 - F) * (1.0 - min(t, T) / T))
    warm = min(1.0, (t + 1) / W) if W > 0 else 1.0
    return float(np.float32(base * warm))


def _decay_args(value, mode):
    """UNet's weight_decay and weight_decay_mode: (None or a finite lambda > 0, "decoupled" or "l2")"""
    if mode not in DECAY_MODES:
        raise ValueError("weight_decay_mode must be one of %s, not %r" % ("|".join(DECAY_MODES), mode))
    if value is None:
        return None, mode
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not (math.isfinite(v) and v > 0.0):
        raise ValueError("weight_decay must be None or a finite float > 0, not %r" % (value,))
    return v, mode


def _accumulate_arg(value):
    """UNet's accumulate_steps: None or 1 (one backward pass per optimizer step), or an int K > 1"""
    if value is None:
        return 1
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1:
        raise _lib.RsuError("accumulate_steps must be None or an int >= 1, not %r" % (value,))
    return int(value)


EMA_SUFFIX = "/ExponentialMovingAverage"   # TensorFlow's name of a variable's shadow
OPTIMIZERS = ("momentum", "adam")


def _fused_update(needed_by=None, variant=None):
    """whether the step is the one-pass update table; RSU_FUSED_UPDATE=0: two launches, the rule and the re-pack. needed_by: raises there"""
    fused = os.environ.get("RSU_FUSED_UPDATE", "1") != "0"
    if needed_by and not fused:
        raise _lib.RsuError("%s needs the fused update pass: RSU_FUSED_UPDATE=0 (rsu_momentum_step / rsu_adam_step) has no %s variant"
                            % (needed_by, variant))
    return fused


class OptimizerStep:
    """The optimizer's half of unet.UNet: its arguments, its state (views into flat buffers laid out like flat_w, read by name on the net)
    and the step. It uses the net's device, names, _slices, n_flat, n_live, flat_w, flat_g, w, pk, repack(), _packed_kernels(), _stream()."""

    def _init_optimizer(self, training, optimizer, clip_grad_norm, ema_decay, ema_warmup, accumulate_steps, weight_decay, weight_decay_mode):
        if optimizer not in OPTIMIZERS:
            raise _lib.RsuError("optimizer must be one of %s, not %r" % ("|".join(OPTIMIZERS), optimizer))
        self.optimizer = optimizer
        self.accumulate_steps = _accumulate_arg(accumulate_steps)
        if self.accumulate_steps > 1 and not training:
            raise _lib.RsuError("a forward-only net takes no optimizer step: it has no gradients to accumulate")
        self.weight_decay, self.weight_decay_mode = _decay_args(weight_decay, weight_decay_mode)
        if self.weight_decay is not None and not training:
            raise ValueError("a forward-only net takes no optimizer step: it has no weights to decay")
        self.lr_schedule = DEFAULT_LR_SCHEDULE   # (schedule, warmup_steps, total_steps, final) of lr_at (set_lr_schedule)
        self.flat_gsum, self._accum_calls = None, 0   # the running sum of the micro-batch gradients; accumulate_gradients() calls since the last step
        self.clip_grad_norm = _clip_arg(clip_grad_norm)
        self.ema_decay, self.ema_warmup = _ema_arg(ema_decay), bool(ema_warmup)
        if self.ema_decay is not None and not training:
            raise _lib.RsuError("a forward-only net takes no optimizer step: it has nothing to average")
        self.flat_ema, self.ema, self._averaged = None, {}, False   # the shadow of flat_w, its per-variable views; inside averaged_weights()?
        self.clip_state = self._clip_ws = None   # the device-resident state record (rsu.h, 8 x 32 bit) and the norm's workspace, with clipping
        self._update_table = None   # the job table of the optimizer's update pass (_build_update_table), built on first use

    def _alloc_optimizer_state(self):
        """the optimizer's buffers, once _alloc_params has laid out flat_w and copied the initial weights in"""
        dev = self.device
        self.flat_acc = torch.zeros(self.n_flat, dtype=torch.float32, device=dev)   # Momentum slots (tf_aerial_images.py:120); Adam: m
        # Adam's second slot v (a Momentum net has none)
        self.flat_v = torch.zeros(self.n_flat, dtype=torch.float32, device=dev) if self.optimizer == "adam" else None
        self.acc = {n: self.flat_acc[o:o + cnt].view(s) for n, (o, cnt, s) in self._slices.items()}
        self.v = {n: self.flat_v[o:o + cnt].view(s) for n, (o, cnt, s) in self._slices.items()} if self.flat_v is not None else {}
        if self.clip_grad_norm is not None:
            # the norm runs over the contiguous flat_g[0:n_live): the padding floats between the variables are zero here and never
            # written, so they add nothing, and the dead dilated pair behind n_live is left out as it is for the update
            lib = _lib.lib()
            assert lib.rsu_clip_state_bytes() == _lib.CLIP_STATE_BYTES
            self.clip_state = torch.zeros(_lib.CLIP_STATE_BYTES // 4, dtype=torch.int32, device=dev)   # zeroed once: its counters accumulate
            self._clip_ws = torch.empty(lib.rsu_grad_norm_ws_floats(self.n_live), dtype=torch.float32, device=dev)
        if self.ema_decay is not None:
            # TensorFlow initialises a shadow to its variable's initial value; the dead dilated pair behind n_live keeps that value
            self.flat_ema = self.flat_w.clone()
            self.ema = {n: self.flat_ema[o:o + cnt].view(s) for n, (o, cnt, s) in self._slices.items()}
        if self.accumulate_steps > 1:
            self.flat_gsum = torch.zeros(self.n_flat, dtype=torch.float32, device=dev)
        self.global_step = 0
        # Adam's float32 accumulators beta1^t, beta2^t (None: not started -- the first apply_adam sets them to its (beta1, beta2),
        # the initial values TensorFlow gives them)
        self.beta1_power = self.beta2_power = None

    def _optimizer_state_dict(self):
        """state_dict() behind the weights: the averages, the slots (with Adam's powers once a step has set them), global_step"""
        d = {n + EMA_SUFFIX: self.ema[n].detach().cpu().numpy().copy() for n in self.ema}
        if self.optimizer == "adam":
            d.update({n + "/Adam": self.acc[n].detach().cpu().numpy().copy() for n in self.names})
            d.update({n + "/Adam_1": self.v[n].detach().cpu().numpy().copy() for n in self.names})
            if self.beta1_power is not None:
                d["beta1_power"], d["beta2_power"] = np.float32(self.beta1_power), np.float32(self.beta2_power)
        else:
            d.update({n + "/Momentum": self.acc[n].detach().cpu().numpy().copy() for n in self.names})
        d["global_step"] = np.int64(self.global_step)
        return d

    def _load_optimizer_state(self, d):
        """load_state_dict() behind the weights (the fallback rules are documented there)"""
        adam = self.optimizer == "adam"
        have_adam = adam and any(n + "/Adam" in d for n in self.names)
        for n in self.names:
            if adam:
                for slot, t in (("/Adam", self.acc[n]), ("/Adam_1", self.v[n])):
                    if have_adam and n + slot in d:
                        t.copy_(torch.from_numpy(np.ascontiguousarray(d[n + slot], dtype=np.float32)))
                    else:
                        t.zero_()
            elif n + "/Momentum" in d:
                self.acc[n].copy_(torch.from_numpy(np.ascontiguousarray(d[n + "/Momentum"], dtype=np.float32)))
            if self.flat_ema is not None:
                self.ema[n].copy_(torch.from_numpy(np.ascontiguousarray(d.get(n + EMA_SUFFIX, d[n]), dtype=np.float32)))
        if adam:
            if have_adam and "beta1_power" in d and "beta2_power" in d:
                self.beta1_power, self.beta2_power = np.float32(d["beta1_power"]), np.float32(d["beta2_power"])
            else:
                self.beta1_power = self.beta2_power = None
        self.global_step = int(d.get("global_step", 0))
        self._accum_calls = 0   # (a half-accumulated step belongs to the weights that were replaced)

    def set_lr_schedule(self, schedule="staircase", warmup_steps=0, total_steps=0, final=0.0):
        """the learning-rate curve of learning_rate(): the arguments of lr_at (validated here, ValueError). The default is the
        reference's tf.train.exponential_decay staircase. Not part of state_dict(): the curve is a function of global_step, which is."""
        lr_at(0, 0.0, schedule, warmup_steps, total_steps, final)
        self.lr_schedule = (schedule, int(warmup_steps), int(total_steps), float(final))

    def learning_rate(self, lr0):
        """the rate of the next optimizer step, lr_at(global_step, lr0, *lr_schedule) -- by default tf.train.exponential_decay(lr,
        global_step, 1000, 0.95, staircase=True) (tf_aerial_images.py:116-117), float32. apply_momentum / apply_adam and the logged
        `learning_rate` scalar both read it here."""
        return lr_at(self.global_step, lr0, *getattr(self, "lr_schedule", DEFAULT_LR_SCHEDULE))

    def decaying_parameters(self):
        """(parameters that weight decay touches, live parameters): the packed kernels of the update table against everything stepped"""
        decays = sum(self._slices[n][1] for _kind, n, _sh, _segs in self._packed_kernels())
        return decays, sum(self._slices[n][1] for n in self.names if self._slices[n][0] < self.n_live)

    def _decay_call(self, lr_t):
        """the (decay, mode) arguments of the decaying update pass at the scheduled rate lr_t (rsu_optim.h): decoupled: f32(lr_t) *
        f32(lambda), one float32 product; l2: lambda. None where the decoupled product is zero -- a schedule that has reached a rate of 0
        -- and the step is the plain one (the entry takes no decay of 0). Raises where there is no such pass (RSU_FUSED_UPDATE=0)."""
        _fused_update("weight_decay", "decaying")
        if self.weight_decay_mode == "l2":
            return float(np.float32(self.weight_decay)), _lib.DECAY_L2
        d = float(np.float32(lr_t) * np.float32(self.weight_decay))
        if d == 0.0:
            return None
        if not (math.isfinite(d) and d > 0.0):
            raise _lib.RsuError("weight_decay: f32(lr) * f32(lambda) = %r at step %d is not a finite float32 (lr %r, lambda %r)"
                                % (d, self.global_step, lr_t, self.weight_decay))
        return d, _lib.DECAY_DECOUPLED

    def _build_update_table(self):
        """the job table of rsu_update_table_run: one entry per conv / transposed-conv kernel (with its packed copies), the variables between
        them (biases, colour adjust, the 1x1 head) as plain Momentum ranges; covers [0, n_live) of the flat buffers once. An Adam net: the
        table of rsu_update_table_run_adam (every entry also gets its slice of flat_v; acc holds m). Cached as self._update_table."""
        lib = _lib.lib()
        if not hasattr(self, "pk"):
            self.repack()
        adam = self.optimizer == "adam"
        entries, plain_lo = [], 0   # ("plain", lo, hi) / ("tensor", name, (kind, shape, segments))
        for kind, n, sh, segs in self._packed_kernels():
            o, c, _ = self._slices[n]
            if plain_lo < o:
                entries.append(("plain", plain_lo, o))
            entries.append(("tensor", n, (kind, sh, segs)))
            plain_lo = (o + c + 3) // 4 * 4   # (the 16-byte aligned start of the next variable)
        if plain_lo < self.n_live:
            entries.append(("plain", plain_lo, self.n_live))
        esz = lib.rsu_update_table_entry_bytes()
        host = ctypes.create_string_buffer(esz * len(entries))
        keep = []
        for idx, e in enumerate(entries):
            if e[0] == "plain":
                lo, hi = e[1], e[2]
                rc = lib.rsu_update_table_add_plain(host, idx, _ptr(self.flat_w[lo:hi]), _ptr(self.flat_acc[lo:hi]), _ptr(self.flat_g[lo:hi]), hi - lo)
                v = self.flat_v[lo:hi] if adam else None
            else:
                n, (kind, sh, segs) = e[1], e[2]
                w, a, g = _ptr(self.w[n]), _ptr(self.acc[n]), _ptr(self.g[n])
                bw = None
                if kind == _PACK_CONVT_FWD:
                    cout, cin = sh[2], sh[3]
                    bw = (ctypes.c_void_p * 1)(self.pk[n, "bwd"].data_ptr()) if self.training else None
                    rc = lib.rsu_update_table_add(host, idx, kind, w, a, g, _ptr(self.pk[n, "fwd"]), bw, cin, cout, None, 0)
                elif kind == _PACK_CONV_FIRST:
                    rc = lib.rsu_update_table_add(host, idx, kind, w, a, g, _ptr(self.pk[n, "fwd"]), None, 3, sh[3], None, 0)
                else:
                    bw = (ctypes.c_void_p * len(segs))(*[self.pk[n, "bwd", si].data_ptr() for si in range(len(segs))]) if self.training else None
                    rc = lib.rsu_update_table_add(host, idx, kind, w, a, g, _ptr(self.pk[n, "fwd"]), bw, sh[2], sh[3], (ctypes.c_int * len(segs))(*segs), len(segs))
                keep.append(bw)
                v = self.v[n] if adam else None
            if rc != 1:
                raise _lib.RsuError("rsu_update_table_add(%s) failed: %d" % (e[1], rc))
            if adam:
                _lib.check(lib.rsu_update_table_set_second_slot(host, idx, _ptr(v)), "rsu_update_table_set_second_slot(%s)" % (e[1],))
        nb = ctypes.c_int(0)
        _lib.check(lib.rsu_update_table_finish(host, len(entries), ctypes.byref(nb)), "rsu_update_table_finish")
        self._update_table = (torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(self.device), len(entries), nb.value)
        return self._update_table

    def _grad_norm(self):
        """a clipping net, in front of its update pass and on the same stream: the norm of flat_g[0:n_live) and the factor for
        clip_grad_norm into self.clip_state (rsu.h rsu_grad_norm). Under data parallelism the caller has finished the gradient exchange,
        so every rank reads the same all-reduced gradient and computes the same bits: no collective of its own."""
        _fused_update("clip_grad_norm", "clipped")
        call("rsu_grad_norm", _ptr(self.flat_g), self.n_live, self.clip_grad_norm, _ptr(self._clip_ws), _ptr(self.clip_state), self._stream())

    # ------------------------------------------------------------------ gradient accumulation
    def accumulate_gradients(self):
        """an accumulating net (accumulate_steps = K > 1), behind every backward_device() and on the current stream -- the main stream,
        which has joined the side streams at the end of the pass, and which every side-stream launch of the NEXT pass waits for
        (schedule.side), so no gradient is overwritten before it has been read here. One rsu_grad_accumulate launch (rsu.h), no host
        synchronisation: call 0 of a step assigns flat_gsum = flat_g (the previous step's sum is forgotten, not zeroed), calls 0 < j < K-1
        add flat_gsum += flat_g, call K-1 adds the other way, flat_g += flat_gsum: flat_g[0:n_live) then holds
        ((g_0 + g_1) + ...) + g_{K-1} in float32 and the exchange, _grad_norm, the update tables and _ema_step read the buffer they
        always read. Under data parallelism the exchange comes after the K-th call. A (K+1)-th call without a step raises. On a net
        that does not accumulate: nothing, no launch."""
        K = self.accumulate_steps
        if K == 1:
            return
        self._not_averaged("accumulate_gradients")
        j = self._accum_calls
        if j >= K:
            raise _lib.RsuError("accumulate_gradients: %d calls since the last optimizer step on a net with accumulate_steps=%d; "
                                "apply_%s comes first" % (j, K, self.optimizer))
        if j < K - 1:
            call("rsu_grad_accumulate", _ptr(self.flat_gsum), _ptr(self.flat_g), self.n_live, 1 if j == 0 else 0, self._stream())
        else:
            call("rsu_grad_accumulate", _ptr(self.flat_g), _ptr(self.flat_gsum), self.n_live, 0, self._stream())
        self._accum_calls = j + 1

    def _accumulated(self, what):
        """apply_momentum / apply_adam on an accumulating net: flat_g holds the sum only after exactly accumulate_steps calls"""
        if self.accumulate_steps > 1 and self._accum_calls != self.accumulate_steps:
            raise _lib.RsuError("%s after %d of %d accumulate_gradients() calls: flat_g does not hold the sum of the step's gradients yet"
                                % (what, self._accum_calls, self.accumulate_steps))

    def clip_stats(self):
        """The state record of a clipping net, read back once (a synchronisation: call it per epoch, not per step): steps, clipped and
        skipped count the updates so far, norm / scale / sumsq and the two flags describe the last one. None on a net without clipping."""
        if self.clip_state is None:
            return None
        raw = self.clip_state.cpu().numpy()
        f = raw.view(np.float32)
        flags = int(raw[3])
        return {"steps": int(raw[4]), "clipped": int(raw[5]), "skipped": int(raw[6]), "norm": float(f[1]), "scale": float(f[2]),
                "sumsq": float(f[0]), "last_clipped": bool(flags & _lib.CLIP_CLIPPED), "last_skipped": bool(flags & _lib.CLIP_NONFINITE)}

    # ------------------------------------------------------------------ moving average of the weights
    def _ema_step(self):
        """an averaging net, at the end of its optimizer step, on the update pass's stream and behind it: flat_ema[0:n_live) moves towards
        the weights the step has just written, at the decay of update number global_step (already advanced). One launch (rsu.h
        rsu_ema_step), no host synchronisation. A clipping net hands its record on: a step the update pass skipped moves no average.
        Under data parallelism every rank averages the same weights: nothing is exchanged."""
        if self.flat_ema is None:
            return
        omd = np.float32(1.0) - ema_decay_at(self.ema_decay, self.global_step, self.ema_warmup)
        call("rsu_ema_step", _ptr(self.flat_ema), _ptr(self.flat_w), self.n_live, float(omd), _ptr(self.clip_state), self._stream())

    def _not_averaged(self, what):
        if self._averaged:
            raise _lib.RsuError("%s inside averaged_weights(): flat_w holds the averages there, forward passes only" % what)

    def _swap_averages(self):
        tmp = self.flat_w.clone()
        self.flat_w.copy_(self.flat_ema)
        self.flat_ema.copy_(tmp)
        self.repack()

    @contextlib.contextmanager
    def averaged_weights(self):
        """Forward-only use of the averages: on entry flat_w and flat_ema exchange their contents (all n_flat floats, device copies
        through a temporary, on the current stream) and repack() rebuilds the bf16 MFMA copies, so every forward launch inside -- packed
        convs, biases, colour adjust, the 1x1 head -- reads the averages; on exit they exchange back and repack() runs again.
        apply_momentum, apply_adam, backward_device, state_dict, load_state_dict and a nested entry raise RsuError inside. A net without
        averages: a no-op context.
        What the exit leaves, checked against the code: flat_w and flat_ema hold their earlier bits (three whole-buffer copies each way);
        the optimizer slots, flat_g and global_step are never touched; every packed buffer is rewritten by repack() from the restored
        flat_w. There is ONE set of packed buffers (self.pk: no double-buffered backward packs exist in this tree), the pack table is
        built once in __init__ and covers every pk tensor a training net has, backward packs included, and rsu_pack_table_run writes
        the bits the update pass writes for the same weights (rsu.h; tests/test_gpu_ops.py, tests/test_gpu_adam.py) -- so the packed
        copies are those a following training step expects, and the update table, which holds pointers to the same buffers, stays
        valid. tests/test_gpu_ema.py compares all of it bit for bit and takes one more step beside a twin."""
        if self.flat_ema is None:
            yield self
            return
        self._not_averaged("averaged_weights")
        self._swap_averages()
        self._averaged = True
        try:
            yield self
        finally:
            self._averaged = False
            self._swap_averages()

    # ------------------------------------------------------------------ the step
    def _step(self, kind, lr0, gscale, hyper):
        """One step of rule `kind` ("momentum": hyper = (momentum,); "adam": hyper = (beta1, beta2, epsilon)): the checks, the scheduled rate,
        the decay arguments and the gradient norm (both refuse RSU_FUSED_UPDATE=0 before anything is touched), then ONE update launch,
        rsu_update_table_run[_adam][_decay | _clip], then the counters, the powers and the moving average."""
        what = "apply_" + kind
        if self.optimizer != kind:
            raise _lib.RsuError("%s on a net built with optimizer=%r" % (what, self.optimizer))
        self._not_averaged(what)
        self._accumulated(what)
        lr_t = self.learning_rate(lr0)
        decay = self._decay_call(lr_t) if self.weight_decay is not None else None
        if self.clip_grad_norm is not None:
            self._grad_norm()
        if kind == "adam":
            beta1, beta2, epsilon = hyper
            if self.beta1_power is None:
                self.beta1_power, self.beta2_power = np.float32(beta1), np.float32(beta2)
            alpha, b1p, b2p = adam_scalars(lr_t, self.beta1_power, self.beta2_power, beta1, beta2)
            entry, slots = "_adam", (self.flat_w, self.flat_acc, self.flat_v, self.flat_g)
            scalars = (float(alpha), float(np.float32(beta1)), float(np.float32(beta2)), float(np.float32(epsilon)), gscale)
        else:
            entry, slots, scalars = "", (self.flat_w, self.flat_acc, self.flat_g), (lr_t, hyper[0], gscale)
        arm = "_decay" if decay is not None else "_clip" if self.clip_grad_norm is not None else ""
        if arm or _fused_update():
            tab = self._update_table or self._build_update_table()
            state = (*(decay or ()), _ptr(self.clip_state)) if arm else ()   # (decay, mode, record) | (record,) | nothing
            call("rsu_update_table_run" + entry + arm, _ptr(tab[0]), tab[1], tab[2], *scalars, *state, self._stream())
        else:
            call("rsu_%s_step" % kind, *[_ptr(t) for t in slots], *scalars, self.n_live, self._stream())
            self.repack()
        self.global_step += 1
        self._accum_calls = 0
        if kind == "adam":
            self.beta1_power, self.beta2_power = b1p, b2p
        self._ema_step()

    def apply_momentum(self, lr0, momentum, gscale=1.0):
        """MomentumOptimizer step on every live variable (tf_aerial_images.py:120-121) and the re-pack of the bf16 MFMA copies, in one
        pass over the parameters (rsu_update_table_run; RSU_FUSED_UPDATE=0: rsu_momentum_step, then the batched re-pack -- same bits).
        A net built with clip_grad_norm: rsu_grad_norm, then rsu_update_table_run_clip, whose gscale is this gscale times the factor on
        the device. A step whose gradient is not finite leaves weights, slots and packed copies as they are but STILL COUNTS as a step:
        the host does not know (that is the point), so global_step and the decay staircase advance -- and under Adam the beta powers,
        while m and v stay untouched; clip_stats() tells how often it happened.
        A net built with weight_decay: rsu_update_table_run_decay in place of either pass (behind rsu_grad_norm on a clipping net, whose
        record it reads: a skipped step decays nothing)."""
        self._step("momentum", lr0, gscale, (momentum,))

    def apply_adam(self, lr0, beta1=0.9, beta2=0.999, epsilon=1e-8, gscale=1.0):
        """tf.train.AdamOptimizer step on every live variable (TensorFlow 1.x ApplyAdam at the decayed rate learning_rate(lr0)) and the
        re-pack of the bf16 MFMA copies, in one pass over the parameters (rsu_update_table_run_adam; RSU_FUSED_UPDATE=0: rsu_adam_step,
        then the batched re-pack -- same bits). alpha and the beta powers are float32 host arithmetic (adam_scalars); global_step and
        the powers advance after the launch. The dead level-(L-1) dilated pair is never stepped.
        A net built with clip_grad_norm: rsu_grad_norm, then rsu_update_table_run_adam_clip; a skipped step still advances global_step
        and the beta powers (see apply_momentum).
        A net built with weight_decay: rsu_update_table_run_adam_decay in place of either pass; the decoupled decay is taken at the
        scheduled rate learning_rate(lr0), not at the bias-corrected alpha."""
        self._step("adam", lr0, gscale, (beta1, beta2, epsilon))
