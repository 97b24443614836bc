"""No GPU: which ABI entries one optimizer step calls, in which order and with which arguments, for every arm of the step -- optimizer x
clipping x weight decay (none, decoupled, l2, decoupled at a scheduled rate of 0) x RSU_FUSED_UPDATE x moving average -- on a stub net
that has only the attributes the step reads, with the module-level `call` replaced by a recorder. The expected calls are written out
below, independent of the code under test; the scalars are restated in float32 here."""
import ctypes

import numpy as np
import pytest
import torch

from road_segmentation_unet_amd import optim as step_module   # the module through whose `call` the step reaches the ABI
from road_segmentation_unet_amd._lib import RsuError
from road_segmentation_unet_amd.unet import UNet

f32 = np.float32
STREAM = 0x5EED
N_LIVE, STEP0, K = 6, 5, 2
LR0, MU, GSCALE, CLIP, LAMBDA, EMA = 0.01, 0.9, 0.5, 2.5, 1e-4, 0.999
B1, B2, EPS = 0.9, 0.999, 1e-8
TABLE_ENTRIES, TABLE_BLOCKS = 3, 7
CONSTANT, ZERO_RATE = ("constant", 0, 0, 0.0), ("linear", 0, STEP0, 0.0)   # the linear curve has reached 0 at step STEP0
LR_T = float(f32(LR0))
ALPHA = float(f32(LR_T) * np.sqrt(f32(1) - f32(B2)) / (f32(1) - f32(B1)))   # Adam's first step: the powers are (beta1, beta2)
OMD = float(f32(1) - min(f32(EMA), f32(1 + STEP0 + 1) / f32(10 + STEP0 + 1)))   # the average's update number is the advanced global_step
DECAYS = {"none": (None, "decoupled", CONSTANT), "decoupled": (LAMBDA, "decoupled", CONSTANT), "l2": (LAMBDA, "l2", CONSTANT),
          "zero_rate": (LAMBDA, "decoupled", ZERO_RATE)}


def _stub(optimizer, clip, decay, ema, record):
    net = object.__new__(UNet)
    net.optimizer = optimizer
    net.flat_w, net.flat_acc, net.flat_g = torch.zeros(8), torch.zeros(8), torch.zeros(8)
    net.flat_v = torch.zeros(8) if optimizer == "adam" else None
    net.flat_ema, net.ema_decay, net.ema_warmup = (torch.zeros(8), EMA, True) if ema else (None, None, True)
    net.clip_grad_norm = CLIP if clip else None
    net.clip_state, net._clip_ws = (torch.zeros(8, dtype=torch.int32), torch.zeros(2)) if clip else (None, None)
    net.weight_decay, net.weight_decay_mode, net.lr_schedule = DECAYS[decay]
    net._update_table = (torch.zeros(16, dtype=torch.uint8), TABLE_ENTRIES, TABLE_BLOCKS)
    net.n_live, net.global_step = N_LIVE, STEP0
    net.accumulate_steps, net._accum_calls, net._averaged = K, K, False   # (the K calls of an accumulating net are in: it may step)
    net.beta1_power = net.beta2_power = None
    net._stream = lambda: STREAM
    net.repack = lambda: record.append(("repack",))
    return net


def _p(t):
    return ("ptr", t.data_ptr()) if t is not None else None


def _recorder(record):
    def call(name, *args):
        record.append((name,) + tuple(("ptr", a.value) if isinstance(a, ctypes.c_void_p) else a for a in args))
    return call


def _apply(net):
    if net.optimizer == "adam":
        net.apply_adam(LR0, B1, B2, EPS, gscale=GSCALE)
    else:
        net.apply_momentum(LR0, MU, gscale=GSCALE)


def _expected(net, decay, fused):
    """the calls of one step, in order"""
    adam, clip = net.optimizer == "adam", net.clip_grad_norm is not None
    lr_t = 0.0 if decay == "zero_rate" else LR_T
    rule = (float(f32(lr_t) * np.sqrt(f32(1) - f32(B2)) / (f32(1) - f32(B1))), float(f32(B1)), float(f32(B2)), float(f32(EPS)), GSCALE) if adam \
        else (lr_t, MU, GSCALE)
    table = (_p(net._update_table[0]), TABLE_ENTRIES, TABLE_BLOCKS)
    state = _p(net.clip_state)
    want = []
    if clip:
        want.append(("rsu_grad_norm", _p(net.flat_g), N_LIVE, CLIP, _p(net._clip_ws), state, STREAM))
    if decay == "decoupled":
        want.append(("rsu_update_table_run_adam_decay" if adam else "rsu_update_table_run_decay",) + table + rule
                    + (float(f32(LR_T) * f32(LAMBDA)), 1, state, STREAM))
    elif decay == "l2":
        want.append(("rsu_update_table_run_adam_decay" if adam else "rsu_update_table_run_decay",) + table + rule
                    + (float(f32(LAMBDA)), 0, state, STREAM))
    elif clip:
        want.append(("rsu_update_table_run_adam_clip" if adam else "rsu_update_table_run_clip",) + table + rule + (state, STREAM))
    elif fused:
        want.append(("rsu_update_table_run_adam" if adam else "rsu_update_table_run",) + table + rule + (STREAM,))
    elif adam:
        want += [("rsu_adam_step", _p(net.flat_w), _p(net.flat_acc), _p(net.flat_v), _p(net.flat_g)) + rule + (N_LIVE, STREAM), ("repack",)]
    else:
        want += [("rsu_momentum_step", _p(net.flat_w), _p(net.flat_acc), _p(net.flat_g)) + rule + (N_LIVE, STREAM), ("repack",)]
    if net.flat_ema is not None:
        want.append(("rsu_ema_step", _p(net.flat_ema), _p(net.flat_w), N_LIVE, OMD, state, STREAM))
    return want


@pytest.mark.parametrize("ema", [False, True])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("decay", list(DECAYS))
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
def test_one_step_issues_these_calls(optimizer, clip, decay, fused, ema, monkeypatch):
    record = []
    monkeypatch.setattr(step_module, "call", _recorder(record))
    if fused:
        monkeypatch.delenv("RSU_FUSED_UPDATE", raising=False)
    else:
        monkeypatch.setenv("RSU_FUSED_UPDATE", "0")
    net = _stub(optimizer, clip, decay, ema, record)
    if not fused and (clip or decay != "none"):
        # the two-launch step has no clipping and no decaying variant: refused before anything is touched or launched
        with pytest.raises(RsuError, match="RSU_FUSED_UPDATE"):
            _apply(net)
        assert record == []
        assert net.global_step == STEP0 and net._accum_calls == K and net.beta1_power is None and net.beta2_power is None
        return
    _apply(net)
    want = _expected(net, decay, fused)
    assert [c[0] for c in record] == [c[0] for c in want]
    assert record == want
    assert net.global_step == STEP0 + 1 and net._accum_calls == 0
    if optimizer == "adam":
        assert (net.beta1_power, net.beta2_power) == (f32(B1) * f32(B1), f32(B2) * f32(B2))
        assert net.beta1_power.dtype == np.float32 and net.beta2_power.dtype == np.float32
    else:
        assert net.beta1_power is None and net.beta2_power is None


def test_the_ladder_table_is_what_it_says():
    """the arithmetic the expected calls rest on: the rate that has reached 0, alpha of the first Adam step, the average's decay"""
    assert LR_T == float(f32(0.01)) and OMD == float(f32(1) - f32(7) / f32(16)) == 0.5625
    # (float32 against float64: 1 - f32(0.999) carries 2^-24 / 1e-3 = 6e-5 of relative error, its root half of that, on alpha = 3.2e-3)
    assert abs(ALPHA - 0.01 * np.sqrt(1 - 0.999) / (1 - 0.9)) < 3.2e-3 * 4e-5


@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
def test_a_second_adam_step_uses_the_advanced_powers_and_a_wrong_front_refuses(optimizer, monkeypatch):
    record = []
    monkeypatch.setattr(step_module, "call", _recorder(record))
    monkeypatch.delenv("RSU_FUSED_UPDATE", raising=False)
    net = _stub(optimizer, False, "none", False, record)
    with pytest.raises(RsuError, match="optimizer="):
        net.apply_momentum(LR0, MU) if optimizer == "adam" else net.apply_adam(LR0)
    assert record == [] and net.global_step == STEP0 and net._accum_calls == K
    if optimizer == "adam":
        _apply(net)
        net._accum_calls = K
        _apply(net)
        b1p, b2p = f32(B1) * f32(B1), f32(B2) * f32(B2)
        assert record[1][4] == float(f32(LR_T) * np.sqrt(f32(1) - b2p) / (f32(1) - b1p))
        assert (net.beta1_power, net.beta2_power) == (b1p * f32(B1), b2p * f32(B2)) and net.global_step == STEP0 + 2
