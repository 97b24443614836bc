"""CPU: the Adam flags of the driver and the float32 host arithmetic of UNet.apply_adam (alpha, the beta powers, the decayed rate)
against a numpy restatement of tf.train.AdamOptimizer."""
import numpy as np
import pytest

from road_segmentation_unet_amd.cli import parse_options
from road_segmentation_unet_amd.model import Options
from road_segmentation_unet_amd.unet import adam_scalars


def test_adam_flags_parse():
    o = parse_options(["--optimizer=adam", "--adam_beta1=0.8", "--adam_beta2=0.99", "--adam_epsilon=1e-6"])
    assert (o.optimizer, o.adam_beta1, o.adam_beta2, o.adam_epsilon) == ("adam", 0.8, 0.99, 1e-6)


def test_adam_flag_defaults_are_tensorflows():
    o = parse_options([])
    assert (o.optimizer, o.adam_beta1, o.adam_beta2, o.adam_epsilon) == ("momentum", 0.9, 0.999, 1e-8)
    assert o.lr == 0.01 and o.momentum == 0.9   # the reference's defaults stay


def test_unknown_optimizer_is_rejected():
    with pytest.raises(ValueError):
        Options(optimizer="rmsprop")
    with pytest.raises(ValueError):
        parse_options(["--optimizer=sgd"])


def _tf_adam_host(lr0, beta1, beta2, steps, step0):
    """AdamOptimizer with lr = exponential_decay(lr0, global_step, 1000, 0.95, staircase=True): per step the float32 alpha of
    ApplyAdam (from the powers before the step) and the powers after AdamOptimizer._finish"""
    f = np.float32
    b1p, b2p = f(beta1), f(beta2)   # the accumulators' initial values
    out = []
    for t in range(steps):
        gs = step0 + t
        lr_t = f(lr0) * f(0.95) ** f(gs // 1000)
        alpha = lr_t * np.sqrt(f(1) - b2p) / (f(1) - b1p)
        b1p, b2p = b1p * f(beta1), b2p * f(beta2)
        out.append((lr_t, alpha, b1p, b2p))
    return out


@pytest.mark.parametrize("beta1,beta2", [(0.9, 0.999), (0.8, 0.99)])
def test_adam_host_scalars_match_tensorflow(beta1, beta2):
    """the bookkeeping apply_adam does (learning_rate -> adam_scalars -> powers), over several steps across the staircase at 1000"""
    from road_segmentation_unet_amd.unet import UNet

    class Host:   # the parts of UNet the host arithmetic uses, no device
        learning_rate = UNet.learning_rate
    h = Host()
    h.global_step = 997
    b1p, b2p = np.float32(beta1), np.float32(beta2)
    ref = _tf_adam_host(0.003, beta1, beta2, 6, 997)
    for lr_t, alpha, rb1, rb2 in ref:
        assert np.float32(h.learning_rate(0.003)) == lr_t
        a, b1p, b2p = adam_scalars(h.learning_rate(0.003), b1p, b2p, beta1, beta2)
        for got in (a, b1p, b2p):
            assert isinstance(got, np.float32)
        assert (a, b1p, b2p) == (alpha, rb1, rb2)
        h.global_step += 1
    # the decay engaged on the way: steps 997..999 at lr0, 1000.. at 0.95 lr0
    assert ref[0][0] == np.float32(0.003) and ref[-1][0] == np.float32(0.003) * np.float32(0.95)
    # and the first step's alpha is lr * sqrt(1 - b2) / (1 - b1) (float32 1 - 0.999 is good to ~1e-5 relative)
    a1 = adam_scalars(0.001, 0.9, 0.999, 0.9, 0.999)[0]
    assert abs(float(a1) / (0.001 * np.sqrt(0.001) / 0.1) - 1) < 1e-4
