"""-m gpu: a dropped network gives its device memory back AT ONCE, by reference counting, not at Python's next full collection. A long-running
process (a sweep over configurations, the test suite) drops many networks and keeps many objects alive; CPython then runs full collections
rarely, and a network kept alive by a reference cycle would hold its activations, gradients and workspaces -- gigabytes at full size --
until one happens. With the collector switched off: a UNet that has run a training step and an evaluation pass, a forward-only one, and a
ConvolutionalModel after train_step() and evaluate() (with the centre-line flags, which add buffers) are gone when the last name is."""
import gc
import weakref

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from road_segmentation_unet_amd.unet import UNet, input_size_needed  # noqa: E402

L, ROOT, P, B = 3, 16, 20, 2      # the small config of the other model tests


@pytest.fixture
def no_collector():
    gc.collect()
    torch.cuda.synchronize()
    gc.disable()
    yield
    gc.enable()


def _inputs(n=B):
    rng = np.random.RandomState(3)
    S = input_size_needed(P, L)
    return rng.rand(n, S, S, 3).astype(np.float32), (rng.rand(n, P, P) < 0.3).astype(np.int64)


def _gone(ref, base, what):
    torch.cuda.synchronize()
    assert ref() is None, "%s is kept alive by a reference cycle: %s" % (what, [type(x).__name__ for x in gc.get_referrers(ref())])
    assert torch.cuda.memory_allocated() == base, (what, torch.cuda.memory_allocated() - base)


@pytest.mark.parametrize("training", [True, False], ids=["training", "forward-only"])
def test_a_dropped_unet_frees_its_buffers_without_a_collection(no_collector, training):
    base = torch.cuda.memory_allocated()
    X, y = _inputs()
    net = UNet(L, ROOT, True, B, P, device="cuda:0", params=U.init_params(L, ROOT, True, seed=13, bias_scale=0.05), training=training)
    net.x.copy_(torch.from_numpy(X))
    if training:
        net.labels.copy_(torch.from_numpy(y))
        net.forward_device()
        net.backward_device(1.0 / (B * P * P))
        net.apply_momentum(0.01, 0.9)
        net.forward_device(keep=1.0)
        net.evaluate_device()
    else:   # a forward-only net, as predict() builds them
        net.forward_device()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() > base
    ref = weakref.ref(net)
    del net
    _gone(ref, base, "UNet(training=%s)" % training)


def test_a_dropped_model_frees_its_buffers_without_a_collection(no_collector):
    from road_segmentation_unet_amd.model import ConvolutionalModel, Options
    base = torch.cuda.memory_allocated()
    X, y = _inputs(3)
    m = ConvolutionalModel(Options(num_layers=L, root_size=ROOT, patch_size=P, batch_size=B, dilated_layers=True, dropout=1.0, lr=0.01, seed=5,
                                   logdir=None, validate_centerlines=True, centerline_min_branch=2, validate_junctions=True),
                           device="cuda:0", params=U.init_params(L, ROOT, True, seed=13, bias_scale=0.05))
    m.train_step(X[:B], y[:B])
    out = m.evaluate(X, y)
    assert "jn_f1" in out and "graph" in m._mask_metrics.ws and torch.cuda.memory_allocated() > base
    del out
    ref, net = weakref.ref(m), weakref.ref(m.net)
    del m
    assert net() is None
    _gone(ref, base, "ConvolutionalModel")
