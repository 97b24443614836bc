"""No GPU: the second public header include/rsu_optim.h (weight decay inside the update pass) and the learning-rate schedules. The
library exports what the header declares and _lib.SIGNATURES_OPTIM binds exactly that, while rsu.h and SIGNATURES stay in sync with each
other; tests/test_gpu_optim_fenced.py leaves no launching entry of the header out (the rule of tests/test_fence_host.py); unet.lr_at
against its definitions; the flag parsers; and tests/decay_util.py, the float32 restatement the GPU tests compare with, against float64
formulas."""
import inspect
import math
import os
import re

import numpy as np
import pytest

from road_segmentation_unet_amd import _lib
from road_segmentation_unet_amd import model as M
from road_segmentation_unet_amd.cli import parse_options
from road_segmentation_unet_amd.unet import DECAY_MODES, LR_SCHEDULES, UNet, lr_at
from tests import decay_util as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)


def _symbols(name):
    return sorted(set(re.findall(r"\b(rsu_[a-zA-Z0-9_]+)\s*\(", _header(name))))


# ------------------------------------------------------------------------------------------- ABI
def test_library_exports_the_second_header_and_the_table_binds_it():
    L = _lib.lib()
    syms = _symbols("rsu_optim.h")
    assert syms == ["rsu_update_table_run_adam_decay", "rsu_update_table_run_decay"]
    for s in syms:
        assert hasattr(L, s), "librsu_hip.so does not export %s" % s
        assert getattr(L, s).argtypes == _lib.SIGNATURES_OPTIM[s][1] and getattr(L, s).restype is _lib.SIGNATURES_OPTIM[s][0]
    assert sorted(_lib.SIGNATURES_OPTIM) == syms, "ctypes table and rsu_optim.h out of sync"
    assert sorted(_lib.SIGNATURES) == _symbols("rsu.h"), "ctypes table and rsu.h out of sync"
    assert not set(_lib.SIGNATURES) & set(_lib.SIGNATURES_OPTIM)
    text = _header("rsu_optim.h")
    assert '#include "rsu.h"' in text
    defs = dict(re.findall(r"^#define (RSU_DECAY_\w+) (\d+)", text, flags=re.M))
    assert (int(defs["RSU_DECAY_L2"]), int(defs["RSU_DECAY_DECOUPLED"])) == (_lib.DECAY_L2, _lib.DECAY_DECOUPLED) == (D.L2, D.DECOUPLED)
    # the argument lists of the header and of the table have the same lengths and the same float positions
    for ret, name, args in re.findall(r"^(int) (rsu_\w+)\(([^;]*?)\);", text, flags=re.M | re.S):
        kinds = ["f" if a.strip().startswith("float") else "x" for a in args.split(",")]
        table = ["f" if t is _lib._f else "x" for t in _lib.SIGNATURES_OPTIM[name][1]]
        assert kinds == table, (name, kinds, table)


def test_the_fenced_file_covers_every_launching_entry_of_the_second_header():
    """tests/test_fence_host.py's rule for rsu.h, for rsu_optim.h and tests/test_gpu_optim_fenced.py"""
    from tests import test_gpu_optim_fenced as G
    protos = re.findall(r"^(int|size_t) (rsu_\w+)\(([^;]*?)\);", _header("rsu_optim.h"), flags=re.M | re.S)
    launching = [n for r, n, a in protos if r == "int" and "rsu_stream_t" in a]
    assert len(launching) == 2 and not [n for r, n, a in protos if r == "size_t"]
    tests = {n: f for n, f in vars(G).items() if n.startswith("test_") and callable(f)}
    for entry in launching:
        assert (entry in G.FENCED) != (entry in G.NOT_FENCED), "%s: in exactly one of FENCED and NOT_FENCED" % entry
    assert set(G.FENCED) | set(G.NOT_FENCED) <= set(launching)
    for entry, names in G.FENCED.items():
        assert names, entry
        for n in names:
            assert n in tests, (entry, n)
            assert re.search(r'"%s"' % entry, inspect.getsource(tests[n]) + "".join(inspect.getsource(h) for h in G.HELPERS.get(n, ()))), \
                "%s is not launched by %s" % (entry, n)
    for entry, reason in G.NOT_FENCED.items():
        assert "writes no device memory" in reason, (entry, reason)
    assert "pytest.mark.gpu" in inspect.getsource(G)
    # and the launching entries of rsu.h did not grow: the new ones live in the second header
    assert not [n for n in _symbols("rsu.h") if "decay" in n]


# ------------------------------------------------------------------------------------------- lr_at
@pytest.mark.parametrize("lr0", [0.01, 0.003, 1e-4])
def test_lr_at_defaults_have_the_bits_of_the_reference_expression(lr0):
    for t in (0, 999, 1000, 25000):
        ref = f32(lr0) * f32(0.95) ** f32(t // 1000)
        got = lr_at(t, lr0)
        assert isinstance(got, float) and f32(got).tobytes() == f32(ref).tobytes() and got == float(ref), (t, got, ref)
        assert lr_at(t, lr0, "staircase", 0, 0, 0.0) == got and lr_at(t, lr0, total_steps=77, final=0.5) == got   # (T and F are not read)

    class Host:   # UNet.learning_rate on the parts it reads
        learning_rate = UNet.learning_rate
        global_step = 25000
    assert Host().learning_rate(lr0) == lr_at(25000, lr0)
    h = Host()
    h.lr_schedule = ("cosine", 0, 50000, 0.0)
    assert h.learning_rate(lr0) == lr_at(25000, lr0, "cosine", 0, 50000, 0.0) == float(f32(lr0 * 0.5 * (1.0 + math.cos(math.pi / 2))))


def test_lr_at_warmup():
    lr0 = 0.01
    assert lr_at(0, lr0, "constant", warmup_steps=10) == float(f32(lr0 / 10))
    assert lr_at(4, lr0, "constant", warmup_steps=10) == float(f32(lr0 * 0.5))
    assert lr_at(9, lr0, "constant", warmup_steps=10) == float(f32(lr0)) == lr_at(10 ** 6, lr0, "constant", warmup_steps=10)
    # on top of the staircase: the float32 base times the ramp, rounded once
    base = float(f32(lr0) * f32(0.95) ** f32(0))
    assert lr_at(0, lr0, warmup_steps=10) == float(f32(base * 0.1)) and lr_at(9, lr0, warmup_steps=10) == base
    assert lr_at(1003, lr0, warmup_steps=2000) == float(f32(float(f32(lr0) * f32(0.95) ** f32(1)) * (1004 / 2000)))
    assert lr_at(0, lr0, "constant", warmup_steps=1) == float(f32(lr0))
    rates = [lr_at(t, lr0, "constant", warmup_steps=10) for t in range(12)]
    assert all(b > a for a, b in zip(rates[:9], rates[1:10])) and rates[9] == rates[10] == rates[11]


@pytest.mark.parametrize("schedule", ["cosine", "linear"])
def test_lr_at_cosine_and_linear(schedule):
    lr0, T, Fi = 0.01, 100, 0.1
    at = lambda t, W=0: lr_at(t, lr0, schedule, W, T, Fi)  # noqa: E731
    assert at(0) == float(f32(lr0))
    assert at(50) == pytest.approx(lr0 * 0.55, rel=2e-7)
    for t in (100, 101, 5000):
        assert at(t) == float(f32(lr0 * 0.1)) or at(t) == pytest.approx(lr0 * 0.1, rel=2e-7)
        assert at(t) == at(100)
    if schedule == "linear":
        assert at(25) == pytest.approx(lr0 * (0.1 + 0.9 * 0.75), rel=2e-7)
    else:
        assert at(25) == pytest.approx(lr0 * (0.1 + 0.9 * 0.5 * (1 + math.sqrt(0.5))), rel=2e-7)
    rates = [at(t) for t in range(130)]
    assert all(b <= a for a, b in zip(rates, rates[1:])) and rates[0] > rates[99] > rates[100]
    # with warm-up: the ramp up to step W - 1, never increasing after it
    W = 10
    warm = [at(t, W) for t in range(130)]
    assert warm[0] == pytest.approx(rates[0] / W, rel=2e-7) and all(b > a for a, b in zip(warm[:W - 1], warm[1:W]))
    assert warm[W - 1:] == rates[W - 1:] and all(b <= a for a, b in zip(warm[W - 1:], warm[W:]))
    # final = 0 and final = 1
    assert lr_at(100, lr0, schedule, 0, T, 0.0) == 0.0 and lr_at(63, lr0, schedule, 0, T, 1.0) == float(f32(lr0))
    assert lr_at(0, lr0, schedule, 0, 1, 0.0) == float(f32(lr0)) and lr_at(1, lr0, schedule, 0, 1, 0.0) == 0.0


@pytest.mark.parametrize("kw", [dict(step=-1), dict(step=1.5), dict(step=True), dict(step=None), dict(lr0=float("nan")), dict(lr0=float("inf")),
                                dict(lr0=-0.01), dict(lr0="x"), dict(lr0=None), dict(schedule="exponential"), dict(schedule=None),
                                dict(warmup_steps=-1), dict(warmup_steps=2.0), dict(warmup_steps=None), dict(total_steps=-5),
                                dict(total_steps=1.5), dict(schedule="cosine"), dict(schedule="linear", total_steps=0),
                                dict(schedule="cosine", total_steps=10, final=1.5), dict(final=-0.1), dict(final=float("nan")),
                                dict(final="x"), dict(final=True)], ids=str)
def test_lr_at_bad_arguments_raise(kw):
    args = dict(step=3, lr0=0.01, schedule="staircase", warmup_steps=0, total_steps=0, final=0.0)
    args.update(kw)
    with pytest.raises(ValueError):
        lr_at(**args)


# ------------------------------------------------------------------------------------------- flags
def test_flag_parsers():
    assert M.parse_weight_decay(0) == 0.0 and M.parse_weight_decay("1e-4") == 1e-4 and M.parse_weight_decay(0.5) == 0.5
    for bad in (-1e-4, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError):
            M.parse_weight_decay(bad)
    assert [M.parse_weight_decay_mode(m) for m in DECAY_MODES] == ["decoupled", "l2"]
    for bad in ("L2", "adamw", "", None, 1):
        with pytest.raises(ValueError):
            M.parse_weight_decay_mode(bad)
    assert [M.parse_lr_schedule(s) for s in LR_SCHEDULES] == ["staircase", "constant", "cosine", "linear"]
    for bad in ("step", "", None, 0):
        with pytest.raises(ValueError):
            M.parse_lr_schedule(bad)
    assert M.parse_lr_steps(0, "lr_warmup_steps") == 0 and M.parse_lr_steps(np.int64(7), "lr_total_steps") == 7
    for bad in (-1, 1.0, "3", None, True):
        with pytest.raises(ValueError):
            M.parse_lr_steps(bad, "lr_total_steps")
    assert M.parse_lr_final(0) == 0.0 and M.parse_lr_final("0.25") == 0.25 and M.parse_lr_final(1) == 1.0
    for bad in (-0.01, 1.01, float("nan"), "x", None, False):
        with pytest.raises(ValueError):
            M.parse_lr_final(bad)


def test_options_and_command_line():
    for o in (M.Options(), parse_options([])):
        assert (o.weight_decay, o.weight_decay_mode, o.lr_schedule, o.lr_warmup_steps, o.lr_total_steps, o.lr_final) == \
            (0.0, "decoupled", "staircase", 0, 0, 0.0)
    p = parse_options(["--weight_decay=1e-4", "--weight_decay_mode=l2", "--lr_schedule=cosine", "--lr_warmup_steps=2", "--lr_total_steps=500",
                       "--lr_final=0.05"])
    assert (p.weight_decay, p.weight_decay_mode, p.lr_schedule, p.lr_warmup_steps, p.lr_total_steps, p.lr_final) == (1e-4, "l2", "cosine", 2, 500, 0.05)
    assert parse_options(["--lr_schedule=linear"]).lr_total_steps == 0      # (0 with cosine | linear: cli.main resolves it to the run's length)
    for bad in ("--weight_decay=-1", "--weight_decay=nan", "--weight_decay=inf", "--weight_decay_mode=adamw", "--lr_schedule=poly",
                "--lr_warmup_steps=-1", "--lr_total_steps=-1", "--lr_final=1.5", "--lr_final=-0.5", "--lr_final=nan"):
        with pytest.raises(ValueError):
            parse_options([bad])
    defs = {d[0]: d for d in M.EXTRA_FLAG_DEFS}
    assert defs["weight_decay"][1:3] == (float, 0.0) and "0 = off" in defs["weight_decay"][3] and "never includes" in defs["weight_decay"][3]
    assert defs["weight_decay_mode"][1:3] == (str, "decoupled") and defs["lr_schedule"][1:3] == (str, "staircase")
    assert defs["lr_warmup_steps"][1:3] == (int, 0) and defs["lr_total_steps"][1:3] == (int, 0) and defs["lr_final"][1:3] == (float, 0.0)


def test_steps_per_epoch_is_the_length_of_the_training_loop():
    for n, b in ((100, 16), (96, 16), (16, 16), (15, 16), (17, 16), (1000, 1)):
        assert M.steps_per_epoch(n, b) == len(list(range(0, n - b, b)))
    assert M.steps_per_epoch(96, 16) == 5 and M.steps_per_epoch(16, 16) == 0     # (the final batch is dropped even when full)


# ------------------------------------------------------------------------------------------- the restatement
def _data(seed=3, n=4099):
    rng = np.random.RandomState(seed)
    w = (rng.standard_normal(n) * 0.2).astype(f32)
    a = (rng.standard_normal(n) * 1e-2).astype(f32)
    g = (rng.standard_normal(n) * 1e-2).astype(f32)
    v = (rng.rand(n) * 1e-4 + 1e-6).astype(f32)
    return w, a, g, v


@pytest.mark.parametrize("mode", [D.L2, D.DECOUPLED], ids=["l2", "decoupled"])
def test_restatement_momentum_against_float64(mode):
    w, a, g, _ = _data()
    lr, mu, gs = 0.01, 0.9, float(f32(0.5) * f32(0.37))
    decay = 0.1 if mode == D.L2 else float(f32(lr) * f32(0.1))
    w1, a1 = D.momentum_decay(w, a, g, lr, mu, gs, decay, mode)
    assert w1.dtype == np.float32 and a1.dtype == np.float32
    rw, ra = D.momentum_decay_f64(w, a, g, lr, mu, gs, decay, mode)
    # a handful of float32 roundings per result: 4 ulp of the largest term, far below the 1e-3 |w| the decay moves
    np.testing.assert_allclose(a1, ra, rtol=4e-7, atol=4e-7 * float(np.abs(ra).max()))
    np.testing.assert_allclose(w1, rw, rtol=4e-7, atol=1e-9)
    # the decay is there: against the plain rule the weights differ by about lr * lambda * |w|
    pw, pa = D.momentum_decay(w, a, g, lr, mu, gs, decay, mode, decays=False)
    np.testing.assert_array_equal(pw, D.momentum(w, a, g, lr, mu, gs)[0])
    np.testing.assert_allclose(pw.astype(np.float64) - w1, 1e-3 * w.astype(np.float64), rtol=1e-3, atol=2e-8)
    assert (pa == a1).all() if mode == D.DECOUPLED else not (pa == a1).all()


@pytest.mark.parametrize("mode", [D.L2, D.DECOUPLED], ids=["l2", "decoupled"])
def test_restatement_adam_against_float64(mode):
    w, m, g, v = _data(5)
    alpha, b1, b2, eps, gs = 1.234e-3, 0.9, 0.999, 1e-8, 0.5
    decay = 0.1 if mode == D.L2 else float(f32(0.01) * f32(0.1))
    w1, m1, v1 = D.adam_decay(w, m, v, g, alpha, b1, b2, eps, gs, decay, mode)
    assert w1.dtype == np.float32 and m1.dtype == np.float32 and v1.dtype == np.float32
    rw, rm, rv = D.adam_decay_f64(w, m, v, g, alpha, b1, b2, eps, gs, decay, mode)
    np.testing.assert_allclose(m1, rm, rtol=1e-6, atol=1e-6 * float(np.abs(rm).max()))
    np.testing.assert_allclose(v1, rv, rtol=1e-6, atol=0)
    np.testing.assert_allclose(w1, rw, rtol=1e-6, atol=1e-6 * alpha * 30)     # (|m / sqrt(v)| stays below 30 for this data)
    pw, pm, pv = D.adam_decay(w, m, v, g, alpha, b1, b2, eps, gs, decay, mode, decays=False)
    for got, ref in zip((pw, pm, pv), D.adam(w, m, v, g, alpha, b1, b2, eps, gs)):
        np.testing.assert_array_equal(got, ref)
    assert float(np.abs(pw.astype(np.float64) - w1).mean()) > 1e-4 * float(np.abs(w).mean())
    if mode == D.DECOUPLED:   # the slots see the data gradient only
        np.testing.assert_array_equal(pm, m1)
        np.testing.assert_array_equal(pv, v1)


def test_restatement_l2_is_the_plain_rule_on_the_transformed_gradient():
    """what tests/test_gpu_optim_fenced.py asks of the kernel, asked of the restatement first"""
    w, a, g, v = _data(7)
    gs = float(f32(0.5) * f32(0.61))
    g1 = D.l2_gradient(w, g, gs, 0.1)
    np.testing.assert_array_equal(g1, (f32(gs) * g) + (f32(0.1) * w))
    for got, ref in zip(D.adam_decay(w, a, v, g, 1e-3, 0.9, 0.999, 1e-8, gs, 0.1, D.L2), D.adam(w, a, v, g1, 1e-3, 0.9, 0.999, 1e-8, 1.0)):
        np.testing.assert_array_equal(got, ref)
    for got, ref in zip(D.momentum_decay(w, a, g, 0.01, 0.9, gs, 0.1, D.L2), D.momentum(w, a, g1, 0.01, 0.9, 1.0)):
        np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(D.decayed_weights(w, 1e-3), w - f32(1e-3) * w)
