"""No GPU: the third public header include/rsu_loss.h (the focal cross-entropy heads). The library exports what the header declares and
_lib.SIGNATURES_LOSS binds exactly that, disjoint from the other two tables, while rsu.h and SIGNATURES stay in sync;
tests/test_gpu_loss_fenced.py leaves no launching entry of the header out (the rule of tests/test_fence_host.py); the flag, its parser
and the UNet property; model.focal_loss_terms against torch float64; and the header's gradient rule, restated in numpy float32
(tests/focal_util.rule_f32), against float64 autograd at the tolerances the GPU tests grant the kernels -- on test_head's inputs and on
logits scaled until p_o and p_t underflow to exactly 0 in float32."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import unet_oracle as U
from road_segmentation_unet_amd import _lib
from road_segmentation_unet_amd import model as M
from road_segmentation_unet_amd.cli import parse_options
from road_segmentation_unet_amd.unet import UNet
from tests import focal_util as FU
from tests import hiputil as hu
from tests.head_util import NPIX, _inputs, _weight_map, _with_ignored

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ENTRIES = ["rsu_head_eval_focal", "rsu_head_fwd_bwd_focal"]


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)


def _symbols(name):
    return sorted(set(re.findall(r"\b(rsu_[a-zA-Z0-9_]+)\s*\(", _header(name))))


# ------------------------------------------------------------------------------------------- ABI
def test_library_exports_the_third_header_and_the_table_binds_it():
    L = _lib.lib()
    syms = _symbols("rsu_loss.h")
    assert syms == ENTRIES
    for s in syms:
        assert hasattr(L, s), "librsu_hip.so does not export %s" % s
        assert getattr(L, s).argtypes == _lib.SIGNATURES_LOSS[s][1] and getattr(L, s).restype is _lib.SIGNATURES_LOSS[s][0]
    assert sorted(_lib.SIGNATURES_LOSS) == syms, "ctypes table and rsu_loss.h out of sync"
    assert sorted(_lib.SIGNATURES) == _symbols("rsu.h"), "ctypes table and rsu.h out of sync"
    assert sorted(_lib.SIGNATURES_OPTIM) == _symbols("rsu_optim.h"), "ctypes table and rsu_optim.h out of sync"
    tables = [set(_lib.SIGNATURES), set(_lib.SIGNATURES_OPTIM), set(_lib.SIGNATURES_LOSS)]
    assert not (tables[0] & tables[1]) and not (tables[0] & tables[2]) and not (tables[1] & tables[2])
    text = _header("rsu_loss.h")
    assert '#include "rsu.h"' in text
    # the argument lists of the header and of the table: the same lengths, floats (by value) and longs / ints in the same positions
    protos = re.findall(r"^(int) (rsu_\w+)\(([^;]*?)\);", text, flags=re.M | re.S)
    assert sorted(n for _, n, _ in protos) == ENTRIES
    for _ret, name, args in protos:
        kinds = []
        for a in args.split(","):
            a = " ".join(a.split())
            kinds.append("f" if re.fullmatch(r"float \w+", a) else "l" if re.fullmatch(r"long \w+", a) else "i" if re.fullmatch(r"int \w+", a) else "p")
            assert kinds[-1] != "p" or "*" in a or a.startswith("rsu_stream_t "), (name, a)
        table = ["f" if t is _lib._f else "l" if t is _lib._l else "i" if t is _lib._i else "p" for t in _lib.SIGNATURES_LOSS[name][1]]
        assert kinds == table, (name, kinds, table)
    assert [i for i, t in enumerate(_lib.SIGNATURES_LOSS["rsu_head_fwd_bwd_focal"][1]) if t is _lib._f] == [6, 8, 9, 19]
    assert [i for i, t in enumerate(_lib.SIGNATURES_LOSS["rsu_head_eval_focal"][1]) if t is _lib._f] == [6]


def test_the_fenced_file_covers_every_launching_entry_of_the_third_header():
    """tests/test_fence_host.py's rule for rsu.h, for rsu_loss.h and tests/test_gpu_loss_fenced.py"""
    from tests import test_gpu_loss_fenced as G
    protos = re.findall(r"^(int|size_t) (rsu_\w+)\(([^;]*?)\);", _header("rsu_loss.h"), flags=re.M | re.S)
    launching = [n for r, n, a in protos if r == "int" and "rsu_stream_t" in a]
    assert sorted(launching) == ENTRIES and not [n for r, n, a in protos if r == "size_t"]   # (no new size functions)
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
    # and the launching entries of the other two headers did not grow: the new ones live in the third
    assert not [n for n in _symbols("rsu.h") + _symbols("rsu_optim.h") if "focal" in n]


# ------------------------------------------------------------------------------------------- flag, parser, property
def test_parse_focal_gamma_and_the_flag():
    assert M.parse_focal_gamma(0) == 0.0 and M.parse_focal_gamma("2") == 2.0 and M.parse_focal_gamma(0.5) == 0.5
    assert isinstance(M.parse_focal_gamma(np.float32(2)), float)
    for bad in (-1e-3, -1, float("nan"), float("inf"), -float("inf"), "x", "", None, True, (1, 2)):
        with pytest.raises(ValueError):
            M.parse_focal_gamma(bad)
    for o in (M.Options(), parse_options([])):
        assert o.focal_gamma == 0.0 and isinstance(o.focal_gamma, float)
    assert parse_options(["--focal_gamma=2"]).focal_gamma == 2.0 and parse_options(["--focal_gamma", "0.5"]).focal_gamma == 0.5
    assert M.Options(focal_gamma="1.5").focal_gamma == 1.5
    for bad in ("--focal_gamma=-1", "--focal_gamma=nan", "--focal_gamma=inf"):
        with pytest.raises(ValueError):
            parse_options([bad])
    with pytest.raises(SystemExit):
        parse_options(["--focal_gamma=two"])
    d = {d[0]: d for d in M.EXTRA_FLAG_DEFS}["focal_gamma"]
    assert d[1:3] == (float, 0.0)
    text = " ".join(d[3].split())
    for needle in ("0 = off", "logged loss", "validation loss / objective", "focal objective", "gradient shrinks", "--lr needs retuning",
                   "multiplies --class_weights, --border_weight and the weight map", "--dice_weight adds to it unchanged"):
        assert needle in text, needle


def test_unet_property_rejects_without_a_device():
    class Host:   # UNet.focal_gamma on the one attribute it keeps
        focal_gamma = UNet.focal_gamma
    h = Host()
    h.focal_gamma = 2
    assert h.focal_gamma == 2.0 and isinstance(h.focal_gamma, float)
    h.focal_gamma = "0.5"
    assert h.focal_gamma == 0.5
    h.focal_gamma = 0.0
    assert h.focal_gamma == 0.0
    for bad in (-0.5, float("nan"), float("inf"), "x", None, (1,)):
        with pytest.raises(_lib.RsuError):
            h.focal_gamma = bad
        assert h.focal_gamma == 0.0
    assert "focal_gamma" in inspect.signature(UNet.__init__).parameters
    assert inspect.signature(UNet.__init__).parameters["focal_gamma"].default == 0.0


# ------------------------------------------------------------------------------------------- focal_loss_terms
def _torch_terms(p1, labels, gamma, cw, pw):
    p1, lab = torch.tensor(np.asarray(p1, np.float64)).reshape(-1), torch.tensor(np.asarray(labels).reshape(-1))
    valid = (lab == 0) | (lab == 1)
    p1, y = p1[valid], lab[valid]
    pt = torch.where(y == 1, p1, 1 - p1)
    om = torch.ones_like(pt)
    if cw is not None:
        om = om * torch.tensor(cw, dtype=torch.float64)[y]
    if pw is not None:
        om = om * torch.tensor(np.asarray(pw, np.float64)).reshape(-1)[valid]
    return float((om * (1 - pt) ** gamma * -torch.log(pt)).sum()), float(om.sum())


@pytest.mark.parametrize("gamma", [0, 0.5, 2, 5])
@pytest.mark.parametrize("weighted", [False, True])
def test_focal_loss_terms_against_torch_float64(gamma, weighted):
    rng = np.random.RandomState(11)
    p1 = rng.rand(3, 37, 41).astype(f32) * 0.998 + 0.001
    labels = (rng.rand(3, 37, 41) < 0.2).astype(np.int64)
    cw, pw = (FU.CLASS_W, _weight_map(rng).reshape(3, 37, 41)) if weighted else (None, None)
    if weighted:
        labels, ign = _with_ignored(rng, labels.reshape(-1))
        labels, pw = labels.reshape(3, 37, 41), pw.copy()
        pw.reshape(-1)[np.nonzero(ign)[0][:3]] = [np.inf, np.nan, -1e30]     # ignored by selection
    got = M.focal_loss_terms(p1, labels, gamma, cw, pw)
    ref = _torch_terms(p1, labels, gamma, cw, pw)
    assert all(isinstance(v, float) and np.isfinite(v) for v in got)
    assert got[0] == pytest.approx(ref[0], rel=1e-12) and got[1] == pytest.approx(ref[1], rel=1e-12)
    if gamma == 0:   # the weighted cross-entropy
        valid = (labels == 0) | (labels == 1)
        pt = np.where(labels == 1, p1.astype(np.float64), 1.0 - p1.astype(np.float64))[valid]
        om = np.ones(pt.size) if cw is None else np.asarray(cw)[labels[valid]] * pw.astype(np.float64)[valid]
        assert got[0] == pytest.approx(float((om * -np.log(pt)).sum()), rel=1e-12)
    else:
        assert got[0] < M.focal_loss_terms(p1, labels, 0, cw, pw)[0]
    # corners: p_t == 1 adds exactly nothing, shapes must agree, gamma is parsed
    assert M.focal_loss_terms([1.0, 0.0], [1, 0], gamma or 2) == (0.0, 2.0)
    with pytest.raises(ValueError):
        M.focal_loss_terms(p1, labels.reshape(-1)[:-1], gamma)
    with pytest.raises(ValueError):
        M.focal_loss_terms(p1, labels, -1.0)


# ------------------------------------------------------------------------------------------- the rule, float32 against float64 autograd
def _restated_head(act, w, b, labels, class_w, pixel_w, inv, gamma):
    """the head with the header's rule in float32: the checker's logits, rule_f32, the checker's 1x1 backward, bf16 dact"""
    logits = U.conv1x1_fwd(act, w, b).astype(f32)
    p1, terms, dl = FU.rule_f32(logits, labels, gamma, FU.omega_of(labels, class_w, pixel_w), inv)
    rdx, rdw, rdb = U.conv1x1_bwd(act, w, dl)
    return p1, float(terms.astype(np.float64).sum()), logits, dl, hu.q(U.relu_bwd(act, rdx)), rdw, rdb


@pytest.mark.parametrize("C", [64, 16])
@pytest.mark.parametrize("gamma", FU.GAMMAS)
def test_rule_in_float32_against_float64_autograd(C, gamma):
    rng, act, w, b, labels = _inputs(C)
    pixel_w = _weight_map(rng)
    labels, ign = _with_ignored(rng, labels)
    inv = 1.0 / (2 * NPIX)
    ref = FU.Ref(act, w, b, labels, FU.CLASS_W, np.where(ign, 1.0, pixel_w), inv, gamma)
    p1, loss, _, dl, dact, dw, db = _restated_head(act, w, b, labels, FU.CLASS_W, pixel_w, inv, gamma)
    what = "restated rule C=%d gamma=%g" % (C, gamma)
    assert np.isfinite(dl).all() and np.isfinite(loss)
    hu.assert_f32_close(p1, ref.prob, what + " prob", rtol=1e-4, atol_scale=1e-6)
    assert abs(loss - ref.loss_sum) <= 2e-5 * abs(ref.loss_sum), (what, loss, ref.loss_sum)
    hu.assert_bf16_close(dact, ref.dact, what + " dact")
    hu.assert_f32_close(dw, ref.dw, what + " dw")
    hu.assert_f32_close(db, ref.db, what + " db")
    assert not dact[ign].any() and not np.signbit(dact[ign]).any()
    if gamma == 2.0:
        # what tests/test_gpu_focal.py asks of the kernel's rounding, asked of the restatement first: the helper's mismatch and
        # mean-signed-error bounds hold on the unscaled inputs
        mismatch, bias, n = hu.assert_bf16_rounded(dact, ref.dact, what + " dact")
        print("%s: mismatch %.2e bias %+.4f ulp over %d elements" % (what, mismatch, bias, n))


@pytest.mark.parametrize("C", [64, 16])
def test_rule_with_gamma_zero_is_the_cross_entropy_gradient(C):
    """(no pixel of these inputs has p_o == 0) against the reference of the weighted head, tests/head_util.Ref without its Dice term"""
    from tests.head_util import Ref as CERef
    rng, act, w, b, labels = _inputs(C)
    pixel_w = _weight_map(rng)
    inv = 1.0 / (2 * NPIX)
    ref = CERef(act, w, b, labels, FU.CLASS_W, pixel_w, inv, lam=0.0)
    _, loss, _, dl, dact, dw, db = _restated_head(act, w, b, labels, FU.CLASS_W, pixel_w, inv, 0.0)
    assert np.isfinite(dl).all() and abs(loss - ref.ce_sum) <= 2e-5 * abs(ref.ce_sum)
    hu.assert_bf16_close(dact, ref.dact, "gamma 0 dact")
    hu.assert_f32_close(dw, ref.dw, "gamma 0 dw")
    hu.assert_f32_close(db, ref.db, "gamma 0 db")
    focal = FU.Ref(act, w, b, labels, FU.CLASS_W, pixel_w, inv, 0.0)
    np.testing.assert_allclose(focal.dw, ref.dw, rtol=1e-12, atol=1e-18)
    assert focal.loss_sum == pytest.approx(ref.ce_sum, rel=1e-12)


@pytest.mark.parametrize("C", [64, 16])
@pytest.mark.parametrize("gamma", FU.GAMMAS)
def test_rule_in_float32_on_saturated_logits(C, gamma):
    """logits scaled until hundreds of pixels have p_o == 0 and hundreds p_t == 0 in float32: no NaN, no inf, the same tolerances"""
    rng, act, w, b, labels = _inputs(C)
    w = (w * f32(FU.SATURATE)).astype(f32)
    pixel_w = _weight_map(rng)
    inv = 1.0 / (2 * NPIX)
    ref = FU.Ref(act, w, b, labels, FU.CLASS_W, pixel_w, inv, gamma)
    p1, loss, logits, dl, dact, dw, db = _restated_head(act, w, b, labels, FU.CLASS_W, pixel_w, inv, gamma)
    po = np.where(labels == 1, 1 - p1, p1)
    p0 = np.exp(logits[:, 0] - logits.max(1)) / (np.exp(logits[:, 0] - logits.max(1)) + np.exp(logits[:, 1] - logits.max(1)))
    pt_zero = int(((np.where(labels == 1, p1, p0)) == 0).sum())
    po_zero = int(((np.where(labels == 1, p0, p1)) == 0).sum())
    print("C=%d: %d pixels with p_o == 0, %d with p_t == 0" % (C, po_zero, pt_zero))
    assert po_zero > 100 and pt_zero > 100 and po.size == NPIX
    what = "saturated rule C=%d gamma=%g" % (C, gamma)
    for name, a in (("dlogits", dl), ("dact", dact), ("dw", dw), ("db", db), ("prob", p1)):
        assert np.isfinite(a).all(), (what, name)
    assert np.isfinite(loss) and abs(loss - ref.loss_sum) <= 2e-5 * abs(ref.loss_sum), (what, loss, ref.loss_sum)
    hu.assert_f32_close(p1, ref.prob, what + " prob", rtol=1e-4, atol_scale=1e-6)
    hu.assert_bf16_close(dact, ref.dact, what + " dact")
    hu.assert_f32_close(dw, ref.dw, what + " dw")
    hu.assert_f32_close(db, ref.db, what + " db")
    # the trap the host dispatch exists for: gamma == 0 in these expressions IS NaN where p_o == 0
    _, _, d0 = FU.rule_f32(logits, labels, 0.0, FU.omega_of(labels, FU.CLASS_W, pixel_w), inv)
    assert np.isnan(d0).any()
