"""-m gpu: the launching entry points of include/rsu_loss.h inside a fenced arena (tests/fence_util.py), as tests/test_gpu_fenced.py
holds those of include/rsu.h: rsu_head_fwd_bwd_focal without and with the Dice term (behind rsu_head_dice_sums) and rsu_head_eval_focal
at npix = 3 * 37 * 41 (odd: no multiple of any block) for every C the heads admit, with ignored labels, class weights and a weight map,
each workspace exactly its size function's (rsu_head_dice_ws_floats / rsu_head_eval_ws_floats). After Arena.check: no NaN in any
result (an element never written, or a stray read of the bands, is one), and the results against the float64 reference.

FENCED is the registry tests/test_focal_host.py checks against include/rsu_loss.h without a GPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import fence_util as F  # noqa: E402
from tests import focal_util as FU  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests.head_util import LAM, NPIX, SMOOTH, _inputs, _weight_map, _with_ignored  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

HEAD_C = [8, 16, 32, 64, 128, 256, 512]      # every C the heads admit (rsu_api: 8 .. 512, C / 8 a power of two)
GAMMA = 2.0


def _host(t):
    return t.detach().to(torch.float32).cpu().numpy()


def _launch(A, C, inv, st):
    """the three launch sequences of the header, each with outputs and a workspace of its own"""
    p = lambda n: hu.ptr(A[n])  # noqa: E731
    head = (p("act"), p("w"), p("b"), p("labels"))
    call("rsu_head_fwd_bwd_focal", *head, p("cw"), p("pw"), GAMMA, None, 0.0, 0.0, p("prob_f"), p("loss_f"), p("wsum_f"), p("dact_f"), p("dw_f"),
         p("db_f"), p("ws_f"), NPIX, C, inv, st)
    call("rsu_head_dice_sums", *head, p("pw"), p("prob_s"), p("dsums"), p("ws_d"), NPIX, C, st)
    call("rsu_head_fwd_bwd_focal", *head, p("cw"), p("pw"), GAMMA, p("dsums"), LAM, SMOOTH, p("prob_d"), p("loss_d"), p("wsum_d"), p("dact_d"),
         p("dw_d"), p("db_d"), p("ws_d"), NPIX, C, inv, st)
    call("rsu_head_eval_focal", *head, p("cw"), p("pw"), GAMMA, p("prob_e"), p("esums"), p("hist"), p("ws_e"), NPIX, C, st)


@pytest.mark.parametrize("C", HEAD_C)
def test_focal_heads(C, placement="aligned"):
    assert NPIX == 3 * 37 * 41 and NPIX % 2 == 1
    rng, act, w, b, labels = _inputs(C)
    pixel_w = _weight_map(rng)
    labels, ign = _with_ignored(rng, labels)
    inv = 1.0 / (2 * NPIX)
    L = lib()
    z = lambda name, *s: F.state(name, np.zeros(s, np.float32))  # noqa: E731
    o32 = lambda name, *s: F.out(name, s, torch.float32)  # noqa: E731
    specs = [F.bf16("act", act), F.f32("w", w), F.f32("b", b), F.raw("labels", labels), F.f32("cw", np.asarray(FU.CLASS_W, np.float32)),
             F.f32("pw", pixel_w)]
    for k in ("f", "d"):
        specs += [o32("prob_" + k, NPIX), F.out("dact_" + k, (NPIX, C)), o32("dw_" + k, C, 2), o32("db_" + k, 2), z("loss_" + k, 1), z("wsum_" + k, 1)]
    specs += [o32("prob_s", NPIX), o32("dsums", 3), o32("prob_e", NPIX), z("esums", 5), F.state("hist", np.zeros((2, 256), np.int64)),
              F.ws("ws_f", L.rsu_head_dice_ws_floats(NPIX, C)), F.ws("ws_d", L.rsu_head_dice_ws_floats(NPIX, C)),
              F.ws("ws_e", L.rsu_head_eval_ws_floats(NPIX, C))]
    A = F.Arena(hu.DEV, specs, placement=placement)
    _launch(A, C, inv, hu.stream())
    what = "focal heads C=%d" % C
    A.check(what)
    for s in specs:
        if s.kind in ("out", "state"):
            assert not bool(torch.isnan(A[s.name].to(torch.float32)).any()), (what, s.name)
    safe_pw = np.where(~ign, pixel_w, 1.0)
    refs = {"f": FU.Ref(act, w, b, labels, FU.CLASS_W, safe_pw, inv, GAMMA), "d": FU.Ref(act, w, b, labels, FU.CLASS_W, safe_pw, inv, GAMMA, lam=LAM)}
    for k, r in refs.items():
        hu.assert_f32_close(_host(A["prob_" + k]), r.prob, what + " prob_" + k, rtol=1e-4, atol_scale=1e-6)
        hu.assert_bf16_close(_host(A["dact_" + k]), r.dact, what + " dact_" + k)
        hu.assert_f32_close(_host(A["dw_" + k]), r.dw, what + " dw_" + k)
        hu.assert_f32_close(_host(A["db_" + k]), r.db, what + " db_" + k)
        assert abs(float(_host(A["loss_" + k])[0]) - r.loss_sum) <= 2e-5 * abs(r.loss_sum), (k, r.loss_sum)
        assert abs(float(_host(A["wsum_" + k])[0]) - r.wsum) <= 2e-5 * r.wsum
        assert not bool(torch.any(A["dact_" + k].view(torch.int16)[torch.from_numpy(ign).to(hu.DEV)] != 0)), "ignored rows are +0"
    r = refs["f"]
    hu.assert_f32_close(_host(A["dsums"]), r.sums, what + " dice sums", rtol=2e-5)
    hu.assert_f32_close(_host(A["esums"]), np.array([r.loss_sum, r.wsum, r.sums[0], r.sums[1], r.sums[2]]), what + " eval sums", rtol=2e-5)
    prob = A["prob_e"].cpu().numpy()
    bins = np.minimum(255, (prob * np.float32(256)).astype(np.int64))
    hist = np.stack([np.bincount(bins[labels == l], minlength=256) for l in (0, 1)]).astype(np.int64)
    np.testing.assert_array_equal(A["hist"].cpu().numpy(), hist)


# ------------------------------------------------------------------------------------------- the registry (tests/test_focal_host.py)
# launching entry of include/rsu_loss.h -> the cases that launch it inside an arena (HELPERS: what a case calls it through)
FENCED = {
    "rsu_head_fwd_bwd_focal": ["test_focal_heads"],
    "rsu_head_eval_focal": ["test_focal_heads"],
}
NOT_FENCED = {}
HELPERS = {"test_focal_heads": (_launch,)}
