"""-m gpu: the launching entry points of include/rsu_cldice.h inside a fenced arena (tests/fence_util.py), as tests/test_gpu_loss_fenced.py
holds those of include/rsu_loss.h: rsu_cldice_fwd and rsu_cldice_bwd at (3, 37, 41) -- a sliver beside the forward's 32-pixel tile and
beside the backward's 16-pixel one, images smaller than the halo at 16 iterations -- with iters 3 and 16, tied values and ignored labels;
rsu_head_fwd_bwd_aux at npix = 3 * 37 * 41 for every C the heads admit, without and with the Dice term (behind rsu_head_dice_sums). Every
workspace is exactly its size function's (rsu_cldice_ws_floats / rsu_head_dice_ws_floats). After Arena.check: no NaN in any result (an
element never written, or a stray read of the bands, is one), and the results against the references of tests/test_gpu_cldice.py.

FENCED is the registry tests/test_cldice_host.py checks against include/rsu_cldice.h without a GPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cldice_util as CU  # noqa: E402
from tests import fence_util as F  # noqa: E402
from tests import focal_util as FU  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests.head_util import LAM, NPIX, SMOOTH, _inputs, _weight_map, _with_ignored  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

HEAD_C = [8, 16, 32, 64, 128, 256, 512]      # every C the heads admit
SHAPE = (3, 37, 41)
GAMMA = 2.0


def _host(t):
    return t.detach().to(torch.float32).cpu().numpy()


def _launch_cldice(A, iters, st):
    p = lambda n: hu.ptr(A[n])  # noqa: E731
    call("rsu_cldice_fwd", p("prob"), p("labels"), iters, p("skel_p"), p("skel_y"), p("sums"), p("ws"), *SHAPE, st)
    call("rsu_cldice_bwd", p("prob"), p("labels"), p("skel_p"), p("skel_y"), p("sums"), iters, CU.SCALE, CU.SMOOTH, p("gprob"), p("ws"), *SHAPE, st)


@pytest.mark.parametrize("kind", ["tied4", "saturated"])
@pytest.mark.parametrize("iters", [3, 16])
def test_cldice_fwd_bwd(iters, kind, placement="aligned"):
    p, labels = CU.INPUTS[kind](SHAPE)
    assert ((labels != 0) & (labels != 1)).sum() > labels.size // 20
    o32 = lambda name, *s: F.out(name, s, torch.float32)  # noqa: E731
    specs = [F.f32("prob", p), F.raw("labels", labels), o32("skel_p", *SHAPE), o32("skel_y", *SHAPE), o32("gprob", *SHAPE),
             F.state("sums", np.zeros(4, np.float32)), F.ws("ws", lib().rsu_cldice_ws_floats(*SHAPE, iters))]
    A = F.Arena(hu.DEV, specs, placement=placement)
    _launch_cldice(A, iters, hu.stream())
    what = "clDice fenced k=%d %s" % (iters, kind)
    A.check(what)
    for n in ("skel_p", "skel_y", "gprob", "sums", "ws"):      # (the forward writes every element of its workspace)
        assert not bool(torch.isnan(A[n]).any()), (what, n)
    sp, sy, sums, gprob = hostio.cldice_gradient(p, labels, iters, CU.SCALE, CU.SMOOTH)
    y = (labels == 1).astype(np.float32)
    assert np.array_equal(_host(A["skel_p"]).view(np.int32), hostio.soft_skeleton(p, iters).view(np.int32)), what
    assert np.array_equal(_host(A["skel_y"]).view(np.int32), hostio.soft_skeleton(y, iters).view(np.int32)), what
    got = _host(A["sums"]).astype(np.float64)
    assert np.all(np.abs(got - sums) <= 2e-5 * np.abs(sums)), (what, got, sums)
    hu.assert_f32_close(_host(A["gprob"]), gprob, what + " gprob")


def _launch_aux(A, C, inv, st):
    """the aux head without and with the Dice term, each with outputs and a workspace of its own"""
    p = lambda n: hu.ptr(A[n])  # noqa: E731
    head = (p("act"), p("w"), p("b"), p("labels"))
    call("rsu_head_fwd_bwd_aux", *head, p("cw"), p("pw"), GAMMA, None, 0.0, 0.0, p("prob_f"), p("loss_f"), p("wsum_f"), p("dact_f"), p("dw_f"),
         p("db_f"), p("ws_f"), NPIX, C, inv, p("gprob"), st)
    call("rsu_head_dice_sums", *head, p("pw"), p("prob_s"), p("dsums"), p("ws_d"), NPIX, C, st)
    call("rsu_head_fwd_bwd_aux", *head, p("cw"), p("pw"), 0.0, p("dsums"), LAM, SMOOTH, p("prob_d"), p("loss_d"), p("wsum_d"), p("dact_d"),
         p("dw_d"), p("db_d"), p("ws_d"), NPIX, C, inv, p("gprob"), st)


@pytest.mark.parametrize("C", HEAD_C)
def test_aux_head(C, placement="aligned"):
    rng, act, w, b, labels = _inputs(C)
    pixel_w = _weight_map(rng)
    labels, ign = _with_ignored(rng, labels)
    inv = 1.0 / (2 * NPIX)
    gp = (rng.standard_normal(NPIX) * 4.0 * inv).astype(np.float32)
    L = lib()
    z = lambda name, *s: F.state(name, np.zeros(s, np.float32))  # noqa: E731
    o32 = lambda name, *s: F.out(name, s, torch.float32)  # noqa: E731
    specs = [F.bf16("act", act), F.f32("w", w), F.f32("b", b), F.raw("labels", labels), F.f32("cw", np.asarray(FU.CLASS_W, np.float32)),
             F.f32("pw", pixel_w), F.f32("gprob", gp)]
    for k in ("f", "d"):
        specs += [o32("prob_" + k, NPIX), F.out("dact_" + k, (NPIX, C)), o32("dw_" + k, C, 2), o32("db_" + k, 2), z("loss_" + k, 1), z("wsum_" + k, 1)]
    specs += [o32("prob_s", NPIX), o32("dsums", 3), F.ws("ws_f", L.rsu_head_dice_ws_floats(NPIX, C)), F.ws("ws_d", L.rsu_head_dice_ws_floats(NPIX, C))]
    A = F.Arena(hu.DEV, specs, placement=placement)
    _launch_aux(A, C, inv, hu.stream())
    what = "aux head fenced C=%d" % C
    A.check(what)
    for s in specs:
        if s.kind in ("out", "state"):
            assert not bool(torch.isnan(A[s.name].to(torch.float32)).any()), (what, s.name)
    safe_pw = np.where(~ign, pixel_w, 1.0)
    refs = {"f": CU.AuxRef(act, w, b, labels, FU.CLASS_W, safe_pw, inv, GAMMA, gp),
            "d": CU.AuxRef(act, w, b, labels, FU.CLASS_W, safe_pw, inv, 0.0, gp, lam=LAM, smooth=SMOOTH)}
    for k, r in refs.items():
        hu.assert_f32_close(_host(A["prob_" + k]), r.prob, what + " prob_" + k, rtol=1e-4, atol_scale=1e-6)
        hu.assert_bf16_close(_host(A["dact_" + k]), r.dact, what + " dact_" + k)
        hu.assert_f32_close(_host(A["dw_" + k]), r.dw, what + " dw_" + k)
        hu.assert_f32_close(_host(A["db_" + k]), r.db, what + " db_" + k)
        assert abs(float(_host(A["loss_" + k])[0]) - r.loss_sum) <= 2e-5 * abs(r.loss_sum), (k, r.loss_sum)
        assert abs(float(_host(A["wsum_" + k])[0]) - r.wsum) <= 2e-5 * r.wsum
        assert not bool(torch.any(A["dact_" + k].view(torch.int16)[torch.from_numpy(ign).to(hu.DEV)] != 0)), "ignored rows are +0"
    hu.assert_f32_close(_host(A["dsums"]), refs["d"].sums, what + " dice sums", rtol=2e-5)


# ------------------------------------------------------------------------------------------- the registry (tests/test_cldice_host.py)
# launching entry of include/rsu_cldice.h -> the cases that launch it inside an arena (HELPERS: what a case calls it through)
FENCED = {
    "rsu_cldice_fwd": ["test_cldice_fwd_bwd"],
    "rsu_cldice_bwd": ["test_cldice_fwd_bwd"],
    "rsu_head_fwd_bwd_aux": ["test_aux_head"],
}
NOT_FENCED = {}
HELPERS = {"test_cldice_fwd_bwd": (_launch_cldice,), "test_aux_head": (_launch_aux,)}
