"""-m gpu: the launching entry points of include/rsu_optim.h inside a fenced arena (tests/fence_util.py), as tests/test_gpu_fenced.py
holds those of include/rsu.h: rsu_update_table_run_decay and rsu_update_table_run_adam_decay over the table of
test_gpu_fenced.test_update_and_pack_tables -- a 3x3 conv kernel of two concat sources (24 + 16 -> 40), a transposed-conv kernel
(72 -> 40), the first conv (3 -> 72), a plain range of 1003 floats -- for {momentum, adam} x {l2, decoupled} x {clip_state NULL, a
clipping record with 0 < scale < 1, a record with RSU_CLIP_NONFINITE}, lambda = 0.1 and lr = 0.01 (the decay moves a weight by about
1e-3 of itself, far above every tolerance here).

What a case is held to: the EXISTING entries of rsu.h, run in arenas of their own on inputs transformed on the host -- decoupled: the
weights pre-decayed as w - f32(d) * w; l2 under Adam: the gradient f32(f32(gscale' g) + f32(lambda w)) with gscale 1 -- must give the
same BITS in the weights, the slots and the packed copies. l2 under Momentum goes against the numpy restatement (tests/decay_util.py) at
the tolerance test_update_and_pack_tables grants the Momentum rule: the existing rule's mu * acc + gscale * g may be contracted by the
compiler, so the bits of two kernels cannot be promised equal there.

FENCED is the registry tests/test_optim_host.py checks against include/rsu_optim.h without a GPU."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import decay_util as D  # noqa: E402
from tests import fence_util as F  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

f32 = np.float32
EINVAL = -22
LAMBDA, LR, MU, GSCALE = 0.1, 0.01, 0.9, 0.5
ALPHA, B1, B2, EPS = 1.234e-3, 0.9, 0.999, 1e-8
RTOL, ATOL = 1e-6, 1e-7            # test_gpu_fenced.test_update_and_pack_tables, the Momentum rule
SEGS, CC = [24, 16], 40
KEYS = ("conv", "convT", "first", "plain")
DECAYS = ("conv", "convT", "first")   # the entries of rsu_update_table_add; "plain" is the range of rsu_update_table_add_plain
PACKS = {"conv_fwd": (9, CC, SEGS, 1), "conv_bwd0": (9, 24, [CC], 1), "conv_bwd1": (9, 16, [CC], 1), "convT_fwd": (1, 40, [72], 4),
         "convT_bwd": (4, 72, [40], 1)}
PACK_KEYS = tuple(PACKS) + ("first",)


def _rand(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(f32)


@functools.lru_cache(maxsize=None)
def _inputs():
    """the variables, gradients and slots of every case, drawn once and never written"""
    rng = np.random.RandomState(17)
    var = {"conv": _rand(rng, 3, 3, 40, CC, scale=0.1), "convT": _rand(rng, 2, 2, 40, 72, scale=0.1), "first": _rand(rng, 3, 3, 3, 72, scale=0.3),
           "plain": _rand(rng, 1003)}
    grads = {k: _rand(rng, *t.shape, scale=1e-2) for k, t in var.items()}
    accs = {k: _rand(rng, *t.shape, scale=1e-2) for k, t in var.items()}
    vs = {k: (rng.rand(*t.shape) * 1e-4).astype(f32) for k, t in var.items()}
    bad = grads["plain"].copy()
    bad[501] = np.inf
    return var, grads, accs, vs, bad


def _packed(name, taps, rows, segs, mult=1):
    seg = (ctypes.c_int * len(segs))(*segs)
    return F.out(name, (mult * lib().rsu_packed_bytes(taps, rows, seg, len(segs)) // 2,))


class _Table:
    """one arena with the four variables, their slots and gradients, the packed copies an update table points at (`u_`: packed once from
    the initial weights), a second set for rsu_pack_* of the new weights (`s_`), the table, and the record of rsu_grad_norm"""

    def __init__(self, adam, var, grads, clip, placement="aligned"):
        _, _, accs, vs, bad = _inputs()
        L = lib()
        self.adam = adam
        specs = []
        for k in KEYS:
            specs += [F.state("w_" + k, var[k]), F.state("a_" + k, accs[k]), F.f32("g_" + k, grads[k])]
            if adam:
                specs.append(F.state("v_" + k, vs[k]))
        for tag in ("u", "s"):
            specs += [_packed("%s_%s" % (tag, k), *a) for k, a in PACKS.items()]
            specs.append(F.out(tag + "_first", (L.rsu_packed_first_bytes(72) // 2,)))
        esz = L.rsu_update_table_entry_bytes()
        specs += [F.out("utable", (esz * 4,), torch.uint8), F.f32("g_norm", bad if clip == "nonfinite" else _inputs()[1]["plain"]),
                  F.ws("nws", L.rsu_grad_norm_ws_floats(1003)), F.state("state", np.zeros(8, np.int32))]
        self.A = A = F.Arena(hu.DEV, specs, placement=placement)
        self.p = p = lambda k: hu.ptr(A[k])  # noqa: E731
        self.st = st = hu.stream()
        host = ctypes.create_string_buffer(esz * 4)
        self.seg = seg = (ctypes.c_int * 2)(*SEGS)
        bw = (ctypes.c_void_p * 2)(A["u_conv_bwd0"].data_ptr(), A["u_conv_bwd1"].data_ptr())
        bwT = (ctypes.c_void_p * 1)(A["u_convT_bwd"].data_ptr())
        assert L.rsu_update_table_add(host, 0, 0, p("w_conv"), p("a_conv"), p("g_conv"), p("u_conv_fwd"), bw, 40, CC, seg, 2) == 1
        assert L.rsu_update_table_add(host, 1, 2, p("w_convT"), p("a_convT"), p("g_convT"), p("u_convT_fwd"), bwT, 72, 40, None, 0) == 1
        assert L.rsu_update_table_add(host, 2, 4, p("w_first"), p("a_first"), p("g_first"), p("u_first"), None, 3, 72, None, 0) == 1
        assert L.rsu_update_table_add_plain(host, 3, p("w_plain"), p("a_plain"), p("g_plain"), 1003) == 1
        if adam:
            for i, k in enumerate(KEYS):
                assert L.rsu_update_table_set_second_slot(host, i, p("v_" + k)) == 0
        nb = ctypes.c_int(0)
        assert L.rsu_update_table_finish(host, 4, ctypes.byref(nb)) == 0
        self.nb = nb.value
        A["utable"].copy_(torch.frombuffer(bytearray(host.raw), dtype=torch.uint8))
        self.pack("u")
        self.scale = 1.0
        if clip is not None:
            call("rsu_grad_norm", p("g_norm"), 1003, 0.05, p("nws"), p("state"), st)
        torch.cuda.synchronize()
        if clip is not None:
            rec = A["state"].cpu().numpy()
            self.scale = float(rec.view(f32)[2])
            assert (int(rec[3]) & 2) == (2 if clip == "nonfinite" else 0) and (clip == "nonfinite" or 0 < self.scale < 1), rec
        self.before = A.mem.clone()

    def pack(self, tag):
        """the per-tensor rsu_pack_* calls from the weights as they are now"""
        p, st, seg = self.p, self.st, self.seg
        call("rsu_pack_conv_fwd", p("w_conv"), p(tag + "_conv_fwd"), 3, 40, CC, seg, 2, st)
        call("rsu_pack_conv_bwd", p("w_conv"), p(tag + "_conv_bwd0"), 3, 40, 0, 24, CC, st)
        call("rsu_pack_conv_bwd", p("w_conv"), p(tag + "_conv_bwd1"), 3, 40, 24, 16, CC, st)
        call("rsu_pack_convT_fwd", p("w_convT"), p(tag + "_convT_fwd"), 72, 40, st)
        call("rsu_pack_convT_bwd", p("w_convT"), p(tag + "_convT_bwd"), 72, 40, st)
        call("rsu_pack_conv_first", p("w_first"), p(tag + "_first"), 72, st)

    def state_ptr(self, clip):
        return self.p("state") if clip is not None else None

    def run_existing(self, clip, gscale=GSCALE):
        """the entry of rsu.h for this rule, with or without the record"""
        p, st, tab = self.p, self.st, (self.p("utable"), 4, self.nb)
        if self.adam and clip:
            call("rsu_update_table_run_adam_clip", *tab, ALPHA, B1, B2, EPS, gscale, p("state"), st)
        elif self.adam:
            call("rsu_update_table_run_adam", *tab, ALPHA, B1, B2, EPS, gscale, st)
        elif clip:
            call("rsu_update_table_run_clip", *tab, LR, MU, gscale, p("state"), st)
        else:
            call("rsu_update_table_run", *tab, LR, MU, gscale, st)

    def decay_entry(self, decay, mode, clip_state, table=True, nentries=4, nblocks=None):
        """rc of the entry of rsu_optim.h for this rule (no exception: the error cases read it)"""
        tab = (self.p("utable") if table else None, nentries, self.nb if nblocks is None else nblocks)
        if self.adam:
            return getattr(lib(), "rsu_update_table_run_adam_decay")(*tab, ALPHA, B1, B2, EPS, GSCALE, decay, mode, clip_state, self.st)
        return getattr(lib(), "rsu_update_table_run_decay")(*tab, LR, MU, GSCALE, decay, mode, clip_state, self.st)

    def host(self, name):
        torch.cuda.synchronize()
        return self.A[name].detach().cpu().numpy()

    def bits(self, name):
        t = self.A[name]
        return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)

    def slots(self):
        return ("w_", "a_", "v_") if self.adam else ("w_", "a_")


def _same_bits(X, Y, names, what):
    for n in names:
        assert torch.equal(X.bits(n).cpu(), Y.bits(n).cpu()), "%s: %s differs in its bits" % (what, n)


@pytest.mark.parametrize("clip", [None, "clip", "nonfinite"], ids=["null", "clip", "nonfinite"])
@pytest.mark.parametrize("mode", ["l2", "decoupled"])
@pytest.mark.parametrize("rule", ["momentum", "adam"])
def test_update_table_decay(rule, mode, clip, placement="aligned"):
    """rsu_update_table_run_decay / rsu_update_table_run_adam_decay (module docstring)"""
    adam, m = rule == "adam", D.L2 if mode == "l2" else D.DECOUPLED
    var, grads, accs, vs, _ = _inputs()
    decay = float(f32(LAMBDA)) if m == D.L2 else float(f32(LR) * f32(LAMBDA))
    what = "update table decay, %s %s %s" % (rule, mode, clip)
    T = _Table(adam, var, grads, clip, placement)
    A = T.A
    state_before = A["state"].clone()
    assert T.decay_entry(decay, m, T.state_ptr(clip)) == 0, what
    if clip == "nonfinite":
        # 8. a skipped step: every byte of the arena -- weights, slots, packed copies, table, record, bands -- is what it was
        torch.cuda.synchronize()
        assert torch.equal(A.mem, T.before), what + ": a skipped step wrote something"
        A.check(what)
        return
    T.pack("s")
    # 1. no band, input or table byte changed; the record is read only; no NaN in a result
    A.check(what)
    assert torch.equal(A["utable"], T.before[A.place["utable"][0]:A.place["utable"][1]]), "the device table was written"
    assert torch.equal(A["state"], state_before), "the record was written"
    for k in KEYS:
        for s in T.slots():
            assert np.isfinite(T.host(s + k)).all(), s + k
    # 2. the packed copies are rsu_pack_* of the new weights, and new
    for k in PACK_KEYS:
        assert not bool(torch.isnan(A["u_" + k].float()).any()), k
        assert torch.equal(T.bits("u_" + k), T.bits("s_" + k)), what + ": update pass against rsu_pack_*: " + k
        lo, hi, _ = A.place["u_" + k]
        assert not torch.equal(A.mem[lo:hi], T.before[lo:hi]), what + ": the update pass left the old copy: " + k
    # 3. the plain range: the bits of the existing entry on the same inputs (U: the undecayed run, also the yardstick of 7.)
    U = _Table(adam, var, grads, clip, placement)
    U.run_existing(clip)
    U.A.check(what + ": undecayed run")
    _same_bits(T, U, [s + "plain" for s in T.slots()], what + ": plain range against the existing entry")
    gs = f32(GSCALE) * f32(T.scale)
    assert U.scale == T.scale
    if m == D.DECOUPLED:
        # 4. the existing entry on weights pre-decayed on the host: w - f32(d) * w, two float32 roundings
        pre = {k: (D.decayed_weights(var[k], decay) if k in DECAYS else var[k]) for k in KEYS}
        R = _Table(adam, pre, grads, clip, placement)
        R.run_existing(clip)
        R.A.check(what + ": reference run")
        _same_bits(T, R, [s + k for k in KEYS for s in T.slots()] + ["u_" + k for k in PACK_KEYS], what + ": against the pre-decayed run")
    elif adam:
        # 5. the existing Adam entry with gscale = 1 on the gradient f32(f32(gscale' g) + f32(lambda w)); the plain range: f32(gscale' g)
        g1 = {k: D.l2_gradient(var[k], grads[k], gs, decay, decays=k in DECAYS) for k in KEYS}
        R = _Table(adam, var, g1, None, placement)
        R.run_existing(None, gscale=1.0)
        R.A.check(what + ": reference run")
        _same_bits(T, R, [s + k for k in KEYS for s in T.slots()] + ["u_" + k for k in PACK_KEYS], what + ": against the transformed gradient")
    else:
        # 6. the numpy restatement at the Momentum rule's tolerance
        for k in KEYS:
            rw, ra = D.momentum_decay(var[k], accs[k], grads[k], LR, MU, gs, decay, m, decays=k in DECAYS)
            np.testing.assert_allclose(T.host("a_" + k), ra, rtol=RTOL, atol=ATOL, err_msg=k)
            np.testing.assert_allclose(T.host("w_" + k), rw, rtol=RTOL, atol=ATOL, err_msg=k)
    # 7. the decay is far above that tolerance: most weights of every decaying entry moved by more than 100 x (atol + rtol |w|)
    for k in DECAYS:
        wd, wu = T.host("w_" + k).astype(np.float64), U.host("w_" + k).astype(np.float64)
        far = np.abs(wd - wu) > 100.0 * (ATOL + RTOL * np.abs(wu))
        assert far.mean() > 0.5, (what, k, float(far.mean()))


@pytest.mark.parametrize("rule", ["momentum", "adam"])
def test_update_table_decay_argument_errors(rule):
    """9. RSU_EINVAL, and not one byte of the arena written: what the plain run rejects (a NULL table, no entries, no workgroups), a decay
    that is 0, negative, inf or nan, a mode that is neither constant, a clip_state that is not 4-byte aligned"""
    var, grads, _, _, _ = _inputs()
    T = _Table(rule == "adam", var, grads, "clip")
    d, ok = float(f32(LR) * f32(LAMBDA)), T.p("state")
    odd = ctypes.c_void_p(T.A["state"].data_ptr() + 2)
    cases = [dict(decay=d, mode=1, clip_state=ok, table=False), dict(decay=d, mode=1, clip_state=ok, nentries=0),
             dict(decay=d, mode=1, clip_state=ok, nblocks=0), dict(decay=0.0, mode=1, clip_state=ok), dict(decay=-1e-3, mode=0, clip_state=None),
             dict(decay=float("inf"), mode=1, clip_state=None), dict(decay=float("nan"), mode=0, clip_state=ok),
             dict(decay=d, mode=2, clip_state=ok), dict(decay=d, mode=-1, clip_state=None), dict(decay=d, mode=1, clip_state=odd)]
    for kw in cases:
        assert T.decay_entry(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert torch.equal(T.A.mem, T.before), "a refused call wrote something"
    T.A.check("update table decay, refused calls")


# ------------------------------------------------------------------------------------------- the registry (tests/test_optim_host.py)
# launching entry of include/rsu_optim.h -> the cases that launch it inside an arena (HELPERS: what a case calls it through)
FENCED = {
    "rsu_update_table_run_decay": ["test_update_table_decay", "test_update_table_decay_argument_errors"],
    "rsu_update_table_run_adam_decay": ["test_update_table_decay", "test_update_table_decay_argument_errors"],
}
NOT_FENCED = {}
HELPERS = {"test_update_table_decay": (_Table,), "test_update_table_decay_argument_errors": (_Table,)}
