"""-m gpu: include/rsu.h promises of every launching entry "All calls are asynchronous on that stream and re-entrant per stream", and the
training step's two-queue schedule (schedule.py, pool.BatchUploader, dist.py) stands on it. Every other test hands the library
torch.cuda.current_stream() while that is the null stream and synchronises behind the call: a launch that goes to stream 0 and not to
`stream`, a wait for the device inside an entry and a missing fork or join in the schedule all pass there.

Entry level. Every case of test_gpu_aligned_min.CASES and test_gpu_ws_history.EXTRA, and one case each of the paths and routes fenced
files, runs through stream_util.on_stream: twice on the default stream (the reference), then under a fresh stream with a gate (a device
sleep with an event behind it) in front of every call. The same calls, the same bytes in every output and state, and every call back on
the host while its gate is still closed.

Positive controls, with stand-in "entries" (Python functions registered with the wrapper) and no library fault: (a) one that writes
its output on the default stream fails on the bytes of that output -- which also proves that a side stream of this runtime is concurrent
with the null stream: every test of this file fails loudly if it is not; (b) one that synchronises raises GateOpen; (c) one that
keeps to the current stream passes.

Re-entrant per stream. Two fresh streams, two sets of buffers with different data, a gate on each, the calls issued alternately: each
result is, byte for byte, that of the same call alone.

Net level. The launch schedule under perturbation: two training steps (a forward-only pass followed at once by another batch; an
evaluation with every mask stage; the batch uploader) with a 1 ms gate in front of the calls of the main stream only, of the side
streams only, and of all of them under a fresh stream -- each bit-equal to the ungated run on the default stream.

STREAMED / NOT_STREAMED are the registry tests/test_streams_host.py checks against the twelve headers without a GPU."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import fence_util as F  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests import routes_util as RU  # noqa: E402
from tests import stream_util as SU  # noqa: E402
from tests import test_gpu_fenced as G  # noqa: E402
from tests import test_gpu_paths_fenced as GP  # noqa: E402
from tests import test_gpu_routes_fenced as GR  # noqa: E402
from tests import test_gpu_ws_history as H  # noqa: E402
from tests import ws_util as WU  # noqa: E402
from road_segmentation_unet_amd._lib import RsuSrc, call, lib  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("side_streams_are_concurrent")]

# the cases of the two newest headers (their fenced files keep their own registries): id -> (case function, arguments, environment, entries)
NEWEST = {
    "paths_uneven": (GP._case, ("uneven",), {}, ["rsu_segment_paths"]),
    "routes_pruned": (GR._case, ("pruned",), {}, ["rsu_graph_routes", "rsu_route_score"]),
}
CASES = dict(H.ALL, **NEWEST)

_TAKES_A_STREAM = set(SU.launching())
STREAMED = {}          # entry (with an rsu_stream_t parameter) -> the case ids that run it on a gated side stream
for _id, (_fn, _args, _envv, _entries) in CASES.items():
    for _e in _entries:
        if _e in _TAKES_A_STREAM:
            STREAMED.setdefault(_e, []).append(_id)
NOT_STREAMED = {}      # entry -> why it is not run (none: every entry that takes a stream launches on it)


# =========================================================================================== the positive controls
X = np.arange(1, 4097, dtype=np.float32)


def _standin_library(how):
    """a library of one stand-in entry: y = 2 x by a torch op on the default stream ("default"), on the current stream ("current"), or on
    the current stream with a wait for it in front of the return ("synchronises")"""
    def rsu_standin(x, y):
        if how == "default":
            with torch.cuda.stream(torch.cuda.default_stream()):
                torch.mul(x, 2.0, out=y)
        else:
            torch.mul(x, 2.0, out=y)
        if how == "synchronises":
            torch.cuda.current_stream().synchronize()
        return 0
    return types.SimpleNamespace(rsu_standin=rsu_standin)


def _standin(how):
    """(case, device): the case builds a fenced arena and calls the stand-in; it compares nothing itself, on_stream does"""
    library = _standin_library(how)

    def case(placement="aligned"):
        A = F.Arena(hu.DEV, [F.f32("x", X), F.out("y", X.shape, torch.float32)], placement=placement)
        assert library.rsu_standin(A["x"], A["y"]) == 0
        A.check("stand-in %s" % how)
    return case, SU.Device(library, ["rsu_standin"])


def _control_a():
    case, device = _standin("default")
    try:
        SU.on_stream(case, ["rsu_standin"], name="control (a) default-stream write", device=device)
    except SU.StreamError as e:
        return e
    return None


@pytest.fixture(scope="module")
def side_streams_are_concurrent():
    """control (a), once: without it nothing in this file proves anything"""
    err = _control_a()
    SU.record("control (a): a stand-in that writes on the default stream: %s" % ("StreamError on %s" % (err.found[0][:2],) if err else "PASSED"))
    if err is None:
        pytest.fail("a write on the default stream passed on_stream: a side stream of this runtime is not concurrent with the null stream "
                    "(or the gates do not hold), and no test of this file proves anything", pytrace=False)
    return err


def test_control_a_write_on_the_default_stream_fails_on_its_bytes(side_streams_are_concurrent):
    err = side_streams_are_concurrent
    assert [f[:2] for f in err.found] == [(0, "y")] and err.found[0][2] > 0, str(err)


def test_control_b_an_entry_that_synchronises_returns_with_its_gate_open():
    case, device = _standin("synchronises")
    with pytest.raises(SU.GateOpen) as e:
        SU.on_stream(case, ["rsu_standin"], name="control (b) synchronises", device=device)
    assert e.value.entry == "rsu_standin" and e.value.host_ms >= 0.5 * e.value.gate_ms and not isinstance(e.value, AssertionError), str(e.value)
    SU.record("control (b): a stand-in that synchronises: GateOpen after %.3f ms under a gate of %.3f ms" % (e.value.host_ms, e.value.gate_ms))


def test_control_c_a_write_on_the_current_stream_passes():
    case, device = _standin("current")
    g = SU.on_stream(case, ["rsu_standin"], name="control (c) current-stream write", device=device)
    assert g.noted and all(closed for _e, closed, _ms in g.noted) and g.arena_gates == 1
    SU.record("control (c): a stand-in that writes on the current stream: passed")


# =========================================================================================== entry level
@pytest.mark.parametrize("case", sorted(CASES))
def test_entry_on_a_gated_side_stream(case, monkeypatch, capfd):
    through = lambda fn, entries, *a, **kw: SU.on_stream(fn, entries, *a, addresses=H.ADDRESSES.get(case, ()), name=case, **kw)  # noqa: E731
    if case in NEWEST:
        fn, args, env, entries = NEWEST[case]
        g = through(fn, entries, *args)
    else:
        g = H._run(case, monkeypatch, capfd, through)
    ran = {e for e, _closed, _ms in g.noted}
    for entry, ids in STREAMED.items():
        assert case not in ids or entry in ran, (entry, sorted(ran))


# =========================================================================================== re-entrant per stream
def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(hu.DEV)


def _bf16(a):
    return _f32(a).to(torch.bfloat16).contiguous()


def _conv_fwd(seed):
    N, H_, W, Cin, Cout = 2, 37, 41, 64, 64
    rng = np.random.RandomState(100 + seed)
    x, b = _bf16(rng.standard_normal((N, H_, W, Cin))), _f32(rng.standard_normal(Cout) * 0.1)
    wp = hu.pack_conv_fwd((rng.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(np.float32))
    y = torch.zeros((N, H_ - 2, W - 2, Cout), dtype=torch.bfloat16, device=hu.DEV)
    keep = (x, b, wp)

    def launch():
        s = (RsuSrc * 1)(RsuSrc(x.data_ptr(), H_, W, Cin, 0, 0))
        call("rsu_conv2d_fwd", s, 1, hu.ptr(wp), hu.ptr(b), hu.ptr(y), N, H_, W, Cout, 1, 1, 0, hu.stream())
    return [launch], [y], keep


def _bwd_weight(seed):
    N, H_, W, Cin, Cout, dil, _ = G.CONV[0]
    Ho, Wo = H_ - 2 * dil, W - 2 * dil
    rng = np.random.RandomState(200 + seed)
    x, dz = _bf16(rng.standard_normal((N, H_, W, Cin))), _bf16(rng.standard_normal((N, Ho, Wo, Cout)) * 0.1)
    dw = torch.zeros((3, 3, Cin, Cout), dtype=torch.float32, device=hu.DEV)
    db = torch.zeros(Cout, dtype=torch.float32, device=hu.DEV)
    ws = torch.full((int(lib().rsu_conv2d_bwd_weight_ws_floats(Cin, Cin, Cout)),), float("nan"), dtype=torch.float32, device=hu.DEV)   # its own

    def launch():
        s = hu.src_of(x, H_, W)
        call("rsu_conv2d_bwd_weight", ctypes.byref(s), hu.ptr(dz), hu.ptr(dw), hu.ptr(db), hu.ptr(ws), N, Ho, Wo, Cin, 0, Cout, dil, 0, hu.stream())
    return [launch], [dw, db], (x, dz, ws)


def _head(seed):
    C, npix = 16, 2 * 20 * 20
    rng = np.random.RandomState(300 + seed)
    act, w, b = _bf16(rng.standard_normal((npix, C))), _f32(rng.standard_normal((C, 2)) * 0.3), _f32(rng.standard_normal(2) * 0.1)
    labels = torch.from_numpy((rng.rand(npix) < 0.3).astype(np.int64)).to(hu.DEV)
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=hu.DEV)  # noqa: E731
    prob, loss, dw, db = z(npix), z(1), z(C, 2), z(2)
    dact = torch.zeros((npix, C), dtype=torch.bfloat16, device=hu.DEV)
    ws = torch.full((int(lib().rsu_head_ws_floats(npix, C)),), float("nan"), dtype=torch.float32, device=hu.DEV)

    def launch():
        call("rsu_head_fwd_bwd", hu.ptr(act), hu.ptr(w), hu.ptr(b), hu.ptr(labels), hu.ptr(prob), hu.ptr(loss), hu.ptr(dact), hu.ptr(dw), hu.ptr(db),
             hu.ptr(ws), npix, C, 1.0 / npix, hu.stream())
    return [launch], [prob, loss, dact, dw, db], (act, w, b, labels, ws)


def _thin(seed):
    from tests import thin_util as TU
    shape, iters = (2, 130, 70), 64
    rng = np.random.RandomState(400 + seed)
    prob = _f32(np.where(TU.masks("smooth3" if seed == 1 else "smooth1.5", shape), 0.9, 0.1) + rng.rand(*shape) * 0.05)
    labels = torch.from_numpy(np.ascontiguousarray(TU.masks("smooth1.5" if seed == 1 else "smooth3", shape)).astype(np.int64)).to(hu.DEV)
    skel_pred = torch.zeros(shape, dtype=torch.float32, device=hu.DEV)
    skel_true = torch.zeros(shape, dtype=torch.int64, device=hu.DEV)
    acc = torch.zeros(4, dtype=torch.int64, device=hu.DEV)
    info = torch.zeros((shape[0], 2), dtype=torch.int32, device=hu.DEV)
    ws = torch.full((int(lib().rsu_thin_ws_bytes(*shape, iters)) // 8,), -1, dtype=torch.int64, device=hu.DEV)

    def launch():
        call("rsu_mask_thin", hu.ptr(prob), TU.THRESHOLD, hu.ptr(labels), iters, hu.ptr(skel_pred), hu.ptr(skel_true), hu.ptr(acc), hu.ptr(info),
             hu.ptr(ws), *shape, hu.stream())
    return [launch], [skel_pred, skel_true, acc, info], (prob, labels, ws)


def _routes(seed):
    """three rounds of the blocked sweep (max_nodes 256 by tiles of 64 give four; 129 nodes fill three), a chain on one stream and two
    separate chains on the other"""
    node_map, edges, counts = (RU.dev(a) for a in RU.direct_case("chain" if seed == 1 else "split", 129))
    shape, max_nodes = tuple(node_map.shape), 256
    full = lambda s, v: torch.full(s, v, dtype=torch.int32, device=hu.DEV)  # noqa: E731
    nodes, dist, info = full((shape[0], max_nodes, 4), RU.FILL), full((shape[0], max_nodes, max_nodes), RU.FILL), full((shape[0], 4), 0)
    ws = RU.new_ws(shape, max_nodes)

    def launch():
        call("rsu_graph_routes", hu.ptr(node_map), hu.ptr(edges), hu.ptr(counts), 0, int(edges.shape[1]), max_nodes, hu.ptr(nodes), hu.ptr(dist),
             hu.ptr(info), hu.ptr(ws), *shape, hu.stream())
    return [launch], [nodes, dist, info], (node_map, edges, counts, ws)


REENTRANT = {"conv2d_fwd": _conv_fwd, "conv2d_bwd_weight": _bwd_weight, "head_fwd_bwd": _head, "mask_thin": _thin, "graph_routes": _routes}


@pytest.mark.parametrize("entry", sorted(REENTRANT))
def test_two_streams_do_not_disturb_each_other(entry):
    build = REENTRANT[entry]
    alone = []
    for seed in (1, 2):       # each set alone, on the default stream
        launches, outs, _keep = build(seed)
        for f in launches:
            f()
        torch.cuda.synchronize()
        alone.append([t.clone() for t in outs])
    assert not all(WU.bit_equal(a, b) for a, b in zip(*alone)), "the two sets hold the same data"
    assert all(bool(t.float().abs().sum() > 0) and bool(torch.isfinite(t.float()).all()) for t in alone[0][:1])
    sets = [build(1), build(2)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    gates = [SU.Gate(s, SU.FLOOR_MS) for s in streams]
    for k in range(len(sets[0][0])):          # alternately: A then B
        for s, (launches, _outs, _keep) in zip(streams, sets):
            with torch.cuda.stream(s):
                launches[k]()
    issued_behind = [g.closed() for g in gates]
    for s in streams:
        s.synchronize()
    for which, (want, (_l, outs, _k)) in enumerate(zip(alone, sets)):
        bad = [i for i, (w, t) in enumerate(zip(want, outs)) if not WU.bit_equal(w, t)]
        assert not bad, "%s on stream %s beside the other stream: outputs %s differ from the call alone" % (entry, "AB"[which], bad)
    SU.record("re-entrant %-20s two gated streams, calls issued alternately (both gates still closed then: %s): bit-equal to the calls alone"
              % (entry, issued_behind))


# =========================================================================================== net level: the schedule under perturbation
WHERE = ("main", "side", "all")
GATE_MS = 1.0
LR, MOMENTUM = 0.05, 0.9


def _perturbed(where, body):
    """`body()` under Gated(where) with a fixed 1 ms gate; "all": under a fresh stream as well. The device is idle when it starts and
    drained when it ends. Returns (what body returned, the Gated run)."""
    torch.cuda.synchronize()
    if where is None:
        out = body()
        torch.cuda.synchronize()
        return out, None
    stream = torch.cuda.Stream() if where == "all" else torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        with SU.Gated(F.Placement(), GATE_MS, where) as g:
            out = body()
    torch.cuda.synchronize()
    assert g.noted, "no call was gated"
    return out, g


def _device_batches(kind):
    out = [(x.to(hu.DEV), y.to(hu.DEV)) for x, y in H._batches(kind)]
    torch.cuda.synchronize()
    return out


def _two_steps(kind, where):
    """two optimizer steps on a fresh net with nothing between them that waits for the device: the loss, every gradient, every weight and
    Momentum slot behind step 2, and prob"""
    net, batches = H._net(kind), _device_batches(kind)

    def body():
        for x, y in batches[:2]:
            net.x.copy_(x)
            net.labels.copy_(y)
            net.forward_device(keep=1.0)
            net.backward_device(1.0 / (net.B * net.P * net.P))
            net.apply_momentum(LR, MOMENTUM)
    _, g = _perturbed(where, body)
    out = {k: getattr(net, k).clone() for k in ("prob", "loss_sum", "weight_sum", "dice_sums", "flat_g", "flat_w", "flat_acc")}
    for k in ("cldice_sums", "lovasz_sum"):
        if getattr(net, k) is not None:
            out[k] = getattr(net, k).clone()
    assert bool(torch.isfinite(out["flat_g"]).all()) and bool(out["flat_g"].any()) and bool(out["flat_acc"].any())
    return out, g, net


_REFERENCE = {}


def _reference(key, make):
    if key not in _REFERENCE:
        _REFERENCE[key] = make()
    return _REFERENCE[key]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("kind", sorted(H.NETS))
def test_two_steps_with_one_queue_held_back(kind, where):
    want = _reference(("steps", kind), lambda: _two_steps(kind, None)[0])
    got, g, net = _two_steps(kind, where)
    if net.wstreams and where != "all":      # both queues issued calls: the gates held back one of them only
        assert g.skipped > 0, (where, len(g.noted))
    H._same(got, want, "%s: two steps with a 1 ms gate in front of %s calls against the ungated steps" % (kind, where))
    SU.record("net %-10s two steps, gates %-4s: %3d calls gated, %3d not: bit-equal to the ungated steps" % (kind, where, len(g.noted), g.skipped))


def _forward_twice(kind, where):
    """a forward-only pass on a training net, at once another batch into net.x and a second pass: the second prob"""
    net, batches = H._net(kind), _device_batches(kind)

    def body():
        net.x.copy_(batches[0][0])
        net.forward_device(keep=1.0)
        net.x.copy_(batches[2][0])
        net.forward_device(want_logits=True, keep=1.0)
    _, g = _perturbed(where, body)
    return {"prob": net.prob.clone(), "logits": net.logits.clone()}, g


def _forward_once(kind):
    net, batches = H._net(kind), _device_batches(kind)
    net.x.copy_(batches[2][0])
    net.forward_device(want_logits=True, keep=1.0)
    torch.cuda.synchronize()
    return {"prob": net.prob.clone(), "logits": net.logits.clone()}


# (the forward pass of a net without twin blocks issues nothing on a side stream: "plain", "side" would gate no call)
@pytest.mark.parametrize("kind,where", [("dilated", w) for w in WHERE] + [("plain", "main"), ("plain", "all")])
def test_a_forward_pass_behind_a_forward_only_pass(kind, where):
    want = _reference(("forward", kind), lambda: _forward_once(kind))
    got, g = _forward_twice(kind, where)
    assert bool(got["prob"].any()) and bool(torch.isfinite(got["prob"]).all())
    H._same(got, want, "%s: the second of two forward passes, gates in front of %s calls, against a fresh net's" % (kind, where))
    SU.record("net %-10s forward, copy, forward, gates %-4s: %3d calls gated, %3d not: bit-equal to a fresh net's pass" % (kind, where, len(g.noted), g.skipped))


def test_control_a_missing_join_shows_under_the_gates_of_the_side_stream():
    """the net-level runs have teeth: with the schedule's join taken away (here, in the test; no product code) the decoder of a dilated
    net reads the twin blocks' outputs while the gated side stream has not written them, and prob differs -- a mismatch, nothing else:
    every buffer read is the net's own"""
    want = _reference(("forward", "dilated"), lambda: _forward_once("dilated"))
    net, batches = H._net("dilated"), _device_batches("dilated")
    net.sched.join = lambda: None

    def body():
        net.x.copy_(batches[2][0])
        net.forward_device(want_logits=True, keep=1.0)
    _, g = _perturbed("side", body)
    assert g.skipped > 0 and not WU.bit_equal(net.prob.clone(), want["prob"]), "a forward pass without its join still gave the joined pass's prob"
    SU.record("control: a dilated forward pass with its join removed, gates side: prob differs from the joined pass, as it must")


def _routes_model():
    from tests import test_gpu_graph as TG
    return TG._model(**dict(H.MODEL, validate_routes=True))


def _evaluations(where):
    model, sets = _routes_model(), H._eval_sets()
    model.net.ensure_tuned(training=False, keep=1.0)      # (evaluate()'s tuning pass times launches: not under the gates)
    out, g = _perturbed(where, lambda: [model.evaluate(X_, y_) for X_, y_ in sets])
    return out, g


@pytest.mark.parametrize("where", WHERE)
def test_an_evaluation_with_one_queue_held_back(where):
    want = _reference("evaluate", lambda: _evaluations(None)[0])
    assert "apls" in want[1] and want[1]["segments_true"] > 0 and not WU.bit_equal(want[0]["hist"], want[1]["hist"]), sorted(want[1])
    got, g = _evaluations(where)
    for i in (0, 1):
        H._same(got[i], want[i], "evaluate() of set %d with a 1 ms gate in front of %s calls against the ungated one" % (i, where))
    SU.record("model      two evaluations with routes, gates %-4s: %3d calls gated, %3d not: bit-equal to the ungated ones" % (where, len(g.noted), g.skipped))


@pytest.mark.parametrize("where", WHERE)
def test_the_uploader_hands_over_every_batch(where):
    """BatchUploader.stage / commit over three batches through its two slots. "side": a gate on the uploader's stream in front of each
    stage (the compute stream runs ahead); "main": a gate on the compute stream in front of each commit (the uploader runs ahead);
    "all": both, with a fresh compute stream. net.x and net.labels behind each commit against the host arrays."""
    from road_segmentation_unet_amd.pool import BatchUploader
    kind = "plain"
    net = H._net(kind)
    host = [(x.numpy(), y.numpy()) for x, y in H._batches(kind)]
    up = BatchUploader(net)
    torch.cuda.synchronize()
    compute = torch.cuda.Stream() if where == "all" else torch.cuda.current_stream()
    seen = []
    with torch.cuda.stream(compute):
        for i, (x, y) in enumerate(host):
            slot = i % 2
            if where in ("side", "all"):
                SU.Gate(up.stream, GATE_MS)
            up.stage(slot, x, y)
            if where in ("main", "all"):
                SU.Gate(compute, GATE_MS)
            up.commit(slot)
            seen.append((net.x.clone(), net.labels.clone()))      # (on the compute stream, behind the commit)
    torch.cuda.synchronize()
    for i, ((x, y), (gx, gy)) in enumerate(zip(host, seen)):
        assert np.array_equal(gx.cpu().numpy(), x.astype(np.float32)) and np.array_equal(gy.cpu().numpy(), y), "batch %d (%s)" % (i, where)
    assert not np.array_equal(host[0][0], host[2][0])
    SU.record("uploader   three batches through two slots, gates %-4s: net.x and net.labels behind every commit are the host arrays" % where)
