"""No GPU: the workspace fills of tests/fence_util.py and ws_util.history_free have teeth, and tests/test_gpu_ws_history.py leaves no entry
with a workspace out. On CPU tensors: under every fill a workspace starts as that fill and nothing else changes (bands, outputs and
check() are today's); "rolled" is a permutation of the snapshot and differs from it. Three torch "kernels" with the faults the pattern
is blind to -- a partial maximum read from a slot no block wrote, a step skipped because a counter nobody cleared reads 0, a minimum taken
with a slot nobody set to infinity -- pass history_free under the pattern alone and fail under another fill. The inputs of the
per-image convergence cases of the thin and graph fenced files do on the host what their docstrings claim. The registry check parses
the ten headers: every launching entry with a `ws` or `kws` pointer is in HISTORY or in NOT_RUN. ws_util.refiller puts the fill back in
front of every library call that receives a workspace (through real entry points that refuse their arguments), Arena.refill restores
the starting bytes at any address and size, and a table of device addresses is compared with them as arena offsets."""
import numpy as np
import pytest
import torch

from tests import align_util as au
from tests import fence_util as F
from tests import ws_util as WU

CPU = "cpu"
BAND = 4096
N_WS = 1000


def _arena(fill, snapshots=None, mode="aligned"):
    rng = np.random.RandomState(0)
    x = rng.standard_normal((3, 37, 8)).astype(np.float32)
    P = F.Placement(mode, [{"x": 16, "acc": 8}], fill=fill, snapshots=snapshots)
    specs = [F.bf16("x", x), F.out("y", (3, 37, 8)), F.ws("ws", N_WS), F.ws("iws", 77, torch.int64), F.state("acc", np.zeros(5, np.float32))]
    return F.Arena(CPU, specs, band=BAND, placement=P), P


def _snapshots():
    """what the two workspaces hold after a "run": distinct values everywhere"""
    A, P = _arena("pattern")
    A["ws"].copy_(torch.arange(N_WS, dtype=torch.float32) + 1)
    A["iws"].copy_(torch.arange(77, dtype=torch.int64) * 3 + 5)
    return P.workspaces()


@pytest.mark.parametrize("mode", ["aligned", "minimum"])
@pytest.mark.parametrize("fill", F.FILLS)
def test_a_workspace_starts_as_its_fill_and_nothing_else_changes(fill, mode):
    snaps = _snapshots()
    assert sorted(snaps) == [(0, "iws"), (0, "ws")] and all(v.dtype == torch.uint8 for v in snaps.values())
    A, P = _arena(fill, snaps, mode)
    assert P.fill == fill and F.Placement().fill == "pattern" and A.placement is P
    ws, iws = A.payload_bytes("ws"), A.payload_bytes("iws")
    if fill == "pattern":
        assert (ws.view(torch.int16) == F.PATTERN).all() and (iws.view(torch.int16) == F.PATTERN).all() and torch.isnan(A["ws"]).all()
    elif fill == "zeros":
        assert not ws.any() and not iws.any()
    elif fill == "ones":
        assert (ws == 0xFF).all() and (iws == 0xFF).all() and torch.isnan(A["ws"]).all() and (A["iws"] == -1).all()
        assert (A["ws"].view(torch.int32) != 0x7FA57FA5).all()      # a NaN, with another payload
    else:
        for name, t, count in (("ws", A["ws"], N_WS), ("iws", A["iws"], 77)):
            was = snaps[(0, name)].view(t.dtype)
            k = (count // 3) | 1
            assert F.roll_shift(count) == k and k % 2 == 1 and 0 < k < count
            assert torch.equal(t, torch.roll(was, k)) and not torch.equal(t, was)
            assert torch.equal(t.sort().values, was.sort().values)       # a permutation of the snapshot
            assert int(t[k]) == int(was[0])                              # element 0 went to element k, whole elements
    # everything else is as under the pattern: the bands, the output, the state and the input as given; check() passes
    assert torch.isnan(A["y"]).all() and (A.payload_bytes("y").view(torch.int16) == F.PATTERN).all()
    assert not A["acc"].any() and not torch.isnan(A["x"].float()).any()
    for _, _, s, e, _ in A.regions:
        assert e == s or not A._diff(s, e).any()
    A.check("untouched")
    # and check() still catches a write into a band (of the workspace too) and into an input
    for name, side, at in (("y", "behind", A.place["y"][1]), ("ws", "behind", A.place["ws"][1] + 4), ("ws", "front", A.place["ws"][0] - 1),
                           ("x", "input", A.place["x"][0] + 3)):
        keep = int(A.mem[at])
        A.mem[at] = (keep + 1) & 0xFF
        with pytest.raises(F.FenceError) as e:
            A.check("one byte")
        assert (e.value.tensor, e.value.side, e.value.count) == (name, side, 1), str(e.value)
        A.mem[at] = keep
    A.check("restored")


def test_a_rolled_fill_needs_its_snapshot_and_fills_only_workspaces():
    with pytest.raises(AssertionError, match="no snapshot"):
        _arena("rolled", {})
    with pytest.raises(AssertionError):
        F.Placement(fill="ffff")
    snaps = _snapshots()
    P = F.Placement(fill="rolled", snapshots=snaps)
    F.Arena(CPU, [F.out("y", (4,))], band=BAND, placement=P)                 # arena 0 without a workspace: nothing is asked for
    with pytest.raises(AssertionError, match="no snapshot"):                  # the snapshots are keyed by (arena index, name)
        F.Arena(CPU, [F.ws("ws", N_WS)], band=BAND, placement=P)


# ------------------------------------------------------------------------------------------- positive controls: history_free has teeth
X = np.array([-3.5, -1.25, -7.0, -2.0, -9.0, -4.0], np.float32)       # three "blocks" of two


def _reads_before_writing(A):
    """a maximum over per-block partials: three blocks write their slot, the last pass reads FOUR (a grid rounded up) with an fmax that
    drops NaN -- so the pattern and 0xFF drop out, a zero or another call's partial does not"""
    part = A["ws"]
    part[:3] = A["x"].reshape(3, 2).max(dim=1).values
    A["y"][0] = torch.fmax(torch.fmax(part[0], part[1]), torch.fmax(part[2], part[3]))


def _skips_on_a_stale_counter(A):
    """two step launches over ping-pong planes; a launch adds the number of pixels it changed to its own counter and the launch behind
    returns at once where that is 0 ("a fixed point: out already holds it"). Nobody clears the counters: 0x7FA5... + 1 is not 0, and
    neither is 0 + 1, but 0xFFFFFFFF + 1 is"""
    cnt, planes = A["cws"], A["pws"].view(2, -1)
    x = A["x"].reshape(-1)
    step = lambda v: torch.where(v > 8, v - 1, v)  # noqa: E731
    planes[1] = step(x)
    cnt[0] += int((planes[1] != x).sum())          # (an integer atomic add: wraps)
    if int(cnt[0]) != 0:
        planes[0] = step(planes[1])
    else:
        planes[0] = planes[0]                      # returns at once: plane 0 is taken to hold the fixed point
    A["y"].copy_(planes[0])


def _min_with_an_unset_slot(A):
    """the smallest pixel index of every label by an atomic minimum into a slot nobody set to "infinity": the pattern is large enough"""
    slot, lab = A["ws"], A["x"].reshape(-1)
    for i in range(lab.numel()):
        slot[lab[i]] = min(int(slot[lab[i]]), i + 100)
    A["y"].copy_(slot[lab])


def _control(kernel):
    def case(placement="aligned"):
        if kernel is _reads_before_writing:
            A = F.Arena(CPU, [F.f32("x", X), F.out("y", (1,), torch.float32), F.ws("ws", 4)], band=BAND, placement=placement)
            kernel(A)
            want = np.array([X.max()], np.float32)
        elif kernel is _skips_on_a_stale_counter:
            x = np.array([9, 3, 7, 8, 1, 4], np.int32)               # one pixel changes in the first step (9 -> 8), none in the second
            A = F.Arena(CPU, [F.raw("x", x), F.out("y", (6,), torch.int32), F.ws("pws", 12, torch.int32), F.ws("cws", 2, torch.int32)],
                        band=BAND, placement=placement)
            kernel(A)
            want = np.array([8, 3, 7, 8, 1, 4], np.int32)
        else:
            lab = np.array([2, 0, 2, 1, 0, 1, 1], np.int64)
            A = F.Arena(CPU, [F.raw("x", lab), F.out("y", (7,), torch.int32), F.ws("ws", 3, torch.int32)], band=BAND, placement=placement)
            kernel(A)
            want = np.array([100, 101, 100, 103, 101, 103, 103], np.int32)
        A.check(kernel.__name__)
        assert A["y"].numpy().tobytes() == want.tobytes(), (kernel.__name__, A["y"].numpy(), want)      # the case's own comparison
    return case


CONTROLS = {_reads_before_writing: {"zeros"}, _skips_on_a_stale_counter: {"ones"}, _min_with_an_unset_slot: {"zeros", "ones", "rolled"}}


@pytest.mark.parametrize("kernel", list(CONTROLS), ids=lambda k: k.__name__)
def test_a_fault_the_pattern_is_blind_to_fails_under_another_fill(kernel):
    """the argument for the fills, executable: each faulty kernel passes its fenced case as the suite ran it until now -- pattern fill,
    reference comparison, Arena.check -- and is caught by exactly the fills named above"""
    case = _control(kernel)
    case()                                                         # today's run
    WU.history_free(case, (), fills=(), record=False)              # the pattern run alone
    failing = set()
    for fill in WU.FILLS:
        try:
            WU.history_free(case, (), fills=(fill,), record=False)
        except AssertionError as e:
            assert repr(fill) in str(e), str(e)                    # the failure names the fill
            failing.add(fill)
    assert failing == CONTROLS[kernel], (kernel.__name__, failing)


def test_history_free_passes_a_kernel_that_writes_before_it_reads_and_sees_a_changed_state():
    def good(placement="aligned"):
        A = F.Arena(CPU, [F.f32("x", X), F.out("y", (1,), torch.float32), F.state("acc", np.zeros(2, np.float32)), F.ws("ws", 4)],
                    band=BAND, placement=placement)
        A["ws"][:3] = A["x"].reshape(3, 2).max(dim=1).values
        A["y"][0] = A["ws"][:3].max()
        A["acc"].add_(A["y"][0])
        A.check("good")

    WU.history_free(good, (), record=False)

    def leaks_into_a_state(placement="aligned"):                    # no output changes, a state does, by less than any tolerance would see
        A = F.Arena(CPU, [F.state("acc", np.ones(2, np.float32)), F.out("y", (1,), torch.float32), F.ws("ws", 4)], band=BAND, placement=placement)
        A["y"][0] = 1.0
        A["acc"][1:2].add_(torch.nan_to_num(A["ws"][1], nan=0.0) * 1e-6)
        A["ws"][0] = 3.0

    with pytest.raises(WU.HistoryError) as e:
        WU.history_free(leaks_into_a_state, (), record=False)
    assert e.value.fill == "rolled" and e.value.found[0][:2] == (0, "acc") and e.value.found[0][3] >= 4, str(e.value)

    def no_workspace(placement="aligned"):
        F.Arena(CPU, [F.out("y", (1,), torch.float32)], band=BAND, placement=placement)

    with pytest.raises(AssertionError, match="no arena of this case holds a workspace"):
        WU.history_free(no_workspace, (), record=False)


def test_bit_equal():
    a = torch.tensor([0.0, 1.5, float("nan")])
    assert WU.bit_equal(a, a.clone()) and not WU.bit_equal(a, torch.tensor([-0.0, 1.5, float("nan")]))
    assert WU.bit_equal({"k": (a, 3, 0.5)}, {"k": (a.clone(), 3, 0.5)}) and not WU.bit_equal({"k": (a, 3)}, {"k": (a, 4)})
    assert not WU.bit_equal(0.0, -0.0) and not WU.bit_equal(1, 1.0) and not WU.bit_equal(a, a.double())
    assert WU.bit_equal(np.arange(3), np.arange(3)) and not WU.bit_equal(np.arange(3), np.arange(3.0))


# ------------------------------------------------------------------------------------------- the inputs of the per-image convergence cases
def test_the_thin_case_converges_at_another_launch_per_image():
    from tests import test_gpu_thin_fenced as GT
    from tests import thin_util as TU
    from road_segmentation_unet_amd import hostio
    prob, lab = GT.early_inputs()
    assert prob.shape == GT.EARLY_SHAPE and GT.EARLY_ITERS == 64 and (lab[1] == -1).any() and (lab[1] == 2).any()
    at = {i: hostio.mask_thin(prob, TU.THRESHOLD, lab, i) for i in (1, TU.K, 2 * TU.K, GT.EARLY_ITERS)}
    start = ((prob >= TU.THRESHOLD) & ((lab == 0) | (lab == 1))).astype(np.float32), np.where(lab == 1, 1, lab)
    for side in (0, 1):
        # image 0: something is deleted, and the fixed point is there when the first launch ends: its last iteration deleted nothing
        assert (at[1][side][0] != start[side][0]).any() and at[TU.K][3][0, side] == 0
        assert np.array_equal(at[TU.K][side][0], at[64][side][0])
        # image 1: the first and the second launch end in mid-flight; at 64 iterations it has long converged
        assert at[TU.K][3][1, side] > 0 and at[2 * TU.K][3][1, side] > 0 and at[64][3][1, side] == 0
        assert (at[2 * TU.K][side][1] != at[64][side][1]).any()
    assert at[64][2].min() > 20 and not at[64][3].any()              # what the fenced case asks of its counts and info


def test_the_graph_case_ends_its_delete_phase_at_another_launch_per_image_and_side():
    from tests import test_gpu_graph_fenced as GG
    from tests import graph_util as GU
    from road_segmentation_unet_amd import hostio
    prob, lab = GG.early_inputs()
    assert prob.shape == GG.EARLY_SHAPE and GU.MAX_BRANCH == 4 * GU.R and (lab[1] == -1).any() and (lab[1] == 2).any()
    pred = (prob >= GU.THRESHOLD) & ((lab == 0) | (lab == 1))
    true = lab == 1
    pruned = {L: (hostio.prune_mask(pred, L), hostio.prune_mask(true, L)) for L in (GU.R, 2 * GU.R, 3 * GU.R, GU.MAX_BRANCH)}
    P, T = 0, 1
    last = pruned[GU.MAX_BRANCH]
    # image 0, prediction: the spur is gone after one launch's rounds and stays gone; truth: outline unchanged, the lone line gone
    assert np.array_equal(pruned[GU.R][P][0], last[P][0]) and int(pred[0].sum()) - int(last[P][0].sum()) == 5
    assert np.array_equal(pruned[GU.R][T][0], last[T][0]) and int(true[0].sum()) - int(last[T][0].sum()) == 9
    # image 1, prediction: regrown to its full length, two ends; truth: the spur of 40 is lost, and only after the second launch's rounds
    assert np.array_equal(last[P][1], pred[1]) and int(pred[1].sum()) == 200
    assert int(true[1].sum()) - int(last[T][1].sum()) == 40 and not np.array_equal(pruned[2 * GU.R][T][1], last[T][1])
    assert np.array_equal(pruned[3 * GU.R][T][1], last[T][1])
    counts = hostio.skeleton_graph(prob, GU.THRESHOLD, lab, GU.MAX_BRANCH)[4]
    assert (counts[[0, 3, 4, 7]] > 0).all() and counts[1] == 2 and counts[5] == 0, counts


# ------------------------------------------------------------------------------------------- the registry covers the ten headers
def test_every_entry_with_a_workspace_is_run_under_every_fill_or_excused():
    from tests import test_gpu_ws_history as H
    protos = au.prototypes()
    takes_ws = lambda e: any("*" in t and n in ("ws", "kws") for t, n in protos[e][1])  # noqa: E731
    launching = [e for e in au.launching(protos) if takes_ws(e)]
    # (rsu_wgrad_group_plan takes no stream: it writes its ws into the table rsu_wgrad_group_run launches from)
    entries = sorted(launching + ["rsu_wgrad_group_plan"])
    assert len(launching) >= 30 and takes_ws("rsu_wgrad_group_plan") and entries == H.workspace_entries(), len(launching)
    for probe in ("rsu_conv2d_fwd_k", "rsu_conv2d_bwd_weight", "rsu_head_fwd_bwd", "rsu_grad_norm", "rsu_mask_thin", "rsu_line_segments", "rsu_color_jitter"):
        assert probe in entries, probe
    for e in entries:
        assert (e in H.HISTORY) != (e in H.NOT_RUN), "%s: in exactly one of HISTORY and NOT_RUN" % e
    assert set(H.HISTORY) | set(H.NOT_RUN) <= set(entries)
    for e, reason in H.NOT_RUN.items():
        assert isinstance(reason, str) and len(reason) > 20, e
    for e, ids in H.HISTORY.items():
        assert ids and set(ids) <= set(H.WS_CASES), e
        for cid in ids:
            assert cid in H.ALL and e in H.ALL[cid][3], (e, cid)      # (that e STARTS from a fill there is asserted when the case runs)
    assert set(H.NOT_RUN) == set(WU.CARRIED) == {"rsu_cldice_bwd"} and "cldice" in H.HISTORY["rsu_cldice_fwd"]
    # the cases: those of the minimum-placement file plus the two of the fenced files, every one a case function that takes a placement
    import inspect
    assert set(H.ALL) == set(H.M.CASES) | set(H.EXTRA) and not set(H.M.CASES) & set(H.EXTRA)
    for cid in H.WS_CASES:
        fn = H.ALL[cid][0]
        assert "placement" in inspect.signature(fn).parameters and fn.__module__.endswith("fenced"), cid
    assert set(H.WS_CASES) <= set(H.ALL) and len(set(H.WS_CASES)) == len(H.WS_CASES)
    for cid in ("thin", "thin_early", "graph", "graph_early", "heads", "wgrad_group", "conv_fwd_k", "bwd_data_k", "cldice", "lovasz"):
        assert cid in H.WS_CASES, cid
    for cid in ("conv_fwd", "pool_junction", "dropout", "tilers"):
        assert cid not in H.WS_CASES, cid


# ------------------------------------------------------------------------------------------- the fill reaches every call, not the first alone
def test_the_fill_is_put_back_in_front_of_every_call_that_receives_the_workspace():
    """refiller() on a CPU arena, through real entry points that refuse their arguments (npix = 0, B = 0: RSU_EINVAL before anything is
    launched or read): a workspace a first call has scribbled on is the fill again when the second call receives it; a call that receives no
    workspace changes nothing; rsu_cldice_bwd keeps what it is handed"""
    from road_segmentation_unet_amd._lib import lib
    import ctypes
    L = lib()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for fill in F.FILLS:
        A0, P0 = _arena("pattern")
        A0["ws"].copy_(torch.arange(N_WS, dtype=torch.float32))
        A, P = _arena(fill, P0.workspaces())
        start = A.payload_bytes("ws").clone()
        with WU.refiller(P) as r:
            L = lib()
            A["ws"].fill_(7.0)                                                      # what "the entry before" left
            assert L.rsu_maxpool2x2_fwd(ptr(A["x"]), ptr(A["y"]), 0, 4, 4, 8, 1.0, 0, None) != 0
            assert (A["ws"] == 7.0).all() and r.refilled == []                      # no workspace among its arguments
            assert L.rsu_cldice_bwd(ptr(A["acc"]), None, None, None, None, 3, 1.0, 1.0, None, ptr(A["ws"]), 0, 4, 4, None) != 0
            assert (A["ws"] == 7.0).all() and r.refilled == []                      # the one entry that reads what another left
            assert L.rsu_bias_grad(ptr(A["x"]), ptr(A["acc"]), ptr(A["ws"]), 0, 16, None) != 0
            assert torch.equal(A.payload_bytes("ws"), start) and r.refilled == [("rsu_bias_grad", 0, "ws")]
            A["ws"].fill_(9.0)
            assert L.rsu_bias_grad(ptr(A["x"]), ptr(A["acc"]), ptr(A["ws"]), 0, 16, None) != 0
            assert torch.equal(A.payload_bytes("ws"), start) and len(r.refilled) == 2
        assert [e for e, _ in r.calls] == ["rsu_maxpool2x2_fwd", "rsu_cldice_bwd", "rsu_bias_grad", "rsu_bias_grad"]
        A.check("refilling writes the payload alone")


def test_a_table_is_compared_with_its_addresses_as_arena_offsets():
    def table(value):
        A = F.Arena(CPU, [F.out("t", (44,), torch.uint8), F.ws("ws", 4)], band=BAND)
        w = A["t"][:40].view(torch.int64)
        w[:] = torch.tensor([A["ws"].data_ptr(), value, A.mem.data_ptr() + A.total - 1, A.mem.data_ptr() + A.total, -1])
        A["t"][40:] = 5
        return A
    a, b = table(12345), table(12345)
    assert not torch.equal(a["t"], b["t"])
    (ra, na), (rb, nb) = WU.rebased(a.payload_bytes("t"), a), WU.rebased(b.payload_bytes("t"), b)
    assert na == nb == 2 and ra.numel() == 44 and int(ra[:8].view(torch.int64)[0]) == a.place["ws"][0]
    # the two addresses inside the arena agree as offsets; the word one past the arena's end is no address of it and still differs
    assert torch.equal(ra[:24], rb[:24]) and torch.equal(ra[32:], rb[32:]) and not torch.equal(ra[24:32], rb[24:32])
    assert not torch.equal(WU.rebased(table(12346).payload_bytes("t"), a)[0][8:16], ra[8:16])      # a plain field is still compared


@pytest.mark.parametrize("mode", ["aligned", "minimum"])
@pytest.mark.parametrize("fill", F.FILLS)
def test_refill_restores_the_starting_bytes_at_any_address_and_size(fill, mode):
    """Arena.refill: the workspace as the arena was built, an odd byte count at an odd address (minimum placement of bytes) and a
    workspace larger than every band included; nothing around it changes"""
    def build(f, snaps=None):
        P = F.Placement(mode, fill=f, snapshots=snaps)
        return F.Arena(CPU, [F.out("y", (3,), torch.float32), F.ws("b", 7, torch.uint8), F.ws("big", 3 * BAND, torch.uint8, band=BAND)],
                       band=BAND, placement=P), P
    A0, P0 = build("pattern")
    A0["b"].copy_(torch.arange(7, dtype=torch.uint8))
    A0["big"].copy_((torch.arange(3 * BAND) % 251).to(torch.uint8))
    A, _ = build(fill, P0.workspaces())
    assert A.place["b"][0] % 2 == (1 if mode == "minimum" else 0)
    start = {n: A.payload_bytes(n).clone() for n in ("b", "big")}
    if fill == "pattern":
        for n, t in start.items():       # the arena's 0x7FA5 words lie on even offsets, low byte first
            odd = (torch.arange(t.numel()) + A.place[n][0]) % 2 == 1
            assert (t[odd] == 0x7F).all() and (t[~odd] == 0xA5).all(), n
    for n in start:
        A[n].fill_(0x3C)
        A.refill(n)
        assert torch.equal(A.payload_bytes(n), start[n]), n
    A.check("refill")
    with pytest.raises(AssertionError):
        A.refill("y")
