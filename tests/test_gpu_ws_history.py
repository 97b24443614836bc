"""-m gpu: no result depends on what a workspace held before the call, nor on what a net or a model did before the step.

Entry level. Every case of test_gpu_aligned_min.CASES whose arenas hold a workspace runs through ws_util.history_free: once with its
workspaces as pattern (the fenced files' own run), then with every byte 0x00, every byte 0xFF, and with the workspaces' own leftovers
rolled by a third -- one parameter per (case, fill), so a failure names the fill. The fill is put back in front of EVERY library call
that receives the workspace, so each entry of a case starts from it, not from what the entry before left for the same input. Each run
makes the case's own assertions; on top of them every output and state must hold the very bytes of the pattern run. The thin and graph families add a case each whose first image
converges inside the first step launch while the second does not (their counters differ per image and per launch: rolled, a stale 0
lands where a launch ran and a stale count where one returned at once).

Net level. A UNet step and a ConvolutionalModel evaluation are compared with the same step on a FRESH net built from the same seed:
tests/test_gpu_soak.py compares two runs of one sequence, and a buffer that leaks from step k into step k + 1 leaks the same way in
both. Then once more with every workspace tensor the net owns overwritten between the steps (0xFF bytes, and a roll of its own contents).

HISTORY / NOT_RUN are the registry tests/test_ws_history_host.py checks against the ten headers without a GPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import test_gpu_aligned_min as M  # noqa: E402
from tests import test_gpu_graph_fenced as GG  # noqa: E402
from tests import test_gpu_thin_fenced as GT  # noqa: E402
from tests import ws_util as WU  # noqa: E402

# the cases of this file beside those of test_gpu_aligned_min.CASES: id -> (case function, arguments, environment, entries)
EXTRA = {
    "thin_early": (GT.test_thin_converges_per_image, (), {}, ["rsu_mask_thin"]),
    "graph_early": (GG.test_graph_converges_per_image, (), {}, ["rsu_skeleton_graph"]),
}
ALL = dict(M.CASES, **EXTRA)
# the cases whose arenas hold a workspace (fence_util.ws); test_the_other_cases_hold_no_workspace builds the arenas of every other case
# and finds none, history_free refuses a case without one
WS_CASES = ("aux_head", "bias_grad", "border_map", "bwd_data_k", "bwd_weight", "bwd_weight_cropped_odd_ox_C8", "cldice", "color_jitter",
            "components", "convT", "convT_gen1", "conv_fwd_k", "conv_fwd_pool_k", "distance", "first_layer", "focal_heads", "graph",
            "graph_early", "heads", "lovasz", "optimizer_passes", "segments", "tables_adam", "tables_adam_clip", "tables_adam_decay",
            "tables_decay", "tables_momentum", "tables_momentum_clip", "thin", "thin_early", "wgrad_group")
# outputs that hold device addresses of their own arena's payloads (the tables of the table-driven launches, copied from the host table):
# every run builds its arenas elsewhere, so they are compared with those addresses turned into arena offsets (ws_util.rebased)
ADDRESSES = dict({cid: ("utable", "ptable") for cid in ("tables_momentum", "tables_adam", "tables_momentum_clip", "tables_adam_clip")},
                 tables_decay=("utable",), tables_adam_decay=("utable",), wgrad_group=("table",))


def workspace_entries():
    """the `int rsu_*` entries of the ten headers with a pointer argument named ws or kws: the launching ones, and rsu_wgrad_group_plan,
    which launches nothing and hands its ws to rsu_wgrad_group_run inside the table"""
    protos = M.au.prototypes()
    return sorted(e for e in protos if protos[e][0] == "int" and WU.takes_a_workspace(e, protos))


# entry -> the case ids in which it STARTS from the fill: history_free puts the fill back into a workspace in front of every call that
# receives it, and fails a case if an entry named here received none
HISTORY = {}
NOT_RUN = {"rsu_cldice_bwd": "it reads the maps rsu_cldice_fwd left in ws (rsu_cldice.h) and cannot start from a fill: the cldice case "
                             "runs it behind a forward that does, under every fill, and compares gprob"}
_WS_ENTRIES = set(workspace_entries())
for _cid in WS_CASES:
    for _e in ALL[_cid][3]:
        if _e in _WS_ENTRIES and _e not in NOT_RUN:
            HISTORY.setdefault(_e, []).append(_cid)
assert set(NOT_RUN) == set(WU.CARRIED)


def _run(case, monkeypatch, capfd, through):
    fn, args, env, entries = ALL[case]
    M._env(monkeypatch, **env)
    fixtures = {"monkeypatch": monkeypatch, "capfd": capfd}
    kw = dict(M._KEYWORDS.get(case, {}))
    if case == "bwd_data_k":
        kw["capfd"] = capfd
    return through(fn, entries, *args, *[fixtures[f] for f in M._FIXTURES.get(case, ())], **kw)


@pytest.mark.parametrize("fill", WU.FILLS)
@pytest.mark.parametrize("case", WS_CASES)
def test_entry_does_not_read_what_its_workspace_held(case, fill, monkeypatch, capfd):
    started = _run(case, monkeypatch, capfd, lambda fn, entries, *a, **kw: WU.history_free(fn, entries, *a, fills=(fill,),
                                                                                           addresses=ADDRESSES.get(case, ()), **kw))
    for entry, ids in HISTORY.items():
        assert case not in ids or entry in started, (entry, started)


@pytest.mark.parametrize("case", sorted(set(ALL) - set(WS_CASES)))
def test_the_other_cases_hold_no_workspace(case, monkeypatch, capfd):
    """WS_CASES leaves no case with a workspace out: the arenas every other case builds hold none"""
    def through(fn, entries, *a, **kw):
        from tests import fence_util as F
        p = F.Placement("aligned")
        fn(*a, placement=p, **kw)
        return p
    p = _run(case, monkeypatch, capfd, through)
    assert p.arenas and not p.workspaces(), sorted(p.workspaces())


# =========================================================================================== net level: a step on a used net
NETS = {
    "dilated": (3, 16, True, 2, 60, {}),       # twin blocks, three-source decoder convs, backward-data in its accumulate mode
    "plain": (2, 16, False, 2, 20, {}),
    "every_term": (2, 16, False, 2, 20, dict(class_weights=(0.75, 1.5), dice_weight=0.5, border_weight=2.0, border_sigma=3.0, focal_gamma=1.5,
                                             cldice_weight=0.4, cldice_iters=3, lovasz_weight=0.3)),
}


def _net(kind):
    from road_segmentation_unet_amd.unet import UNet
    L, root, dilated, B, P, kw = NETS[kind]
    return UNet(L, root, dilated, B, P, seed=29, training=True, **kw)


def _batches(kind):
    """(X1, Y1), (X2, Y2), (X3, Y3): sparse labels (with ignored pixels where the net's head takes them: a weighted pass), an
    all-background batch, dense labels"""
    L, root, dilated, B, P, kw = NETS[kind]
    from road_segmentation_unet_amd.unet import input_size_needed
    S = input_size_needed(P, L)
    g = torch.Generator(device="cpu").manual_seed(41)
    out = []
    for density in (0.15, 0.0, 0.6):
        x = torch.rand((B, S, S, 3), generator=g)
        y = (torch.rand((B, P, P), generator=g) < density).to(torch.int64)
        out.append((x, y))
    if kw:
        out[0][1][0, 3:6, 2:9] = -1
        out[0][1][1, 0, :] = 2
        out[2][1][1, 7:9, 5:P] = -1
    assert not out[1][1].any() and 0.1 < float((out[0][1] == 1).float().mean()) < 0.2 and float((out[2][1] == 1).float().mean()) > 0.5
    return out


def _step(net, batch):
    """one forward and backward pass, no optimizer call: the probabilities, the loss scalars and every gradient"""
    x, y = batch
    net.x.copy_(x)
    net.labels.copy_(y)
    net.forward_device(keep=1.0)
    net.backward_device(1.0 / (net.B * net.P * net.P))
    torch.cuda.synchronize()
    out = {"prob": net.prob.clone(), "loss_sum": net.loss_sum.clone(), "weight_sum": net.weight_sum.clone(), "dice_sums": net.dice_sums.clone(),
           "flat_g": net.flat_g.clone()}
    for k in ("cldice_sums", "lovasz_sum"):
        if getattr(net, k) is not None:
            out[k] = getattr(net, k).clone()
    assert bool(torch.isfinite(out["flat_g"]).all()) and bool(out["flat_g"].any()) and bool(torch.isfinite(out["loss_sum"]).all())
    return out


def _workspaces(net):
    """every workspace tensor the net owns, each once"""
    ts = [net.ws] + list(net.sched.ws_side) + [net.sched.kws] + list(net.sched.kws_side)
    ts += [getattr(net, k, None) for k in ("_cldice_ws", "_lovasz_ws", "_border_ws")]
    seen, out = set(), []
    for t in ts:
        if t is not None and t.numel() and t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            out.append(t)
    return out


def _scribble(net, how):
    torch.cuda.synchronize()
    for t in _workspaces(net):
        flat = t.reshape(-1)
        if how == "ones":
            flat.view(torch.uint8).fill_(0xFF)
        else:
            flat.copy_(torch.roll(flat, (flat.numel() // 3) | 1))
    torch.cuda.synchronize()


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    bad = [k for k in sorted(a) if not WU.bit_equal(a[k], b[k])]
    assert not bad, "%s: %s differ" % (what, bad)


@pytest.mark.parametrize("kind", sorted(NETS))
def test_a_step_does_not_depend_on_what_the_net_did_before(kind):
    b1, b2, b3 = _batches(kind)
    used = _net(kind)
    assert len(_workspaces(used)) >= (5 if kind == "every_term" else 2), [tuple(t.shape) for t in _workspaces(used)]
    r1 = _step(used, b1)
    r2 = _step(used, b2)
    r3 = _step(used, b3)
    assert not WU.bit_equal(r1["flat_g"], r3["flat_g"]) and not WU.bit_equal(r2["prob"], r3["prob"])
    fresh = _step(_net(kind), b3)
    _same(r3, fresh, "%s: the third step of a used net against the same step of a fresh one" % kind)
    for how in ("ones", "rolled"):
        _scribble(used, how)
        _same(_step(used, b1), r1, "%s: step 1 over workspaces overwritten with %s" % (kind, how))
        _scribble(used, how)
        _same(_step(used, b2), r2, "%s: step 2 over workspaces overwritten with %s" % (kind, how))
        _scribble(used, how)
        _same(_step(used, b3), fresh, "%s: step 3 over workspaces overwritten with %s" % (kind, how))


# =========================================================================================== model level: evaluate() and the mask tools
MODEL = dict(validate_components=True, validate_distances=True, validate_centerlines=True, centerline_min_branch=8, validate_junctions=True,
             validate_segments=True, min_road_area=6, max_hole_area=5)
MASK_SHAPE = (2, 130, 70)      # two row tiles of the thinning step, three word columns


def _model():
    from tests import test_gpu_graph as TG
    return TG._model(**MODEL)


def _eval_sets():
    """(X1, Y1): three patches (the last chunk of two is padded), faint inputs, the truth a few thin lines; (X2, Y2): four patches, the
    truth dense blobs with a few ignored pixels"""
    from tests import test_gpu_graph as TG
    X2, y2 = TG._patches(4, seed=33)
    y2 = y2.copy()
    y2[1, :3] = -1
    X1 = TG._patches(3, seed=34)[0] * np.float32(0.05)
    y1 = np.zeros((3, TG.MP, TG.MP), np.int64)
    y1[:, 9, 2:18] = 1
    y1[0, 3:17, 5] = 1
    assert y2.shape == (4, TG.MP, TG.MP) and float((y2 == 1).mean()) > 3 * float((y1 == 1).mean())
    return (X1, y1), (X2, y2)


def test_an_evaluation_does_not_depend_on_the_one_before():
    (X1, y1), (X2, y2) = _eval_sets()
    used = _model()
    first = used.evaluate(X1, y1)
    second = used.evaluate(X2, y2)
    fresh = _model().evaluate(X2, y2)
    assert {"dist_hist", "cl_hist", "jn_hist", "components_pred", "segments_true", "thin_unconverged", "sums", "hist"} <= set(fresh), sorted(fresh)
    assert not WU.bit_equal(first["hist"], fresh["hist"]) and fresh["cl_hist"].any() and fresh["segments_true"] > 0
    _same(second, fresh, "evaluate() behind another evaluation against a fresh model's")
    _same(used.evaluate(X1, y1), first, "evaluate() of the first set again, behind the second")


def _masks():
    """sparse: bars three pixels thick, at their fixed point within the first thinning launch; dense: smooth blobs and noise"""
    from tests import components_util as CU
    from tests import thin_util as TU
    sparse = np.zeros(MASK_SHAPE, bool)
    sparse[0, 20:23, 5:60] = sparse[0, 30:120, 40:43] = sparse[1, 64:67, 3:66] = True
    dense = TU.masks("smooth3", MASK_SHAPE) | TU.masks("rand0.3", MASK_SHAPE)
    return CU.prob_of(sparse), CU.prob_of(np.ascontiguousarray(dense))


def _empty_that_holds(how, log):
    """torch.empty, but every device tensor it returns holds `how`: 0xFF bytes, zeros, or noise. The mask tools take their workspaces
    from torch.empty, that is from the caching allocator: what such a block holds is whatever an earlier tensor left, which a test
    cannot choose by calling the tool twice. This chooses it."""
    real = torch.empty

    def empty(*args, **kw):
        t = real(*args, **kw)
        if t.is_cuda and t.numel():
            raw = t.reshape(-1).view(torch.uint8)
            if how == "noise":
                raw.copy_(torch.randint(0, 256, (raw.numel(),), dtype=torch.uint8, device=t.device, generator=log["rng"]))
            else:
                raw.fill_(0xFF if how == "ones" else 0)
            log["filled"] += 1
        return t
    return empty


@pytest.mark.parametrize("tool", ["centerlines", "road_graph", "postprocess_masks"])
def test_a_mask_tool_does_not_depend_on_the_call_before(tool, monkeypatch):
    """the same masks behind a call on other masks of the same shape, on a fresh model, and with every torch.empty block the tool takes
    (its workspaces, and outputs it writes in full) holding 0xFF bytes, zeros and noise: the same bytes each time"""
    sparse, dense = _masks()
    if tool == "postprocess_masks":
        sparse, dense = sparse[..., None], dense[..., None]
    used = _model()
    first = getattr(used, tool)(sparse)
    second = getattr(used, tool)(dense)
    fresh = getattr(_model(), tool)(dense)
    assert WU.bit_equal(second, fresh), "%s behind a call on other masks of the same shape against a fresh model's" % tool
    assert WU.bit_equal(getattr(used, tool)(sparse), first) and not WU.bit_equal(first, fresh), tool
    for how in ("ones", "zeros", "noise"):
        log = {"filled": 0, "rng": torch.Generator(device="cuda").manual_seed(3)}
        with monkeypatch.context() as mp:
            mp.setattr(torch, "empty", _empty_that_holds(how, log))
            got = getattr(used, tool)(dense)
        # (the components workspace and stats; the thin and graph workspaces; those two and the segments workspace)
        assert log["filled"] >= (3 if tool == "road_graph" else 2), (tool, log["filled"])
        assert WU.bit_equal(got, fresh), "%s with its torch.empty blocks holding %s" % (tool, how)
    if tool == "postprocess_masks":
        assert used.last_postprocess_stats is not None and (fresh != dense).any()      # the clean-up did something
    elif tool == "centerlines":
        assert 0 < fresh.sum() < (dense >= 0.5).sum()
    else:
        assert len(fresh) == MASK_SHAPE[0] and all(g["segments"] > 0 for g in fresh)
