"""-m gpu: include/rsu_routes.h against the host restatements hostio.graph_routes and hostio.route_score (which tests/test_routes_host.py
holds to scipy's shortest paths and to hand cases): both entries over the thinned bank of tests/segments_util.py, both sides and both
score directions; direct inputs (line ends and hand-written rows) with node counts around the 64-node blocks; max_nodes that is no
multiple of 64 and one below the bank's node counts; an empty image beside a full one; one pixel and one row of tiles; max_edges below
the count; acc over two calls; ConvolutionalModel.evaluate() with --validate_routes, road_graph(distances=True) and the command line's
--road_graph_distances above them. Every comparison is equality of the bytes."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import graph_util as GU  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests import routes_util as RU  # noqa: E402
from tests import segments_util as SU  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402

RT_KEYS = {"apls_true_to_pred", "apls_pred_to_true", "apls", "graph_nodes_pred", "graph_nodes_true", "graph_nodes_dropped_pred",
           "graph_nodes_dropped_true"} | {"route_%s_%s" % (k, d) for k in ("pairs", "unmatched", "broken") for d in ("true_to_pred", "pred_to_true")}


def _both(name, shape, L, max_nodes, what):
    """both sides' graphs on the device against the restatement, then both score directions"""
    got, want = [], []
    for side in (0, 1):
        w = RU.bank_host(name, shape, L, side, max_nodes)
        g, _ = RU.check(*RU.bank_inputs(name, shape, L, side), side, max_nodes, what + (side,), want=w)
        got.append(g)
        want.append(w)
    for a in (0, 1):
        RU.check_score(got[a], got[1 - a], RU.bank_score(name, shape, L, a, max_nodes), what + ("score", a))
    return want


# ------------------------------------------------------------------------------------------- the bank
@pytest.mark.parametrize("L", SU.PRUNES)
@pytest.mark.parametrize("shape", RU.SHAPES, ids=SU.shape_id)
def test_both_entries_equal_the_host_over_the_bank(shape, L):
    most = pairs = 0
    for name in RU.BANK:
        want = _both(name, shape, L, RU.MAX_NODES, (name, shape, L))
        most = max(most, max(int(w[2][:, 0].max()) for w in want))
        pairs += int(RU.bank_score(name, shape, L, 0)[1][0])
    assert most > (40 if shape[1] == 64 and L else 128) and pairs > 0, (most, pairs)      # one block only in the smallest pruned case


# ------------------------------------------------------------------------------------------- direct inputs
@pytest.mark.parametrize("kind", sorted(RU.DIRECT_KINDS))
@pytest.mark.parametrize("count", RU.DIRECT_COUNTS)
def test_direct_inputs(kind, count):
    m, e, c = RU.direct_case(kind, count)
    for max_nodes in sorted({256, count, max(count - 1, 1)}):
        got, want = RU.check(m, e, c, 0, max_nodes, (kind, count, max_nodes))
        assert want[2][0, :2].tolist() == [count, min(count, max_nodes)]
    D = want[1][0, :count, :count]
    assert np.array_equal(D, RU.reference_distances(count, RU.DIRECT_KINDS[kind](count)))
    assert not (kind == "chain" and (D == RU.INF).any()) and not (kind == "split" and count > 1 and not (D == RU.INF).any())
    RU.check_score(got, got, RU.host_score(want, want), (kind, count, "self"))


# ------------------------------------------------------------------------------------------- max_nodes
def test_max_nodes_that_is_no_multiple_of_the_tile():
    """100 nodes' room: masked loads and stores in the second block; the bank's 139 and 115 nodes do not fit, its 77 and 79 do"""
    name, shape = "smooth1.5~smooth3", (2, 230, 97)
    for L in SU.PRUNES:
        want = _both(name, shape, L, 100, (name, shape, L, 100))
        assert want[0][2][:, 1].tolist() == [100, 100] and want[1][2][:, 1].tolist() == ([100, 100], [77, 79])[L > 0]


def test_max_nodes_below_the_node_count():
    """256 rows for 404 and 395 nodes: nodes are dropped, rows skipped, and everything past the stored count keeps its fill"""
    name, shape = "smooth1.5~smooth3", (2, 230, 97)
    want = _both(name, shape, 0, 256, (name, shape, 0, 256))
    info = want[0][2]
    assert info[:, 0].tolist() == [404, 395] and info[:, 1].tolist() == [256, 256] and (info[:, 3] > 50).all() and (info[:, 2] > 50).all()
    assert want[1][2][:, 1].tolist() == [139, 115] and (want[1][1][0, 139:] == RU.FILL).all() and (want[1][1][0, :, 139:] == RU.FILL).all()


# ------------------------------------------------------------------------------------------- shapes and batches
def test_an_empty_image_beside_a_full_one():
    name, shape = "smooth1.5~smooth3", (2, 230, 97)
    for empty in (0, 1):
        m, e, c = (np.array(a) for a in RU.bank_inputs(name, shape, 8, 0))
        m[empty], c[empty] = 0, 0
        got, want = RU.check(m, e, c, 0, 256, ("empty", empty))
        assert want[2][empty].tolist() == [0, 0, 0, 0] and want[2][1 - empty, 0] > 190 and (want[1][empty] == RU.FILL).all()
        match, acc = RU.host_score(want, want)
        assert (match[empty] == RU.FILL).all() and acc[0] > 1000
        RU.check_score(got, got, (match, acc), ("empty", empty, "score"))


def test_one_pixel_and_one_row_of_tiles():
    one = (np.array([[[-1]]], np.int32), np.full((1, 1, 8), SU.FILL, np.int32), np.array([[1, 0, 0, 0]], np.int32))
    one[1][0, 0] = (1, 1, 0, 0, -1, -1, 0, 1)      # an isolated pixel: a node without an edge
    got, want = RU.check(*one, 0, 1, "one pixel")
    assert want[0].tolist() == [[[-1, 0, 0, 1]]] and want[1].tolist() == [[[0]]] and want[2].tolist() == [[1, 1, 0, 0]]
    RU.check(np.zeros((1, 1, 1), np.int32), one[1], np.zeros((1, 4), np.int32), 0, 1, "one empty pixel")
    shape = (1, 3, 1024)
    seen = 0
    for name in RU.BANK:
        for side in (0, 1):
            inp = RU.bank_inputs(name, shape, 0, side)
            got, want = RU.check(*inp, side, 64, (name, shape, side))
            seen += int(want[2][0, 0])
    assert seen > 20


def test_max_edges_below_the_count():
    name, shape = "smooth1.5~smooth3", (2, 230, 97)
    m, e, c = RU.bank_inputs(name, shape, 8, 1)
    full = RU.bank_host(name, shape, 8, 1, 256)
    assert int(c[:, 2].min()) > 40
    got, want = RU.check(m, np.array(e[:, :20]), c, 1, 256, "twenty rows")
    assert (want[2][:, 2] <= 20).all() and (want[2][:, 2] < full[2][:, 2]).all() and np.array_equal(want[0], full[0])
    assert (want[1] == RU.INF).sum() > (full[1] == RU.INF).sum()


def test_acc_accumulates_over_two_calls():
    name, shape = "smooth1.5~smooth3", (2, 230, 97)
    g = [RU.run_routes(*(RU.dev(a) for a in RU.bank_inputs(name, shape, 8, side)), side, 256) for side in (0, 1)]
    want = [RU.bank_score(name, shape, 8, a, 256)[1] for a in (0, 1)]
    assert want[0][0] > 1000 and want[1][0] > 100 and want[0][1] > 0
    match, acc = RU.run_score(g[0], g[1])
    assert acc.cpu().numpy().tolist() == want[0].tolist()
    RU.run_score(g[1], g[0], acc=acc)
    assert acc.cpu().numpy().tolist() == (want[0] + want[1]).tolist()
    again = torch.tensor([1, 2, 3, 4], dtype=torch.int64, device=hu.DEV)      # what acc held stays in it
    RU.run_score(g[0], g[1], acc=again)
    assert again.cpu().numpy().tolist() == (want[0] + np.array([1, 2, 3, 4])).tolist()
    first = [t.cpu().numpy().tobytes() for t in g[0]]      # two runs, byte for byte
    assert [t.cpu().numpy().tobytes() for t in RU.run_routes(*(RU.dev(a) for a in RU.bank_inputs(name, shape, 8, 0)), 0, 256)] == first


# ------------------------------------------------------------------------------------------- evaluate(), road_graph(), the command line
def _host_routes(chunks, thr, max_iters, min_branch, max_edges, max_nodes, snap):
    """mask_thin -> skeleton_graph -> line_segments -> graph_routes per side -> route_score per direction: what evaluate() must return"""
    acc, info = np.zeros((2, 4), np.int64), np.zeros(8, np.int64)
    for prob, yb in chunks:
        sp, st, _, _ = hostio.mask_thin(prob, thr, yb, max_iters)
        op, ot = hostio.skeleton_graph(sp, 0.5, st, min_branch)[:2] if min_branch else (sp, st)
        seg = hostio.line_segments(op, 0.5, ot, max_edges)
        g = [hostio.graph_routes(seg[5 + side], seg[side], seg[2], side, max_nodes) for side in (0, 1)]
        for side in (0, 1):
            info[4 * side:4 * side + 4] += g[side][2].sum(axis=0)
        acc[0] += hostio.route_score(*g[1], *g[0], snap)[1]
        acc[1] += hostio.route_score(*g[0], *g[1], snap)[1]
    return hostio.route_metrics(acc[0], acc[1], info)


def test_evaluate_with_routes(monkeypatch):
    from road_segmentation_unet_amd import mask_metrics as M      # (it issues the calls)
    from tests import test_gpu_graph as TG
    N = 5
    X, y = TG._patches(N)
    y[1, :3] = -1
    kw = dict(validate_centerlines=True, centerline_min_branch=2, validate_segments=True, relaxed_slack=2)
    m = TG._model(validate_routes=True, **kw)
    chunks = TG._chunks(m, X, y)
    thr = round(float(np.median(np.concatenate([c[0].reshape(-1) for c in chunks]))) * 256.0) / 256.0
    calls = []
    real = M.call
    monkeypatch.setattr(M, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    out = m.evaluate(X, y, threshold=thr)
    assert calls.count("rsu_line_segments") == 3 and calls.count("rsu_graph_routes") == 6 and calls.count("rsu_route_score") == 6
    want = _host_routes(TG._chunks(m, X, y), thr, 64, 2, 4096, 256, 8)
    assert want["graph_nodes_true"] > 0 and want["route_pairs_true_to_pred"] > 0 and want["graph_nodes_dropped_true"] == 0
    assert RT_KEYS <= set(out) and {k: out[k] for k in RT_KEYS} == want
    assert {k: m.evaluate(X, y, threshold=thr)[k] for k in RT_KEYS} == want          # again: the counters are zeroed per pass
    # a table of four nodes per patch and another snap: the rest is counted as dropped
    small = TG._model(validate_routes=True, max_graph_nodes=4, route_snap=3, **kw)
    got = small.evaluate(X, y, threshold=thr)
    want2 = _host_routes(TG._chunks(small, X, y), thr, 64, 2, 4096, 4, 3)
    assert {k: got[k] for k in RT_KEYS} == want2 and want2["graph_nodes_dropped_true"] > 0
    # _validate returns the scalars, and --save_best_metric=apls selects on them
    best = TG._model(validate_routes=True, save_best_metric="apls", **kw)
    got = best._validate((X, y), 1)
    assert RT_KEYS <= set(got) and got["apls"] == best.evaluate(X, y)["apls"] and best.best_val_score == got["apls"]
    # the flag off: the parent's calls, buffers and keys, and nothing else
    del calls[:]
    plain_model = TG._model(**kw)
    plain = plain_model.evaluate(X, y, threshold=thr)
    mm = plain_model._mask_metrics
    assert "rsu_graph_routes" not in calls and "rsu_route_score" not in calls and "routes" not in mm.lay and not RT_KEYS & set(plain)
    assert sorted(mm.ws) == sorted(["thin", "dist", "skel_pred", "skel_true", "info", "graph", "segments", "edges_pred", "edges_true", "counts"])
    assert set(out) - set(plain) == RT_KEYS and all(np.array_equal(out[k], plain[k]) for k in plain)
    assert set(m._mask_metrics.ws) - set(mm.ws) == {"routes", "match"} | {"%s_%s" % (a, b) for a in ("node", "rt_nodes", "rt_dist", "rt_info")
                                                                         for b in ("pred", "true")}


def test_road_graph_with_distances_and_without(monkeypatch):
    from road_segmentation_unet_amd import mask_metrics as M
    from tests import test_gpu_graph as TG
    calls = []
    real = M.call
    monkeypatch.setattr(M, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    shape = (2, 230, 97)
    prob = np.array(GU.pair("smooth1.5~smooth3", shape, False)[0])
    model = TG._model(centerline_min_branch=8)
    plain = model.road_graph(prob, threshold=0.5)
    assert calls == ["rsu_mask_thin", "rsu_skeleton_graph", "rsu_line_segments"]      # the flag off: nothing new is called or returned
    assert all(list(g) == ["nodes", "edges", "segments"] for g in plain) and model.road_graph(prob, threshold=0.5, distances=False) == plain
    skel = hostio.skeleton_graph(hostio.mask_thin(prob, 0.5, None, 64)[0], 0.5, None, 8)[0]
    ref = hostio.line_segments(skel, 0.5, None, 4096)
    for cap, g in ((256, model.road_graph(prob, threshold=0.5, distances=True)),
                   (50, TG._model(centerline_min_branch=8, road_graph_distances=True, max_graph_nodes=50).road_graph(prob, threshold=0.5))):
        assert calls[-1] == "rsu_graph_routes" and calls.count("rsu_route_score") == 0
        nodes, dist, info = hostio.graph_routes(ref[5], ref[0], ref[2], 0, cap)
        for n in range(2):
            k = int(info[n, 1])
            assert list(g[n]) == ["nodes", "edges", "segments", "node_index", "nodes_dropped", "distances"]
            assert {q: g[n][q] for q in plain[n]} == plain[n]
            assert g[n]["node_index"] == nodes[n, :k, 0].tolist() and g[n]["nodes_dropped"] == int(info[n, 0]) - k and (k == 50) == (cap == 50)
            assert g[n]["distances"] == [[None if v >= RU.INF else int(v) / 70.0 for v in row] for row in dist[n, :k, :k]]
            if cap == 256:      # the table's ids are the graph's node ids, in ascending |id|
                assert sorted(g[n]["node_index"], key=abs) == g[n]["node_index"] and set(g[n]["node_index"]) == {v["id"] for v in g[n]["nodes"]}
                assert any(v is None for row in g[n]["distances"] for v in row) and any(v for row in g[n]["distances"] for v in row)


def test_cli_save_road_graph_with_and_without_distances(tmp_path):
    from PIL import Image
    from road_segmentation_unet_amd.cli import main
    rng = np.random.RandomState(4)
    ev = tmp_path / "eval"
    ev.mkdir()
    H, W = 48, 40
    for i in range(2):
        Image.fromarray((rng.rand(H, W, 3) * 255).astype(np.uint8)).save(ev / ("test_%d.png" % i))
    argv = ["--num_layers=2", "--root_size=16", "--patch_size=16", "--stride=16", "--batch_size=4", "--num_epoch=0", "--eval_data_dir=%s" % ev,
            "--pred_batch_size=2", "--seed=5", "--logdir=", "--centerline_max_iters=32", "--centerline_min_branch=2", "--save_road_graph",
            "--max_segments=64"]

    def run(name, extra):
        save = tmp_path / name
        assert main(argv + ["--save_path=%s" % save] + extra) == 0
        d = [d for d in os.listdir(save) if os.path.isdir(save / d)]
        files = sorted(f for f in os.listdir(save / d[0]) if f.startswith("graph_"))
        assert len(d) == 1 and files == ["graph_001.json", "graph_002.json"]
        return [open(save / d[0] / f).read() for f in files]

    off = run("off", [])
    on = run("on", ["--road_graph_distances", "--max_graph_nodes=64"])
    assert run("off2", ["--max_graph_nodes=7", "--route_snap=2"]) == off      # without the flag its companions change nothing
    for a, b in zip(off, on):
        a, b = json.loads(a), json.loads(b)
        assert list(a) == ["nodes", "edges", "segments"] and list(b) == list(a) + ["node_index", "nodes_dropped", "distances"]
        assert {k: b[k] for k in a} == a and b["nodes_dropped"] == 0 and set(b["node_index"]) == {v["id"] for v in a["nodes"]}
        k = len(b["node_index"])
        assert len(b["distances"]) == k and all(len(row) == k for row in b["distances"]) and all(b["distances"][i][i] == 0 for i in range(k))
