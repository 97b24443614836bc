"""-m gpu: include/rsu_paths.h against the host restatement hostio.segment_paths (which tests/test_paths_host.py holds to the header's
promises with links formed apart from it): rsu_segment_paths over the thinned pairs of tests/segments_util.py pruned at L in {0, 8}, both
sides, at shapes from one pixel to sixteen tiles in a row; hand masks (single pixels, rings on tile and block borders, a branched block,
serpentines at and one past max_len, chains across tiles and images); truncation at max_edges and at max_points; pos = NULL; two runs
byte for byte; ConvolutionalModel.road_graph() with --road_graph_paths and the command line above it. Every comparison is equality of the
bytes; elements the entry does not touch must keep the fill they started with."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import graph_util as GU  # noqa: E402
from tests import paths_util as PU  # noqa: E402
from tests import segments_util as SU  # noqa: E402
from tests import thin_util as TU  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402


# ------------------------------------------------------------------------------------------- the bank
@pytest.mark.parametrize("L", SU.PRUNES)
@pytest.mark.parametrize("shape", SU.SHAPES, ids=[SU.shape_id(s) for s in SU.SHAPES])
def test_segment_paths_equal_the_host_over_the_thinned_bank(shape, L):
    kinds = np.zeros(3, np.int64)
    for name in TU.pair_names():
        for side in (0, 1):      # side 1: the truth's segments
            seg, edges, counts = PU.bank_inputs(name, shape, L, side)
            want = PU.bank_host(name, shape, L, side)
            PU.check(seg, edges, counts, side, PU.MAX_LEN, shape[1] * shape[2], (name, shape, L, side), want=want)
            kinds += want[4][:, 1:].sum(axis=0)
    if min(shape[1:]) > 8:   # the cases are not trivial
        assert kinds[0] > 50 and kinds[2] > 0, kinds


# ------------------------------------------------------------------------------------------- hand masks
def test_hand_masks():
    for name, mask in PU.hand_cases().items():
        seg, edges, counts = PU.inputs_of(mask)
        got, want = PU.check(seg, edges, counts, 0, 4096, mask.shape[1] * mask.shape[2], name)
        assert want[4][:, 1:].sum() == counts[:, 0].sum() > 0, name
    small = PU.host(*PU.inputs_of(PU.hand_cases()["small"]), 0, 4096, 12 * 16)
    assert small[2][:, 0].tolist() == [PU.OPEN] * 4 + [PU.RING] * 2 + [PU.BRANCHED]


def test_serpentines_at_max_len_and_one_past_it():
    for (max_len, n), mask in PU.serpentine_cases().items():
        seg, edges, counts = PU.inputs_of(mask)
        got, want = PU.check(seg, edges, counts, 0, max_len, 64 * 64, ("serpentine", max_len, n))
        assert want[2][0, 0] == (PU.OPEN if n <= max_len else PU.LONG) and want[4][0, 0] == (n if n <= max_len else 0)


def test_images_that_converge_at_different_launches():
    seg, edges, counts = PU.inputs_of(PU.uneven(), cap=8)
    for max_len in (4096, 1400, 1399):      # rounds to spare; exactly enough; the line too long
        got, want = PU.check(seg, edges, counts, 0, max_len, 40 * 300, ("uneven", max_len))
        assert want[4][:, 0].tolist() == [1400 if max_len >= 1400 else 0, 15, 0]


# ------------------------------------------------------------------------------------------- truncation, NULL, determinism
def test_truncation_at_max_edges_and_max_points():
    shape, name = (2, 230, 97), "smooth1.5~smooth3"
    hw = shape[1] * shape[2]
    seg, edges, counts = PU.bank_inputs(name, shape, 8, 0)
    full = PU.bank_host(name, shape, 8, 0)
    count, total = int(counts[:, 0].max()), int(full[4][:, 0].max())
    assert count > 20 and total > 400
    for cap in (1, 5, count - 1, count):      # rows past max_edges are dropped and their pixels skipped
        got, want = PU.check(seg, np.ascontiguousarray(edges[:, :cap]), counts, 0, PU.MAX_LEN, hw, ("max_edges", cap))
        assert (want[3] > 0).sum() <= (full[3] > 0).sum() and np.array_equal(want[2], full[2][:, :cap])
    for max_points in (1, total // 2, total - 1, total):      # the tail is untouched, info[0] the true number
        got, want = PU.check(seg, edges, counts, 0, PU.MAX_LEN, max_points, ("max_points", max_points))
        assert np.array_equal(want[0], full[0][:, :max_points]) and np.array_equal(want[4], full[4])
    got, want = PU.check(seg, edges, counts, 0, 10, hw, "max_len 10")
    assert (want[2] == PU.LONG).any() and (want[2] == PU.OPEN).any()


def test_pos_null_and_two_runs_give_identical_bytes():
    shape, name = (2, 230, 97), "rand0.45~rand0.55"
    seg, edges, counts = PU.bank_inputs(name, shape, 0, 1)
    want = PU.bank_host(name, shape, 0, 1)
    assert want[4][:, 3].min() > 0      # branched rows too
    s, e, c = PU.dev(seg), PU.dev(edges), PU.dev(counts)
    first = PU.run_paths(s, e, c, 1, PU.MAX_LEN, shape[1] * shape[2])
    second = PU.run_paths(s, e, c, 1, PU.MAX_LEN, shape[1] * shape[2])
    PU.same(first, want, "first")
    for a, b in zip(first, second):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    without = PU.run_paths(s, e, c, 1, PU.MAX_LEN, shape[1] * shape[2], want_pos=False)
    assert without[3] is None
    PU.same(without, want, "pos = NULL")


# ------------------------------------------------------------------------------------------- the model and the command line
def _host_graphs(prob, L, cap, max_len, eps, iters=64):
    skel = hostio.skeleton_graph(hostio.mask_thin(prob, 0.5, None, iters)[0], 0.5, None, L)[0]
    ref = hostio.line_segments(skel, 0.5, None, cap)
    N, H, W = prob.shape
    out = hostio.segment_paths(ref[3], ref[0], ref[2], 0, max_len, H * W)
    graphs = []
    for n in range(N):
        g = hostio.road_graph(ref[0][n], int(ref[2][n, 0]), ref[5][n], H, W, paths=(out[0][n], out[1][n], out[2][n]))
        for e in g["edges"]:
            if eps > 0 and len(e["path"]) > 2:
                e["path"] = hostio.simplify_path(np.asarray(e["path"], np.int64), eps).tolist()
        g["segments"], g["unordered"] = int(ref[2][n, 0]), int(out[4][n, 3])
        graphs.append(g)
    return graphs


def test_road_graph_with_paths_and_without(monkeypatch):
    from road_segmentation_unet_amd import mask_metrics as M
    from tests import test_gpu_graph as TG
    calls = []
    real = M.call
    monkeypatch.setattr(M, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    shape = (2, 230, 97)
    prob = np.array(GU.pair("smooth1.5~smooth3", shape, False)[0])
    plain = TG._model(centerline_min_branch=8).road_graph(prob, threshold=0.5)
    assert calls == ["rsu_mask_thin", "rsu_skeleton_graph", "rsu_line_segments"]      # the flag off: nothing new is called or returned
    skel = hostio.skeleton_graph(hostio.mask_thin(prob, 0.5, None, 64)[0], 0.5, None, 8)[0]
    ref = hostio.line_segments(skel, 0.5, None, 4096)
    for n in range(2):
        want = hostio.road_graph(ref[0][n], int(ref[2][n, 0]), ref[5][n], shape[1], shape[2])
        want["segments"] = int(ref[2][n, 0])
        assert plain[n] == want and list(plain[n]) == ["nodes", "edges", "segments"]
    for max_len, eps in ((4096, 0.0), (12, 0.0), (4096, 1.0)):
        del calls[:]
        g = TG._model(centerline_min_branch=8, road_graph_paths=True, max_path_length=max_len, road_graph_simplify=eps).road_graph(prob, threshold=0.5)
        assert calls == ["rsu_mask_thin", "rsu_skeleton_graph", "rsu_line_segments", "rsu_segment_paths"]
        want = _host_graphs(prob, 8, 4096, max_len, eps)
        assert g == want
        kinds = {e["kind"] for q in g for e in q["edges"]}
        assert "open" in kinds and ("long" in kinds) == (max_len == 12)
        for q, w in zip(g, plain):      # the rest of the dict is the plain one's
            assert q["nodes"] == w["nodes"] and q["segments"] == w["segments"]
            assert [{k: v for k, v in e.items() if k not in ("kind", "path")} for e in q["edges"]] == w["edges"]
        if eps:
            full = _host_graphs(prob, 8, 4096, max_len, 0.0)
            assert sum(len(e["path"]) for q in g for e in q["edges"]) < sum(len(e["path"]) for q in full for e in q["edges"])


def test_cli_save_road_graph_with_and_without_paths(tmp_path):
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
    on = run("on", ["--road_graph_paths", "--max_path_length=64"])
    assert run("off2", ["--max_path_length=7", "--road_graph_simplify=2"]) == off      # without the flag its companions change nothing
    points = 0
    for a, b in zip(off, on):
        a, b = json.loads(a), json.loads(b)
        assert list(a) == ["nodes", "edges", "segments"] and list(b) == ["nodes", "edges", "segments", "unordered"]
        assert a["nodes"] == b["nodes"] and a["segments"] == b["segments"] and len(a["edges"]) == len(b["edges"])
        for e, q in zip(a["edges"], b["edges"]):
            assert list(e) == ["id", "a", "b", "pixels", "length", "contacts", "ends"] and list(q) == list(e) + ["kind", "path"]
            assert {k: q[k] for k in e} == e and len(q["path"]) == (q["pixels"] if q["kind"] in ("open", "ring") else 0)
            points += len(q["path"])
        assert b["unordered"] == sum(q["kind"] in ("branched", "long") for q in b["edges"])
    assert points > 0
