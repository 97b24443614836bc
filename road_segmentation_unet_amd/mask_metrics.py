"""The chain from a mask to a road graph, in one place: the entry points of rsu_components.h, rsu_distance.h, rsu_thin.h, rsu_graph.h,
rsu_segments.h, rsu_paths.h and rsu_routes.h as functions of tensors, their workspaces, and the integer mask metrics of a validation pass -- the layout of their one
accumulator (layout), the launches of a chunk (MaskMetrics.run) and the reading of the all-reduced counters (decode).
ConvolutionalModel.evaluate() and the mask tools (postprocess_masks, centerlines, road_graph) drive it; nothing here knows a model."""
import ctypes
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import hostio
from ._lib import call, lib
from .hostio import DIST_BINS, DIST_MAX_SIDE, GRAPH_MAX_SIDE, SEGMENTS_MAX_SIDE, THIN_MAX_SIDE


def ptr(t):
    """a tensor's device address for the C ABI; None stays None (NULL: the entry skips that output)"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream(device):
    """the current stream of `device`, as the hipStream_t every entry takes last"""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ------------------------------------------------------------------ the entry points: tensors (or None) in, each argument order written once
def components_pair_count(prob, threshold, labels, connectivity, acc, ws, st):
    """rsu_components.h: acc[4] += {components of prob >= threshold, of labels == 1, sum |pred - true|, images with a counted pixel}"""
    call("rsu_components_pair_count", ptr(prob), float(threshold), ptr(labels), int(connectivity), ptr(acc), ptr(ws), *prob.shape, st)


def components_filter(prob, threshold, connectivity, min_area, max_hole, out, stats, ws, st):
    """rsu_components.h: small road components removed, small holes filled; stats int64 [N, 6]"""
    call("rsu_components_filter", ptr(prob), float(threshold), int(connectivity), int(min_area), int(max_hole), ptr(out), ptr(stats), ptr(ws),
         *prob.shape, st)


def distance_hist(prob, threshold, labels, acc, ws, st):
    """rsu_distance.h: acc[2 * DIST_BINS] += the predicted road pixels by their distance to the truth, the true ones by theirs to the prediction"""
    call("rsu_distance_hist", ptr(prob), float(threshold), ptr(labels), ptr(acc), ptr(ws), *prob.shape, st)


def mask_thin(prob, threshold, labels, max_iters, skel_pred, skel_true, acc, info, ws, st):
    """rsu_thin.h: the two skeletons; acc[4] += {|S_P|, |S_P and T|, |S_T|, |S_T and P|}; info int32 [N, 2] != 0 where a side still moved"""
    call("rsu_mask_thin", ptr(prob), float(threshold), ptr(labels), int(max_iters), ptr(skel_pred), ptr(skel_true), ptr(acc), ptr(info), ptr(ws),
         *prob.shape, st)


def skeleton_graph(prob, threshold, labels, min_branch, out_pred, out_true, junc_pred, junc_true, acc, ws, st):
    """rsu_graph.h: the skeletons pruned of branches of at most min_branch pixels (out_* may be the inputs), their junction pixels, and
    acc[8] += the node counts {pixels, ends, isolated, junction pixels} of each side"""
    call("rsu_skeleton_graph", ptr(prob), float(threshold), ptr(labels), int(min_branch), ptr(out_pred), ptr(out_true), ptr(junc_pred),
         ptr(junc_true), ptr(acc), ptr(ws), *prob.shape, st)


def line_segments(prob, threshold, labels, max_edges, edges_pred, edges_true, counts, seg_pred, seg_true, node_pred, node_true, acc, ws, st):
    """rsu_segments.h: the skeletons cut at their node zones, one measured row per segment; counts int32 [N, 4]; acc[16] += the rows' sums"""
    call("rsu_line_segments", ptr(prob), float(threshold), ptr(labels), int(max_edges), ptr(edges_pred), ptr(edges_true), ptr(counts),
         ptr(seg_pred), ptr(seg_true), ptr(node_pred), ptr(node_true), ptr(acc), ptr(ws), *prob.shape, st)


def segment_paths(seg, edges, counts, side, max_len, max_points, paths, offsets, kind, pos, info, ws, st):
    """rsu_paths.h: the pixels of every stored segment of one side of line_segments in their order along it; paths int32 [N, max_points],
    offsets int32 [N, max_edges + 1], kind int32 [N, max_edges], pos int32 [N, H, W] or None, info int32 [N, 4]"""
    call("rsu_segment_paths", ptr(seg), ptr(edges), ptr(counts), int(side), int(edges.shape[1]), int(max_len), int(max_points), ptr(paths),
         ptr(offsets), ptr(kind), ptr(pos), ptr(info), ptr(ws), *seg.shape, st)


def graph_routes(node_map, edges, counts, side, nodes, dist, info, ws, st):
    """rsu_routes.h: the node table of one side of line_segments and the length of the shortest path between every two nodes; nodes int32
    [N, max_nodes, 4], dist int32 [N, max_nodes, max_nodes] (70 per orthogonal link, 99 per diagonal one; hostio.ROUTES_INF: no path),
    info int32 [N, 4] = {nodes, nodes stored, edges used, rows skipped}"""
    call("rsu_graph_routes", ptr(node_map), ptr(edges), ptr(counts), int(side), int(edges.shape[1]), int(nodes.shape[1]), ptr(nodes), ptr(dist),
         ptr(info), ptr(ws), *node_map.shape, st)


def route_score(a, b, slack, match, acc, st):
    """rsu_routes.h: one direction of the path-length score between two graphs (nodes, dist, info) of graph_routes with one max_nodes;
    match int32 [N, max_nodes]; acc[4] += {pairs, sum q, unmatched, broken}"""
    call("rsu_route_score", ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(b[0]), ptr(b[1]), ptr(b[2]), int(a[0].shape[1]), int(slack), ptr(match),
         ptr(acc), int(a[0].shape[0]), st)


# ------------------------------------------------------------------ workspaces
# header -> (its size function, the element type of the width its `align` note asks of ws)
_WS = {"components": ("rsu_components_ws_bytes", torch.int32), "distance": ("rsu_distance_ws_bytes", torch.int32),
       "thin": ("rsu_thin_ws_bytes", torch.int64), "graph": ("rsu_graph_ws_bytes", torch.int64),
       "segments": ("rsu_segments_ws_bytes", torch.int64), "paths": ("rsu_paths_ws_bytes", torch.int64),
       "routes": ("rsu_routes_ws_bytes", torch.int32)}


def workspace(entry, shape, extra, device, message, ok=True, zero=False):
    """The workspace of rsu_<entry>.h's launches on `shape` = (n, H, W) and the header's `extra` size arguments (thin: max_iters; graph:
    min_branch; segments: max_edges; paths: max_edges, max_len; routes: max_nodes). ValueError(message) where the header takes no such sizes (its size function returns 0) or the caller's
    own guard `ok` fails. No entry reads what its workspace held: torch.empty, or zeros for a buffer that is kept."""
    fn, dtype = _WS[entry]
    need = int(getattr(lib(), fn)(*(int(v) for v in tuple(shape) + tuple(extra)))) if ok else 0
    if need == 0:
        raise ValueError(message)
    return (torch.zeros if zero else torch.empty)(need // dtype.itemsize, dtype=dtype, device=device)


def thin_stack(t, device, threshold, max_iters, min_branch, message):
    """The centre-lines of a stack of masks on the device (rsu_mask_thin with labels64 = NULL: every pixel counted), with min_branch > 0
    pruned in place (rsu_skeleton_graph; the sizes rsu_thin.h takes are the ones rsu_graph.h takes): t float32 [n, H, W], contiguous, on
    the host or on `device` -> the DEVICE tensor of the same shape, exactly 1.0 on the skeleton of {t >= threshold} and 0.0 elsewhere.
    ValueError(message), before anything is copied, for sizes rsu_thin.h does not take."""
    shape, st = tuple(t.shape), stream(device)
    ws = workspace("thin", shape, (max_iters,), device, message, ok=min(shape) >= 1)
    t = t.to(device)
    out = torch.empty_like(t)
    mask_thin(t, threshold, None, max_iters, out, None, None, None, ws, st)
    if min_branch > 0:
        skeleton_graph(out, 0.5, None, min_branch, out, None, None, None, None, workspace("graph", shape, (min_branch,), device, message), st)
    return out


# ------------------------------------------------------------------ the accumulator of a validation pass
class Flags(namedtuple("Flags", "components distances centerlines min_branch junctions segments routes")):
    """The resolved --validate_components, --validate_distances, --validate_centerlines, --centerline_min_branch, --validate_junctions,
    --validate_segments and --validate_routes: junctions, segments and min_branch count only with centre-lines, routes only with
    segments; the graph stage is on iff one of min_branch > 0 and junctions is."""
    __slots__ = ()

    def __new__(cls, components=False, distances=False, centerlines=False, min_branch=0, junctions=False, segments=False, routes=False):
        cl = bool(centerlines)
        sg = cl and bool(segments)
        return super().__new__(cls, bool(components), bool(distances), cl, int(min_branch) if cl else 0, cl and bool(junctions), sg,
                               sg and bool(routes))

    @classmethod
    def of(cls, options):
        return cls(*(getattr(options, k, 0) for k in ("validate_components", "validate_distances", "validate_centerlines",
                                                      "centerline_min_branch", "validate_junctions", "validate_segments", "validate_routes")))

    @property
    def graph(self):
        return self.min_branch > 0 or self.junctions

    @property
    def any(self):
        return self.components or self.distances or self.centerlines


# stage -> its parts in the accumulator, in order: THE statement of the layout (int64 counters each)
STAGES = OrderedDict([
    ("components", (("counts", 4),)),                                                        # rsu_components_pair_count's four
    ("distances", (("hist", 2 * DIST_BINS),)),                                               # rsu_distance_hist of the two masks
    ("centerlines", (("hist", 2 * DIST_BINS), ("counts", 4), ("unconverged", 1))),           # ... of the two skeletons; rsu_mask_thin's four; info != 0
    ("graph", (("nodes", 8), ("jn_hist", 2 * DIST_BINS), ("jn_counts", 4))),                 # rsu_skeleton_graph's eight; the junction pixels' histogram and clusters
    ("segments", (("acc", 16), ("counts_sum", 4))),                                          # rsu_line_segments' sixteen; the patches' summed counts
    ("routes", (("acc", 8), ("info", 8))),                                                   # rsu_route_score's four, truth -> prediction then back; the patches' summed info of both sides
])


def layout(flags):
    """name -> slice of the accumulator for the stages `flags` switch on, in STAGES' order without gaps: "<stage>" and "<stage>.<part>".
    A stage that is off has no name here."""
    out, at = OrderedDict(), 0
    for stage, parts in STAGES.items():
        if getattr(flags, stage):
            out[stage] = slice(at, at + sum(n for _, n in parts))
            for part, n in parts:
                out["%s.%s" % (stage, part)] = slice(at, at + n)
                at += n
    return out


def total(flags):
    """the accumulator's length"""
    return max([s.stop for s in layout(flags).values()] + [0])


def decode(flags, counts, relaxed_slack):
    """The keys evaluate() gains from the mask stages, in their order, from `counts` = the all-reduced accumulator (float64 [total(flags)];
    integers, exact below 2^53):
      components:  "components_pred" / "components_true" (the components summed over the patches, ignored pixels background in both) and
                   "b0_error" = sum |predicted - true| / max(patches with a counted pixel, 1);
      distances:   "dist_hist" (int64 [2, 64]) and the keys of hostio.relaxed_metrics of it at relaxed_slack. Distances are per patch: a
                   true road just outside a patch is not seen;
      centerlines: "cl_hist", the keys of hostio.centerline_metrics and "thin_unconverged" (image sides still moving at the last iteration);
      graph:       with min_branch > 0 cl_len_pred / cl_len_true are the PRUNED centre-lines' pixel counts (cldice_hard stays on the
                   unpruned skeletons); with junctions "jn_hist" and the keys of hostio.graph_metrics;
      segments:    the keys of hostio.segment_metrics;
      routes:      the keys of hostio.route_metrics."""
    lay, c, slack = layout(flags), np.rint(np.asarray(counts)).astype(np.int64), int(relaxed_slack)
    if c.shape != (total(flags),):
        raise ValueError("decode: %s counters for a layout of %d" % (c.shape, total(flags)))
    out = {}
    if flags.components:
        cc = c[lay["components"]]
        out["components_pred"], out["components_true"] = int(cc[0]), int(cc[1])
        out["b0_error"] = float(cc[2]) / max(float(cc[3]), 1.0)
    if flags.distances:
        out["dist_hist"] = c[lay["distances.hist"]].reshape(2, DIST_BINS)
        out.update(hostio.relaxed_metrics(out["dist_hist"], slack))
    if flags.centerlines:
        out["cl_hist"] = c[lay["centerlines.hist"]].reshape(2, DIST_BINS)
        out.update(hostio.centerline_metrics(out["cl_hist"], c[lay["centerlines.counts"]], slack))
        out["thin_unconverged"] = int(c[lay["centerlines.unconverged"]][0])
    if flags.graph:
        nodes = c[lay["graph.nodes"]]
        if flags.min_branch > 0:
            out["cl_len_pred"], out["cl_len_true"] = int(nodes[0]), int(nodes[4])
        if flags.junctions:
            out["jn_hist"] = c[lay["graph.jn_hist"]].reshape(2, DIST_BINS)
            out.update(hostio.graph_metrics(out["jn_hist"], c[lay["graph.jn_counts"]], nodes, slack))
    if flags.segments:
        out.update(hostio.segment_metrics(c[lay["segments.acc"]].reshape(2, 8), c[lay["segments.counts_sum"]]))
    if flags.routes:
        acc = c[lay["routes.acc"]]
        out.update(hostio.route_metrics(acc[:4], acc[4:], c[lay["routes.info"]]))
    return out


class MaskMetrics:
    """The device side of the mask stages of a validation pass in chunks of B patches of P x P: ONE int64 accumulator `acc` of
    total(flags) counters, written by the launches through the views `part` (whole int64 offsets: every view keeps the 8-byte alignment
    the headers ask of acc), and `ws`, the named device buffers of the stages that are on. reset() in front of a pass, run() behind
    every chunk's head, then decode() of the all-reduced acc. Every launch treats ignored pixels (labels other than 0 / 1) as background
    on both sides, so a chunk's padding patches add exactly nothing."""

    def __init__(self, flags, device, B, P, connectivity, max_iters, max_segments, relaxed_slack, max_nodes=256, route_snap=8):
        self.flags, self.lay = flags, layout(flags)
        self.max_nodes, self.route_snap = int(max_nodes), int(route_snap)
        self.connectivity, self.max_iters, self.max_segments, self.relaxed_slack = int(connectivity), int(max_iters), int(max_segments), int(relaxed_slack)
        shape, small = (B, P, P), B * P * P * 8 < 0x7ffffff0   # (the labels below 2 GiB)
        labels_limit = " (sides up to %d, the labels below 2 GiB)"

        def outside(flag, header, limits=""):
            return "%s: a batch of %d patches of %d x %d pixels is outside %s's limits%s" % (flag, B, P, P, header, limits)

        def kept(entry, message, extra=(), ok=True):
            return workspace(entry, shape, extra, device, message, ok=ok, zero=True)

        def zeros(shape, dtype):
            return torch.zeros(shape, dtype=dtype, device=device)

        w = self.ws = {}
        if flags.components:
            w["components"] = kept("components", outside("--validate_components", "rsu_components.h"))
        if flags.distances:
            w["distances"] = kept("distance", outside("--validate_distances", "rsu_distance.h", labels_limit % DIST_MAX_SIDE), ok=small)
        if flags.centerlines:   # the two skeletons, info, and the workspaces of rsu_mask_thin and of the skeletons' rsu_distance_hist
            message = outside("--validate_centerlines", "rsu_thin.h", labels_limit % THIN_MAX_SIDE)
            w.update(thin=kept("thin", message, (self.max_iters,), ok=small), dist=kept("distance", message),
                     skel_pred=zeros(shape, torch.float32), skel_true=zeros(shape, torch.int64), info=zeros((B, 2), torch.int32))
        if flags.graph:   # rsu_skeleton_graph's workspace; for the junctions their two pixel masks and the workspace of their pair count
            w["graph"] = kept("graph", outside("--centerline_min_branch / --validate_junctions", "rsu_graph.h", labels_limit % GRAPH_MAX_SIDE),
                              (flags.min_branch,), ok=small)
            if flags.junctions:   # (their rsu_distance_hist re-uses the centre-lines' "dist")
                w.update(comp=kept("components", outside("--validate_junctions", "rsu_components.h")),
                         junc_pred=zeros(shape, torch.float32), junc_true=zeros(shape, torch.int64))
        if flags.segments:   # the workspace, the two segment tables of max_segments rows per patch and the per-patch counts
            w["segments"] = kept("segments", outside("--validate_segments", "rsu_segments.h", " (sides up to %d, 16 bytes per pixel below 2 GiB)"
                                                     % SEGMENTS_MAX_SIDE), (self.max_segments,))
            w.update(edges_pred=zeros((B, self.max_segments, 8), torch.int32), edges_true=zeros((B, self.max_segments, 8), torch.int32),
                     counts=zeros((B, 4), torch.int32))
        if flags.routes:   # the two node maps of rsu_line_segments; per side the node table, the distances and info; match and the workspace
            w["routes"] = kept("routes", outside("--validate_routes", "rsu_routes.h", " (sides up to %d, --max_graph_nodes^2 distances per patch "
                                                 "below 2 GiB)" % hostio.ROUTES_MAX_SIDE), (self.max_nodes,))
            for side in ("pred", "true"):
                w.update({"node_" + side: zeros(shape, torch.int32), "rt_nodes_" + side: zeros((B, self.max_nodes, 4), torch.int32),
                          "rt_dist_" + side: zeros((B, self.max_nodes, self.max_nodes), torch.int32), "rt_info_" + side: zeros((B, 4), torch.int32)})
            w["match"] = zeros((B, self.max_nodes), torch.int32)
        self.acc = zeros(total(flags), torch.int64)
        self.part = {name: self.acc[s] for name, s in self.lay.items()}

    def reset(self):
        self.acc.zero_()

    def run(self, prob, labels, threshold):
        """the launches of one chunk on its probabilities and labels, on the current stream; nothing is read back"""
        f, w, part, st = self.flags, self.ws, self.part, stream(prob.device)
        if f.components:
            components_pair_count(prob, threshold, labels, self.connectivity, part["components"], w["components"], st)
        if f.distances:
            distance_hist(prob, threshold, labels, part["distances"], w["distances"], st)
        if f.centerlines:   # both skeletons and the four counts, then the distance histogram of the skeletons
            sp, sl = w["skel_pred"], w["skel_true"]
            mask_thin(prob, threshold, labels, self.max_iters, sp, sl, part["centerlines.counts"], w["info"], w["thin"], st)
            if f.graph:   # prune the two skeletons in place and / or mark their junction pixels: the cl_* keys but cldice_hard then describe the pruned lines
                prune = f.min_branch > 0
                skeleton_graph(sp, 0.5, sl, f.min_branch, sp if prune else None, sl if prune else None, w.get("junc_pred"), w.get("junc_true"),
                               part["graph.nodes"], w["graph"], st)
            distance_hist(sp, 0.5, sl, part["centerlines.hist"], w["dist"], st)
            if f.segments:   # the segments of the two (pruned) skeletons; the patches' counts are summed on the device
                line_segments(sp, 0.5, sl, self.max_segments, w["edges_pred"], w["edges_true"], w["counts"], None, None, w.get("node_pred"),
                              w.get("node_true"), part["segments.acc"], w["segments"], st)
                part["segments.counts_sum"].add_(w["counts"].sum(dim=0))
                if f.routes:   # both graphs' distances, then the score from the truth to the prediction and back
                    graphs = []
                    for side, name in enumerate(("pred", "true")):
                        g = (w["rt_nodes_" + name], w["rt_dist_" + name], w["rt_info_" + name])
                        graph_routes(w["node_" + name], w["edges_" + name], w["counts"], side, *g, w["routes"], st)
                        part["routes.info"][4 * side:4 * side + 4].add_(g[2].sum(dim=0))
                        graphs.append(g)
                    route_score(graphs[1], graphs[0], self.route_snap, w["match"], part["routes.acc"][:4], st)
                    route_score(graphs[0], graphs[1], self.route_snap, w["match"], part["routes.acc"][4:], st)
            part["centerlines.unconverged"].add_((w["info"] != 0).sum())   # (on the device: no read-back)
            if f.junctions:   # how far the junction pixels of one side lie from the other's, and the junctions as 8-connected clusters
                distance_hist(w["junc_pred"], 0.5, w["junc_true"], part["graph.jn_hist"], w["dist"], st)
                components_pair_count(w["junc_pred"], 0.5, w["junc_true"], 8, part["graph.jn_counts"], w["comp"], st)

    def decode(self, tail):
        return decode(self.flags, tail, self.relaxed_slack)
