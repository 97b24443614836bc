"""The pointer alignments of the C ABI: for every entry point that launches (an `int rsu_*` that takes an rsu_stream_t, in all ten public
headers) and for the table-filling calls whose pointers a later launch dereferences, the smallest alignment of each pointer argument at
which the launch is exact -- the widest single access or atomic the kernels make through it, never less than the element size; for a
workspace the largest need of anything carved out of it. The same numbers stand as "align" notes at the entries in include/*.h and as
checks in csrc/rsu_api.hip (RSU_EINVAL, before anything is launched, for a non-NULL pointer below its number).

ALIGN is written by argument NAME (a reader compares it with the prototype); rows() gives it as (entry, argument position, key, bytes),
the positions taken from the prototypes of the headers. A key is the parameter's name, or, for a pointer that travels inside a host-side
struct or array, "<parameter>.<field>" / "<parameter>[]" (rsu_src_t.ptr, the pointers of an rsu_wgrad_job_t, packed_bwd[i]).

tests/test_align_limits_host.py holds the C ABI to this table without a GPU (fake addresses, never dereferenced);
tests/test_gpu_aligned_min.py runs every entry with each buffer placed at exactly the largest number any of its uses states."""
import os
import re

HOST = 0    # host memory, read before the call returns (records, host-side tables and descriptor arrays): no device alignment applies
BYTE = 1    # a tensor of bytes: every address is aligned, there is nothing to refuse

HEADERS = ("rsu.h", "rsu_optim.h", "rsu_loss.h", "rsu_cldice.h", "rsu_lovasz.h", "rsu_components.h", "rsu_distance.h", "rsu_thin.h",
           "rsu_graph.h", "rsu_segments.h")

_SRC = {"srcs": HOST, "srcs.ptr": 16}
_CONV_FWD = dict(_SRC, packed_fwd=16, bias=4, y=16)
_CONV_POOL = dict(_CONV_FWD, pooled=16, code=8)
_BWD_DATA = {"dz": 16, "packed_bwd": 16, "dx": 16, "relu_src": 16}
_HEAD = {"act": 16, "w": 4, "b": 4, "prob": 4}
_HEAD_TRAIN = dict(_HEAD, labels=8, loss_sum=4, dact=16, dw=4, db=4, ws=4)
_HEAD_W = dict(_HEAD_TRAIN, class_w=4, pixel_w=4, weight_sum=4)
_HEAD_EVAL = dict(_HEAD, labels=8, class_w=4, pixel_w=4, sums=4, hist=8, ws=4)
_TABLE_RUN = {"dev_table": 8}
_TILES = {"imgs": 4, "tiles": 4}
_OVERLAP = {"prob": 4, "acc": 4, "hits": 4}
_PATCHES = {"images": 4, "labels": BYTE, "recs": HOST, "x_out": 4, "labels_out": 8}

ALIGN = {
    # ---- weight packing: k_pack reads floats and stores bf16 one by one; k_pack_many stores 16-byte groups (16-byte loads only where the
    # address allows them: it tests the address, not the count)
    "rsu_pack_conv_fwd": {"w_hwio": 4, "packed": 2, "seg_c": HOST},
    "rsu_pack_conv_bwd": {"w_hwio": 4, "packed": 2},
    "rsu_pack_convT_fwd": {"k_hwoi": 4, "packed": 2},
    "rsu_pack_convT_bwd": {"k_hwoi": 4, "packed": 2},
    "rsu_pack_conv_first": {"w_hwio": 4, "packed": 2},
    "rsu_pack_table_add": {"host_table": HOST, "w": 4, "packed": 16, "seg_c": HOST},
    "rsu_pack_table_run": _TABLE_RUN,
    # ---- head / tail
    "rsu_color_adjust_fwd": {"x": 4, "w": 4, "b": 4, "out16": 16},
    "rsu_conv_first_fwd": {"in16": 16, "packed": 16, "b": 4, "y": 16},
    "rsu_color_conv_first_fwd": {"x": 4, "w0": 4, "b0": 4, "packed": 16, "b": 4, "y": 16},
    "rsu_conv_first_bwd_weight": {"in16": 16, "dz": 16, "dw1": 4, "gx": 4, "db": 16, "ws": 16},
    "rsu_color_adjust_bwd": {"gx": 4, "w1": 4, "dW0": 4, "db0": 4},
    "rsu_head_fwd": dict(_HEAD, logits=4),
    "rsu_head_fwd_bwd": _HEAD_TRAIN,
    "rsu_head_fwd_bwd_w": _HEAD_W,
    "rsu_head_dice_sums": dict(_HEAD, labels=8, pixel_w=4, dice_sums=4, ws=4),
    "rsu_head_fwd_bwd_dice": dict(_HEAD_W, dice_sums=4),
    "rsu_head_eval": _HEAD_EVAL,
    "rsu_head_fwd_bwd_focal": dict(_HEAD_W, dice_sums=4),
    "rsu_head_eval_focal": _HEAD_EVAL,
    "rsu_head_fwd_bwd_aux": dict(_HEAD_W, dice_sums=4, gprob=4),
    "rsu_border_map": {"labels": 8, "mul": 4, "out": 4, "d2": 4, "ws": 4},
    # ---- 3x3 convolutions: 16-byte pieces of every bf16 tensor and of the packed weights, float4 slabs, 8 code bytes per store
    "rsu_conv2d_fwd": _CONV_FWD,
    "rsu_conv2d_fwd_k": dict(_CONV_FWD, kws=16),
    "rsu_conv2d_fwd_pool": _CONV_POOL,
    "rsu_conv2d_fwd_pool_k": dict(_CONV_POOL, kws=16),
    "rsu_conv2d_bwd_data": _BWD_DATA,
    "rsu_conv2d_bwd_data_k": dict(_BWD_DATA, kws=16),
    "rsu_conv2d_bwd_weight": {"src": HOST, "src.ptr": 16, "dz": 16, "dw": 16, "db": 16, "ws": 16},
    "rsu_wgrad_group_plan": {"jobs": HOST, "jobs.src.ptr": 16, "jobs.dz": 16, "jobs.dw": 16, "jobs.db": 16, "ws": 16, "host_table": HOST},
    "rsu_wgrad_group_run": {"host_table": HOST, "dev_table": 8},
    "rsu_bias_grad": {"dz": 16, "db": 4, "ws": 4},
    # ---- pools, dropout
    "rsu_maxpool2x2_fwd": {"x": 16, "y": 16},
    "rsu_maxpool2x2_fwd_code": {"x": 16, "y": 16, "code": 8},
    "rsu_pool_skip_relu_bwd": {"y_act": 16, "dpool": 16, "dskip": 16, "dz": 16},
    "rsu_pool_skip_relu_bwd_code": {"y_act": 16, "code": 8, "dpool": 16, "dskip": 16, "dz": 16},
    "rsu_dropout_fwd": {"x": 16, "y": 16},
    # ---- transposed convolutions
    "rsu_convT2x2_fwd": {"x": 16, "packed_fwd": 16, "bias": 4, "y": 16},
    "rsu_convT2x2_bwd_data": {"dy": 16, "packed_bwd": 16, "dx": 16, "relu_src": 16},
    "rsu_convT2x2_bwd_weight": {"x": 16, "dy": 16, "dK": 16, "db": 16, "ws": 16},
    # ---- optimizer (float4 passes; the state record and the norm's workspace are 32-bit words)
    "rsu_momentum_step": {"w": 16, "acc": 16, "g": 16},
    "rsu_update_table_add_plain": {"host_table": HOST, "w": 16, "acc": 16, "g": 16},
    "rsu_update_table_add": {"host_table": HOST, "w": 16, "acc": 16, "g": 16, "packed_fwd": 16, "packed_bwd": HOST, "packed_bwd[]": 16,
                             "seg_c": HOST},
    "rsu_update_table_run": _TABLE_RUN,
    "rsu_adam_step": {"w": 16, "m": 16, "v": 16, "g": 16},
    "rsu_update_table_set_second_slot": {"host_table": HOST, "v": 16},
    "rsu_update_table_run_adam": _TABLE_RUN,
    "rsu_grad_norm": {"g": 16, "ws": 4, "state": 4},
    "rsu_update_table_run_clip": dict(_TABLE_RUN, state=4),
    "rsu_update_table_run_adam_clip": dict(_TABLE_RUN, state=4),
    "rsu_update_table_run_decay": dict(_TABLE_RUN, clip_state=4),
    "rsu_update_table_run_adam_decay": dict(_TABLE_RUN, clip_state=4),
    "rsu_ema_step": {"ema": 16, "w": 16, "clip_state": 4},
    "rsu_grad_accumulate": {"dst": 16, "src": 16},
    # ---- tilers, loaders, post-processing: float by float (12-byte pixels are three floats), int64 labels and counters
    "rsu_extract_tiles": _TILES,
    "rsu_overlap_add": _OVERLAP,
    "rsu_overlap_finish": {"acc": 4, "hits": 4, "out": 4},
    "rsu_extract_tiles_rect": _TILES,
    "rsu_overlap_add_rect": _OVERLAP,
    "rsu_affine_patches": _PATCHES,
    "rsu_elastic_patches": _PATCHES,
    "rsu_color_jitter": {"x": 4, "recs": HOST, "ws": 8},
    "rsu_quantize_mask": {"masks": 4, "out": 4},
    "rsu_quantize_mask_rect": {"masks": 4, "out": 4},
    "rsu_labels_for_patches": {"masks": 4, "labels": 8},
    "rsu_confusion_counts": {"predictions": 8, "labels": 8, "counts": 8},
    # ---- the loss terms and metrics of the family headers
    "rsu_cldice_fwd": {"prob": 4, "labels": 8, "skel_p": 4, "skel_y": 4, "sums": 4, "ws": 4},
    "rsu_cldice_bwd": {"prob": 4, "labels": 8, "skel_p": 4, "skel_y": 4, "sums": 4, "gprob": 4, "ws": 4},
    "rsu_lovasz_fwd": {"prob": 4, "labels": 8, "loss_sum": 4, "ws": 8},
    "rsu_lovasz_fwd_bwd": {"prob": 4, "labels": 8, "gprob": 4, "loss_sum": 4, "ws": 8},
    "rsu_components_label": {"prob": 4, "labels": 4, "area": 4, "edge": BYTE, "ws": 4},
    "rsu_components_filter": {"prob": 4, "out": 4, "stats": 8, "ws": 4},
    "rsu_components_pair_count": {"prob": 4, "labels64": 8, "acc": 8, "ws": 4},
    "rsu_mask_distance": {"prob": 4, "labels64": 8, "d2_pred": 4, "d2_true": 4, "ws": 4},
    "rsu_distance_hist": {"prob": 4, "labels64": 8, "acc": 8, "ws": 4},
    "rsu_mask_thin": {"prob": 4, "labels64": 8, "skel_pred": 4, "skel_true": 8, "acc": 8, "info": 4, "ws": 8},
    "rsu_skeleton_graph": {"prob": 4, "labels64": 8, "out_pred": 4, "out_true": 8, "junc_pred": 4, "junc_true": 8, "acc": 8, "ws": 8},
    "rsu_line_segments": {"prob": 4, "labels64": 8, "edges_pred": 4, "edges_true": 4, "counts": 4, "seg_pred": 4, "seg_true": 4,
                          "node_pred": 4, "node_true": 4, "acc": 8, "ws": 8},
}

# The carve-ups behind the workspace numbers above, each checked at every admissible shape by tests/test_align_limits_host.py
# (test_every_carve_up_keeps_its_alignment) from the same formulas as the launchers: (entry, what lies at which offset, the need there).
CARVE_UPS = """
rsu_head_eval / _focal   ws floats: [nb][5] sums, then u32 [nb][512] at 5 nb floats                          4 at a multiple of 4
rsu_grad_norm            ws floats: [nb] sums, then u32 [nb] flags                                            4 at a multiple of 4
rsu_lovasz_*             ws bytes: u64 keys [B Pn], then int counts [2 tiles], then float partial [tiles]     8 first, 4 at multiples of 8
rsu_mask_thin            ws bytes: three u64 planes, then u32 counters                                        8 first, 4 at a multiple of 8
rsu_skeleton_graph       ws bytes: one or five u64 planes, then u32 counters                                  8 first, 4 at a multiple of 8
rsu_line_segments        ws bytes: float planes [4 N H W], then four int arrays                               4 everywhere (the header asks 8)
rsu_components_*         ws bytes: five int arrays [N H W], then int [N][4]                                   4 everywhere
rsu_cldice_*             ws floats: [2 iters + 1][N] sums, then per-tile partials                             4 everywhere
rsu_conv_first_bwd_weight ws floats: tmp [9][16][Cout], then the slabs at 144 Cout, stride 144 Cout + Cout    16 at multiples of 4 floats (Cout % 8 == 0)
rsu_conv2d_bwd_weight    ws floats: slabs of 9 Cin_total Cout + Cout floats (the bias row behind the taps)    16 at multiples of 4 floats (Cout % 8 == 0)
rsu_convT2x2_bwd_weight  ws floats: slabs of 4 Cout Cin + roundup(Cout, 4) floats                             16 at multiples of 4 floats
rsu_wgrad_group_plan     ws floats: the jobs' slabs back to back, each nsplit x (taps CsOut CfOut + bias row) 16 at multiples of 4 floats
rsu_conv2d_*_k           kws floats: slices of kslab_stride = slots x 8 waves x NST x 512 floats              16 at multiples of 512 floats
rsu_color_jitter         ws bytes: int64 [records][chunks][3]                                                 8 everywhere
"""


def _root():
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text(name):
    with open(os.path.join(_root(), "include", name)) as f:
        return f.read()


def prototypes():
    """{entry: [(type, name), ...]} of every `int rsu_*(...)` and `size_t rsu_*(...)` prototype of the ten headers, comments removed"""
    out = {}
    for h in HEADERS:
        text = re.sub(r"/\*.*?\*/", " ", header_text(h), flags=re.S)
        for ret, name, args in re.findall(r"^(int|size_t) (rsu_\w+)\(([^;]*?)\);", text, flags=re.M | re.S):
            params = []
            for a in args.split(","):
                a = " ".join(a.split())
                if a in ("void", ""):
                    continue
                m = re.match(r"^(.*?)(\w+)$", a)
                params.append((m.group(1).strip(), m.group(2)))
            out[name] = (ret, params)
    return out


def launching(protos=None):
    protos = protos or prototypes()
    return sorted(n for n, (ret, params) in protos.items() if ret == "int" and any(t == "rsu_stream_t" for t, _ in params))


def pointer_params(params):
    return [n for t, n in params if "*" in t]


def position(params, key):
    names = [n for _, n in params]
    return names.index(re.split(r"[.\[]", key)[0])


def rows():
    """the table as (entry, argument position, key, bytes), in header order of the arguments"""
    protos = prototypes()
    out = []
    for entry, keys in ALIGN.items():
        params = protos[entry][1]
        out += sorted((entry, position(params, k), k, v) for k, v in keys.items())
    return out


def need(entry, key):
    return ALIGN[entry][key]


def header_notes():
    """{entry: {key: bytes}} from the `align (rsu_a, rsu_b): key bytes, key bytes, ... .` notes of the headers ("host" = HOST, "byte" = BYTE)"""
    out = {}
    for h in HEADERS:
        for entries, body in re.findall(r"align \(((?:rsu_\w+(?:, )?)+)\): (.*?)\. \*/", " ".join(header_text(h).replace("\n *", " ").split())):
            pairs = {}
            for item in body.split(","):
                key, val = item.split()
                pairs[key] = {"host": HOST, "byte": BYTE}.get(val, None) if not val.isdigit() else int(val)
            for e in entries.split(", "):
                assert e not in out, "two align notes for %s" % e
                out[e] = pairs
    return out
