"""-m gpu: every launching entry point at the MINIMUM placement. The fenced cases of tests/test_gpu_fenced.py and of the nine
tests/test_gpu_*_fenced.py files hand the kernels payloads on 256-byte boundaries; the headers promise less ("align" notes,
tests/align_util.ALIGN), and a caller who places its buffers back to back, or passes a view, gives a kernel exactly that. Here each case
function of those files runs again with fence_util.Placement("minimum"): every payload starts at a 256-byte boundary plus its own minimum
-- an address that is a multiple of the table's number and of nothing larger. Every comparison is the case's own: the same oracle or host
mirror, the same tolerance or bit equality, the same Arena.check.

How a payload gets its number. A case runs twice. The first run (today's placement) only records, through a wrapper around the library's
functions, which payload of which arena each call receives as which argument; a payload's minimum is then the largest number the table
states for any (entry, argument) it was passed as, or its element size (a packed buffer is written by rsu_pack_* at 2 and read by a conv
at 16: it sits at 16). The second run places the payloads there, and the same wrapper checks that every call of the first run is made again
and that every payload's address is its number modulo twice its number. Nothing is launched with a pointer below its number.

One run per entry, at the family's awkward shape where the fenced files have one and at its smallest otherwise; one more per kernel
generation where an entry has two (RSU_FWD_GEN = 2, RSU_CT_GEN = 1); no forced tile-shape matrices, no positive controls. A cropped
rsu_src_t gets one case of its own: an odd ox and C = 8 on top of the minimum base, so that the window's pixel addresses are 16 modulo
32, through the forward conv and the weight gradient.

PLACED / NOT_PLACED are the registry tests/test_align_limits_host.py checks against align_util.ALIGN without a GPU."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

from tests import align_util as au  # noqa: E402
from tests import fence_util as F  # noqa: E402
from tests import components_util as CU  # noqa: E402
from tests import graph_util as GU  # noqa: E402
from tests import test_gpu_cldice_fenced as GC  # noqa: E402
from tests import test_gpu_components_fenced as GCC  # noqa: E402
from tests import test_gpu_distance_fenced as GD  # noqa: E402
from tests import test_gpu_fenced as G  # noqa: E402
from tests import test_gpu_graph_fenced as GG  # noqa: E402
from tests import test_gpu_loss_fenced as GL  # noqa: E402
from tests import test_gpu_lovasz_fenced as GLV  # noqa: E402
from tests import test_gpu_optim_fenced as GO  # noqa: E402
from tests import test_gpu_segments_fenced as GS  # noqa: E402
from tests import test_gpu_thin_fenced as GT  # noqa: E402
from road_segmentation_unet_amd._lib import lib  # noqa: E402

_PROTOS = au.prototypes()


def _int(a):
    return a if isinstance(a, int) else getattr(a, "value", None)


def device_pointers(entry, args):
    """(key, address) of every non-NULL device pointer of one call, by the keys of align_util.ALIGN[entry]"""
    keys, out = au.ALIGN[entry], []
    for (typ, name), a in zip(_PROTOS[entry][1], args):
        if a is None or "*" not in typ:
            continue
        if name + ".ptr" in keys:                                     # rsu_src_t: an array of nsrc (the next argument), or byref(one)
            srcs = [a._obj] if hasattr(a, "_obj") else list(a)[:args[1] if name == "srcs" else 1]
            out += [(name + ".ptr", s.ptr) for s in srcs]
        elif name == "jobs":
            for j in list(a)[:args[1]]:
                out += [("jobs.src.ptr", j.src.ptr), ("jobs.dz", j.dz), ("jobs.dw", j.dw), ("jobs.db", j.db)]
        elif name + "[]" in keys:
            out += [(name + "[]", v) for v in a]
        elif keys[name] != au.HOST:
            out.append((name, _int(a)))
    return [(k, v) for k, v in out if v]


class Recorder:
    """wraps the library's functions of the table while a case runs: .calls = [(entry, [(key, address), ...])], .need = {(arena index,
    spec name): bytes} over the arenas of `placement`"""

    def __init__(self, placement):
        self.placement, self.calls = placement, []

    def __enter__(self):
        L = self.L = lib()
        self.saved = {e: getattr(L, e) for e in au.ALIGN}
        for e, fn in self.saved.items():
            setattr(L, e, self._wrap(e, fn))
        return self

    def __exit__(self, *exc):
        for e, fn in self.saved.items():
            setattr(self.L, e, fn)

    def _wrap(self, entry, fn):
        def wrapped(*args):
            self.calls.append((entry, device_pointers(entry, args)))
            return fn(*args)
        return wrapped

    def payload(self, addr):
        for i, A in enumerate(self.placement.arenas):
            off = addr - A.mem.data_ptr()
            for name, (start, end, _) in A.place.items():
                if start <= off < end:
                    return i, name, off - start
        return None      # (not arena memory)

    def need(self):
        need = {}
        for entry, ptrs in self.calls:
            for key, addr in ptrs:
                hit, al = self.payload(addr), au.need(entry, key)
                if hit and al != au.BYTE:
                    assert hit[2] % al == 0, (entry, key, hit)      # a pointer into a payload keeps the payload's alignment
                    need[hit[:2]] = max(need.get(hit[:2], 0), al)
        return need


def at_minimum(case, entries, *args, **kw):
    """`case(*args, placement=...)` recorded under today's placement, then run with every payload at its minimum; `entries`: the entries the
    registry says this case runs"""
    first = F.Placement("aligned")
    with Recorder(first) as r1:
        case(*args, placement=first, **kw)
    need = r1.need()
    ran = {e for e, _ in r1.calls}
    assert set(entries) <= ran, "the registry names %s for this case, it ran %s" % (sorted(set(entries) - ran), sorted(ran))
    second = F.Placement("minimum", [{n: b for (i, n), b in need.items() if i == k} for k in range(len(first.arenas))])
    with Recorder(second) as r2:
        case(*args, placement=second, **kw)
    assert [e for e, _ in r2.calls] == [e for e, _ in r1.calls] and len(second.arenas) == len(first.arenas)
    assert r2.need() == need, (r2.need(), need)
    for k, A in enumerate(second.arenas):
        for s in A.specs:
            m = max(s.minimum, need.get((k, s.name), 0))
            assert A[s.name].data_ptr() % (2 * m) == m, (s.name, m)      # a multiple of its number and of nothing larger
    for entry, ptrs in r2.calls:                                         # and no call anywhere below its table value
        for key, addr in ptrs:
            assert addr % max(au.need(entry, key), 1) == 0, (entry, key)


def _env(monkeypatch, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


_PACK_TABLE = ["rsu_pack_conv_fwd", "rsu_pack_conv_bwd", "rsu_pack_convT_fwd", "rsu_pack_convT_bwd", "rsu_pack_conv_first", "rsu_pack_table_add",
               "rsu_pack_table_run", "rsu_update_table_add", "rsu_update_table_add_plain", "rsu_conv2d_fwd"]
_HEADS = ["rsu_head_fwd", "rsu_head_fwd_bwd", "rsu_head_fwd_bwd_w", "rsu_head_dice_sums", "rsu_head_fwd_bwd_dice", "rsu_head_eval"]
# case id -> (the case function of a fenced file, its arguments, the environment it runs in, the entries it is the registry's run of)
CASES = {
    "conv_fwd": (G._conv_fwd, (G.CONV[0], 0), {}, ["rsu_pack_conv_fwd", "rsu_conv2d_fwd"]),
    "conv_fwd_gen2": (G._conv_fwd, (G.CONV[0], 1), {"RSU_FWD_GEN": "2"}, ["rsu_conv2d_fwd"]),
    "conv_fwd_cropped_odd_ox_C8": (G.test_conv2d_fwd_cropped_sources, ([(25, 29)], [8], 19, 23, 16, 0), {}, ["rsu_conv2d_fwd"]),
    "conv_fwd_k": (G.test_conv2d_fwd_k_split, (0,), {}, ["rsu_conv2d_fwd_k"]),
    "conv_fwd_pool": (G.test_conv2d_fwd_pool, (G.POOL[0], 1, 0), {}, ["rsu_conv2d_fwd_pool"]),
    "conv_fwd_pool_k": (G.test_conv2d_fwd_pool, (G.POOL[0], 1, 1), {}, ["rsu_conv2d_fwd_pool_k"]),
    "bwd_data": (G._bwd_data, (G.CONV[0], "mask"), {}, ["rsu_pack_conv_bwd", "rsu_conv2d_bwd_data"]),
    "bwd_data_gen2": (G._bwd_data, (G.CONV[0], "accumulate"), {"RSU_FWD_GEN": "2"}, ["rsu_conv2d_bwd_data"]),
    "bwd_data_k": (G._bwd_data, ((1, 20, 20, 512, 512, 1, False), "mask"), {"RSU_PLAN_DEBUG": "1"}, ["rsu_conv2d_bwd_data_k"]),
    "bwd_weight": (G._wgrad, (G.CONV[0],), {}, ["rsu_conv2d_bwd_weight"]),
    "bias_grad": (G.test_bias_grad, (3 * 37 * 41, 16), {}, ["rsu_bias_grad"]),
    "bwd_weight_cropped_odd_ox_C8": (G._wgrad, ((2, 19, 23, 8, 16, 1, True),), {}, ["rsu_conv2d_bwd_weight"]),
    "wgrad_group": (G.test_wgrad_group, (), {}, ["rsu_wgrad_group_plan", "rsu_wgrad_group_run"]),
    "convT": (G._convT, (G.CONVT[0],), {}, ["rsu_pack_convT_fwd", "rsu_pack_convT_bwd", "rsu_convT2x2_fwd", "rsu_convT2x2_bwd_data", "rsu_convT2x2_bwd_weight"]),
    "convT_gen1": (G._convT, (G.CONVT[0],), {"RSU_CT_GEN": "1"}, ["rsu_convT2x2_fwd", "rsu_convT2x2_bwd_data"]),
    "first_layer": (G._first, (G.FIRST[1],), {}, ["rsu_pack_conv_first", "rsu_color_adjust_fwd", "rsu_conv_first_fwd", "rsu_color_conv_first_fwd",
                                                  "rsu_conv_first_bwd_weight", "rsu_color_adjust_bwd"]),
    "pool_junction": (G._pool_junction, ((2, 10, 14, 24),), {}, ["rsu_maxpool2x2_fwd", "rsu_maxpool2x2_fwd_code", "rsu_pool_skip_relu_bwd",
                                                                 "rsu_pool_skip_relu_bwd_code"]),
    "dropout": (G.test_dropout_fwd, (1003 * 8,), {}, ["rsu_dropout_fwd"]),
    "heads": (G.test_heads, (8,), {}, _HEADS),
    "border_map": (G.test_border_map, (), {}, ["rsu_border_map"]),
    "optimizer_passes": (G.test_momentum_adam_ema_accumulate_norm, (1003,), {}, ["rsu_momentum_step", "rsu_adam_step", "rsu_grad_norm", "rsu_ema_step",
                                                                               "rsu_grad_accumulate"]),
    "tables_momentum": (G.test_update_and_pack_tables, ("momentum",), {}, _PACK_TABLE + ["rsu_update_table_run"]),
    "tables_adam": (G.test_update_and_pack_tables, ("adam",), {}, ["rsu_update_table_set_second_slot", "rsu_update_table_run_adam"]),
    "tables_momentum_clip": (G.test_update_and_pack_tables, ("momentum_clip",), {}, ["rsu_update_table_run_clip"]),
    "tables_adam_clip": (G.test_update_and_pack_tables, ("adam_clip",), {}, ["rsu_update_table_run_adam_clip"]),
    "tables_decay": (GO.test_update_table_decay, ("momentum", "l2", "clip"), {}, ["rsu_update_table_run_decay"]),
    "tables_adam_decay": (GO.test_update_table_decay, ("adam", "decoupled", "clip"), {}, ["rsu_update_table_run_adam_decay"]),
    "tilers": (G.test_tilers_square_and_rect, (), {}, ["rsu_extract_tiles", "rsu_overlap_add", "rsu_overlap_finish", "rsu_extract_tiles_rect",
                                                       "rsu_overlap_add_rect"]),
    "quantize": (G.test_quantize_labels_confusion, (), {}, ["rsu_quantize_mask", "rsu_quantize_mask_rect", "rsu_labels_for_patches", "rsu_confusion_counts"]),
    "patches": (G.test_affine_and_elastic_patches, (), {}, ["rsu_affine_patches", "rsu_elastic_patches"]),
    "color_jitter": (G.test_color_jitter, (37, 33), {}, ["rsu_color_jitter"]),
    "focal_heads": (GL.test_focal_heads, (8,), {}, ["rsu_head_fwd_bwd_focal", "rsu_head_eval_focal"]),
    "cldice": (GC.test_cldice_fwd_bwd, (3, "tied4"), {}, ["rsu_cldice_fwd", "rsu_cldice_bwd"]),
    "aux_head": (GC.test_aux_head, (8,), {}, ["rsu_head_fwd_bwd_aux"]),
    "lovasz": (GLV.test_lovasz_fwd_and_fwd_bwd, (GLV.SHAPES[0], "quant4"), {}, ["rsu_lovasz_fwd", "rsu_lovasz_fwd_bwd"]),
    "components": (GCC.test_components_entries, (GCC.SHAPES[0], CU.CONNECTIVITIES[1]), {}, ["rsu_components_label", "rsu_components_filter",
                                                                                            "rsu_components_pair_count"]),
    "distance": (GD.test_distance_entries, (GD.SHAPES[0],), {}, ["rsu_mask_distance", "rsu_distance_hist"]),
    "thin": (GT.test_thin_entry, GT.CASES[0], {}, ["rsu_mask_thin"]),
    "graph": (GG.test_graph_entry, ((3, 63, 65), GU.R + 1), {}, ["rsu_skeleton_graph"]),
    "segments": (GS.test_segments_entry, GS.CASES[0], {}, ["rsu_line_segments"]),
}
# what a case needs beside its own arguments: the fixtures of the test function it is, or the keywords of the helper
_FIXTURES = {"conv_fwd_k": ("capfd", "monkeypatch"), "conv_fwd_pool": ("monkeypatch", "capfd"), "conv_fwd_pool_k": ("monkeypatch", "capfd"),
             "wgrad_group": ("monkeypatch",)}
_KEYWORDS = {"bwd_data_k": {"k": True}, "bwd_weight_cropped_odd_ox_C8": {"crop": (25, 29)}}

PLACED = {}          # entry -> the case ids that are its runs at the minimum placement
for _id, (_fn, _args, _envv, _entries) in CASES.items():
    for _e in _entries:
        PLACED.setdefault(_e, []).append(_id)
NOT_PLACED = {}      # entry -> why it cannot be placed (none)


@pytest.mark.parametrize("case", sorted(CASES))
def test_entry_at_its_minimum_alignment(case, monkeypatch, capfd):
    fn, args, env, entries = CASES[case]
    _env(monkeypatch, **env)
    fixtures = {"monkeypatch": monkeypatch, "capfd": capfd}
    kw = dict(_KEYWORDS.get(case, {}))
    if case == "bwd_data_k":
        kw["capfd"] = capfd
    at_minimum(fn, entries, *args, *[fixtures[f] for f in _FIXTURES.get(case, ())], **kw)
    if "cropped_odd_ox_C8" in case:
        # the window's first pixel: (oy W + ox) pixels of 16 bytes behind a base that is 16 modulo 32, with ox odd and oy W + ox even
        H0, W0, h, w = 25, 29, 19, 23
        oy, ox = (H0 - h) // 2, (W0 - w) // 2
        assert ox % 2 == 1 and ((oy * W0 + ox) * 8 * 2 + 16) % 32 == 16
