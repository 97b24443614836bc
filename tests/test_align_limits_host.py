"""The pointer alignments of the C ABI, on the host (no GPU is needed: the addresses are fakes and are never dereferenced, every call below
is refused before anything is launched, or fills a host-side table only). tests/align_util.ALIGN states, per entry and pointer argument,
the alignment the kernels need; here the C ABI returns RSU_EINVAL and _lib.call raises for a pointer at base + align / 2 while every other
pointer sits on a 256-byte boundary, and at base + align the same call gets PAST the alignment check and fails a LATER host check (the
2-GiB refusal, as in tests/test_large_limits_host.py) or, for a table-filling call, succeeds -- which proves the order of the checks and
still launches nothing. The registry test parses the ten headers: every launching entry is in the table, every pointer parameter of
its prototype has a value, and the "align" note at the prototype states the same numbers.

Nothing here or anywhere else launches a kernel with a pointer below its table value: that half is host-only by construction, and
tests/test_gpu_aligned_min.py runs every entry AT its table value."""
import ctypes

import pytest

from road_segmentation_unet_amd import _lib
from road_segmentation_unet_amd._lib import RsuAffine, RsuElastic, RsuError, RsuJitter, RsuSrc, RsuWgradJob
from tests import align_util as au

EINVAL = -22
BASE = 1 << 32          # fake device addresses: BASE + i * STEP, all multiples of 256
STEP = 1 << 20
_PROTOS = au.prototypes()
BIG = 4097              # images of 64 x 64 x 64 bf16 elements (512 KiB): one more than fits below 2 GiB

# entry -> scalar arguments by name. Where the entry has a size check behind its argument checks the geometry is VALID and one image (or
# element) past the 2-GiB limit, so that a call that gets past the alignment check is RSU_E2BIG; everywhere else it is the smallest valid one.
_HEAD = dict(npix=(1 << 24) + 1, C=64, inv_count=1e-6, gamma=2.0, dice_scale=1.0, smooth=1.0)
_CONV = dict(nsrc=1, N=BIG, Hin=66, Win=66, Cout=64, dil=1, relu=1, ncu=0, keep=1.0, key=0, kws_floats=1 << 20)
_BWD = dict(accumulate=0, N=BIG, H=66, W=66, Cin_total=64, ci_off=0, ci_cnt=64, Cout=64, dil=1, ncu=0, kws_floats=1 << 20)
_POOL = dict(N=BIG, H=64, W=64, C=64, Hs=56, Ws=56, keep=1.0, key=0)
_CONVT = dict(N=2 * BIG, H=32, W=32, Cin=64, Cout=32, ncu=0, out_scale=1.0)
_FIRST = dict(N=BIG, H=66, W=66, Cout=64, dil=1, ncu=0)
_RUN = dict(nentries=1, total_blocks=1, lr=0.1, mu=0.9, gscale=1.0, alpha=0.1, beta1=0.9, beta2=0.99, epsilon=1e-8, decay=0.1, mode=0)
_MASK = dict(threshold=0.5, N=256, H=1024, W=1024, max_iters=1, min_branch=0)
_SMALL = dict(threshold=0.5, connectivity=4, invert=0, min_area=0, max_hole=0, N=1, B=1, H=8, W=8, iters=1, scale=1.0, smooth=1.0, accumulate=0)
_PATCH = dict(nrec=1, nimg=1, He=13378, Hl=13376, S=10, P=8)       # one extended image of 13378^2 x 12 bytes reaches 2 GiB
CASES = {
    "rsu_pack_conv_fwd": dict(k=3, Cin=8, Cout=8, nseg=0), "rsu_pack_conv_bwd": dict(k=3, Cin_total=8, ci_off=0, ci_cnt=8, Cout=8),
    "rsu_pack_convT_fwd": dict(Cin=8, Cout=8), "rsu_pack_convT_bwd": dict(Cin=8, Cout=8), "rsu_pack_conv_first": dict(Cout=8),
    "rsu_pack_table_add": dict(index=0, kind=0, k=3, Cin_total=8, ci_off=0, ci_cnt=8, Cout=8, nseg=0),
    "rsu_pack_table_run": _RUN,
    "rsu_color_adjust_fwd": dict(npix=1 << 27, keep=1.0, key=0),
    "rsu_conv_first_fwd": _FIRST, "rsu_color_conv_first_fwd": _FIRST, "rsu_conv_first_bwd_weight": _FIRST,
    "rsu_color_adjust_bwd": dict(Cout=8, scale=1.0, accumulate=0),
    "rsu_head_fwd": _HEAD, "rsu_head_fwd_bwd": _HEAD, "rsu_head_fwd_bwd_w": _HEAD, "rsu_head_dice_sums": _HEAD, "rsu_head_fwd_bwd_dice": _HEAD,
    "rsu_head_eval": _HEAD, "rsu_head_fwd_bwd_focal": _HEAD, "rsu_head_eval_focal": _HEAD, "rsu_head_fwd_bwd_aux": _HEAD,
    "rsu_border_map": dict(N=256, H=1024, W=1024, w0=1.0, sigma=1.0),
    "rsu_conv2d_fwd": _CONV, "rsu_conv2d_fwd_k": _CONV, "rsu_conv2d_fwd_pool": _CONV, "rsu_conv2d_fwd_pool_k": _CONV,
    "rsu_conv2d_bwd_data": _BWD, "rsu_conv2d_bwd_data_k": _BWD,
    "rsu_conv2d_bwd_weight": dict(N=BIG, Ho=64, Wo=64, Cin_total=64, ci_off=0, Cout=64, dil=1, ncu=0),
    "rsu_wgrad_group_plan": dict(njobs=1, N=BIG, ncu=0),
    "rsu_wgrad_group_run": {},
    "rsu_bias_grad": dict(npix=(1 << 24) + 1, C=64),
    "rsu_maxpool2x2_fwd": _POOL, "rsu_maxpool2x2_fwd_code": _POOL, "rsu_pool_skip_relu_bwd": _POOL, "rsu_pool_skip_relu_bwd_code": _POOL,
    "rsu_dropout_fwd": dict(n=(1 << 30) + 8, keep=0.8, key=7),
    "rsu_convT2x2_fwd": _CONVT, "rsu_convT2x2_bwd_data": _CONVT, "rsu_convT2x2_bwd_weight": _CONVT,
    "rsu_momentum_step": dict(lr=0.1, mu=0.9, gscale=1.0, n=4),
    "rsu_update_table_add_plain": dict(index=0, n=4),
    "rsu_update_table_add": dict(index=0, kind=0, Cin_total=8, Cout=8, nseg=0),
    "rsu_update_table_run": _RUN, "rsu_update_table_run_adam": _RUN, "rsu_update_table_run_clip": _RUN, "rsu_update_table_run_adam_clip": _RUN,
    "rsu_update_table_run_decay": _RUN, "rsu_update_table_run_adam_decay": _RUN,
    "rsu_adam_step": dict(alpha=0.1, beta1=0.9, beta2=0.99, epsilon=1e-8, gscale=1.0, n=4),
    "rsu_update_table_set_second_slot": dict(index=0),
    "rsu_grad_norm": dict(n=1 << 46, max_norm=1.0), "rsu_ema_step": dict(n=1 << 46, one_minus_decay=0.5), "rsu_grad_accumulate": dict(n=1 << 46, assign=0),
    "rsu_extract_tiles": dict(nimg=1, H=8, S=8, P=8, stride=1, t0=0, ntiles=1),
    "rsu_overlap_add": dict(nimg=1, H=8, P=8, stride=1, t0=0, ntiles=1),
    "rsu_overlap_finish": dict(n=4),
    "rsu_extract_tiles_rect": dict(nimg=(1 << 31) - 1, H=32769, W=32769, S=32768, P=32768, stride=1, t0=0, ntiles=3000000000),
    "rsu_overlap_add_rect": dict(nimg=1, H=8, W=8, P=8, stride=1, t0=0, ntiles=1),
    "rsu_affine_patches": _PATCH, "rsu_elastic_patches": _PATCH,
    "rsu_color_jitter": dict(nrec=1, S=13378),
    "rsu_quantize_mask": dict(nimg=1, S=8, patch_size=4, threshold=0.5),
    "rsu_quantize_mask_rect": dict(nimg=(1 << 31) - 1, H=2, W=2, patch_size=1, threshold=0.5),
    "rsu_labels_for_patches": dict(nimg=1, S=8, patch_size=4, threshold=0.5),
    "rsu_confusion_counts": dict(n=4),
    "rsu_cldice_fwd": _SMALL, "rsu_cldice_bwd": _SMALL, "rsu_lovasz_fwd": _SMALL, "rsu_lovasz_fwd_bwd": _SMALL,
    "rsu_components_label": _SMALL, "rsu_components_filter": _SMALL, "rsu_components_pair_count": _SMALL,
    "rsu_mask_distance": _MASK, "rsu_distance_hist": _MASK, "rsu_mask_thin": _MASK, "rsu_skeleton_graph": _MASK,
    "rsu_line_segments": dict(_MASK, N=128, max_edges=1),
}

# what a call that got past the alignment check returns: the table-filling calls succeed (they write the host table only) ...
_FILLS = {"rsu_pack_table_add": 1, "rsu_update_table_add_plain": 1, "rsu_update_table_add": 1, "rsu_update_table_set_second_slot": 0}
# ... and these entries have NO later host check to fail at: behind the alignment check stands the launch itself, so the second half of the
# test is left out for them (entry -> reason)
_NO_SIZE = "no size check: every index of its kernels is 64-bit, nothing but the launch follows the argument checks"
NO_LATER_CHECK = dict({e: "packs one weight tensor; its only checks are the argument checks in front of the alignment check" for e in (
    "rsu_pack_conv_fwd", "rsu_pack_conv_bwd", "rsu_pack_convT_fwd", "rsu_pack_convT_bwd", "rsu_pack_conv_first")}, **{
    e: "runs a device table: the sizes were checked when the table was filled" for e in (
        "rsu_pack_table_run", "rsu_update_table_run", "rsu_update_table_run_adam", "rsu_update_table_run_clip", "rsu_update_table_run_adam_clip",
        "rsu_update_table_run_decay", "rsu_update_table_run_adam_decay")}, **{
    "rsu_wgrad_group_run": "the one other check (the host table's magic word) returns the same RSU_EINVAL; the sizes were checked by the plan",
    "rsu_color_adjust_bwd": "fixed-size tensors (12 outputs from 9 x 12 x Cout sums)",
    "rsu_momentum_step": _NO_SIZE, "rsu_adam_step": _NO_SIZE, "rsu_extract_tiles": _NO_SIZE, "rsu_overlap_add": _NO_SIZE,
    "rsu_overlap_add_rect": _NO_SIZE, "rsu_overlap_finish": _NO_SIZE, "rsu_quantize_mask": _NO_SIZE, "rsu_labels_for_patches": _NO_SIZE,
    "rsu_confusion_counts": _NO_SIZE,
    "rsu_cldice_fwd": "its size rule (B H W below 2^31) is part of the argument check in front", "rsu_cldice_bwd": "as rsu_cldice_fwd",
    "rsu_lovasz_fwd": "its size rule (H W up to 2^20) is part of the argument check in front", "rsu_lovasz_fwd_bwd": "as rsu_lovasz_fwd",
    "rsu_components_label": "its size rule (H W up to 2^20) is part of the argument check in front",
    "rsu_components_filter": "as rsu_components_label", "rsu_components_pair_count": "as rsu_components_label"})

_KEEP = []   # host-side records and tables of the calls: alive until the module goes


def _table(entry):
    """a host table for the entry: zeroed; for rsu_update_table_set_second_slot holding one plain entry; for rsu_wgrad_group_run every word
    the magic word of a planned table (a plan cannot be made without a device: the word is all the entry reads before it refuses)"""
    L = _lib.lib()
    if entry == "rsu_wgrad_group_run":
        n = L.rsu_wgrad_group_table_bytes() // 4
        return (ctypes.c_uint32 * n)(*([0x57474754] * n))
    t = ctypes.create_string_buffer(4 * max(L.rsu_update_table_entry_bytes(), L.rsu_pack_table_entry_bytes(), L.rsu_wgrad_group_table_bytes()))
    if entry == "rsu_update_table_set_second_slot":
        assert L.rsu_update_table_add_plain(t, 0, BASE, BASE + STEP, BASE + 2 * STEP, 4) == 1
    return t


def _args(entry, moved=None, by=0):
    """the call: every device pointer of the table on its own 256-byte boundary, the one under `moved` displaced by `by` bytes"""
    params, scal, keys = _PROTOS[entry][1], CASES[entry], au.ALIGN[entry]
    addr = {k: BASE + i * STEP + (by if k == moved else 0) for i, k in enumerate(sorted(keys))}
    src = lambda k, H, W, C: RsuSrc(addr[k], H, W, C, 0, 0)   # noqa: E731
    out = []
    for typ, name in params:
        if typ == "rsu_stream_t":
            v = None
        elif "*" not in typ:
            v = scal[name]
        elif "rsu_src_t" in typ:
            v = (RsuSrc * 1)(src(name + ".ptr", 66, 66, 64))
        elif "rsu_wgrad_job_t" in typ:
            v = (RsuWgradJob * 1)(RsuWgradJob(_lib.WGRAD_CONV3X3, src("jobs.src.ptr", 66, 66, 64), addr["jobs.dz"], addr["jobs.dw"], addr["jobs.db"],
                                              64, 64, 64, 0, 64, 1))
        elif "rsu_affine_t" in typ:
            v = (RsuAffine * 1)(RsuAffine(0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0))
        elif "rsu_elastic_t" in typ:
            v = (RsuElastic * 1)(RsuElastic(0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0, 1))
        elif "rsu_jitter_t" in typ:
            v = (RsuJitter * 1)(RsuJitter((ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (ctypes.c_float * 9)(), 0.0, 0))
        elif name == "host_table":
            v = _table(entry)
        elif typ.endswith("* const*"):     # rsu_update_table_add's array of backward-data packs
            v = (ctypes.c_void_p * 1)(addr["packed_bwd[]"])
        elif name == "seg_c":
            v = None
        else:
            assert keys[name] not in (au.HOST,), (entry, name)
            v = addr[name]
        if "*" in typ and v is not None and not isinstance(v, int):
            _KEEP.append(v)
        out.append(v)
    return out


_DEVICE = [(e, k) for e, p, k, v in au.rows() if v not in (au.HOST, au.BYTE)]


def test_the_table_covers_every_entry_and_the_headers_state_it():
    launching = au.launching(_PROTOS)
    assert len(launching) >= 73 and "rsu_conv2d_fwd" in launching and "rsu_line_segments" in launching, len(launching)
    assert set(launching) <= set(au.ALIGN), sorted(set(launching) - set(au.ALIGN))
    # the entries of the table that do not launch: the calls that store device pointers in a table for a later launch
    assert set(au.ALIGN) - set(launching) == {"rsu_pack_table_add", "rsu_update_table_add_plain", "rsu_update_table_add",
                                              "rsu_update_table_set_second_slot", "rsu_wgrad_group_plan"}
    assert sorted(CASES) == sorted(au.ALIGN) and set(NO_LATER_CHECK) <= set(au.ALIGN) and not set(NO_LATER_CHECK) & set(_FILLS)
    notes = au.header_notes()
    for entry, keys in au.ALIGN.items():
        params = _PROTOS[entry][1]
        ptrs = [n for n in au.pointer_params(params)]
        assert sorted({k.split(".")[0].split("[")[0] for k in keys}) == sorted(ptrs), (entry, ptrs, sorted(keys))
        for k, v in keys.items():
            typ = dict((n, t) for t, n in params)[k.split(".")[0].split("[")[0]]
            assert v in (au.HOST, au.BYTE, 2, 4, 8, 16), (entry, k, v)
            if "." in k or "[" in k:
                assert keys[k.split(".")[0].split("[")[0]] == au.HOST, (entry, k)     # a device pointer inside a host struct or array
            elif v != au.HOST:      # never less than the element size
                size = 8 if ("int64_t" in typ or "long long" in typ) else 4 if ("float" in typ or "int32_t" in typ or "uint32_t" in typ) else 1
                assert v >= size and (v == au.BYTE) == ("uint8_t" in typ), (entry, k, v, typ)
        assert notes.get(entry) == keys, "%s: the align note of the header says %s, the table %s" % (entry, notes.get(entry), keys)
    assert set(notes) == set(au.ALIGN)
    assert [r[:2] for r in au.rows() if r[0] == "rsu_conv2d_fwd"] == [("rsu_conv2d_fwd", 0), ("rsu_conv2d_fwd", 0), ("rsu_conv2d_fwd", 2),
                                                                      ("rsu_conv2d_fwd", 3), ("rsu_conv2d_fwd", 4)]


def test_the_gpu_file_places_every_entry():
    """tests/test_gpu_aligned_min.py names, for every entry of the table, the fenced case that runs it at the minimum placement, or says
    why the entry cannot be placed; the cases are case functions of the fenced files that take a placement"""
    import inspect
    from tests import test_gpu_aligned_min as M
    for entry in au.ALIGN:
        assert (entry in M.PLACED) != (entry in M.NOT_PLACED), "%s: in exactly one of PLACED and NOT_PLACED" % entry
    assert set(M.PLACED) | set(M.NOT_PLACED) <= set(au.ALIGN) and all(M.NOT_PLACED.values())
    for cid, (fn, args, env, entries) in M.CASES.items():
        assert "placement" in inspect.signature(fn).parameters and fn.__module__.startswith("tests.test_gpu_") and fn.__module__.endswith("fenced"), cid
        assert entries and set(env) <= {"RSU_FWD_GEN", "RSU_CT_GEN", "RSU_PLAN_DEBUG"}, cid
    gens = {tuple(env.items()) for _, _, env, _ in M.CASES.values()}
    assert (("RSU_FWD_GEN", "2"),) in gens and (("RSU_CT_GEN", "1"),) in gens
    assert "pytest.mark.gpu" in inspect.getsource(M)
    # the recorder's view of a call: a cropped source, a job, an array of packs
    from road_segmentation_unet_amd._lib import RsuSrc
    s = (RsuSrc * 2)(RsuSrc(4096, 9, 9, 8, 0, 0), RsuSrc(8192, 9, 9, 8, 0, 0))
    got = M.device_pointers("rsu_conv2d_fwd", (s, 2, ctypes.c_void_p(256), None, 512, 1, 9, 9, 8, 1, 1, 0, None))
    assert got == [("srcs.ptr", 4096), ("srcs.ptr", 8192), ("packed_fwd", 256), ("y", 512)]
    got = M.device_pointers("rsu_conv2d_bwd_weight", (ctypes.byref(s[1]), 16, 32, None, 64, 1, 7, 7, 8, 0, 8, 1, 0, None))
    assert got == [("src.ptr", 8192), ("dz", 16), ("dw", 32), ("ws", 64)]


@pytest.mark.parametrize("entry,key", _DEVICE, ids=["%s-%s" % ek for ek in _DEVICE])
def test_entry_refuses_a_pointer_below_its_alignment_and_takes_it_at_it(entry, key):
    fn, al = getattr(_lib.lib(), entry), au.need(entry, key)
    assert fn(*_args(entry, key, al // 2)) == EINVAL, "%s: %s at base + %d is not refused" % (entry, key, al // 2)
    with pytest.raises(RsuError, match="rc=-22"):
        _lib.call(entry, *_args(entry, key, al // 2))
    if entry in NO_LATER_CHECK:
        return
    want = _FILLS.get(entry, _lib.E2BIG)
    assert fn(*_args(entry, key, al)) == want, "%s: %s at base + %d does not reach the check behind the alignment check" % (entry, key, al)
    assert fn(*_args(entry)) == want


def test_null_keeps_its_meaning():
    """an optional pointer that is NULL is not "misaligned": the calls reach their size check as before"""
    L, p = _lib.lib(), BASE
    assert L.rsu_head_eval(p, p, p, p, None, None, p, p, p, p, (1 << 24) + 1, 64, None) == _lib.E2BIG
    assert L.rsu_conv2d_bwd_data(p, p, p, None, 0, BIG, 66, 66, 64, 0, 64, 64, 1, 0, None) == _lib.E2BIG
    assert L.rsu_pool_skip_relu_bwd_code(None, p, p, None, p, BIG, 64, 64, 64, 0, 0, 1.0, 0, None) == _lib.E2BIG
    assert L.rsu_mask_thin(p, 0.5, None, 1, p, None, None, None, p, 512, 1024, 1024, None) == _lib.E2BIG
    assert L.rsu_ema_step(p, p + (1 << 50), 1 << 46, 0.5, None, None) == _lib.E2BIG


def test_every_carve_up_keeps_its_alignment():
    """the offsets behind which a workspace continues with another array, from the formulas of the launchers (align_util.CARVE_UPS), at
    every admissible channel count: the float4 slabs of the weight gradients start at multiples of 4 floats, the 32-bit words behind the
    64-bit planes and keys at multiples of 8 bytes by construction (a count of 8-byte words)"""
    L = _lib.lib()
    for cout in range(8, 2049, 8):
        assert (9 * 16 * cout) % 4 == 0 and (9 * 16 * cout + cout) % 4 == 0                       # rsu_conv_first_bwd_weight: tmp, slab stride
        for cin in (8, 24, 72, 200, 2040):
            assert (9 * cin * cout + cout) % 4 == 0                                                # rsu_conv2d_bwd_weight: slab stride
            assert (4 * cout * cin + (cout + 3) // 4 * 4) % 4 == 0                                 # rsu_convT2x2_bwd_weight
            assert L.rsu_conv2d_bwd_weight_ws_floats(cin, cin, cout) % (9 * cin * cout + cout) == 0
    for n, h, w in ((1, 1, 1), (3, 37, 41), (2, 1024, 1023)):
        assert L.rsu_thin_ws_bytes(n, h, w, 7) % 8 == 0 and L.rsu_graph_ws_bytes(n, h, w, 3) % 8 == 0 and L.rsu_lovasz_ws_bytes(n, min(h, 64), w) % 4 == 0
