"""What the ordered-polyline tests share (tests/test_paths_host.py, test_gpu_paths.py, test_gpu_paths_fenced.py, test_gpu_paths_large.py): the
inputs of include/rsu_paths.h taken from hostio.line_segments on the thinned pairs of tests/segments_util.py and on hand-drawn masks, the
host references of hostio.segment_paths computed once per case, and the launch helper of the entry. A plain module, imported by name."""
import functools

import numpy as np

from tests import components_util as CU
from tests import segments_util as SU

MAX_SIDE, MAX_EDGES, MAX_LEN_LIMIT = 1024, 65536, 1 << 20   # rsu_paths.h RSU_PATHS_MAX_SIDE, RSU_PATHS_MAX_EDGES, RSU_PATHS_MAX_LEN
BLOCK, TILE_W, TILE_H = 256, 64, 16                         # csrc/paths.hip PT_BLOCK, PT_TW x PT_TH (the classify tile)
FILL = -9            # what paths, offsets and kind hold before a launch: elements the entry does not touch keep it
MAX_LEN = 4096       # max_len of the bank's cases: above every segment of theirs
NAMES = ("paths", "offsets", "kind", "pos", "info")
HOST_SHAPES = [(2, 64, 64), (1, 65, 63), (2, 230, 97)]
OPEN, RING, BRANCHED, LONG = 0, 1, 2, 3
DIRS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def rounds(max_len):
    """R = ceil(log2(max_len)), the jump launches of a call; the header states 5 + R launches"""
    return (max_len - 1).bit_length()


def ws_layout(N, H, W, max_edges, max_len):
    """the layout include/rsu_paths.h states: two arc buffers of 16 N H W bytes, an int32 plane, two int32 [N][max_edges], int32 [max(R, 1)][N]"""
    return -(-(N * H * W * 36 + (2 * N * max_edges + max(rounds(max_len), 1) * N) * 4) // 8) * 8


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def bank_inputs(name, shape, min_branch, side):
    """(seg, edges, counts) of one side of hostio.line_segments on the thinned pair `name` pruned at min_branch: shared, read-only"""
    out = SU.host_pair(name, tuple(shape), min_branch)
    return out[3 + side], out[side], out[2]


@functools.lru_cache(maxsize=None)
def bank_host(name, shape, min_branch, side, max_len=MAX_LEN):
    seg, edges, counts = bank_inputs(name, shape, min_branch, side)
    return host(seg, edges, counts, side, max_len, shape[1] * shape[2])


def host(seg, edges, counts, side, max_len, max_points):
    from road_segmentation_unet_amd import hostio
    return _frozen(hostio.segment_paths(seg, edges, counts, side, max_len, max_points, fill=FILL))


def inputs_of(mask, cap=64, side=0):
    """(seg, edges, counts) of side `side` of hostio.line_segments on a bool [N, H, W] (the same mask as prediction and truth)"""
    from road_segmentation_unet_amd import hostio
    out = hostio.line_segments(CU.prob_of(mask), SU.THRESHOLD, mask.astype(np.int64), cap, fill=SU.FILL)
    return _frozen((out[3 + side], out[side], out[2]))


def link_mask(s):
    """the path links of a bool [H, W], written apart from hostio's: a set of frozenset({index, index})"""
    H, W = s.shape
    inside = lambda y, x: 0 <= y < H and 0 <= x < W and bool(s[y, x])   # noqa: E731
    links = set()
    for y, x in zip(*np.nonzero(s)):
        for dy, dx in DIRS:
            if not inside(y + dy, x + dx):
                continue
            if dy and dx and (inside(y + dy, x) or inside(y, x + dx)):
                continue
            links.add(frozenset((int(y) * W + int(x), int(y + dy) * W + int(x + dx))))
    return links


# ------------------------------------------------------------------------------------------- hand-drawn masks
def _image(H, W, pixels):
    m = np.zeros((H, W), bool)
    for y, x in pixels:
        m[y, x] = True
    return m


def serpentine(H, W, length):
    """the first `length` pixels of a line that runs along the even rows and turns through one pixel of the odd rows at alternating ends"""
    pts, y, right = [], 0, True
    while y < H:
        xs = range(W) if right else range(W - 1, -1, -1)
        pts += [(y, x) for x in xs]
        if y + 2 < H:
            pts.append((y + 1, W - 1 if right else 0))
        y, right = y + 2, not right
    assert length <= len(pts)
    return _image(H, W, pts[:length])


def hollow(m, y, x, side=4):
    m[y, x:x + side] = m[y + side - 1, x:x + side] = m[y:y + side, x] = m[y:y + side, x + side - 1] = True


def hand_cases():
    """name -> (bool [N, H, W], {label: kind} of some of its segments, or None)"""
    out = {}
    small = np.zeros((7, 12, 16), bool)
    small[0, 5, 7] = True                                        # a single pixel
    small[1, 5, 7:9] = True                                      # two pixels
    small[2, 3:7, 4] = small[2, 6, 4:9] = True                   # an L-corner
    for i in range(8):                                           # a staircase
        small[3, 2 + i, 3 + i] = small[3, 2 + i, 4 + i] = True
    small[4, 4:6, 6:8] = True                                    # the 2 x 2 block: a ring of four
    small[5, 4, 7] = small[5, 5, 6] = small[5, 5, 8] = small[5, 6, 7] = True   # the diamond: a ring of four diagonal links
    small[6, 4:7, 6:9] = True                                    # the 3 x 3 block: branched
    out["small"] = small
    out["diagonal"] = SU.diagonal(200, 200)[None]                # through thirteen classify tiles in both axes
    stairs = np.zeros((1, 70, 200), bool)                        # a staircase across tile borders in both axes, two pixels per row
    for i in range(70):
        stairs[0, i, 2 * i:2 * i + 3] = True
    out["stairs"] = stairs
    rings = np.zeros((1, 24, 96), bool)
    hollow(rings[0], 2, 63)                                      # its smallest pixel: index 255, the last of a block, the last column of a tile
    hollow(rings[0], 10, 64)                                     # index 1024: the first pixel of a block, the first column of the next tile
    assert 2 * 96 + 63 == BLOCK - 1 and (10 * 96 + 64) % BLOCK == 0 and TILE_W == 64
    out["rings"] = rings
    two = np.zeros((2, 20, 20), bool)                            # a chain that ends in the last row of image 0 above one that starts in
    two[0, 10:, 5] = two[1, :10, 5] = True                       # the first row of image 1
    out["two_images"] = two
    return out


def serpentine_cases():
    """(max_len, length) -> bool [1, 64, 64]: exactly max_len pixels (open) and one more (too long), at max_len 64 and 65"""
    return {(L, n): serpentine(64, 64, n)[None] for L in (64, 65) for n in (L, L + 1)}


def uneven():
    """bool [3, 40, 300]: image 0 holds a serpentine of 1400 pixels (eleven doublings), image 1 a few short lines (three), image 2
    nothing: the images converge at different jump launches"""
    m = np.zeros((3, 40, 300), bool)
    m[0] = serpentine(40, 300, 1400)
    m[1, 5, 10:17] = m[1, 20:25, 100] = m[1, 30, 200:203] = True
    return m


# ------------------------------------------------------------------------------------------- launches (GPU tests)
def ws_bytes(shape, max_edges, max_len):
    from road_segmentation_unet_amd._lib import lib
    return int(lib().rsu_paths_ws_bytes(shape[0], shape[1], shape[2], int(max_edges), int(max_len)))


def new_ws(shape, max_edges, max_len):
    """a workspace of the advertised size, filled with a pattern: the entry must not count on its contents"""
    import torch
    from tests import hiputil as hu
    need = ws_bytes(shape, max_edges, max_len)
    assert need > 0 and need % 8 == 0
    return torch.full((need // 8,), 0x7FA57FA57FA57FA5, dtype=torch.int64, device=hu.DEV)


def dev(a):
    import torch
    from tests import hiputil as hu
    return torch.from_numpy(np.array(a)).to(hu.DEV)   # (a copy: the shared arrays are read-only)


def run_paths(seg_t, edges_t, counts_t, side, max_len, max_points, want_pos=True, ws=None):
    """(paths, offsets, kind, pos, info) as device tensors (pos None unless asked for). paths, offsets and kind start as FILL, pos and
    info as a sentinel"""
    import torch
    from road_segmentation_unet_amd._lib import call
    from tests import hiputil as hu
    shape, cap = tuple(seg_t.shape), int(edges_t.shape[1])
    ws = new_ws(shape, cap, max_len) if ws is None else ws
    N = shape[0]
    full = lambda s, v: torch.full(s, v, dtype=torch.int32, device=hu.DEV)   # noqa: E731
    paths, offsets, kind = full((N, max_points), FILL), full((N, cap + 1), FILL), full((N, cap), FILL)
    pos = full(shape, -0x5A5A5A5A) if want_pos else None
    info = full((N, 4), -0x5A5A5A5A)
    call("rsu_segment_paths", hu.ptr(seg_t), hu.ptr(edges_t), hu.ptr(counts_t), int(side), cap, int(max_len), int(max_points), hu.ptr(paths),
         hu.ptr(offsets), hu.ptr(kind), hu.ptr(pos), hu.ptr(info), hu.ptr(ws), shape[0], shape[1], shape[2], hu.stream())
    return paths, offsets, kind, pos, info


def same(got, want, what):
    """byte for byte; an output not asked for is None on the device side"""
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            raise AssertionError((what, name, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def check(seg, edges, counts, side, max_len, max_points, what, want=None, **kw):
    """the entry on the device against hostio.segment_paths; returns (got, want)"""
    want = host(seg, edges, counts, side, max_len, max_points) if want is None else want
    got = run_paths(dev(seg), dev(edges), dev(counts), side, max_len, max_points, **kw)
    same(got, want, what)
    return got, want
