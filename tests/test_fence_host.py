"""No GPU: the fence of tests/fence_util.py has teeth, and tests/test_gpu_fenced.py leaves no launching entry point out. numpy / torch
on the CPU play the kernels on a CPU arena: a clean one passes; a byte written just behind or just in front of a payload, at the far
end of a band, into an input, or behind a workspace at advertised + 1 floats raises with the tensor, the side and the offset; a read
one element past an input, multiplied by zero, yields NaN and fails the comparison the GPU cases use. Every one of these claims is proved
twice: under today's layout (payloads on 256-byte boundaries) and under Placement("minimum") (each payload at a boundary plus its own
minimum alignment: tests/test_gpu_aligned_min.py runs every entry point there). The registry check parses
include/rsu.h: every `int rsu_*` entry that takes an rsu_stream_t is in FENCED or NOT_FENCED, every size function is named by a case."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import fence_util as F
from tests import hiputil as hu

CPU = "cpu"
N_WS = 1000   # the "advertised" workspace, floats


PLACEMENTS = ["aligned", "minimum"]
MINIMA = {"x": 16, "acc": 8}     # under "minimum": x as the 16-byte pieces of a bf16 tensor, acc as a 64-bit counter; the others at their element size


def _placement(mode):
    return F.Placement(mode, [MINIMA] * 2)


def _arena(placement="aligned"):
    rng = np.random.RandomState(0)
    x = rng.standard_normal((3, 37, 8)).astype(np.float32)      # 1776 bytes as bf16: no multiple of 512
    lab = (rng.rand(37) < 0.5).astype(np.uint8)                 # an odd byte count: the band behind it starts on an odd address
    A = F.Arena(CPU, [F.bf16("x", x), F.raw("labels", lab), F.out("y", (3, 37, 8)), F.ws("ws", N_WS), F.state("acc", np.zeros(5, np.float32))],
                placement=_placement(placement))
    return A, hu.q(x)


def _kernel(A):
    """y = 2 x through the workspace"""
    n = A["x"].numel()
    A["ws"][:n // 2] = A["x"].reshape(-1)[:n // 2].float()
    A["y"].copy_((A["x"].float() * 2).to(torch.bfloat16))
    A["acc"].add_(1)


def test_layout(placement="aligned"):
    A, _ = _arena(placement)
    assert A.mem.numel() == A.total and A.mem.data_ptr() % F.ALIGN == 0 and A.placement.arenas == [A]
    prev_end = 0
    for s in A.specs:
        start, end, behind = A.place[s.name]
        # "aligned": on a 256-byte boundary; "minimum": the boundary plus the payload's minimum m, an ADDRESS that is a multiple of m and of
        # nothing larger (x 16, acc 8, the float workspace 4, y 2 as bf16, the byte labels 1)
        m = {"x": 16, "labels": 1, "y": 2, "ws": 4, "acc": 8}[s.name]
        assert start % F.ALIGN == (m if placement == "minimum" else 0) and start - prev_end >= F.BAND and end - start == s.nbytes
        if placement == "minimum":
            assert A[s.name].data_ptr() % (2 * m) == m
        assert behind >= F.BAND and (s.kind != "ws" or behind >= s.nbytes)
        assert A[s.name].data_ptr() == A.mem.data_ptr() + start
        prev_end = end
    assert A.total - prev_end >= F.BAND
    big = F.Arena(CPU, [F.ws("ws", 3 << 18), F.out("y", (4,))], placement=_placement(placement))     # 3 MiB workspace: its band is its own size
    assert big.place["y"][0] - big.place["ws"][1] >= (3 << 20) + F.BAND
    # every byte is a payload or belongs to exactly one region
    cover = np.zeros(A.total, np.int32)
    for _, _, s, e, _ in A.regions:
        cover[s:e] += 1
    for s in A.specs:
        cover[A.place[s.name][0]:A.place[s.name][1]] += 1
    assert (cover == 1).all()
    # the pattern: NaN as bf16 and as float32, absurd as an integer
    assert torch.isnan(A["y"]).all() and torch.isnan(A["ws"]).all()
    assert int(A.mem[:8].view(torch.int64)[0]) == 0x7FA57FA57FA57FA5


def test_clean_kernel_passes(placement="aligned"):
    A, x = _arena(placement)
    _kernel(A)
    A.check("clean")
    hu.assert_bf16_close(A["y"].float().numpy(), 2.0 * x.astype(np.float64), "y = 2 x")


def _violation(where, placement):
    A, _ = _arena(placement)
    _kernel(A)
    name, side, off = where
    start, end, _b = A.place[name]
    at = {"front": start, "behind": end, "input": start}[side] + off
    A.mem[at] = (int(A.mem[at]) + 1) & 0xFF
    with pytest.raises(F.FenceError) as e:
        A.check("case")
    return e.value


VIOLATIONS = [("y", "behind", 0), ("labels", "behind", 0), ("y", "front", -1), ("x", "front", -1),
              ("y", "behind", F.BAND - 1), ("y", "front", -F.BAND), ("x", "front", -F.BAND), ("acc", "behind", F.BAND - 1),
              ("x", "input", 0), ("x", "input", 1775), ("labels", "input", 36),
              ("ws", "behind", 4), ("ws", "behind", 2 * 4 * N_WS - 1)]


@pytest.mark.parametrize("name,side,off", VIOLATIONS, ids=lambda v: str(v))
def test_every_violation_raises_with_tensor_side_and_offset(name, side, off, placement="aligned"):
    """one byte: just behind a payload (an odd-sized one too), just in front, at the far end of a band (the arena's first and last byte
    included), inside an input, behind the workspace at advertised + 1 floats and at twice the advertised size"""
    e = _violation((name, side, off), placement)
    assert (e.tensor, e.side, e.first, e.last, e.count) == (name, side, off, off, 1), str(e)
    assert "case" in str(e) and ("%s %s:" % (name, side)) in str(e) and ("first at offset %+d" % off) in str(e) and "1 byte(s)" in str(e)


def test_workspace_overrun_of_one_float(placement="aligned"):
    A, _ = _arena(placement)
    _kernel(A)
    wide = A.mem[A.place["ws"][0]:A.place["ws"][0] + 4 * (N_WS + 1)].view(torch.float32)
    wide[N_WS] = 1.0      # the float at advertised + 1
    with pytest.raises(F.FenceError) as e:
        A.check("one slab too many")
    assert (e.value.tensor, e.value.side, e.value.first) == ("ws", "behind", 0) and e.value.last <= 3, str(e.value)


def test_several_violations_are_all_listed(placement="aligned"):
    A, _ = _arena(placement)
    A.mem[A.place["y"][1]:A.place["y"][1] + 10] = 0
    A["x"].view(torch.int16)[0, 0, 0].add_(1)
    with pytest.raises(F.FenceError) as e:
        A.check("two")
    assert "y behind: 10 byte(s) changed, first at offset +0, last at offset +9" in str(e.value) and "x input:" in str(e.value)


def test_stray_read_times_zero_is_nan(placement="aligned"):
    """a "kernel" that reads one element past its input and multiplies it by zero: in an exact-size torch tensor it reads allocator
    padding and adds 0; in the arena it reads the pattern, 0 * NaN = NaN, and the comparison of the GPU cases fails"""
    A, x = _arena(placement)
    n = x.size
    wide = A.mem[A.place["x"][0]:A.place["x"][0] + 2 * (n + 1)].view(torch.bfloat16).float()
    y = (wide[:n] * 2 + wide[n] * 0).reshape(x.shape)
    A["y"].copy_(y.to(torch.bfloat16))
    A.check("a stray read writes nothing")
    with pytest.raises(AssertionError, match="out of tolerance"):
        hu.assert_bf16_close(A["y"].float().numpy(), 2.0 * x.astype(np.float64), "y = 2 x")
    with pytest.raises(AssertionError, match="out of tolerance"):
        hu.assert_f32_close(A["y"].float().numpy(), 2.0 * x.astype(np.float64), "y = 2 x", rtol=1e-2)
    with pytest.raises(AssertionError):
        np.testing.assert_array_equal(A["y"].float().numpy(), hu.q(2.0 * x))


def test_unwritten_output_is_nan_and_poisoned_margins(placement="aligned"):
    A, x = _arena(placement)
    assert torch.isnan(A["y"]).all()
    B = F.Arena(CPU, [F.bf16("src", np.ones((2, 6, 7, 8), np.float32))], placement=F.Placement(placement, [{"src": 16}]))
    assert B["src"].data_ptr() % 32 == (16 if placement == "minimum" else 0)
    B.poison_outside("src", 1, 2, 3, 4)
    t = B["src"].float()
    assert (t[:, 1:4, 2:6] == 1).all() and int(torch.isnan(t).sum()) == 2 * (6 * 7 - 3 * 4) * 8
    B.check("margins are part of the input as given")


# ------------------------------------------------------------------------------------------- the same claims under Placement("minimum")
@pytest.mark.parametrize("claim", [test_layout, test_clean_kernel_passes, test_workspace_overrun_of_one_float, test_several_violations_are_all_listed,
                                   test_stray_read_times_zero_is_nan, test_unwritten_output_is_nan_and_poisoned_margins], ids=lambda f: f.__name__)
def test_claim_holds_at_the_minimum_placement(claim):
    """every payload at a 256-byte boundary plus its own minimum (x 16, acc 8, ws 4, y 2, labels 1): exact payload ends, every gap byte
    attributed once, the bands, the NaN of an unwritten output and of a stray read, the poisoned margins"""
    claim(placement="minimum")


@pytest.mark.parametrize("name,side,off", VIOLATIONS, ids=lambda v: str(v))
def test_every_violation_raises_at_the_minimum_placement(name, side, off):
    """the positive controls, with the same tensors, sides and offsets: the far ends of the bands and the arena's last byte included"""
    test_every_violation_raises_with_tensor_side_and_offset(name, side, off, placement="minimum")


# ------------------------------------------------------------------------------------------- the registry covers rsu.h
def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "rsu.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = re.findall(r"^(int|size_t) (rsu_\w+)\(([^;]*?)\);", text, flags=re.M | re.S)
    launching = [n for r, n, a in protos if r == "int" and "rsu_stream_t" in a]
    sizes = [n for r, n, a in protos if r == "size_t" and (n.endswith("_ws_floats") or n.endswith("_ws_bytes") or n in ("rsu_packed_bytes", "rsu_packed_first_bytes"))]
    return launching, sizes


def test_the_registry_covers_every_launching_entry_and_every_size_function():
    from tests import test_gpu_fenced as G
    launching, sizes = _header()
    assert len(launching) >= 56 and len(sizes) >= 15 and "rsu_conv2d_fwd" in launching and "rsu_packed_bytes" in sizes, (len(launching), len(sizes))
    tests = {n: f for n, f in vars(G).items() if n.startswith("test_") and callable(f)}
    source = inspect.getsource(G)
    for entry in launching:
        assert (entry in G.FENCED) != (entry in G.NOT_FENCED), "%s: in exactly one of FENCED and NOT_FENCED" % entry
    assert set(G.FENCED) | set(G.NOT_FENCED) <= set(launching), sorted((set(G.FENCED) | set(G.NOT_FENCED)) - set(launching))
    for entry, names in G.FENCED.items():
        assert names, entry
        for n in names:
            assert n in tests, (entry, n)
            assert re.search(r'"%s"' % entry, inspect.getsource(tests[n]) + "".join(inspect.getsource(h) for h in G.HELPERS.get(n, ()))), \
                "%s is not launched by %s" % (entry, n)
    for entry, reason in G.NOT_FENCED.items():
        assert "writes no device memory" in reason, (entry, reason)
    for fn in sizes:
        names = G.SIZES.get(fn)
        assert names, "%s: no fenced case carves a buffer of exactly this size" % fn
        for n in names:
            assert n in tests, (fn, n)
            assert fn in inspect.getsource(tests[n]) + "".join(inspect.getsource(h) for h in G.HELPERS.get(n, ())), (fn, n)
    assert set(G.SIZES) <= set(sizes)
    assert "pytest.mark.gpu" in source
