"""CPU: gradient accumulation on the host side -- the --accumulate_steps flag and its rejection, dist.micro_indices, the dropout key with
its micro-batch term, the numpy float32 restatement of the pass that the device tests compare against, and every argument check of
rsu_grad_accumulate, which returns before anything touches a device."""
import os
import re

import numpy as np
import pytest

from road_segmentation_unet_amd import _lib
from road_segmentation_unet_amd.cli import parse_options
from road_segmentation_unet_amd.dist import micro_indices, shard_indices
from road_segmentation_unet_amd.model import EXTRA_FLAG_DEFS, Options, micro_batch_size, parse_accumulate_steps
from road_segmentation_unet_amd.unet import dropout_key_value
from tests import accum_util as au

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
EINVAL, E2BIG = -22, -7


# ------------------------------------------------------------------------------------------- the flag
def test_flag_default_and_parsing():
    assert Options().accumulate_steps == 1 and parse_options([]).accumulate_steps == 1      # off by default
    assert parse_options(["--accumulate_steps=2", "--batch_size=8"]).accumulate_steps == 2
    assert Options(accumulate_steps=5).accumulate_steps == 5                                 # the default batch of 25 divides
    assert Options(accumulate_steps=np.int64(5)).accumulate_steps == 5
    defs = {d[0]: d for d in EXTRA_FLAG_DEFS}
    assert defs["accumulate_steps"][1:3] == (int, 1)
    assert "per micro-batch" in defs["accumulate_steps"][3] and "Dice" in defs["accumulate_steps"][3]


@pytest.mark.parametrize("value", [0, -1, -4, 1.5, 2.0, "2", None, True, False, float("nan")])
def test_parse_accumulate_steps_rejects(value):
    with pytest.raises(ValueError):
        parse_accumulate_steps(value)


def test_options_reject_bad_and_non_dividing_values():
    for bad in ("--accumulate_steps=0", "--accumulate_steps=-2"):
        with pytest.raises(ValueError):
            parse_options([bad])
    with pytest.raises(ValueError, match="25.*2"):
        parse_options(["--accumulate_steps=2"])                  # 25 patches do not cut into 2 micro-batches
    with pytest.raises(ValueError):
        Options(batch_size=8, accumulate_steps=3)
    assert Options(batch_size=8, accumulate_steps=4).accumulate_steps == 4


def test_micro_batch_size_names_all_three_numbers():
    assert micro_batch_size(8, 1, 1) == 8 and micro_batch_size(8, 2, 2) == 2 and micro_batch_size(24, 2, 3) == 4
    with pytest.raises(ValueError) as e:
        micro_batch_size(12, 2, 4)
    assert all(re.search(r"\b%d\b" % v, str(e.value)) for v in (12, 2, 4)), str(e.value)
    with pytest.raises(ValueError):
        micro_batch_size(0, 1, 2)


# ------------------------------------------------------------------------------------------- micro_indices
@pytest.mark.parametrize("world,K,batch,offset", [(1, 1, 6, 0), (1, 2, 8, 8), (2, 2, 8, 16), (4, 3, 24, 5), (2, 1, 10, 3), (1, 4, 4, 0)])
def test_micro_indices_cut_the_ranks_share_contiguously(world, K, batch, offset):
    indices = np.random.RandomState(world * 10 + K).permutation(64)
    parts = [micro_indices(indices, offset, batch, r, world, m, K) for r in range(world) for m in range(K)]
    per = batch // (world * K)
    assert all(len(p) == per for p in parts)
    np.testing.assert_array_equal(np.concatenate(parts), indices[offset:offset + batch])     # disjoint, contiguous, in order, the whole batch
    for r in range(world):   # the K parts of a rank are that rank's shard, in order
        np.testing.assert_array_equal(np.concatenate([micro_indices(indices, offset, batch, r, world, m, K) for m in range(K)]),
                                      shard_indices(indices, offset, batch, r, world))
    if K == 1:
        for r in range(world):
            np.testing.assert_array_equal(micro_indices(indices, offset, batch, r, world, 0, 1), shard_indices(indices, offset, batch, r, world))


def test_micro_indices_rejects_what_does_not_divide():
    indices = np.arange(32)
    with pytest.raises(ValueError, match="10.*2.*3"):
        micro_indices(indices, 0, 10, 0, 2, 0, 3)
    for micro in (-1, 2):
        with pytest.raises(ValueError):
            micro_indices(indices, 0, 8, 0, 2, micro, 2)


# ------------------------------------------------------------------------------------------- the dropout key
def test_dropout_key_is_todays_key_at_micro_step_0():
    for seed in (0, 5, 2017, 2017 + 7919 * 3, 2 ** 31 - 1):
        for site in (0, 1, 4, 9):
            for step in (0, 1, 999, 1000, 123456):
                today = (seed * 0x9E3779B9 + site * 0x85EBCA6B + step * 0xC2B2AE35) & 0xFFFFFFFF
                assert dropout_key_value(seed, site, step) == today == dropout_key_value(seed, site, step, 0) == au.host_dropout_key(seed, site, step)
                keys = [dropout_key_value(seed, site, step, m) for m in range(4)]
                assert keys == [au.host_dropout_key(seed, site, step, m) for m in range(4)]
                assert len(set(keys)) == 4 and all(0 <= k < 2 ** 32 for k in keys)


def test_micro_step_multiplier_is_odd_and_its_own():
    """an odd multiplier maps micro_step one-to-one modulo 2^32; it differs from the three others, so (step, micro) = (s, 1) is not (s + 1, 0)"""
    m = (dropout_key_value(0, 0, 0, 1) - dropout_key_value(0, 0, 0, 0)) & 0xFFFFFFFF
    assert m & 1 and m not in (0x9E3779B9, 0x85EBCA6B, 0xC2B2AE35)
    assert dropout_key_value(3, 2, 10, 1) != dropout_key_value(3, 2, 11, 0) and dropout_key_value(3, 2, 10, 1) != dropout_key_value(3, 3, 10, 0)


# ------------------------------------------------------------------------------------------- the restatement
def test_restatement_assign_forgets_and_add_rounds_once():
    a = np.array([1.0, 2.0 ** 24, -0.0, np.inf, np.inf, np.nan, 1e38, 0.1], f32)
    b = np.array([2.0 ** -24, 1.0, -0.0, -np.inf, 1.0, 1.0, 3e38, 0.2], f32)
    out = au.host_accumulate(np.full(8, np.nan, f32), b, True)
    assert au.same(out, b) and out is not b                       # assign: the nan in dst is forgotten
    out = au.host_accumulate(a, b, False)
    assert out.dtype == f32
    assert out[0] == f32(1.0) and out[1] == f32(2.0 ** 24)        # one rounding to float32: 1 + 2^-24 and 2^24 + 1 round to even
    assert np.signbit(out[2]) and out[2] == 0.0                   # -0 + -0 = -0
    assert np.isnan(out[3]) and out[4] == np.inf and np.isnan(out[5]) and out[6] == np.inf   # inf - inf, inf + 1, nan + 1, overflow
    assert out[7].tobytes() == (f32(0.1) + f32(0.2)).tobytes()


def test_restatement_sum_order_is_left_to_right():
    a, b, c = f32(2.0 ** 24), f32(1.0), f32(1.0)
    assert au.host_sum([[a], [b], [c]])[0] == f32(2.0 ** 24)      # (a + b) + c: each 1 is lost; a + (b + c) would give 2^24 + 2
    assert au.host_sum([[b], [c], [a]])[0] == f32(2.0 ** 24 + 2.0)
    rng = np.random.RandomState(0)
    g = [rng.randn(1000).astype(f32) for _ in range(4)]
    want = ((g[0] + g[1]).astype(f32) + g[2]).astype(f32) + g[3]
    assert au.same(au.host_sum(g), want.astype(f32))
    assert au.same(au.host_sum(g[:1]), g[0])


# ------------------------------------------------------------------------------------------- the ABI
def test_symbol_is_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "rsu.h")).read()
    assert "optimizer: gradient accumulation over micro-batches (new)" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint rsu_grad_accumulate\s*\(([^)]*)\)", code)
    assert m, "rsu_grad_accumulate is not declared in rsu.h"
    assert len(m.group(1).split(",")) == 5 == len(_lib.SIGNATURES["rsu_grad_accumulate"][1])
    share = re.search(r"#define RSU_GRAD_ACCUMULATE_BLOCK_FLOATS (\d+)", code)
    assert share and int(share.group(1)) == _lib.GRAD_ACCUMULATE_BLOCK_FLOATS
    hdr = open(os.path.join(ROOT, "road_segmentation_unet_amd", "csrc", "optim.h")).read()
    assert re.search(r"constexpr int EW_ACC_EPB = (\d+);", hdr).group(1) == share.group(1)
    assert hasattr(_lib.lib(), "rsu_grad_accumulate")


def test_pure_host_argument_checks():
    """every RSU_EINVAL of rsu_grad_accumulate and its RSU_E2BIG, with addresses that are never dereferenced: each call fails its checks
    before any HIP call"""
    acc = _lib.lib().rsu_grad_accumulate
    d, s = 0x100000, 0x200000      # 16-byte aligned, 1 MiB apart
    for assign in (0, 1):
        assert acc(None, s, 8, assign, None) == EINVAL
        assert acc(d, None, 8, assign, None) == EINVAL
        for n in (0, -1, -4):
            assert acc(d, s, n, assign, None) == EINVAL
        for off in (4, 8, 12):
            assert acc(d + off, s, 8, assign, None) == EINVAL       # dst not 16-byte aligned
            assert acc(d, s + off, 8, assign, None) == EINVAL       # src not 16-byte aligned
        # overlapping ranges: the same buffer, src starting inside dst, dst starting inside src, the last float4 of dst shared
        assert acc(d, d, 8, assign, None) == EINVAL
        assert acc(d, d + 16, 8, assign, None) == EINVAL
        assert acc(d + 16, d, 8, assign, None) == EINVAL
        assert acc(d, d + 4 * 1024 - 16, 1024, assign, None) == EINVAL
        # a grid of 2^31 - 1 workgroups or more (checked before the overlap test: the ranges below would overlap)
        assert acc(d, s, (2 ** 31 - 1) * _lib.GRAD_ACCUMULATE_BLOCK_FLOATS, assign, None) == E2BIG
