"""No GPU: hiputil.assert_bf16_rounded has teeth. torch on the CPU plays the kernel on two of test_gpu_ops.CONV_SHAPES with that test's
seeds and distributions; the reference is a float64 conv. A float32 conv rounded once to nearest (what a correct MFMA kernel does) must
pass with a wide margin; every mistake the statistic exists for -- a truncating store, partial sums kept in bf16, the bias added after
the conversion, truncated weight copies, a single element 2 ulps off, an output that is mostly zeros -- must raise."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import hiputil as hu

SHAPES = [
    # N, H, W, Cin, Cout, relu  (test_gpu_ops.CONV_SHAPES rows)
    (2, 37, 41, 64, 64, True),
    (1, 30, 30, 16, 16, False),
]


def _rand(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _trunc(a):
    """bf16 by dropping the low 16 bits of the float32 (towards zero)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _rne(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float32)


def _conv(x, w, dtype):
    """NHWC x HWIO valid 3x3 conv, no bias, in `dtype`"""
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).permute(0, 3, 1, 2)
    wt = torch.from_numpy(np.ascontiguousarray(w)).to(dtype).permute(3, 2, 0, 1)
    return F.conv2d(xt, wt).permute(0, 2, 3, 1).contiguous()


class Case:
    def __init__(self, N, H, W, Cin, Cout, relu):
        rng = np.random.RandomState(Cin * 7 + Cout + H)   # test_conv2d_fwd's inputs
        self.x = hu.q(_rand(rng, N, H, W, Cin))
        self.w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
        self.b = _rand(rng, Cout, scale=0.1)
        self.relu, self.Cin = relu, Cin
        self.bt = torch.from_numpy(self.b)
        self.ref = self.act(_conv(self.x, hu.q(self.w), torch.float64) + self.bt.double()).numpy()   # float64, not rounded
        self.good = _rne(self.act(_conv(self.x, hu.q(self.w), torch.float32) + self.bt)).numpy()       # fp32 accumulate, one RNE

    def act(self, t):
        return torch.relu(t) if self.relu else t


def _raises_twice(case, got, what):
    """`got` must raise as it is, and -- with the few elements that the 1-ulp tolerance of assert_bf16_close already catches (small
    results of cancelling sums) replaced by the right values -- raise again on the statistic alone"""
    with pytest.raises(AssertionError):
        hu.assert_bf16_rounded(got, case.ref, what)
    refq = hu.q(case.ref)
    tol = hu.BF16_ULP * np.abs(refq) + 2e-5 * float(np.abs(refq).max())
    inside = np.where(np.abs(got - refq) <= tol, got, case.good)
    hu.assert_bf16_close(inside, case.ref, what)
    with pytest.raises(AssertionError, match="not one round-to-nearest"):
        hu.assert_bf16_rounded(inside, case.ref, what + ", within 1 ulp everywhere")


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def case(request):
    return Case(*request.param)


def test_float32_accumulate_one_rounding_passes_with_margin(case):
    mismatch, bias, n = hu.assert_bf16_rounded(case.good, case.ref, "float32 conv")
    print("float32 stand-in: mismatch %.6f bias %+.5f n %d" % (mismatch, bias, n))
    assert n >= 10000
    assert mismatch <= 0.002 and abs(bias) <= 0.01, (mismatch, bias, n)   # the margin the limits 0.01 / 0.02 were derived with


def test_truncating_store_raises(case):
    with pytest.raises(AssertionError, match="bias -0\\.[45]"):
        hu.assert_bf16_rounded(_trunc(case.ref.astype(np.float32)), case.ref, "truncated")


def test_two_bf16_rounded_halves_raise(case):
    h = case.Cin // 2
    qw = hu.q(case.w)
    a = _rne(_conv(case.x[..., :h], qw[:, :, :h], torch.float32) + case.bt)
    b = _rne(_conv(case.x[..., h:], qw[:, :, h:], torch.float32))
    _raises_twice(case, _rne(case.act(a + b)).numpy(), "bf16 partial sums")


def test_bias_after_the_rounding_raises(case):
    got = _rne(case.act(_rne(_conv(case.x, hu.q(case.w), torch.float32)) + case.bt)).numpy()
    _raises_twice(case, got, "bias after the conversion")


def test_truncated_weight_copy_raises(case):
    got = _rne(case.act(_conv(case.x, _trunc(case.w), torch.float32) + case.bt)).numpy()
    _raises_twice(case, got, "truncated weights")


def test_one_element_two_ulps_off_raises(case):
    refq = hu.q(case.ref)
    mant = np.abs(refq) / 2.0 ** np.floor(np.log2(np.maximum(np.abs(refq), 1e-30)))
    cand = np.where(np.abs(refq) >= 0.5 * np.abs(refq).max(), mant, np.inf)   # a large element low in its binade: 2 ulps are 2^-6 relative there
    idx = np.unravel_index(np.argmin(cand), cand.shape)
    got = case.good.copy()
    got[idx] = refq[idx] + 2 * 2.0 ** (np.floor(np.log2(abs(refq[idx]))) - 7)
    assert hu.q(got[idx]) == got[idx]
    with pytest.raises(AssertionError, match="1/%d elements out of tolerance" % got.size):
        hu.assert_bf16_rounded(got, case.ref, "one element 2 ulps off")


def test_mostly_zero_output_raises(case):
    keep = (np.random.RandomState(1).rand(*case.ref.shape) < (0.6 if case.relu else 0.3))   # ReLU already zeroes half
    got, ref = case.good * keep, case.ref * keep
    assert (hu.q(ref) == 0).mean() > 0.69
    with pytest.raises(AssertionError, match="not measurable"):
        hu.assert_bf16_rounded(got, ref, "70 % zeros")


def test_too_few_elements_raise(case):
    got, ref = case.good[:1, :6, :6], case.ref[:1, :6, :6]
    assert got.size < 10000
    with pytest.raises(AssertionError, match="not measurable"):
        hu.assert_bf16_rounded(got, ref, "a handful of elements")
