"""conv1x1_stats (read-once 1x1 convolution forward + BatchNorm partial
sums) against the exact-arithmetic method of tests/ops/_exact.py:
integer-valued bf16 operands, fp64 reference.

Large operands (|a|, |w| <= 16, outputs round): C bit for bit against
the rounded reference; the slab totals within the fp32 summation bound
M u / (1 - M u), u = 2^-24, relative to sum|v| (sums) and sum v^2 (sums
of squares; v^2 of a bf16 v is exact in fp32) per column. The bound is
that of an fp32 sum of M terms in any order, not a tuned figure.

Small operands (entries in {-1, 0, 1}): nothing rounds and every
partial sum is an integer below 2^24 (checked on the CPU in
test_conv1x1_stats_cpu.py), so the slab totals are exact and the fused
forward equals bn_fwd(gemm_stream(A, W)) bit for bit.
"""

import pytest
import torch

from tests.ops import _conv1x1_stats as cs
from tests.ops import _exact as ex

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sparkdl.ops as ops


@pytest.fixture(autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")


_ids = lambda s: "x".join(map(str, s))  # noqa: E731


def _check_large(M, N, K, cap):
    C = ops.ext()
    A, W = cs.operands(M, N, K, "cuda", cs.LARGE_AMAX)
    want = ex.to_bf16(ex.ref_exact(A, W))
    p = cs.plan(M, N, K, cap)
    assert list(C.conv1x1_stats_plan(M, N, K, cap)) == [p.nch, p.G]
    # NaN-filled slab: every entry must be overwritten
    slab = torch.full((p.G, 2 * N), float("nan"), device="cuda")
    got, out = C.conv1x1_stats(A, W, cap, slab)
    assert out.data_ptr() == slab.data_ptr()
    ex.assert_equal(got, want, "C %s" % ((M, N, K, cap),))
    assert torch.isfinite(slab).all(), "slab rows not fully written"
    s1, s2, sa = cs.column_sums(want)
    tot = slab.double().sum(0)
    gamma = cs.sum_bound(M)
    e1 = (tot[:N] - s1).abs()
    e2 = (tot[N:] - s2).abs()
    print("M=%d N=%d K=%d G=%d: sum err/bound %.3g, sumsq err/bound %.3g"
          % (M, N, K, p.G,
             (e1 / (gamma * sa).clamp_min(1e-300)).max().item(),
             (e2 / (gamma * s2).clamp_min(1e-300)).max().item()))
    assert bool((e1 <= gamma * sa).all())
    assert bool((e2 <= gamma * s2).all())
    # a second call gives the same bits, into a fresh slab
    got2, slab2 = C.conv1x1_stats(A, W, cap)
    assert torch.equal(got2, got)
    assert torch.equal(slab2, slab)


@pytest.mark.parametrize("M,N,K", cs.SHAPES,
                         ids=[_ids(s) for s in cs.SHAPES])
def test_large_operands(M, N, K):
    _check_large(M, N, K, 0)


@pytest.mark.parametrize("K,N", list(cs.CLASSES),
                         ids=[_ids(s) for s in cs.CLASSES])
def test_large_operands_multi_trip(K, N):
    _check_large(cs.LOOP_M, N, K, cs.LOOP_CAP)


def _check_small(M, N, K, cap):
    C = ops.ext()
    A, W = cs.operands(M, N, K, "cuda", 1)
    ref = ex.ref_exact(A, W)
    got, slab = C.conv1x1_stats(A, W, cap)
    ex.assert_equal(got, ex.to_bf16(ref), "C %s" % ((M, N, K, cap),))
    s1, s2, _ = cs.column_sums(ex.to_bf16(ref))
    tot = slab.double().sum(0)
    assert torch.equal(tot[:N], s1) and torch.equal(tot[N:], s2)
    plain = C.gemm_stream(A, W)
    assert torch.equal(plain, got)
    res = cs.residual_operand(M, N, "cuda")
    gamma = torch.linspace(0.5, 1.5, N, device="cuda")
    beta = torch.linspace(-1.0, 1.0, N, device="cuda")
    for relu in (True, False):
        for r in (None, res):
            rm = [torch.zeros(N, device="cuda") for _ in range(2)]
            rv = [torch.ones(N, device="cuda") for _ in range(2)]
            fused = C.bn_fwd_slab(got, r, slab, gamma, beta, rm[0], rv[0],
                                  0.1, 1e-5, relu)
            base = C.bn_fwd(plain, r, gamma, beta, rm[1], rv[1], 0.1,
                            1e-5, True, relu)
            what = "M=%d N=%d K=%d relu=%s res=%s" % (M, N, K, relu,
                                                      r is not None)
            for f, b, name in zip(fused, base,
                                  ("y", "save_mean", "save_rstd", "mask")):
                assert torch.equal(f, b), (what, name)
            assert torch.equal(rm[0], rm[1]), what
            assert torch.equal(rv[0], rv[1]), what


@pytest.mark.parametrize("M,N,K", cs.SHAPES,
                         ids=[_ids(s) for s in cs.SHAPES])
def test_small_operands_fused_forward(M, N, K):
    _check_small(M, N, K, 0)


@pytest.mark.parametrize("K,N", list(cs.CLASSES),
                         ids=[_ids(s) for s in cs.CLASSES])
def test_small_operands_multi_trip(K, N):
    _check_small(cs.LOOP_M, N, K, cs.LOOP_CAP)


def test_bad_arguments_raise():
    C = ops.ext()
    A = torch.zeros(64, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        C.conv1x1_stats(A, torch.zeros(32, 64, device="cuda",
                                       dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):
        C.conv1x1_stats(torch.zeros(64, 96, device="cuda",
                                    dtype=torch.bfloat16),
                        torch.zeros(64, 96, device="cuda",
                                    dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):   # slab of the wrong shape
        C.conv1x1_stats(A, A, 0, torch.zeros(2, 128, device="cuda"))
