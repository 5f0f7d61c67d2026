"""CPU checks of the exact-arithmetic method behind
tests/ops/test_gemm_exact_gpu.py: the bound, the reference, that the
chosen operands really exercise the bf16 rounding (ties included), the
derived GELU bound against torch's own fp32 GELU, and that every shape
sits in the launch class it was chosen for."""

import pytest
import torch

from . import _exact as ex

CPU = "cpu"
# the strided-loop case (128 MiB operands) is the only one left to the GPU
SMALL_GEMM = ([("gemm256",) + s for s in ex.GEMM256_SHAPES]
              + [("stream",) + s for s in ex.STREAM_SHAPES])


def _operands(kind, M, N, K, bias):
    if kind == "gemm256":
        return ex.gemm_operands(
            kind, M, N, K, CPU, ex.GEMM256_AMAX, ex.GEMM256_AMAX,
            ex.GEMM256_BIAS_AMAX if bias else None)
    return ex.gemm_operands(kind, M, N, K, CPU, ex.STREAM_AMAX,
                            ex.STREAM_AMAX)


def test_int_operand_range_and_exactness():
    g = ex.case_generator("range")
    a = ex.int_operand((64, 33), 16, CPU, g)
    assert a.dtype == torch.bfloat16
    assert a.float().abs().max() == 16
    assert torch.equal(a.float(), a.float().round())
    assert a.float().unique().numel() == 33
    b = ex.int_operand((4096,), 8, CPU, g, half=True)
    assert b.dtype == torch.float32
    assert b.abs().max() == 8
    assert torch.equal(b * 2, (b * 2).round())
    assert bool(((b * 2) % 2 != 0).any())
    with pytest.raises(AssertionError):
        ex.int_operand((4,), 17, CPU, g)


def test_case_generators_differ():
    a = ex.int_operand((256,), 16, CPU, ex.case_generator("k", 1, 2, 3, 0))
    b = ex.int_operand((256,), 16, CPU, ex.case_generator("k", 1, 2, 3, 1))
    c = ex.int_operand((256,), 16, CPU, ex.case_generator("k", 1, 2, 3, 0))
    assert torch.equal(a, c) and not torch.equal(a, b)


def test_exact_bound_rejects_over_range():
    assert ex.check_exact_bound(16, 16, 20544) == 16 * 16 * 20544
    with pytest.raises(AssertionError):
        ex.check_exact_bound(16, 16, 65536)          # == 2^24
    with pytest.raises(AssertionError):
        ex.check_exact_bound(16, 16, 65535, 256.0)   # bias tips it over
    with pytest.raises(AssertionError):
        ex.check_exact_bound(16, 16, 32768, 0.5)     # half-integers: 2^23
    ex.check_exact_bound(16, 16, 65535)


def test_every_gpu_case_is_within_the_bound():
    for (M, N, K) in ex.GEMM256_SHAPES:
        ex.check_exact_bound(ex.GEMM256_AMAX, ex.GEMM256_AMAX, K,
                             ex.GEMM256_BIAS_AMAX)
    for (M, N, K) in ex.STREAM_SHAPES + [ex.STREAM_LOOP_SHAPE]:
        ex.check_exact_bound(ex.STREAM_AMAX, ex.STREAM_AMAX, K)
    for (M, N, K) in ex.WGRAD_SHAPES:
        ex.check_exact_bound(ex.WGRAD_AMAX, ex.WGRAD_AMAX, M)


@pytest.mark.parametrize("kind,M,N,K", SMALL_GEMM)
def test_ref_fp32_equals_fp64_and_rounding_is_exercised(kind, M, N, K):
    """fp32 is exact under the bound (so any fp32 accumulation order
    must reproduce it), and the reference is not trivially bf16-exact:
    >= 1% of the outputs are changed by the bf16 store and at least one
    is an exact tie, which is what makes the GPU comparison check RNE."""
    for bias in ((True, False) if kind == "gemm256" else (False,)):
        A, W, b = _operands(kind, M, N, K, bias)
        r64 = ex.ref_exact(A, W, b)
        r32 = ex.ref_exact(A, W, b, dtype=torch.float32)
        assert r64.dtype == torch.float64 and r32.dtype == torch.float32
        assert torch.equal(r32.double(), r64)
        chunked = ex.ref_exact(A, W, b, dtype=torch.float32, chunk_rows=100)
        assert torch.equal(chunked, r32)
        frac, ties = ex.rounding_stats(r64)
        assert frac >= 0.01, (kind, M, N, K, bias, frac)
        assert ties >= 1, (kind, M, N, K, bias, ties)


def test_rounding_stats_on_known_values():
    # 257 and 259 are ties in [256, 512) (ulp 2); 513 rounds down, no
    # tie (ulp 4); 514 is a tie; 128.5 is a tie (ulp 1)
    ref = torch.tensor([1., 256., 257., 259., 513., 514., 128.5, 3.],
                       dtype=torch.float64)
    frac, ties = ex.rounding_stats(ref)
    assert frac == 5 / 8 and ties == 4
    # RNE on the ties: to the even bf16 neighbour
    assert ex.to_bf16(ref).tolist() == [1., 256., 256., 260., 512., 512.,
                                        128., 3.]


@pytest.mark.parametrize("M,N,K", ex.WGRAD_SHAPES)
def test_wgrad_ref_fp32_equals_fp64(M, N, K):
    for call in (0, 1):
        dz, x = ex.wgrad_operands(M, N, K, CPU, call)
        r64 = ex.ref_exact(dz.t(), x.t())
        assert r64.shape == (N, K)
        assert torch.equal(
            ex.ref_exact(dz.t(), x.t(), dtype=torch.float32).double(), r64)
    # the two calls of one shape use different operands
    assert not torch.equal(ex.wgrad_operands(M, N, K, CPU, 0)[0], dz)


def _gelu_cases():
    for (M, N, K) in ex.GELU_SHAPES:
        yield ex.gemm_operands("gelu", M, N, K, CPU, ex.GELU_AMAX[0],
                               ex.GELU_AMAX[1], ex.GELU_BIAS_AMAX)
    for (M, N, K) in ex.GEMM256_SHAPES:
        yield _operands("gemm256", M, N, K, True)
        yield _operands("gemm256", M, N, K, False)


def test_torch_fp32_gelu_satisfies_the_bound():
    """The derived bound holds for an independent fp32 implementation
    (torch's CPU erf-GELU followed by the bf16 store)."""
    for A, W, b in _gelu_cases():
        z = ex.ref_exact(A, W, b)
        y = torch.nn.functional.gelu(z.float()).bfloat16()
        ex.assert_gelu_within_bound(y, z)


def test_gelu_bound_is_tight_enough_to_notice_errors():
    """One bf16 ulp off, tanh-GELU, or a forgotten bias each break it."""
    A, W, b = ex.gemm_operands("gelu", 257, 77, 64, CPU, ex.GELU_AMAX[0],
                               ex.GELU_AMAX[1], ex.GELU_BIAS_AMAX)
    z = ex.ref_exact(A, W, b)
    mid = (z.abs() > 0.4) & (z.abs() < 4)
    assert mid.double().mean() > 0.1     # GELU is non-trivial here
    y = torch.nn.functional.gelu(z.float()).bfloat16()
    two_ulp = (y.view(torch.int16) + 2).view(torch.bfloat16)
    with pytest.raises(AssertionError):
        ex.assert_gelu_within_bound(two_ulp, z)
    tanh = torch.nn.functional.gelu(z.float(), approximate="tanh").bfloat16()
    with pytest.raises(AssertionError):
        ex.assert_gelu_within_bound(tanh, z)
    nobias = torch.nn.functional.gelu(
        ex.ref_exact(A, W).float()).bfloat16()
    with pytest.raises(AssertionError):
        ex.assert_gelu_within_bound(nobias, z)


def test_assert_equal_reports_indices():
    a = torch.zeros(4, 5)
    b = a.clone()
    b[2, 3] = 1
    ex.assert_equal(a, a.clone())
    with pytest.raises(AssertionError, match=r"1 of 20.*\[2, 3\]"):
        ex.assert_equal(a, b, "x")


def test_gemm256_shapes_cover_the_edges():
    for K in (64, 192):
        assert {M for (M, N, k) in ex.GEMM256_SHAPES if k == K} \
            >= set(ex.GEMM256_ROWS), K
        assert {N for (M, N, k) in ex.GEMM256_SHAPES if k == K} \
            >= set(ex.GEMM256_COLS), K
    assert {K for (_, _, K) in ex.GEMM256_SHAPES} == {64, 128, 192}
    assert all(M != N for (M, N, _) in ex.GEMM256_SHAPES)
    nwg = {ex.gemm256_nwg(M, N) for (M, N, _) in ex.GEMM256_SHAPES}
    assert nwg >= {1, 2, 3, 9, 18}
    assert ex.gemm256_nwg(513, 520) == 9 and ex.gemm256_nwg(1281, 513) == 18
    # the swizzle's remainder branch: nwg > 8 with nwg % 8 != 0
    assert any(n > 8 and n % 8 for n in nwg)


def test_wgrad_shapes_land_in_their_classes():
    for (M, N, K), want in ex.WGRAD_SHAPES.items():
        assert M % 64 == 0 and N % 256 == 0 and K % 128 == 0
        assert ex.wgrad_plan(M, N, K) == want, (M, N, K)
    plans = list(ex.WGRAD_SHAPES.values())
    assert any(p[0] == 1 for p in plans)                  # plain store
    assert any(p[3] > 0 for p in plans)                   # empty splits
    # tiles per split 1, 2, 3 (prologue variants) and > 3 (buffer wrap)
    per_split = {p[1] for p in plans} | {p[2] for p in plans}
    assert per_split >= {1, 2, 3, 5}
    # the shapes of the older allclose test never leave the atomic path
    for shape in [(256, 256, 128), (4096, 512, 256), (8192, 256, 384)]:
        assert ex.wgrad_plan(*shape)[0] > 1


def test_stream_shapes_land_in_their_classes():
    for (M, N, K) in ex.STREAM_SHAPES:
        # (64, 64, K) is the one square output of the grid; A and W
        # are independent draws there too
        assert K in (64, 128, 256) and N % 64 == 0
        mblocks, workers = ex.stream_plan(M, N)
        assert mblocks <= workers          # one trip of the worker loop
    assert {ex.stream_plan(M, N)[0] for (M, N, _) in ex.STREAM_SHAPES} \
        == {1, 2, 3}
    M, N, K = ex.STREAM_LOOP_SHAPE
    mblocks, workers = ex.stream_plan(M, N)
    assert (mblocks, workers) == (1026, 1024)   # workers 0, 1 loop twice
    assert M % 1024 == 40                       # ragged last block
    # one block fewer and the loop never takes a second trip
    fewer = ex.stream_plan(M - 1024 - 40, N)
    assert fewer[0] <= fewer[1]
