"""Exact-arithmetic refchecks for the GEMM kernel family (gemm_bias_act,
gemm_stream, wgrad_splitk, transpose_bf16) at tile edges.

Operands are small integers held in bf16, so every fp32 accumulation is
exact and the kernels must reproduce the fp64 reference bit for bit
(after the documented round-to-nearest-even bf16 store); see
tests/ops/_exact.py. The only tolerances here are the derived GELU
bound and one bf16 ulp on outputs computed by the library GEMM.

Odd N in gemm_bias_act: the epilogue's bf16x8 store is a 16-byte access
through a pointer type that promises the compiler 16-byte alignment,
and no documentation at hand makes such a store legal on gfx950 at a
2-byte aligned address. It was not tried: store_out sends every N with
N % 8 != 0 down its element-wise path instead. N in {1, 7, 77, 100}
below run that path, N in {256, 264} the vector one."""

import functools

import pytest
import torch

from . import _exact as ex

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sparkdl.ops as ops
    from sparkdl.ops import functional as F_

DEV = "cuda"
ONE_ULP = dict(rtol=2.0 ** -7, atol=0.0)   # library-computed outputs only


@pytest.fixture(autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")


def _ids(cases):
    return ["-".join(str(int(v)) for v in c) for c in cases]


# ---------------------------------------------------------------------------
# gemm_bias_act
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gemm256_case(kind, M, N, K):
    """Operands and fp64 references of one shape, computed once and
    shared by its variants (never modified)."""
    if kind == "gemm256":
        amax_a = amax_w = ex.GEMM256_AMAX
        bias_amax = ex.GEMM256_BIAS_AMAX
    else:
        amax_a, amax_w = ex.GELU_AMAX
        bias_amax = ex.GELU_BIAS_AMAX
    A, W, bias = ex.gemm_operands(kind, M, N, K, DEV, amax_a, amax_w,
                                  bias_amax)
    return A, W, bias, ex.ref_exact(A, W, bias), ex.ref_exact(A, W)


def _check_gemm256(kind, M, N, K, act, use_bias, save_z):
    A, W, bias, z_bias, z_nobias = _gemm256_case(kind, M, N, K)
    z_ref = z_bias if use_bias else z_nobias
    what = "gemm_bias_act %s act=%d bias=%s" % ((M, N, K), act, use_bias)
    out = ops.ext().gemm_bias_act(A, W, bias if use_bias else None, act,
                                  save_z)
    assert len(out) == (2 if act == 1 and save_z else 1)
    y = out[0]
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    if act == 0:
        ex.assert_equal(y, ex.to_bf16(z_ref), what + " y")
        return
    if save_z:
        ex.assert_equal(out[1], ex.to_bf16(z_ref), what + " z")
    ex.assert_gelu_within_bound(y, z_ref)


@pytest.mark.parametrize("act,use_bias,save_z", ex.GEMM256_VARIANTS,
                         ids=_ids(ex.GEMM256_VARIANTS))
@pytest.mark.parametrize("M,N,K", ex.GEMM256_SHAPES,
                         ids=_ids(ex.GEMM256_SHAPES))
def test_gemm_bias_act_exact(M, N, K, act, use_bias, save_z):
    _check_gemm256("gemm256", M, N, K, act, use_bias, save_z)


@pytest.mark.parametrize("M,N,K", ex.GELU_SHAPES, ids=_ids(ex.GELU_SHAPES))
def test_gemm_bias_gelu_midrange(M, N, K):
    """Small sums, so that z lies where GELU is neither 0 nor z."""
    _check_gemm256("gelu", M, N, K, 1, True, True)
    _check_gemm256("gelu", M, N, K, 1, False, False)


# ---------------------------------------------------------------------------
# gemm_stream
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K", ex.STREAM_SHAPES,
                         ids=_ids(ex.STREAM_SHAPES))
def test_gemm_stream_exact(M, N, K):
    A, W, _ = ex.gemm_operands("stream", M, N, K, DEV, ex.STREAM_AMAX,
                               ex.STREAM_AMAX)
    got = ops.ext().gemm_stream(A, W)
    ex.assert_equal(got, ex.to_bf16(ex.ref_exact(A, W)),
                    "gemm_stream %s" % ((M, N, K),))


def test_gemm_stream_worker_loop_second_trip():
    """1026 m-blocks on 1024 workers: workers 0 and 1 run a second
    block (rows 2^20 .. 2^20+1063), the last one ragged. Every row is
    compared; the reference is fp32 in row chunks (exact under the
    bound, and no fp64 copy of the 128 MiB operand)."""
    M, N, K = ex.STREAM_LOOP_SHAPE
    assert ex.stream_plan(M, N) == (1026, 1024)
    A, W, _ = ex.gemm_operands("stream", M, N, K, DEV, ex.STREAM_AMAX,
                               ex.STREAM_AMAX)
    got = ops.ext().gemm_stream(A, W)
    assert got.shape == (M, N) and got.dtype == torch.bfloat16
    rows = 1 << 16
    bad = []
    for r0 in range(0, M, rows):
        want = ex.to_bf16(ex.ref_exact(A[r0:r0 + rows], W,
                                       dtype=torch.float32))
        wrong = (got[r0:r0 + rows] != want).any(dim=1)
        if bool(wrong.any()):
            bad.append(r0 + int(wrong.nonzero()[0]))
    del A, W, got, want, wrong
    torch.cuda.empty_cache()
    assert not bad, "first wrong row of each 65536-row chunk: %s" % bad


# ---------------------------------------------------------------------------
# wgrad_splitk (fp32 output: the exact reference itself, no rounding)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K", list(ex.WGRAD_SHAPES),
                         ids=_ids(ex.WGRAD_SHAPES))
def test_wgrad_splitk_exact(M, N, K):
    """Twice with different operands: the output is zero-filled by the
    launcher only when splits > 1, so a stale accumulator would show in
    the second call."""
    for call in (0, 1):
        dz, x = ex.wgrad_operands(M, N, K, DEV, call)
        got = ops.ext().wgrad_splitk(dz, x)
        assert got.dtype == torch.float32
        want = ex.ref_exact(dz.t(), x.t())
        ex.assert_equal(got, want.float(),
                        "wgrad_splitk %s plan %s call %d"
                        % ((M, N, K), ex.wgrad_plan(M, N, K), call))
        assert torch.equal(got.double(), want)


# ---------------------------------------------------------------------------
# transpose_bf16
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("R,C", [(1, 1), (7, 513), (65, 9), (513, 7)])
def test_transpose_bf16_edges(R, C):
    g = ex.case_generator("transpose", R, C)
    X = ex.int_operand((R, C), 16, DEV, g) \
        * ex.int_operand((R, C), 16, DEV, g)      # 200+ distinct values
    Y = ops.ext().transpose_bf16(X)
    assert Y.shape == (C, R) and Y.is_contiguous()
    assert torch.equal(Y, X.t().contiguous())


# ---------------------------------------------------------------------------
# routing layer: the Python entry points pick the kernel
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("K,in_house", [(128, True), (512, True),
                                        (96, False)])
def test_conv_gemm_routes_exact(K, in_house):
    """K=128: streaming kernel; K=512: 256x256 kernel with bias=None;
    K=96: library GEMM."""
    M, N = 300, 192
    A, W, _ = ex.gemm_operands("conv_gemm", M, N, K, DEV, 16, 16)
    got = F_._conv_gemm(A, W)
    want = ex.to_bf16(ex.ref_exact(A, W))
    if in_house:
        ex.assert_equal(got, want, "_conv_gemm K=%d" % K)
    else:
        assert torch.allclose(got.float(), want.float(), **ONE_ULP)


def test_conv1x1_backward_exact():
    """dx = dy @ W through transpose_bf16 + the streaming kernel
    (contraction over Cout=64, N=Cin=128); dW on the library GEMM."""
    M, Cin, Cout = 200, 128, 64
    g = ex.case_generator("conv1x1_bwd", M, Cin, Cout)
    x = ex.int_operand((M, Cin), 16, DEV, g).requires_grad_(True)
    w = ex.int_operand((Cout, Cin), 16, DEV, g).requires_grad_(True)
    dy = ex.int_operand((M, Cout), 16, DEV, g)
    ex.check_exact_bound(16, 16, max(M, Cin, Cout))
    y = F_.conv1x1_gemm(x, w)
    ex.assert_equal(y.detach(), ex.to_bf16(ex.ref_exact(x.detach(),
                                                        w.detach())), "y")
    y.backward(dy)
    ex.assert_equal(x.grad, ex.to_bf16(ex.ref_exact(dy, w.detach().t())),
                    "dx")
    dw = ex.to_bf16(ex.ref_exact(dy.t(), x.detach().t()))
    assert w.grad.shape == dw.shape
    assert torch.allclose(w.grad.float(), dw.float(), **ONE_ULP)


@pytest.mark.parametrize("N,fused_dgrad,in_house", [
    (128, None, True),      # transpose_bf16 + the 256x256 kernel
    (100, None, False),     # N % 64 != 0: dy @ weight
    (128, "0", False),      # SPARKDL_FUSED_DGRAD=0: dy @ weight
])
def test_linear_fused_backward_exact(monkeypatch, N, fused_dgrad, in_house):
    if fused_dgrad is None:
        monkeypatch.delenv("SPARKDL_FUSED_DGRAD", raising=False)
    else:
        monkeypatch.setenv("SPARKDL_FUSED_DGRAD", fused_dgrad)
    monkeypatch.delenv("SPARKDL_FUSED_WGRAD", raising=False)
    M, K = 200, 64
    g = ex.case_generator("linear_bwd", M, N, K, fused_dgrad)
    x = ex.int_operand((M, K), 16, DEV, g).requires_grad_(True)
    w = ex.int_operand((N, K), 16, DEV, g).requires_grad_(True)
    b = ex.int_operand((N,), 8, DEV, g, half=True).requires_grad_(True)
    dy = ex.int_operand((M, N), 16, DEV, g)
    ex.check_exact_bound(16, 16, max(M, N, K), 8)
    y = F_.linear_fused(x, w, b)
    ex.assert_equal(y.detach(), ex.to_bf16(
        ex.ref_exact(x.detach(), w.detach(), b.detach())), "y")
    y.backward(dy)
    dx = ex.to_bf16(ex.ref_exact(dy, w.detach().t()))
    if in_house:
        ex.assert_equal(x.grad, dx, "dx")
    else:
        assert x.grad.shape == dx.shape
        assert torch.allclose(x.grad.float(), dx.float(), **ONE_ULP)
    dw = ex.to_bf16(ex.ref_exact(dy.t(), x.detach().t()))
    assert w.grad.shape == dw.shape
    assert torch.allclose(w.grad.float(), dw.float(), **ONE_ULP)
    # integer column sums, |sum| <= 16 * M: exact in fp32
    assert b.grad.dtype == torch.float32
    assert torch.equal(b.grad.double(), dy.double().sum(0))
