"""Exact-arithmetic helpers for the GEMM-family refchecks.

bf16 operands that hold small integers have exact fp32 products, and
their sums stay exact in fp32 while every partial sum stays below 2^24
in magnitude, in ANY accumulation order (MFMA, split atomics, library
GEMM). The only inexact step left is the final fp32 -> bf16 store,
which common.hip.h's f2bf documents as round-to-nearest-even. A kernel
therefore has to reproduce ``ref_exact(...).float().bfloat16()`` bit
for bit (fp32 outputs: the exact reference itself), and any dropped,
doubled, transposed or misplaced fragment changes integers.

This module also holds the shape lists of tests/ops/test_gemm_exact_gpu.py
so that tests/ops/test_exact_helpers_cpu.py can check, without a GPU,
that every shape is in the launch class it was chosen for and that its
operands really exercise the bf16 rounding.

Operands are always drawn on the CPU from a seeded CPU generator and
then moved, so the CPU checks and the GPU tests see the same values.
"""

import math
import zlib

import torch

EXACT_LIMIT = 2 ** 24
AMAX_LIMIT = 16


# ---------------------------------------------------------------------------
# operands, bound, reference
# ---------------------------------------------------------------------------

def case_generator(*key):
    """A CPU generator seeded from the case's own key (kind, shape,
    call number ...), so no two cases share operands."""
    g = torch.Generator(device="cpu")
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def int_operand(shape, amax, device, generator, half=False):
    """Uniform integers in [-amax, amax] as a bf16 tensor on ``device``
    (amax <= 16: every value is exact in bf16). ``half=True`` returns
    fp32 half-integers k/2, |k/2| <= amax, instead: the bias operand.
    ``generator`` is a CPU generator (see module docstring)."""
    assert 1 <= amax <= AMAX_LIMIT, amax
    if half:
        v = torch.randint(-2 * amax, 2 * amax + 1, shape, dtype=torch.int16,
                          generator=generator)
        return (v.float() / 2).to(device)
    v = torch.randint(-amax, amax + 1, shape, dtype=torch.int16,
                      generator=generator)
    return v.to(torch.bfloat16).to(device)


def check_exact_bound(a, b, L, bias_max=0.0):
    """Condition of the method: with |A| <= a, |W| <= b and contraction
    length L every partial sum, bias included, stays below 2^24, so
    fp32 accumulation is exact in any order. A bias (half-integers)
    costs one more bit, so the sum is then held below 2^23. Raises
    AssertionError (a test that violates the bound must fail)."""
    bound = a * b * L + abs(bias_max)
    limit = EXACT_LIMIT if bias_max == 0 else EXACT_LIMIT // 2
    assert bound < limit, (
        "not exact in fp32: %g*%g*%d + %g = %g >= %d"
        % (a, b, L, bias_max, bound, limit))
    return bound


def ref_exact(A, W, bias=None, dtype=torch.float64, chunk_rows=None):
    """A @ W^T (+ bias) computed in ``dtype`` on the operands' device.
    fp64 by default; fp32 (exact too under check_exact_bound) for the
    one case too large for an fp64 copy, in row chunks."""
    Wt = W.to(dtype).t()
    if chunk_rows is None:
        out = A.to(dtype) @ Wt
    else:
        out = torch.cat([a.to(dtype) @ Wt for a in A.split(chunk_rows)])
    if bias is not None:
        out = out + bias.to(dtype)
    return out


def to_bf16(ref):
    """The kernel's store: fp32 value (exact here) -> bf16, RNE."""
    return ref.float().bfloat16()


def rounding_stats(ref):
    """(fraction of entries that bf16 rounding changes, number of exact
    ties) for an exact reference. A tie lies midway between two bf16
    neighbours, i.e. its fp32 image has low 16 bits == 0x8000."""
    f = ref.float()
    assert torch.equal(f.double(), ref.double()), "reference not exact in fp32"
    changed = f.bfloat16().float() != f
    low = f.contiguous().view(torch.int32) & 0xFFFF
    ties = (low == 0x8000) & torch.isfinite(f)
    return changed.double().mean().item(), int(ties.sum().item())


# ---------------------------------------------------------------------------
# GELU bound
# ---------------------------------------------------------------------------

def gelu_f64(z):
    """erf-GELU in fp64, written with erfc so the left tail does not
    cancel: 0.5 z (1 + erf(z/sqrt2)) == 0.5 z erfc(-z/sqrt2)."""
    z = z.double()
    return 0.5 * z * torch.special.erfc(-z * math.sqrt(0.5))


def gelu_bound(z):
    """Allowed |y - gelu(z)| for a bf16 output y computed in fp32 from
    the exact pre-activation z:  2^-8 |g| + 2^-20 |z|.

    First term: one bf16 ulp (RNE's half ulp plus margin for the fp32
    value sitting next to a rounding boundary). Second term: an
    absolute error of 16 fp32 ulp on erf (the OpenCL bound the device
    math library is specified to: 16 * 2^-24 near |erf| = 1) times
    |z|/2; it matters where 1 + erf cancels. Derived, not measured."""
    g = gelu_f64(z)
    return g, 2.0 ** -8 * g.abs() + 2.0 ** -20 * z.double().abs()


def assert_gelu_within_bound(y, z):
    g, tol = gelu_bound(z)
    err = (y.double() - g).abs()
    bad = err > tol
    assert not bool(bad.any()), (
        "%d outputs outside the GELU bound, worst err/bound %.3f at %s"
        % (int(bad.sum()), (err / tol.clamp_min(1e-300)).max().item(),
           bad.nonzero()[:4].tolist()))


# ---------------------------------------------------------------------------
# comparison with a useful failure message
# ---------------------------------------------------------------------------

def assert_equal(got, want, what=""):
    """torch.equal with the differing indices in the message (they
    name the tile / split / K-step that went wrong)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    diff = (got != want).nonzero()
    first = diff[0].tolist()
    raise AssertionError(
        "%s: %d of %d entries differ; first %s got %r want %r; last %s; "
        "rows %d..%d cols %d..%d"
        % (what, diff.shape[0], got.numel(), first,
           got[tuple(first)].item(), want[tuple(first)].item(),
           diff[-1].tolist(), diff[:, 0].min(), diff[:, 0].max(),
           diff[:, -1].min(), diff[:, -1].max()))


# ---------------------------------------------------------------------------
# launch-plan mirrors
# ---------------------------------------------------------------------------

def wgrad_plan(M, N, K):
    """Mirror of launch_wgrad_splitk (csrc/wgrad.hip) and of wgrad_k's
    m-tile partition: (splits, per, tiles in the last non-empty split,
    number of empty splits)."""
    TN, TK, TM = 256, 128, 64
    ntiles = (N // TN) * (K // TK)
    splits = 1
    while ntiles * splits < 1024 and splits < 64 and splits * 2 * TM <= M:
        splits *= 2
    mtiles = M // TM
    per = (mtiles + splits - 1) // splits
    counts = [max(0, min(s * per + per, mtiles) - s * per)
              for s in range(splits)]
    nonempty = [c for c in counts if c > 0]
    return splits, per, nonempty[-1], len(counts) - len(nonempty)


def stream_plan(M, N):
    """Mirror of launch_gemm_stream (csrc/gemm_stream.hip):
    (m-blocks of 1024 rows, workers per 64-wide N-block). Worker w runs
    blocks w, w + workers, ...: a second trip needs mblocks > workers."""
    nnb = N // 64
    mblocks = (M + 1023) // 1024
    workers = max(1, min(mblocks, 1024))
    while workers * nnb < 1024 and workers < mblocks:
        workers += 1
    return mblocks, workers


def gemm256_nwg(M, N):
    """Grid of launch_gemm_bias_act (csrc/gemm_gelu.hip): 256x256
    output tiles. The XCD swizzle takes q = nwg // 8, r = nwg % 8."""
    return ((M + 255) // 256) * ((N + 255) // 256)


# ---------------------------------------------------------------------------
# shapes of the GPU tests
# ---------------------------------------------------------------------------

# gemm_bias_act (M, N, K): every row edge and every column edge once
# with K=64 (single tile, no prefetch) and once with K=192 (buffer
# parity wraps), K=128 (one prefetch) on a few; nwg in {1,2,3,9,18}.
GEMM256_ROWS = (1, 255, 256, 257, 513)
GEMM256_COLS = (1, 7, 77, 100, 256, 264)
GEMM256_SHAPES = [
    (1, 7, 64), (255, 77, 64), (256, 100, 64), (257, 1, 64),
    (513, 256, 64), (257, 264, 64),
    (513, 520, 64),    # nwg = 9: q=1, r=1
    (1281, 513, 64),   # nwg = 18: q=2, r=2
    (1, 100, 128), (257, 77, 128), (513, 264, 128),
    (1, 264, 192), (255, 1, 192), (256, 7, 192), (257, 77, 192),
    (513, 100, 192), (257, 256, 192),
]
# (act, bias, save_z)
GEMM256_VARIANTS = [
    (0, True, False), (0, False, False),
    (1, True, True), (1, True, False), (1, False, False),
]
GEMM256_AMAX = 16       # |z| mostly > 256: odd sums round, many tie
GEMM256_BIAS_AMAX = 8
# second operand set for act=1: small sums, so that a good part of z
# lies where GELU is neither 0 nor z
GELU_SHAPES = [(257, 77, 64), (255, 100, 128), (257, 77, 192)]
GELU_AMAX = (2, 1)
GELU_BIAS_AMAX = 2

STREAM_SHAPES = [(M, N, K) for K in (64, 128, 256) for N in (64, 192)
                 for M in (1, 63, 64, 1000, 1024, 1025, 2066)]
# 1026 m-blocks on 1024 workers: workers 0 and 1 take a second trip
# and the last block has 40 rows
STREAM_LOOP_SHAPE = (1024 * 1024 + 1024 + 40, 64, 64)
STREAM_AMAX = 16

# (M, N, K) -> wgrad_plan
WGRAD_SHAPES = {
    (64, 256, 128): (1, 1, 1, 0),        # splits == 1: plain store
    (128, 256, 128): (2, 1, 1, 0),       # two splits of one tile
    (192, 256, 128): (2, 2, 1, 0),       # 2 + 1 tiles
    (320, 256, 128): (4, 2, 1, 1),       # 2,2,1,0: an empty split
    (448, 512, 256): (4, 2, 1, 0),       # 4 output tiles, short last
    (20480, 256, 128): (64, 5, 5, 0),    # triple buffer wraps
    (20544, 256, 128): (64, 6, 3, 10),   # 53x6 + 3, ten empty splits
}
WGRAD_AMAX = 16


def gemm_operands(kind, M, N, K, device, amax_a, amax_w, bias_amax=None,
                  call=0):
    """(A[M,K], W[N,K], bias[N] or None) for one case, bound checked."""
    g = case_generator(kind, M, N, K, call)
    A = int_operand((M, K), amax_a, device, g)
    W = int_operand((N, K), amax_w, device, g)
    bias = None
    if bias_amax is not None:
        bias = int_operand((N,), bias_amax, device, g, half=True)
    check_exact_bound(amax_a, amax_w, K,
                      0 if bias_amax is None else bias_amax)
    return A, W, bias


def wgrad_operands(M, N, K, device, call):
    """(dZ[M,N], X[M,K]); the contraction runs over M."""
    g = case_generator("wgrad", M, N, K, call)
    dz = int_operand((M, N), WGRAD_AMAX, device, g)
    x = int_operand((M, K), WGRAD_AMAX, device, g)
    check_exact_bound(WGRAD_AMAX, WGRAD_AMAX, M)
    return dz, x
