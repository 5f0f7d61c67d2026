"""Launch-plan mirror, shapes and operands of the conv1x1_stats tests.

``plan`` mirrors conv1x1_stats_plan and the kernel's row partition
(csrc/conv1x1_stats.hip) so that tests/ops/test_conv1x1_stats_cpu.py can
check without a GPU that every shape of the GPU test is in the launch
class it was chosen for. Operands come from tests/ops/_exact.py: seeded
CPU integers, exact in bf16.
"""

import collections

import torch

from tests.ops import _exact as ex

Plan = collections.namedtuple(
    "Plan", "nch nb nnb rows G nblk waves")

WAVES = 16
CHUNK = 64
MAX_PANEL = 128 * 1024
CUS = 256


def plan(M, N, K, max_workers=0):
    """(chunks per N-block, N-block width, N-blocks, rows per wave
    block, slab rows G, row blocks, waves per N-block)."""
    assert K in (64, 128, 256) and N >= CHUNK and N % CHUNK == 0 and M >= 1
    c = 8
    while c > 1 and (N % (c * CHUNK) != 0 or c * CHUNK * K * 2 > MAX_PANEL):
        c //= 2
    nnb = N // (c * CHUNK)
    rows = 16 if (K == 256 or (K == 128 and c >= 4)) else 32
    g = max(8, CUS // nnb // 8 * 8)
    g = max(1, min(g, M // (WAVES * rows)))
    if max_workers > 0:
        g = min(g, max_workers)
    nblk = (M + rows - 1) // rows
    return Plan(c, c * CHUNK, nnb, rows, g, nblk, g * WAVES)


def wave_blocks(p, q):
    """Row blocks [b0, b1) of wave q of an N-block's p.waves waves."""
    return q * p.nblk // p.waves, (q + 1) * p.nblk // p.waves


def block_of(p, bid):
    """(slab row g, N-block) of workgroup bid: the kernel's placement."""
    if p.G % 8 == 0:
        return (bid // (8 * p.nnb)) * 8 + bid % 8, (bid // 8) % p.nnb
    return bid // p.nnb, bid % p.nnb


# (K, N) -> (chunks per N-block, N-blocks, rows per wave block): one
# launch class per site shape of the ResNet-50 table
CLASSES = {
    (64, 64): (1, 1, 32),
    (64, 256): (4, 1, 32),
    (256, 64): (1, 1, 16),
    (256, 128): (2, 1, 16),
    (128, 512): (8, 1, 16),
    (256, 1024): (4, 4, 16),
}
# a lone row; one short of / exactly / two full 16-row sub-blocks plus;
# 1000: ragged last block; 1024 and 1025: the first G > 1 for 32-row
# blocks and its first ragged row; 2066: G = 4 (32-row) or 8 (16-row,
# the XCD placement with N-blocks), last block of 18 or 2 rows
ROWS = (1, 63, 64, 1000, 1024, 1025, 2066)
SHAPES = [(M, N, K) for (K, N) in CLASSES for M in ROWS]
# worker cap 1: 16 waves share 65 (32-row) or 130 (16-row) blocks, 4 to
# 9 trips each, and the last block is ragged
LOOP_M, LOOP_CAP = 2066, 1
LARGE_AMAX = ex.STREAM_AMAX


def operands(M, N, K, device, amax, call=0):
    A, W, _ = ex.gemm_operands("conv1x1_stats", M, N, K, device, amax,
                               amax, call=call)
    return A, W


def column_sums(v):
    """fp64 (sum, sum of squares, sum of |v|) per column of the rounded
    reference v."""
    d = v.double()
    return d.sum(0), (d * d).sum(0), d.abs().sum(0)


def sum_bound(M):
    """Relative bound of an fp32 sum of M terms in any order:
    gamma = M u / (1 - M u), u = 2^-24."""
    mu = M * 2.0 ** -24
    return mu / (1.0 - mu)


def residual_operand(M, N, device, call=0):
    g = ex.case_generator("conv1x1_stats_res", M, N, call)
    return ex.int_operand((M, N), 4, device, g)
