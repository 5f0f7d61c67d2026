"""CPU checks behind tests/ops/test_conv1x1_stats_gpu.py: the launch
plan mirror, the class of every shape, the multi-trip cases, the
exactness condition of the small-operand set and the routing rule."""

import pytest
import torch

from tests.ops import _conv1x1_stats as cs
from tests.ops import _exact as ex


@pytest.mark.parametrize("M,N,K", cs.SHAPES)
def test_shape_is_in_its_class(M, N, K):
    p = cs.plan(M, N, K)
    assert (p.nch, p.nnb, p.rows) == cs.CLASSES[(K, N)]
    assert p.nb * K * 2 <= cs.MAX_PANEL
    assert p.nb * p.nnb == N
    # slab rule of batchnorm.hip: 16*G*N <= (2*M*N) / 8 once M >= 64
    if M >= 64:
        assert 16 * p.G * N * 8 <= 2 * M * N
    # the partition covers every row block exactly once
    cover = [cs.wave_blocks(p, q) for q in range(p.waves)]
    assert cover[0][0] == 0 and cover[-1][1] == p.nblk
    assert all(a[1] == b[0] for a, b in zip(cover, cover[1:]))
    # the placement is a bijection onto (slab row, N-block)
    seen = {cs.block_of(p, b) for b in range(p.G * p.nnb)}
    assert seen == {(g, n) for g in range(p.G) for n in range(p.nnb)}


def test_classes_cover_every_path():
    plans = [cs.plan(M, N, K) for M, N, K in cs.SHAPES]
    assert any(p.G == 1 for p in plans)
    assert any(p.G > 1 and p.G % 8 for p in plans)        # plain placement
    assert any(p.G % 8 == 0 and p.nnb > 1 for p in plans)  # XCD placement
    assert any(p.nblk * p.rows != M for p, (M, _, _) in zip(plans, cs.SHAPES))
    assert any(p.waves > p.nblk for p in plans)            # idle waves


@pytest.mark.parametrize("K,N", list(cs.CLASSES))
def test_loop_case_makes_a_second_trip(K, N):
    p = cs.plan(cs.LOOP_M, N, K, cs.LOOP_CAP)
    assert p.G == 1 and p.waves == 16
    trips = [b1 - b0 for b0, b1 in
             (cs.wave_blocks(p, q) for q in range(p.waves))]
    assert min(trips) >= 2
    assert cs.LOOP_M % p.rows != 0          # the last block is ragged
    assert sum(trips) == p.nblk


def test_batch512_partition_is_balanced():
    """The busiest workgroup carries at most 2 % more rows than the
    mean at the six batch-512 sites."""
    for M, K, N in ((1605632, 64, 64), (1605632, 64, 256),
                    (1605632, 256, 64), (1605632, 256, 128),
                    (401408, 128, 512), (100352, 256, 1024)):
        p = cs.plan(M, N, K)
        per_wg = [cs.wave_blocks(p, (g + 1) * 16 - 1)[1]
                  - cs.wave_blocks(p, g * 16)[0] for g in range(p.G)]
        assert max(per_wg) <= 1.02 * p.nblk / p.G, (M, K, N, max(per_wg))
        assert 16 * p.G * N * 8 <= 2 * M * N
        assert p.G * p.nnb == 256


@pytest.mark.parametrize("M,N,K", cs.SHAPES)
def test_small_operands_keep_sums_exact(M, N, K):
    A, W = cs.operands(M, N, K, "cpu", 1)
    v = ex.to_bf16(ex.ref_exact(A, W))
    assert torch.equal(v.double(), ex.ref_exact(A, W))  # nothing rounds
    _, s2, sa = cs.column_sums(v)
    assert sa.max().item() < ex.EXACT_LIMIT
    assert s2.max().item() < ex.EXACT_LIMIT


def test_large_operands_round():
    A, W = cs.operands(1000, 256, 64, "cpu", cs.LARGE_AMAX)
    changed, _ = ex.rounding_stats(ex.ref_exact(A, W))
    assert changed > 0.25


def test_routing(monkeypatch):
    from sparkdl.ops.functional import conv1x1_stats_route as route
    monkeypatch.delenv("SPARKDL_CONV1X1_STATS", raising=False)
    monkeypatch.delenv("SPARKDL_CONV1X1", raising=False)
    from sparkdl.ops.functional import CONV1X1_STATS_SITES
    table = [(64, 64), (64, 256), (256, 64), (256, 128), (128, 512),
             (256, 1024)]
    for cin, cout in table:
        assert route(cin, cout) == ((cin, cout) in CONV1X1_STATS_SITES)
        assert route(cin, cout, mode="all")
        assert not route(cin, cout, mode="0")
        assert not route(cin, cout, stride=2, mode="all")
    # out of scope: K >= 512 and the stride-2 down_convs
    for cin, cout in ((512, 128), (512, 256), (1024, 256), (1024, 512),
                      (2048, 512), (512, 2048)):
        assert not route(cin, cout) and not route(cin, cout, mode="all")
    for cin, cout in ((256, 512), (512, 1024), (1024, 2048)):
        assert not route(cin, cout, stride=2)
    monkeypatch.setenv("SPARKDL_CONV1X1_STATS", "0")
    assert not any(route(cin, cout) for cin, cout in table)
    monkeypatch.setenv("SPARKDL_CONV1X1_STATS", "1")
    monkeypatch.setenv("SPARKDL_CONV1X1", "all")
    assert not any(route(cin, cout) for cin, cout in table)
