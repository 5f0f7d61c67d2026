"""CPU checks of the method behind tests/ops/test_rowwise_exact_gpu.py:
the float64 references against torch autograd, that the exact operands
really are exact in fp32, the magnitude bounds, that the derived bounds
hold for an independent fp32 implementation and notice small errors,
and that every shape reaches the kernel path it was chosen for."""

import pytest
import torch

from . import _exact as ex
from . import _rowwise as rw

SMALL_LN = [s for s in rw.LN_BWD_SHAPES if s[0] * s[1] <= 1 << 16]


@pytest.mark.parametrize("rows,cols", [(5, 24), (7, 509), (4, 64)])
def test_ln_bwd_ref_matches_autograd_f64(rows, cols):
    g = ex.case_generator("autograd", rows, cols)
    x = torch.randn(rows, cols, generator=g, dtype=torch.float64,
                    requires_grad=True)
    gamma = torch.randn(cols, generator=g, dtype=torch.float64,
                        requires_grad=True)
    beta = torch.zeros(cols, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(rows, cols, generator=g, dtype=torch.float64)
    torch.nn.functional.layer_norm(x, (cols,), gamma, beta,
                                   rw.LN_EPS).backward(dy)
    mean, rstd, _, _ = rw.ln_fwd_ref(x.detach(), gamma.detach(),
                                     beta.detach())
    dx, dgamma, dbeta, _ = rw.ln_bwd_ref(x.detach(), dy, gamma.detach(),
                                         mean, rstd)
    assert torch.allclose(dx, x.grad, rtol=1e-11, atol=1e-13)
    assert torch.allclose(dgamma, gamma.grad, rtol=1e-11, atol=1e-13)
    assert torch.allclose(dbeta, beta.grad, rtol=1e-11, atol=1e-13)


def test_ln_fwd_ref_matches_torch_f64():
    x, gamma, beta, _ = rw.ln_fwd_operands(9, 77)
    _, _, _, y = rw.ln_fwd_ref(x, gamma, beta)
    want = torch.nn.functional.layer_norm(
        x.double(), (77,), gamma.double(), beta.double(), rw.LN_EPS)
    assert torch.allclose(y, want, rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("rows,cols", list(rw.LN_BWD_SHAPES))
def test_ln_bwd_bound_and_operand_ranges(rows, cols):
    col, row = rw.check_ln_bwd_bound(rows, cols)
    assert col < ex.EXACT_LIMIT and row < ex.EXACT_LIMIT
    if rows * cols > 1 << 20:
        return          # same generator code; spare the big draw
    x, dy, gamma, mean, rstd = rw.ln_bwd_exact_operands(rows, cols)
    d = x.float() - mean[:, None]
    assert torch.equal(d, d.round()) and d.abs().max() <= rw.LN_DMAX
    assert torch.equal(mean, mean.round())
    assert torch.equal(torch.log2(rstd), torch.log2(rstd).round())
    assert dy.float().abs().max() <= rw.LN_DYMAX
    assert gamma.abs().max() <= rw.LN_GMAX
    assert torch.equal(gamma, gamma.round())


def test_ln_bwd_bound_rejects_over_range():
    with pytest.raises(AssertionError):
        rw.check_ln_bwd_bound(1 << 18, 64)
    with pytest.raises(AssertionError):
        rw.check_ln_bwd_bound(4, 1 << 17)


@pytest.mark.parametrize("rows,cols", SMALL_LN)
def test_ln_bwd_exact_operands_are_exact_in_fp32(rows, cols):
    """dgamma and dbeta: the fp32 evaluation equals the float64 one for
    every shape, so any accumulation order gives these bits. dx: the
    same where cols is a power of two; elsewhere an fp32 evaluation is
    within ln_dx_bound."""
    ops = rw.ln_bwd_exact_operands(rows, cols)
    dx64, dg64, db64, terms = rw.ln_bwd_ref(*ops)
    dx32, dg32, db32, _ = rw.ln_bwd_ref(*ops, dtype=torch.float32)
    assert torch.equal(dg32.double(), dg64)
    assert torch.equal(db32.double(), db64)
    assert dg64.abs().max() < ex.EXACT_LIMIT
    # column sums in the reverse row order too
    rev = [t.flip(0) for t in ops[:2]] + [ops[2]] + \
        [t.flip(0) for t in ops[3:]]
    _, dgr, dbr, _ = rw.ln_bwd_ref(*rev, dtype=torch.float32)
    assert torch.equal(dgr, dg32) and torch.equal(dbr, db32)
    if cols & (cols - 1) == 0:
        assert torch.equal(dx32.double(), dx64)
    else:
        tol = rw.ln_dx_bound(dx64, terms, ops[4])
        assert bool(((dx32.bfloat16().double() - dx64).abs() <= tol).all())
    if rows * cols >= 64:
        assert dg64.abs().max() > 0 and dx64.abs().max() > 0


def test_ln_dx_bound_notices_small_errors():
    ops = rw.ln_bwd_exact_operands(6, 769)
    dx64, _, _, terms = rw.ln_bwd_ref(*ops)
    tol = rw.ln_dx_bound(dx64, terms, ops[4])
    good = dx64.float().bfloat16()
    assert bool(((good.double() - dx64).abs() <= tol).all())
    # two bf16 ulp off on one element, and a row sum that lost a column
    off = good.clone()
    i = dx64.abs().argmax()
    off.view(-1)[i] = (off.view(-1)[i:i + 1].view(torch.int16) + 2) \
        .view(torch.bfloat16)
    assert bool(((off.double() - dx64).abs() > tol).any())
    # ... which one bf16 ulp sees among 769 only where gamma and dy
    # happen to be large there, but always with the weight of the row
    # sums on the last columns
    seen = {}
    for tail_only in (False, True):
        x, dy, gamma, mean, rstd = rw.ln_bwd_exact_operands(
            6, 769, tail_only=tail_only)
        dx64, _, _, terms = rw.ln_bwd_ref(x, dy, gamma, mean, rstd)
        tol = rw.ln_dx_bound(dx64, terms, rstd)
        dy2 = dy.clone()
        dy2[:, -1] = 0
        lost, _, _, _ = rw.ln_bwd_ref(x, dy2, gamma, mean, rstd)
        lost[:, -1] = dx64[:, -1]
        bad = (lost.float().bfloat16().double() - dx64).abs() > tol
        seen[tail_only] = bad.double().mean().item()
    assert seen[True] > 0.5, seen


def test_ln_fwd_operands_have_the_special_rows():
    x, gamma, beta, kinds = rw.ln_fwd_operands(9, 2056)
    assert kinds.tolist() == [0] * 7 + [1, 2]
    xf = x.float()
    assert xf[-1].min() == xf[-1].max() == 1.5
    assert (xf[-2] - 100).abs().max() <= 1.5 and xf[-2].std() > 0.1
    assert rw.ln_fwd_operands(1, 64)[3].tolist() == [0]
    _, rstd, _, _ = rw.ln_fwd_ref(x, gamma, beta)
    assert abs(rstd[-1].item() - rw.LN_EPS ** -0.5) < 1e-9


def test_ln_stats_emulations_against_f64():
    """What the GPU test scales its rstd bounds from: plain fp32 torch
    is good to ~1e-6 on centred rows, and the one-pass variance in the
    kernel's order loses about two and a half digits at offset 100.
    The constant row (1.5: every partial sum is exact) goes with the
    offset row; its variance is 0 either way."""
    worst_c, worst_o = 0.0, 0.0
    for rows, cols in SMALL_LN:
        x, gamma, beta, kinds = rw.ln_fwd_operands(rows, cols)
        mean64, rstd64, _, _ = rw.ln_fwd_ref(x, gamma, beta)
        m_t, r_t = rw.ln_stats_fp32_torch(x)
        m_k, r_k = rw.ln_stats_fp32_kernel_order(x)
        amax = x.double().abs().max(-1).values
        assert bool(((m_k.double() - mean64).abs() <= 2.0 ** -20 * amax)
                    .all())
        c = kinds == 0
        if c.any():
            worst_c = max(worst_c, rw.rel_err(r_t, rstd64)[c].max().item(),
                          rw.rel_err(r_k, rstd64)[c].max().item())
        if (~c).any():
            worst_o = max(worst_o, rw.rel_err(r_k, rstd64)[~c].max().item())
    assert worst_c < 2e-6, worst_c
    assert 1e-5 < worst_o < 2e-2, worst_o


def test_ln_y_bound_holds_for_fp32_torch_and_notices_errors():
    x, gamma, beta, kinds = rw.ln_fwd_operands(9, 769)
    mean64, rstd64, xg, y64 = rw.ln_fwd_ref(x, gamma, beta)
    # an fp32 two-pass layer norm has no rstd error to speak of on
    # centred rows; the offset row gets what the GPU test allows it
    delta = torch.full((9,), 2.0 ** -20, dtype=torch.float64)
    delta[kinds != 0] = 4 * rw.rel_err(
        rw.ln_stats_fp32_kernel_order(x)[1], rstd64)[kinds != 0].max()
    tol = rw.ln_y_bound(y64, xg, beta, delta)
    y = torch.nn.functional.layer_norm(x.float(), (769,), gamma, beta,
                                       rw.LN_EPS).bfloat16()
    assert bool(((y.double() - y64).abs() <= tol).all())
    two_ulp = (y.view(torch.int16) + 2).view(torch.bfloat16)
    assert bool(((two_ulp.double() - y64).abs() > tol).any())
    nobeta = torch.nn.functional.layer_norm(x.float(), (769,), gamma, None,
                                            rw.LN_EPS).bfloat16()
    assert bool(((nobeta.double() - y64).abs() > tol).any())


# ---------------------------------------------------------------------------
# bias + GELU
# ---------------------------------------------------------------------------

def test_gelu_structure_values_are_exact_in_fp32():
    """The kernel's formulas in fp32: gelu'(0) = 1/2, gelu'(16) = 1,
    gelu(0) = 0, gelu(16) = 16, exactly."""
    z = torch.tensor([0.0, 16.0])
    assert rw.gelu_grad_fp32_as_kernel(z).tolist() == [0.5, 1.0]
    assert rw.gelu_fp32_as_kernel(z).tolist() == [0.0, 16.0]
    assert (rw.gelu_grad_f64(z) - torch.tensor([0.5, 1.0])).abs().max() \
        < 1e-50


@pytest.mark.parametrize("rows,cols", [(5, 24), (3, 7), (300, 40)])
def test_bias_gelu_exact_operands(rows, cols):
    x, bias, dy = rw.bias_gelu_exact_operands(rows, cols)
    z, dx, dbias = rw.bias_gelu_exact_ref(x, bias, dy)
    assert x.dtype == torch.bfloat16 and bias.dtype == torch.float32
    if rows * cols > 30:
        assert set(z.unique().tolist()) == {0.0, 16.0}
    assert torch.equal(dx.float().bfloat16().double(), dx)
    assert torch.equal(dbias.float().double(), dbias)
    g32 = rw.gelu_grad_fp32_as_kernel(x.float() + bias)
    assert torch.equal((dy.float() * g32).double(), dx)
    assert torch.equal(rw.gelu_fp32_as_kernel(x.float() + bias).double(), z)


def test_bias_gelu_value_grid_and_eps():
    x, bias, dy = rw.bias_gelu_value_operands(*rw.BG_VALUE_SHAPES[0])
    z = x.double() + bias.double()
    assert z.min() < -7.9 and z.max() > 7.9
    assert bool((x.float() == 0).any())
    signs = x.view(torch.int16)[x.float() == 0]
    assert bool((signs == 0).any()) and bool((signs != 0).any())   # +-0
    assert bool(((z > -1) & (z < -0.5)).any())       # GELU's minimum
    eps, err = rw.gelu_grad_eps(z)
    assert 1e-8 < err < 5e-7, err
    # forward: torch's fp32 path satisfies the shared GELU bound
    ex.assert_gelu_within_bound(rw.gelu_fp32_as_kernel(z.float()).bfloat16(),
                                z)
    # backward bound holds for fp32 torch, and notices tanh-GELU'
    ref = dy.double() * rw.gelu_grad_f64(z)
    tol = 2.0 ** -8 * ref.abs() + dy.double().abs() * eps
    got = (dy.float() * rw.gelu_grad_fp32_as_kernel(z.float())).bfloat16()
    assert bool(((got.double() - ref).abs() <= tol).all())
    zz = z.clone().requires_grad_(True)
    torch.nn.functional.gelu(zz, approximate="tanh").sum().backward()
    tanh = (dy.double() * zz.grad).float().bfloat16()
    assert bool(((tanh.double() - ref).abs() > tol).any())


# ---------------------------------------------------------------------------
# every shape reaches the path it was chosen for
# ---------------------------------------------------------------------------

def test_ln_shapes_land_on_their_paths():
    for (rows, cols), want in rw.LN_BWD_SHAPES.items():
        assert rw.ln_bwd_path(rows, cols)[0] == want, (rows, cols)
    paths = {s: rw.ln_bwd_path(*s) for s in rw.LN_BWD_SHAPES}
    assert {p[0] for p in paths.values()} == {"reg1", "reg2", "reg4", "lds"}
    # a second trip on both kinds of kernel, with a ragged last quad
    assert paths[(2051, 64)] == ("reg1", 512, True)
    assert paths[(2051, 2056)] == ("lds", 512, True)
    assert 2051 % 4 == 3
    assert not any(p[2] for s, p in paths.items() if s[0] != 2051)
    # waves without a row
    assert {s[0] % 4 for s in paths} == {0, 1, 2, 3}
    # ragged tails on the register kernels and on the fallback
    assert any(c % 8 and p[0] == "lds" for (_, c), p in paths.items())
    assert {p[0] for (_, c), p in paths.items() if c % 8} \
        == {"reg1", "reg2", "reg4", "lds"}
    assert rw.ln_fwd_loops(8197) and not rw.ln_fwd_loops(8192)
    assert sum(rw.ln_fwd_loops(r) for r, _ in rw.LN_FWD_SHAPES) == 1
    # what the older tests reach: no fallback, no second trip
    for s in [(128, 768), (512, 1024), (64, 769)]:
        assert rw.ln_bwd_path(*s)[0] in ("reg2",) and not \
            rw.ln_bwd_path(*s)[2]


def test_bias_gelu_shapes_land_on_their_paths():
    for (rows, cols), want in rw.BG_EXACT_BWD_SHAPES.items():
        assert rw.bias_gelu_bwd_path(rows, cols)[0] == want
        assert rw.bias_gelu_fwd_path(rows, cols)[0] == want
    assert rw.bias_gelu_fwd_path(5, 24)[1:3] == (3, 1)       # 85 x 3 = 255
    assert rw.bias_gelu_fwd_path(300, 40)[1:3] == (5, 1)     # 51 x 5 = 255
    assert rw.bias_gelu_bwd_path(3, 2056)[1] == 2
    assert rw.bias_gelu_bwd_path(2051, 8)[2]
    assert rw.bias_gelu_bwd_path(2051, 9) == ("scalar", 1, True)
    assert 2 * 16384 * 4 // 2 == 65536                       # LDS bytes
    assert rw.bias_gelu_fwd_path(*rw.BG_FWD_LOOP_SHAPE) \
        == ("vec", 1, 0, True)
    assert not rw.bias_gelu_fwd_path(524288, 8)[3]
    assert not any(rw.bias_gelu_fwd_path(*s)[3]
                   for s in rw.BG_EXACT_BWD_SHAPES)
