"""LayerNorm and bias+GELU kernels against float64 references, at the
shapes where each kernel takes another path (see _rowwise.py for the
method and the shape lists; test_rowwise_helpers_cpu.py checks both
without a GPU).

Exact operands: dgamma, dbeta, dbias and, where cols is a power of two,
dx must match the float64 result bit for bit. Random operands: bounds
built from the number formats and from the measured error of a plain
fp32 evaluation of the same formula, never a free absolute term.

Measured, largest over all cases (fp32 reference error -> allowed = 4 x
that; kernel on an MI355X):
  rstd, centred rows (plain fp32 torch, same formula)
                       1.64e-07 -> 6.6e-07;   kernel 1.32e-07
  rstd, offset-100 and constant rows (fp32 emulation of the kernel's
  one-pass order)      5.77e-03 -> 2.31e-02;  kernel 7.26e-03
  gelu' on the z grid (plain fp32 torch, the kernel's formula)
                       1.17e-07 -> 4.66e-07;  kernel: dx leaves the bf16
                       term of its bound by at most 1.3e-08 |dy|
"""

import functools

import pytest
import torch

from . import _exact as ex
from . import _rowwise as rw

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sparkdl.ops as ops

DEV = "cuda"


@pytest.fixture(autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")


def _within(got, ref, tol, what):
    err = (got.double().cpu() - ref).abs()
    bad = err > tol
    assert not bool(bad.any()), (
        "%s: %d of %d outside the bound, worst err/bound %.3f, first %s"
        % (what, int(bad.sum()), bad.numel(),
           (err / tol.clamp_min(1e-300)).max().item(),
           bad.nonzero()[:4].tolist()))


# ---------------------------------------------------------------------------
# LayerNorm backward
# ---------------------------------------------------------------------------

# Which kernel and loop each shape reaches, read off launch_layernorm_bwd
# and layernorm_bwd_part_rows (mirrored by rw.ln_bwd_path):
#   (1,64) (3,8) (5,512) (7,509): reg_k<1>; 1, 3 and 1 idle waves in the
#       last block; (3,8) uses one lane, (7,509) ends in a 5-wide tail
#   (6,1024) (6,769): reg_k<2>; 769 = 512 + 257, tail of 1 in k = 1
#   (9,2047) (9,2048): reg_k<4>, ragged and full
#   (9,2056) (5,2049) (4,8192): kmax 5, 5, 16 -> layernorm_bwd_k, LDS
#       atomics; 8192 is the 64 KiB LDS limit of the binding
#   (2051,64): 513 quads on 512 blocks: block 0 takes rows 2048..2050,
#       its wave 3 has no second row
#   (2051,2056): the same through layernorm_bwd_k
@pytest.mark.parametrize("rows,cols", list(rw.LN_BWD_SHAPES))
def test_layernorm_bwd_exact(rows, cols):
    pow2 = cols & (cols - 1) == 0
    for tail_only in ((False,) if pow2 else (False, True)):
        cpu = rw.ln_bwd_exact_operands(rows, cols, tail_only=tail_only)
        dx64, dg64, db64, terms = rw.ln_bwd_ref(*cpu)
        dx, dgamma, dbeta = ops.ext().layernorm_bwd(
            *[t.to(DEV) for t in cpu])
        what = "ln_bwd %dx%d tail_only=%s " % (rows, cols, tail_only)
        ex.assert_equal(dbeta.cpu(), db64.float(), what + "dbeta")
        ex.assert_equal(dgamma.cpu(), dg64.float(), what + "dgamma")
        if pow2:
            ex.assert_equal(dx.cpu(), ex.to_bf16(dx64), what + "dx")
        else:
            _within(dx, dx64, rw.ln_dx_bound(dx64, terms, cpu[4]),
                    what + "dx")


# ---------------------------------------------------------------------------
# LayerNorm forward
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _rstd_reference_errors():
    """(centred, offset): the largest relative rstd error, over all
    forward cases, of plain fp32 torch on the centred rows and of the
    fp32 emulation of the kernel's one-pass order on the offset and
    constant rows. Computed once, on the CPU."""
    centred = offset = 0.0
    for rows, cols in rw.LN_FWD_SHAPES:
        x, gamma, beta, kinds = rw.ln_fwd_operands(rows, cols)
        _, rstd64, _, _ = rw.ln_fwd_ref(x, gamma, beta)
        c = kinds == 0
        centred = max(centred, rw.rel_err(
            rw.ln_stats_fp32_torch(x)[1], rstd64)[c].max().item())
        if (~c).any():
            offset = max(offset, rw.rel_err(
                rw.ln_stats_fp32_kernel_order(x[~c])[1],
                rstd64[~c]).max().item())
    print("rstd reference error: centred %.3g offset %.3g"
          % (centred, offset))
    return centred, offset


# launch_layernorm_fwd: one wave a row, 4 rows a block, at most 2048
# blocks. Every shape but the last is a single trip; (8197, 64) has 2050
# quads, so blocks 0 and 1 take a second trip and the last quad has one
# row. The column loop takes 1 .. 16 trips (cols 8 .. 8192), with a
# scalar tail where cols % 8 != 0 (509, 769, 2047, 2049).
@pytest.mark.parametrize("rows,cols", rw.LN_FWD_SHAPES)
def test_layernorm_fwd(rows, cols):
    x, gamma, beta, kinds = rw.ln_fwd_operands(rows, cols)
    mean64, rstd64, xg, y64 = rw.ln_fwd_ref(x, gamma, beta)
    y, mean, rstd = ops.ext().layernorm_fwd(
        x.to(DEV), gamma.to(DEV), beta.to(DEV), rw.LN_EPS)
    assert mean.shape == rstd.shape == (rows,)
    what = "ln_fwd %dx%d " % (rows, cols)

    amax = x.double().abs().max(-1).values
    _within(mean, mean64, 2.0 ** -20 * amax, what + "mean")

    ref_c, ref_o = _rstd_reference_errors()
    delta = torch.where(kinds == 0, 4 * ref_c, 4 * ref_o).double()
    err = rw.rel_err(rstd, rstd64)
    c = kinds == 0
    print(what + "rstd rel err: centred %.3g (allowed %.3g) other %.3g "
          "(allowed %.3g)" % (err[c].max().item(), 4 * ref_c,
                              err[~c].max().item() if (~c).any() else 0,
                              4 * ref_o))
    _within(rstd, rstd64, delta * rstd64.abs(), what + "rstd")
    _within(y, y64, rw.ln_y_bound(y64, xg, beta, delta), what + "y")


# ---------------------------------------------------------------------------
# bias + GELU, structure
# ---------------------------------------------------------------------------

# launch_bias_gelu_bwd: one row a block, at most 2048 blocks; cols % 8
# picks bias_gelu_bwd_k (8 columns a thread, 2048 a pass) or the scalar
# kernel (LDS atomics).
#   (1,8): one thread;  (5,24) (300,40): 3 and 5 threads busy
#   (3,2056): thread 0 takes a second pass for columns 2048..2055
#   (2051,8) / (2051,9): blocks 0..2 take a second row
#   (2,16384): 64 KiB of LDS partials, the binding's limit
#   (3,7) (4,1): scalar kernel, fewer columns than a vector / one column
# launch_bias_gelu_fwd on the same shapes: tpr = cols / 8 threads a row;
# tpr = 3 and 5 leave thread 255 without a row (it must drop out),
# (3,2056) has tpr capped at 256 and a second column pass, cols % 8 != 0
# goes to the flat scalar kernel.
@pytest.mark.parametrize("rows,cols", list(rw.BG_EXACT_BWD_SHAPES))
def test_bias_gelu_structure_exact(rows, cols):
    x, bias, dy = rw.bias_gelu_exact_operands(rows, cols)
    z, dx64, dbias64 = rw.bias_gelu_exact_ref(x, bias, dy)
    what = "bias_gelu %dx%d " % (rows, cols)
    y = ops.ext().bias_gelu_fwd(x.to(DEV), bias.to(DEV))
    ex.assert_equal(y.cpu(), ex.to_bf16(z), what + "y")
    dx, dbias = ops.ext().bias_gelu_bwd(x.to(DEV), bias.to(DEV), dy.to(DEV))
    ex.assert_equal(dx.cpu(), ex.to_bf16(dx64), what + "dx")
    ex.assert_equal(dbias.cpu(), dbias64.float(), what + "dbias")


def test_bias_gelu_fwd_grid_stride():
    """2049 blocks' worth of rows on the 2048-block grid: block 0 takes
    a second trip, for the last 3 rows."""
    rows, cols = rw.BG_FWD_LOOP_SHAPE
    x, bias, _ = rw.bias_gelu_exact_operands(rows, cols)
    z, _, _ = rw.bias_gelu_exact_ref(x, bias, torch.zeros(1, cols))
    y = ops.ext().bias_gelu_fwd(x.to(DEV), bias.to(DEV))
    ex.assert_equal(y.cpu(), ex.to_bf16(z), "bias_gelu fwd loop y")


# ---------------------------------------------------------------------------
# bias + GELU, values
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols", rw.BG_VALUE_SHAPES)
def test_bias_gelu_values(rows, cols):
    """z over [-8, 8] with both tails and +-0, vector and scalar kernel.
    Forward within _exact.gelu_bound; backward within
    2^-8 |ref| + |dy| eps, eps = 4 x the error of the plain fp32 torch
    evaluation of the kernel's formula on this grid (1.17e-7 -> 4.66e-7);
    dbias additionally gets rows x 2^-24 of its absolute sum for the
    fp32 summation over the rows."""
    x, bias, dy = rw.bias_gelu_value_operands(rows, cols)
    z = x.double() + bias.double()
    what = "bias_gelu values %dx%d " % (rows, cols)
    y = ops.ext().bias_gelu_fwd(x.to(DEV), bias.to(DEV))
    ex.assert_gelu_within_bound(y.cpu(), z)

    eps, ref_err = rw.gelu_grad_eps(z)
    grad64 = rw.gelu_grad_f64(z)
    ref = dy.double() * grad64
    dx, dbias = ops.ext().bias_gelu_bwd(x.to(DEV), bias.to(DEV), dy.to(DEV))
    # the kernel's own gelu' error, seen through dx where |dy| >= 1
    big = dy.double().abs() >= 1
    seen = ((dx.double().cpu() - ref).abs() - 2.0 ** -8 * ref.abs()) \
        / dy.double().abs()
    print(what + "gelu' fp32 torch err %.3g allowed %.3g; dx excess over "
          "the bf16 term / |dy| %.3g" % (ref_err, eps, seen[big].max()))
    _within(dx, ref, 2.0 ** -8 * ref.abs() + dy.double().abs() * eps,
            what + "dx")
    tol = (dy.double().abs().sum(0) * eps
           + rows * 2.0 ** -24 * ref.abs().sum(0))
    _within(dbias, ref.sum(0), tol, what + "dbias")
