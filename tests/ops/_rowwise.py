"""Operands, float64 references and bounds for the LayerNorm and
bias+GELU refchecks (tests/ops/test_rowwise_exact_gpu.py); checked
without a GPU by tests/ops/test_rowwise_helpers_cpu.py.

Two kinds of operands, all drawn on the CPU from a generator seeded by
the case key (see _exact.py):

* exact ones. layernorm_bwd takes mean and rstd as inputs, so integer
  x - mean, an integer mean, a power-of-two rstd, integer dy and integer
  gamma make every product and every partial sum of dgamma / dbeta an
  exactly representable fp32 number in ANY accumulation order
  (registers, LDS atomics, the partial-slab fold, global atomics): the
  kernel has to reproduce the float64 result bit for bit, and a lost
  row or a dropped column changes integers. For bias+GELU, z = x + bias
  in {0, 16} makes gelu'(z) in {1/2, 1} and gelu(z) in {0, 16}.
* random ones with derived bounds, for the values.
"""

import math

import torch

from ._exact import EXACT_LIMIT, case_generator

WAVE, KVEC = 64, 8
LN_EPS = 1e-5

# ---------------------------------------------------------------------------
# shapes (rows, cols), grouped by the path launch_layernorm_bwd /
# launch_bias_gelu_* takes; ln_bwd_path / bias_gelu_*_path mirror the
# dispatch and test_rowwise_helpers_cpu.py checks every shape against it
# ---------------------------------------------------------------------------

LN_BWD_SHAPES = {
    # kmax = ceil(cols / 512) == 1: layernorm_bwd_reg_k<1>
    (1, 64): "reg1", (3, 8): "reg1", (5, 512): "reg1", (7, 509): "reg1",
    (6, 1024): "reg2", (6, 769): "reg2",          # layernorm_bwd_reg_k<2>
    (9, 2047): "reg4", (9, 2048): "reg4",         # layernorm_bwd_reg_k<4>
    # kmax > 4: layernorm_bwd_k, dgamma / dbeta through LDS atomics
    (9, 2056): "lds", (5, 2049): "lds", (4, 8192): "lds",
    (2051, 64): "reg1",      # 513 row quads on 512 blocks: grid-stride
    (2051, 2056): "lds",     # the same through the fallback
}
LN_FWD_SHAPES = list(LN_BWD_SHAPES) + [(8197, 64)]   # 2050 quads on 2048

BG_EXACT_BWD_SHAPES = {
    (1, 8): "vec", (5, 24): "vec", (300, 40): "vec",
    (3, 2056): "vec",        # 257 vectors a row on 256 threads: 2 passes
    (2051, 8): "vec",        # one row a block, 2048 blocks: grid-stride
    (2, 16384): "vec",       # 64 KiB of LDS partials, the binding's limit
    (3, 7): "scalar", (4, 1): "scalar",
    (2051, 9): "scalar",     # grid-stride
}
BG_FWD_LOOP_SHAPE = (524288 + 3, 8)    # 2049 blocks of 256 rows on 2048
BG_VALUE_SHAPES = [(37, 264), (37, 263)]


def ln_bwd_path(rows, cols):
    """Mirror of launch_layernorm_bwd and layernorm_bwd_part_rows:
    (kernel, blocks, True if some block takes a second trip)."""
    kmax = (cols + WAVE * KVEC - 1) // (WAVE * KVEC)
    kernel = {1: "reg1", 2: "reg2"}.get(kmax, "reg4" if kmax <= 4 else "lds")
    quads = (rows + 3) // 4
    blocks = min(quads, 512)
    return kernel, blocks, quads > blocks


def ln_fwd_loops(rows):
    """ln_grid: True if the forward's grid-stride loop takes a second trip."""
    return (rows + 3) // 4 > 2048


def bias_gelu_fwd_path(rows, cols):
    """Mirror of launch_bias_gelu_fwd: (kernel, threads per row, idle
    threads of a block, True if a block takes a second trip)."""
    if cols % 8:
        return "scalar", 0, 0, (rows * cols + 255) // 256 > 2048
    tpr = min(cols // 8, 256)
    rpb = 256 // tpr
    return "vec", tpr, 256 - tpr * rpb, (rows + rpb - 1) // rpb > 2048


def bias_gelu_bwd_path(rows, cols):
    """Mirror of launch_bias_gelu_bwd: (kernel, column passes of a
    row, True if a block takes a second row)."""
    if cols % 8:
        return "scalar", (cols + 255) // 256, rows > 2048
    return "vec", (cols + 2047) // 2048, rows > 2048


# ---------------------------------------------------------------------------
# LayerNorm backward, exact
# ---------------------------------------------------------------------------

LN_DMAX, LN_DYMAX, LN_GMAX = 8, 4, 2
LN_RSTD = (0.25, 0.5, 1.0)
LN_TAIL = 9


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int32)


def ln_bwd_exact_operands(rows, cols, device="cpu", tail_only=False):
    """(x bf16, dy bf16, gamma fp32, mean fp32, rstd fp32): integer
    x - mean with |x - mean| <= 8, integer per-row mean, rstd a power
    of two, integer |dy| <= 4 and |gamma| <= 2.

    ``tail_only`` zeroes gamma except on the last LN_TAIL columns
    (where it is +-1 or +-2). Where cols is no power of two dx is only
    held to a bf16 ulp, which cannot see one column of several hundred
    missing from the two row sums; with all their weight on the last
    columns, the ones a ragged tail handles, a lost column moves every
    dx of the row by a good part of its value."""
    g = case_generator("ln_bwd_exact", rows, cols, tail_only)
    mean = _randint(g, -4, 4, (rows, 1)).float()
    d = _randint(g, -LN_DMAX, LN_DMAX, (rows, cols)).float()
    x = (mean + d).bfloat16()
    assert torch.equal(x.float(), mean + d)
    dy = _randint(g, -LN_DYMAX, LN_DYMAX, (rows, cols)).bfloat16()
    gamma = _randint(g, -LN_GMAX, LN_GMAX, (cols,)).float()
    if tail_only:
        gamma[:-LN_TAIL] = 0
        t = gamma[-LN_TAIL:]
        t[t == 0] = 1
    rstd = torch.tensor(LN_RSTD)[_randint(g, 0, len(LN_RSTD) - 1,
                                          (rows,)).long()]
    check_ln_bwd_bound(rows, cols)
    return tuple(t.to(device) for t in
                 (x, dy, gamma, mean.flatten().contiguous(), rstd))


def check_ln_bwd_bound(rows, cols):
    """dbeta = sum dy and dgamma = sum dy * xhat over the rows are
    integer multiples of min(rstd) whose partial sums, counted in that
    unit, stay below 2^24: exact in fp32 in any order. The same for the
    two row sums of dx (over cols, with gamma)."""
    unit = min(LN_RSTD)
    col = rows * LN_DYMAX * LN_DMAX * max(LN_RSTD) / unit
    row = cols * LN_DYMAX * LN_GMAX * LN_DMAX * max(LN_RSTD) / unit
    assert col < EXACT_LIMIT and row < EXACT_LIMIT, (rows, cols, col, row)
    return col, row


def ln_bwd_ref(x, dy, gamma, mean, rstd, dtype=torch.float64):
    """LayerNorm backward from saved statistics, evaluated in ``dtype``
    in the order the kernels use. Returns (dx, dgamma, dbeta, terms)
    with terms = (dyg, s1, xhat * s2) for the dx bound."""
    cols = x.shape[-1]
    x, dy, gamma = x.to(dtype), dy.to(dtype), gamma.to(dtype)
    mean, rstd = mean.to(dtype)[:, None], rstd.to(dtype)[:, None]
    xh = (x - mean) * rstd
    dyg = dy * gamma
    s1 = dyg.sum(-1, keepdim=True) / cols
    s2 = (dyg * xh).sum(-1, keepdim=True) / cols
    dx = rstd * (dyg - s1 - xh * s2)
    return dx, (dy * xh).sum(0), dy.sum(0), (dyg, s1.expand_as(dyg), xh * s2)


def ln_dx_bound(ref, terms, rstd):
    """Allowed |dx - ref| where cols is no power of two: one bf16 ulp
    of the result, and 2^-18 of the terms for the two fp32 divisions by
    cols and the roundings of the products and differences that follow
    them (a handful of 2^-24 relative errors; 2^-18 leaves 64 of them).
    """
    dyg, s1, xs2 = terms
    scale = rstd.double()[:, None] * (dyg.abs() + s1.abs() + xs2.abs())
    return 2.0 ** -8 * ref.abs() + 2.0 ** -18 * scale


# ---------------------------------------------------------------------------
# LayerNorm forward
# ---------------------------------------------------------------------------

def ln_fwd_operands(rows, cols, device="cpu"):
    """(x bf16, gamma fp32, beta fp32, kinds): random rows; the last
    row is constant (variance 0: the clamp) when rows >= 2 and the one
    before sits at offset 100 with spread 0.25 when rows >= 3 (bf16
    leaves 99.5, 100, 100.5 ...; the one-pass variance cancels). kinds[r] is 0 centred, 1 offset,
    2 constant. gamma and beta hold bf16 values in fp32."""
    g = case_generator("ln_fwd", rows, cols)
    x = torch.randn(rows, cols, generator=g)
    kinds = torch.zeros(rows, dtype=torch.int8)
    if rows >= 2:
        x[-1] = 1.5
        kinds[-1] = 2
    if rows >= 3:
        x[-2] = 100 + 0.25 * torch.randn(cols, generator=g)
        kinds[-2] = 1
    gamma = torch.randn(cols, generator=g).bfloat16().float()
    beta = torch.randn(cols, generator=g).bfloat16().float()
    return x.bfloat16().to(device), gamma.to(device), beta.to(device), kinds


def ln_fwd_ref(x, gamma, beta, eps=LN_EPS):
    """float64 (mean, rstd, xhat * gamma, y)."""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / (var + eps).sqrt()
    xg = (x - mean) * rstd * gamma.double()
    return mean.flatten(), rstd.flatten(), xg, xg + beta.double()


def ln_stats_fp32_torch(x, eps=LN_EPS):
    """The kernel's formula, E[x^2] - E[x]^2 clamped at 0, in plain
    fp32 torch on the CPU (torch's own summation order)."""
    x = x.float().cpu()
    mean = x.mean(-1)
    var = ((x * x).mean(-1) - mean * mean).clamp_min(0)
    return mean, torch.rsqrt(var + eps)


def ln_stats_fp32_kernel_order(x, eps=LN_EPS):
    """fp32 emulation of layernorm_fwd_k's first pass: lane l adds the
    elements of columns [8 l + 512 k, 8 l + 512 k + 8) one by one for
    k = 0, 1, ..., then the 64 lanes fold in an xor butterfly (offsets
    1, 2, ... 32)."""
    x = x.float().cpu()
    rows, cols = x.shape
    K = (cols + WAVE * KVEC - 1) // (WAVE * KVEC)
    pad = torch.zeros(rows, K * WAVE * KVEC)
    pad[:, :cols] = x          # adding 0.0 changes no partial sum
    pad = pad.view(rows, K, WAVE, KVEC)
    s = torch.zeros(rows, WAVE)
    ss = torch.zeros(rows, WAVE)
    for k in range(K):
        for j in range(KVEC):
            f = pad[:, k, :, j]
            s = s + f
            ss = ss + f * f
    lanes = torch.arange(WAVE)
    off = 1
    while off < WAVE:
        s = s + s[:, lanes ^ off]
        ss = ss + ss[:, lanes ^ off]
        off <<= 1
    mean = s[:, 0] / cols
    var = (ss[:, 0] / cols - mean * mean).clamp_min(0)
    return mean, torch.rsqrt(var + eps)


def rel_err(got, ref64):
    ref64 = ref64.double().cpu()
    return ((got.double().cpu() - ref64).abs() / ref64.abs())


def ln_y_bound(ref_y, xg, beta, delta):
    """|y - ref| <= 2^-8 |ref| + 2^-18 (|xhat gamma| + |beta|)
    + |xhat gamma| delta: the bf16 store, the fp32 evaluation, and the
    relative error delta[row] allowed on rstd. No free absolute term."""
    xg = xg.abs()
    return (2.0 ** -8 * ref_y.abs() + 2.0 ** -18 * (xg + beta.double().abs())
            + xg * delta.double()[:, None])


# ---------------------------------------------------------------------------
# bias + GELU
# ---------------------------------------------------------------------------

BG_DYMAX = 4
K_RSQRT2 = 0.70710678118654752
K_RSQRT2PI = 0.39894228040143268


def bias_gelu_exact_operands(rows, cols, device="cpu"):
    """(x bf16, bias fp32, dy bf16) with integer bias in [-8, 8],
    x in {-bias, 16 - bias} so that z = x + bias is 0 or 16, and
    integer |dy| <= 4."""
    g = case_generator("bias_gelu_exact", rows, cols)
    bias = _randint(g, -8, 8, (cols,)).float()
    z = 16.0 * _randint(g, 0, 1, (rows, cols)).float()
    x = (z - bias).bfloat16()
    assert torch.equal(x.float() + bias, z)
    dy = _randint(g, -BG_DYMAX, BG_DYMAX, (rows, cols)).bfloat16()
    assert rows * BG_DYMAX * 2 < EXACT_LIMIT     # dbias in halves
    return x.to(device), bias.to(device), dy.to(device)


def bias_gelu_exact_ref(x, bias, dy):
    """(y, dx, dbias) in float64 for z in {0, 16}: gelu is 0 or 16 and
    gelu' is 1/2 or 1 (to within 1e-55, far below half an fp32 ulp)."""
    z = x.double() + bias.double()
    assert bool(((z == 0) | (z == 16)).all())
    grad = torch.where(z == 0, 0.5, 1.0).double()
    dx = dy.double() * grad
    return z, dx, dx.sum(0)


def gelu_grad_f64(z):
    z = z.double()
    return (0.5 * torch.special.erfc(-z * math.sqrt(0.5))
            + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi))


def gelu_grad_fp32_as_kernel(z):
    """gelu_grad_f of csrc/bias_gelu.hip in plain fp32 torch."""
    z = z.float()
    return (0.5 * (1.0 + torch.erf(z * K_RSQRT2))
            + z * K_RSQRT2PI * torch.exp(-0.5 * z * z))


def gelu_fp32_as_kernel(z):
    z = z.float()
    return 0.5 * z * (1.0 + torch.erf(z * K_RSQRT2))


def bias_gelu_value_operands(rows, cols, device="cpu"):
    """(x bf16, bias fp32, dy bf16): z = x + bias sweeps [-8, 8] with
    both tails, +-0 and the region around the minimum of GELU; bias is
    0 on even columns (z is then the bf16 grid itself, +-0 included)
    and a non-bf16 fp32 number on odd ones."""
    g = case_generator("bias_gelu_values", rows, cols)
    n = rows * cols
    grid = torch.linspace(-8, 8, n - 8)
    special = torch.tensor([0.0, -0.0, 8.0, -8.0, -0.75, 0.75, -5.5, 5.5])
    x = torch.cat([special, grid])[torch.randperm(n, generator=g)]
    x = x.view(rows, cols).bfloat16()
    x[0, 0], x[1, 0] = 0.0, -0.0
    bias = torch.zeros(cols)
    bias[1::2] = (torch.rand((cols // 2,), generator=g) - 0.5) * 0.3
    dy = torch.randn(rows, cols, generator=g).bfloat16()
    return x.to(device), bias.to(device), dy.to(device)


def gelu_grad_eps(z64):
    """epsilon of the backward bound: 4 x the largest error of the
    plain fp32 torch evaluation of the kernel's formula on this grid."""
    err = (gelu_grad_fp32_as_kernel(z64.float()).double()
           - gelu_grad_f64(z64)).abs().max().item()
    return 4 * err, err
