"""GPU tests for the two-stage (partial-slab) BatchNorm reductions.

The statistics and dgamma/dbeta reductions fold per-block partials in a
fixed order into a slab [G][2*C] that a second kernel sums, with no
float atomics. The shapes below are the smallest that reach each edge
of that geometry (threads per row, rows per block, reduce grid G)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sparkdl.ops as ops


@pytest.fixture(autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")


SHAPES = [
    (1, 8, 5, 5),        # one thread per row, fewer rows than a block holds
    (4, 24, 9, 9),       # 3 threads per row: divides neither 64 nor 256
    (2, 512, 7, 7),      # far fewer rows than slab rows could be
    (3, 2048, 20, 20),   # one row per block pass, widest C
    (8, 64, 56, 56),     # many blocks, 32 rows per block
    (64, 8, 100, 100),   # more row-blocks than the grid cap, ragged tail
    (8, 128, 48, 48),    # every block runs the unrolled row loop, no tail
]


def _nhwc_bf16(t):
    return t.bfloat16().to(memory_format=torch.channels_last)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bn_reduce_exact_integer_sums(shape):
    """Integers in -4..4 are exact in bf16 and every partial sum stays
    below 2**24, so any summation order gives the same fp32 sums: a
    dropped, duplicated or stale partial is a hard mismatch."""
    N, C, H, W = shape
    rows = N * H * W
    g = torch.Generator(device="cuda").manual_seed(11)
    x = _nhwc_bf16(torch.randint(-4, 5, shape, device="cuda", generator=g)
                   .float()).requires_grad_(True)
    dy = _nhwc_bf16(torch.randint(-4, 5, shape, device="cuda", generator=g)
                    .float())
    gamma = torch.ones(C, device="cuda", requires_grad=True)
    beta = torch.zeros(C, device="cuda", requires_grad=True)
    rm = torch.zeros(C, device="cuda")
    rv = torch.zeros(C, device="cuda")

    y = ops.batch_norm_act(x, gamma, beta, rm, rv, momentum=1.0,
                           training=True, relu=False)
    y.backward(dy)

    xd = x.detach().double()
    mean = xd.sum((0, 2, 3)) / rows
    # unbiased variance; rows > 1 at every shape
    var = ((xd * xd).sum((0, 2, 3)) / rows - mean * mean) * rows / (rows - 1)
    print("mean max rel err",
          ((rm.double() - mean).abs() / mean.abs().clamp_min(1e-30)).max()
          .item(),
          "var max rel err", ((rv.double() - var).abs() / var).max().item())
    # momentum 1 from zero: running stats are the batch stats. One
    # rounding for the division, one for int->float of `rows`.
    assert torch.allclose(rm.double(), mean, rtol=4 * 2.0 ** -24, atol=0)
    assert torch.allclose(rv.double(), var, rtol=1e-5, atol=0)
    sum_dy = dy.double().sum((0, 2, 3)).float()
    assert torch.equal(beta.grad, sum_dy), \
        (beta.grad - sum_dy).abs().max()


@pytest.mark.parametrize("relu,res", [(False, False), (True, False),
                                      (True, True)])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bn_reduce_matches_reference(shape, relu, res):
    """Same comparison and tolerances as
    test_kernels_gpu.test_batch_norm_act_matches_reference."""
    torch.manual_seed(7)
    N, C, H, W = shape
    x = torch.randn(N, C, H, W, device="cuda").bfloat16() \
        .to(memory_format=torch.channels_last).requires_grad_(True)
    residual = None
    if res:
        residual = torch.randn_like(x.detach()).requires_grad_(True)
    gamma = torch.rand(C, device="cuda") + 0.5
    beta = torch.randn(C, device="cuda")
    gamma.requires_grad_(True)
    beta.requires_grad_(True)
    rm = torch.zeros(C, device="cuda")
    rv = torch.ones(C, device="cuda")

    y = ops.batch_norm_act(x, gamma, beta, rm, rv, training=True,
                           relu=relu, residual=residual)
    dy = torch.randn_like(y.detach())
    y.backward(dy)

    # fp32 reference
    xr = x.detach().float().requires_grad_(True)
    gr = gamma.detach().clone().requires_grad_(True)
    br = beta.detach().clone().requires_grad_(True)
    rm_r = torch.zeros(C, device="cuda")
    rv_r = torch.ones(C, device="cuda")
    yr = torch.nn.functional.batch_norm(xr, rm_r, rv_r, gr, br, True,
                                        0.1, 1e-5)
    if res:
        rr = residual.detach().float().requires_grad_(True)
        yr = yr + rr
    if relu:
        yr = torch.relu(yr)
    yr.backward(dy.float())

    # Exclude ReLU-boundary elements: bf16 rounding flips the mask where
    # bn(x)+res ~ 0, making both implementations differ by a full dy.
    with torch.no_grad():
        pre = torch.nn.functional.batch_norm(
            x.detach().float(), torch.zeros_like(rm), torch.ones_like(rv),
            gamma.detach(), beta.detach(), True, 0.0, 1e-5)
        if res:
            pre = pre + residual.detach().float()
    interior = (pre.abs() > 3e-2) if relu else torch.ones_like(pre,
                                                               dtype=bool)
    excluded = 1.0 - interior.float().mean().item()
    print("excluded share", excluded)
    assert excluded <= 0.05, excluded
    assert torch.allclose(y.float()[interior], yr.detach()[interior],
                          atol=5e-2, rtol=5e-2)
    assert torch.allclose(rm, rm_r, atol=1e-2, rtol=1e-2)
    assert torch.allclose(rv, rv_r, atol=1e-2, rtol=1e-2)
    assert torch.allclose(x.grad.float()[interior], xr.grad[interior],
                          atol=5e-2, rtol=5e-2), \
        (x.grad.float()[interior] - xr.grad[interior]).abs().max()
    nhw = N * H * W
    assert torch.allclose(gamma.grad, gr.grad, atol=2e-2 * nhw ** 0.5,
                          rtol=2e-2), (gamma.grad - gr.grad).abs().max()
    assert torch.allclose(beta.grad, br.grad, atol=2e-2 * nhw ** 0.5,
                          rtol=2e-2)
    if res:
        assert torch.allclose(residual.grad.float()[interior],
                              rr.grad[interior], atol=5e-2, rtol=5e-2)


@pytest.mark.parametrize("shape", [(8, 64, 56, 56), (3, 2048, 20, 20)],
                         ids=lambda s: "x".join(map(str, s)))
def test_bn_reduce_bitwise_reproducible(shape):
    """Fixed-order folds: two runs from identical inputs and fresh
    running stats agree bit for bit in every output."""
    N, C, H, W = shape
    torch.manual_seed(7)
    x0 = torch.randn(N, C, H, W, device="cuda").bfloat16() \
        .to(memory_format=torch.channels_last)
    r0 = torch.randn_like(x0)
    dy = torch.randn_like(x0)
    gamma0 = torch.rand(C, device="cuda") + 0.5
    beta0 = torch.randn(C, device="cuda")

    def run():
        x = x0.clone(memory_format=torch.preserve_format) \
            .requires_grad_(True)
        r = r0.clone(memory_format=torch.preserve_format) \
            .requires_grad_(True)
        gamma = gamma0.clone().requires_grad_(True)
        beta = beta0.clone().requires_grad_(True)
        rm = torch.zeros(C, device="cuda")
        rv = torch.ones(C, device="cuda")
        y = ops.batch_norm_act(x, gamma, beta, rm, rv, training=True,
                               relu=True, residual=r)
        y.backward(dy)
        return {"y": y.detach(), "running_mean": rm, "running_var": rv,
                "x.grad": x.grad, "residual.grad": r.grad,
                "gamma.grad": gamma.grad, "beta.grad": beta.grad}

    a, b = run(), run()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_bad_arguments_are_refused():
    """The bindings refuse, before any launch, tensors that the kernels
    would read or write out of bounds; a valid call at the same shape
    still runs afterwards and matches the fp32 reference."""
    C = ops.ext()
    torch.manual_seed(3)
    ch = 8
    x = torch.randn(1, 2, 2, ch, device="cuda").bfloat16()   # [N,H,W,C]
    dy = torch.randn_like(x)
    gamma = torch.rand(ch, device="cuda") + 0.5
    beta = torch.randn(ch, device="cuda")
    mean = torch.zeros(ch, device="cuda")
    rstd = torch.ones(ch, device="cuda")
    mask = torch.zeros(x.numel() // 8, device="cuda", dtype=torch.uint8)
    wide = torch.ones(16, device="cuda")

    def bwd(dy=dy, mean=mean, rstd=rstd, mask=mask, relu=False):
        return C.bn_bwd(x, mask, dy, gamma, mean, rstd, True, relu, False)

    def fwd(x=x, rm=None):
        rm = torch.zeros(ch, device="cuda") if rm is None else rm
        rv = torch.ones(ch, device="cuda")
        return C.bn_fwd(x, None, gamma, beta, rm, rv, 0.1, 1e-5, True,
                        False)

    # each with the start of the shared validation's message, so that
    # the refusal is known to come from there and not from later on
    bad = [
        (lambda: bwd(dy=torch.zeros(1, 2, 2, 16, device="cuda",
                                    dtype=torch.bfloat16)),
         "bn_bwd: activations and gradients"),
        (lambda: bwd(mean=wide), "bn_bwd: per-channel tensors"),
        (lambda: bwd(rstd=rstd.double()), "bn_bwd: per-channel tensors"),
        (lambda: bwd(relu=True, mask=mask[:-1]), "bn_bwd: relu backward"),
        (lambda: bwd(relu=True, mask=mask.cpu()), "bn_bwd: relu backward"),
        (lambda: fwd(rm=wide), "bn_fwd: per-channel tensors"),
        (lambda: fwd(x=torch.zeros(1, 2, 2, 12, device="cuda",
                                   dtype=torch.bfloat16)),
         "bn_fwd requires cols%8==0"),
    ]
    for call, message in bad:
        with pytest.raises(RuntimeError, match=message):
            call()

    rm = torch.zeros(ch, device="cuda")
    rv = torch.ones(ch, device="cuda")
    y, save_mean, save_rstd, _ = C.bn_fwd(x, None, gamma, beta, rm, rv, 0.1,
                                          1e-5, True, False)
    dx, dgamma, dbeta = bwd(mean=save_mean, rstd=save_rstd)

    # channels-first views of the NHWC tensors for the reference
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    gr = gamma.clone().requires_grad_(True)
    br = beta.clone().requires_grad_(True)
    rm_r = torch.zeros(ch, device="cuda")
    rv_r = torch.ones(ch, device="cuda")
    yr = torch.nn.functional.batch_norm(xr, rm_r, rv_r, gr, br, True, 0.1,
                                        1e-5)
    yr.backward(dy.float().permute(0, 3, 1, 2))
    nhw = x.numel() // ch
    assert torch.allclose(y.float().permute(0, 3, 1, 2), yr.detach(),
                          atol=5e-2, rtol=5e-2)
    assert torch.allclose(rm, rm_r, atol=1e-2, rtol=1e-2)
    assert torch.allclose(rv, rv_r, atol=1e-2, rtol=1e-2)
    assert torch.allclose(dx.float().permute(0, 3, 1, 2), xr.grad,
                          atol=5e-2, rtol=5e-2)
    assert torch.allclose(dgamma, gr.grad, atol=2e-2 * nhw ** 0.5, rtol=2e-2)
    assert torch.allclose(dbeta, br.grad, atol=2e-2 * nhw ** 0.5, rtol=2e-2)
