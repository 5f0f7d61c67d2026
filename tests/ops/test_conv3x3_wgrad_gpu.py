"""conv3x3_wgrad against the exact-arithmetic method of tests/ops/_exact.py:
with integer |x|, |dy| <= 16 every partial sum over N*H*W <= 3920 pixels
stays below 2^24, in any order, slab and slab sum, so the kernel returns
to_bf16 of the fp64 CPU reference bit for bit."""

import pytest
import torch

from tests.ops import _exact as ex

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sparkdl.ops as ops


@pytest.fixture(autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")


def _ref_dw(x, dy):
    """fp64 dw [Cout,Cin,3,3] for x [N,Cin,H,W], dy [N,Cout,H,W] (CPU)."""
    w = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=torch.float64,
                    requires_grad=True)
    torch.nn.functional.conv2d(x.double(), w, padding=1).backward(dy.double())
    return w.grad


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


# (N, H, W, Cin, Cout, max_workers) -> (rows, imgs, tiles, workers) of
# conv3x3_wgrad_plan, the property the case is here for
WGRAD_CASES = {
    # every neighbour is padding: eight taps are exactly zero
    (1, 1, 1, 64, 64, 0): (1, 46, 1, 1),
    # H != W, two images in one tile, 30 pixels: less than one K-step
    (2, 3, 5, 64, 64, 0): (3, 11, 1, 1),
    # one worker, two tiles, the second 2 of 5 images; two ci blocks
    (7, 7, 7, 128, 64, 1): (7, 5, 2, 1),
    # two co blocks; 196 pixels: the last K-step is partly empty
    (1, 14, 14, 64, 128, 0): (14, 1, 1, 1),
    # four bands per image, halo rows from the neighbours, eight slabs
    (2, 28, 28, 64, 64, 0): (7, 1, 8, 8),
    # short last band at the widest rows
    (1, 10, 56, 64, 64, 0): (4, 1, 3, 3),
    # odd geometry, 3 x 3 block pairs
    (2, 10, 13, 192, 192, 0): (10, 1, 2, 2),
    # 20 tiles on 2 workers: accumulation over ten tiles, two slabs
    (5, 28, 28, 64, 64, 2): (7, 1, 20, 2),
}


@pytest.mark.parametrize("case", list(WGRAD_CASES),
                         ids=["x".join(map(str, c)) for c in WGRAD_CASES])
def test_wgrad_exact(case):
    n, h, w, cin, cout, cap = case
    C = ops.ext()
    plan = tuple(C.conv3x3_wgrad_plan(n, h, w, cin, cout, cap))
    assert plan == WGRAD_CASES[case]
    g = ex.case_generator("conv3x3 wgrad", n, h, w, cin, cout)
    x = ex.int_operand((n, cin, h, w), 16, "cpu", g)
    dy = ex.int_operand((n, cout, h, w), 16, "cpu", g)
    ex.check_exact_bound(16, 16, n * h * w)
    want = ex.to_bf16(_ref_dw(x, dy)).permute(0, 2, 3, 1).contiguous()
    if h == 1 and w == 1:   # only the centre tap sees a pixel
        assert want[:, 1, 1].ne(0).any()
        assert want.ne(0).sum() == want[:, 1, 1].ne(0).sum()
    xg, dyg = _nhwc(x), _nhwc(dy)
    got = C.conv3x3_wgrad(xg, dyg, cap)
    ex.assert_equal(got.cpu(), want, "dw %s" % (case,))
    assert torch.equal(C.conv3x3_wgrad(xg, dyg, cap), got)


def test_wgrad_random_bound():
    """|got - ref| <= 2^-8 |ref| + L 2^-23 (|dy| conv |x|), L = N*H*W: bf16
    half ulp plus fp32 summation bound, each doubled. Derived."""
    n, h, w, cin, cout = 3, 9, 11, 64, 64
    C = ops.ext()
    g = ex.case_generator("conv3x3 wgrad random", n, h, w, cin, cout)
    x = torch.randn(n, cin, h, w, generator=g).bfloat16()
    dy = torch.randn(n, cout, h, w, generator=g).bfloat16()
    ref, mag = _ref_dw(x, dy), _ref_dw(x.abs(), dy.abs())
    xg, dyg = _nhwc(x), _nhwc(dy)
    got = C.conv3x3_wgrad(xg, dyg)
    err = (got.cpu().permute(0, 3, 1, 2).double() - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + n * h * w * 2.0 ** -23 * mag
    print("worst err/bound %.3f" % (err / tol).max().item())
    assert bool((err <= tol).all()), (err / tol).max().item()
    assert torch.equal(C.conv3x3_wgrad(xg, dyg), got)


@pytest.mark.parametrize("n,h,w,cin,cout",
                         [(2, 8, 9, 64, 128), (1, 7, 7, 128, 64)])
def test_autograd_exact(n, h, w, cin, cout):
    g = ex.case_generator("conv3x3 wgrad autograd", n, h, w, cin, cout)
    x = ex.int_operand((n, cin, h, w), 4, "cpu", g)
    wt = ex.int_operand((cout, cin, 3, 3), 4, "cpu", g)
    dy = ex.int_operand((n, cout, h, w), 4, "cpu", g)
    for length in (9 * cin, 9 * cout, n * h * w):
        ex.check_exact_bound(4, 4, length)
    xr = x.double().requires_grad_()
    wr = wt.double().requires_grad_()
    yr = torch.nn.functional.conv2d(xr, wr, padding=1)
    yr.backward(dy.double())

    cl = torch.channels_last
    dyg = dy.cuda().to(memory_format=cl)
    xg = x.cuda().to(memory_format=cl).requires_grad_()
    wg = wt.cuda().to(memory_format=cl).requires_grad_()
    y = ops.conv3x3(xg, wg, wgrad=True)
    y.backward(dyg)
    ex.assert_equal(y.detach().cpu(), ex.to_bf16(yr.detach()), "y")
    ex.assert_equal(xg.grad.cpu(), ex.to_bf16(xr.grad), "dx")
    assert wg.grad.shape == wt.shape
    ex.assert_equal(wg.grad.cpu(), ex.to_bf16(wr.grad), "dw")
    # weight only: no dx, the same dw
    x2 = x.cuda().to(memory_format=cl)
    w2 = wt.cuda().to(memory_format=cl).requires_grad_()
    ops.conv3x3(x2, w2, wgrad=True).backward(dyg)
    assert x2.grad is None
    assert torch.equal(w2.grad, wg.grad)
    # the library's weight gradient still flows when asked for
    w3 = wt.cuda().to(memory_format=cl).requires_grad_()
    ops.conv3x3(x2, w3, wgrad=False).backward(dyg)
    assert w3.grad is not None and w3.grad.shape == wt.shape


def test_bad_arguments_raise():
    C = ops.ext()

    def z(*shape, dtype=torch.bfloat16):
        return torch.zeros(*shape, device="cuda", dtype=dtype)

    with pytest.raises(RuntimeError):   # Cin = 96
        C.conv3x3_wgrad(z(1, 4, 4, 96), z(1, 4, 4, 64))
    with pytest.raises(RuntimeError):   # x and dy differ in H
        C.conv3x3_wgrad(z(1, 4, 4, 64), z(1, 5, 4, 64))
    with pytest.raises(RuntimeError):   # non-contiguous dy
        C.conv3x3_wgrad(z(1, 4, 4, 64), z(1, 4, 4, 128)[..., :64])
    with pytest.raises(RuntimeError):   # fp32 x
        C.conv3x3_wgrad(z(1, 4, 4, 64, dtype=torch.float32), z(1, 4, 4, 64))
