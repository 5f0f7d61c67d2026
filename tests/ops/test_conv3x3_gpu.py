"""conv3x3 (hand-written 3x3 stride-1 pad-1 convolution, forward and
dgrad) against the exact-arithmetic method of tests/ops/_exact.py:
integer-valued bf16 operands, fp64 conv2d on the CPU as reference.

With |x|, |w| <= 16 every partial sum is at most 16*16*9*Cin, below 2^24
for Cin <= 512, so fp32 accumulation is exact in any order and the kernel
has to return to_bf16(reference) bit for bit; typical outputs exceed 256,
so the bf16 rounding takes part. In the autograd test everything is in
{-1, 0, 1}: |dx| <= 9*Cout and |dw| <= N*H*W <= 144 are integers that
bf16 holds exactly, whatever the library's rounding.
"""

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


def _operands(n, h, w, cin, cout, amax, call=0):
    """x [N,Cin,H,W] and wt [Cout,Cin,3,3] on the CPU."""
    g = ex.case_generator("conv3x3", n, h, w, cin, cout, amax, call)
    x = ex.int_operand((n, cin, h, w), amax, "cpu", g)
    wt = ex.int_operand((cout, cin, 3, 3), amax, "cpu", g)
    ex.check_exact_bound(amax, amax, 9 * cin)
    return x, wt


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


# (N, H, W, Cin, Cout, max_workers) -> (rows, imgs, tiles, workers) of
# conv3x3_plan, the property the case is here for
FORWARD_CASES = {
    # every neighbour is padding
    (1, 1, 1, 64, 64, 0): (1, 46, 1, 1),
    # H != W, both images in one tile
    (2, 3, 5, 64, 64, 0): (3, 11, 1, 1),
    # fewer images than a tile holds, two Cin slices
    (3, 7, 7, 128, 64, 0): (7, 5, 1, 1),
    # a full and a partly filled tile on one worker: the slices of the
    # second tile are staged over the first's
    (7, 7, 7, 128, 64, 1): (7, 5, 2, 1),
    # two N-blocks
    (1, 14, 14, 64, 128, 0): (14, 1, 1, 1),
    # 4 bands of 7 rows: halo rows come from the neighbouring bands
    (2, 28, 28, 64, 64, 0): (7, 1, 8, 8),
    # short last band at the widest rows: 4 + 4 + 2 and 6 + 5
    (1, 10, 56, 64, 64, 0): (4, 1, 3, 3),
    (1, 11, 28, 64, 64, 0): (6, 1, 2, 2),
    # odd geometry, three slices, three N-blocks
    (2, 10, 13, 192, 192, 0): (10, 1, 2, 2),
    # 20 tiles on 2 workers: ten trips each, resident weights
    (5, 28, 28, 64, 64, 2): (7, 1, 20, 2),
}


@pytest.mark.parametrize("case", list(FORWARD_CASES),
                         ids=["x".join(map(str, c)) for c in FORWARD_CASES])
def test_forward_exact(case):
    n, h, w, cin, cout, cap = case
    C = ops.ext()
    assert tuple(C.conv3x3_plan(n, h, w, cin, cout, cap)) \
        == FORWARD_CASES[case]
    x, wt = _operands(n, h, w, cin, cout, 16)
    ref = torch.nn.functional.conv2d(x.double(), wt.double(), padding=1)
    want = ex.to_bf16(ref).permute(0, 2, 3, 1).contiguous()
    xg, wg = _nhwc(x), _nhwc(wt)
    got = C.conv3x3(xg, wg, cap)
    ex.assert_equal(got.cpu(), want, "y %s" % (case,))
    assert torch.equal(C.conv3x3(xg, wg, cap), got)


@pytest.mark.parametrize("n,h,w,cin,cout",
                         [(2, 8, 9, 64, 128), (1, 7, 7, 128, 64)])
def test_autograd_exact(n, h, w, cin, cout):
    x, wt = _operands(n, h, w, cin, cout, 1)
    dy = ex.int_operand((n, cout, h, w), 1, "cpu",
                        ex.case_generator("conv3x3 dy", n, h, w, cin, cout))
    ex.check_exact_bound(1, 1, 9 * cout)
    ex.check_exact_bound(1, 1, n * h * w)
    xr = x.double().requires_grad_()
    wr = wt.double().requires_grad_()
    yr = torch.nn.functional.conv2d(xr, wr, padding=1)
    yr.backward(dy.double())

    cl = torch.channels_last
    xg = x.cuda().to(memory_format=cl).requires_grad_()
    wg = wt.cuda().to(memory_format=cl).requires_grad_()
    y = ops.conv3x3(xg, wg)
    assert y.grad_fn is not None and "Conv3x3" in type(y.grad_fn).__name__
    y.backward(dy.cuda().to(memory_format=cl))
    ex.assert_equal(y.detach().cpu(), ex.to_bf16(yr.detach()), "y")
    ex.assert_equal(xg.grad.cpu(), ex.to_bf16(xr.grad), "dx")
    assert xg.grad.shape == x.shape and wg.grad.shape == wt.shape
    assert torch.equal(wg.grad.cpu().double(), wr.grad), "dw"

    # weight only: no dx, the same dw
    x2 = x.cuda().to(memory_format=cl)
    w2 = wt.cuda().to(memory_format=cl).requires_grad_()
    ops.conv3x3(x2, w2).backward(dy.cuda().to(memory_format=cl))
    assert x2.grad is None
    assert torch.equal(w2.grad, wg.grad)


def test_bad_arguments_raise():
    C = ops.ext()

    def z(*shape):
        return torch.zeros(*shape, device="cuda", dtype=torch.bfloat16)

    with pytest.raises(RuntimeError):   # Cin = 96
        C.conv3x3(z(1, 4, 4, 96), z(64, 3, 3, 96))
    with pytest.raises(RuntimeError):   # Cin of x and wt differ
        C.conv3x3(z(1, 4, 4, 64), z(64, 3, 3, 128))
    with pytest.raises(RuntimeError):   # 5x5 taps
        C.conv3x3(z(1, 4, 4, 64), z(64, 5, 5, 64))
    with pytest.raises(RuntimeError):   # non-contiguous x
        C.conv3x3(z(1, 4, 4, 128)[..., :64], z(64, 3, 3, 64))
