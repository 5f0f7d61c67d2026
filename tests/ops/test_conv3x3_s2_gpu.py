"""conv3x3 at stride 2 (csrc/conv3x3_s2.hip, forward and data gradient)
against the exact-arithmetic method of tests/ops/_exact.py: integer-valued
bf16 operands, fp64 conv2d on the CPU as reference.

With |x|, |w| <= 16 every partial sum of the forward is at most
16*16*9*Cin, and of the data gradient at most 16*16*4*Cout (at most four
taps meet in a dx pixel): below 2^24, so fp32 accumulation is exact in any
order and the kernels have to return to_bf16(reference) bit for bit. In
the autograd test everything is in {-1, 0, 1} and N*Ho*Wo <= 256, so the
weight gradient's integers are exact in bf16 whatever the library's
rounding.
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


def _out(h):
    return (h - 1) // 2 + 1


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _conv(x, w):
    return torch.nn.functional.conv2d(x, w, stride=2, padding=1)


# (N, H, W, Cin, Cout, max_workers) -> (rows, imgs, tiles, workers) of
# conv3x3_s2_plan: at most 256 output pixels and 1152 halo pixels
# (2*rows+1)(2*Wo+1) per tile, 32-channel slices
FORWARD_CASES = {
    # every neighbour is padding: 1x1 output, halo 3x3
    (1, 1, 1, 64, 64, 0): (1, 128, 1, 1),
    (1, 2, 2, 64, 64, 0): (1, 128, 1, 1),
    # odd, H != W: right column and bottom row are padding; 3x4 output,
    # halo 7x9, both images in one tile
    (2, 5, 7, 64, 64, 0): (3, 18, 1, 1),
    # even, H != W, four slices
    (1, 6, 8, 128, 64, 0): (3, 18, 1, 1),
    # fewer images than a tile holds (five 7x7 outputs, halo 15x15)
    (3, 14, 14, 64, 64, 0): (7, 5, 1, 1),
    # a full and a partly filled tile on one worker: the slices of the
    # second tile are staged over the first's
    (7, 14, 14, 128, 64, 1): (7, 5, 2, 1),
    # two N-blocks; one 14x14 output, halo 29x29
    (1, 28, 28, 64, 128, 0): (14, 1, 1, 1),
    # 4 bands of 7 rows at the widest rows: halo rows come from the
    # neighbouring bands
    (1, 56, 56, 64, 64, 0): (7, 1, 4, 4),
    # short last band: 11 output rows as 6 + 5
    (1, 22, 56, 64, 64, 0): (6, 1, 2, 2),
    # odd widest width: 5x28 output, halo 11x57
    (1, 9, 55, 64, 64, 0): (5, 1, 1, 1),
    # odd geometry, six slices, three N-blocks; 10x13 output, halo 21x27
    (2, 19, 25, 192, 192, 0): (10, 1, 2, 2),
    # 10 tiles on 2 workers: five trips each
    (10, 28, 28, 64, 64, 2): (14, 1, 10, 2),
}

# the same for conv3x3_s2_dgrad_plan: at most 128 cells of the dy grid and
# 256 halo pixels (rows+1)(Wo+1) per tile, 64-channel slices of Cout
DGRAD_CASES = {
    (1, 1, 1, 64, 64, 0): (1, 64, 1, 1),
    (1, 2, 2, 64, 64, 0): (1, 64, 1, 1),
    # cells lack their last dx row and column; 3x4 cells, halo 4x5
    (2, 5, 7, 64, 64, 0): (3, 10, 1, 1),
    # H = 1: only the classes of dx row 0
    (1, 1, 6, 64, 64, 0): (1, 32, 1, 1),
    # even, H != W, two slices
    (1, 6, 8, 64, 128, 0): (3, 10, 1, 1),
    # fewer images than a tile holds (two 7x7 dy images, halo 8x8)
    (1, 14, 14, 64, 64, 0): (7, 2, 1, 1),
    # a full and a partly filled tile on one worker
    (3, 14, 14, 128, 128, 1): (7, 2, 2, 1),
    # two blocks of dx channels; 14 rows of cells as 7 + 7
    (1, 28, 28, 128, 64, 0): (7, 1, 2, 2),
    # 7 bands of 4 rows at the widest rows
    (1, 56, 56, 64, 64, 0): (4, 1, 7, 7),
    # short last band: 11 rows of cells as 4 + 4 + 3
    (1, 22, 56, 64, 64, 0): (4, 1, 3, 3),
    # odd widest width: 5 rows of 28 cells as 3 + 2
    (1, 9, 55, 64, 64, 0): (3, 1, 2, 2),
    # odd geometry, three slices, three blocks; 10 rows of 13 as 5 + 5
    (2, 19, 25, 192, 192, 0): (5, 1, 4, 4),
    # 20 tiles on 2 workers: ten trips each, resident weights
    (10, 28, 28, 64, 64, 2): (7, 1, 20, 2),
}


def _ids(cases):
    return ["x".join(map(str, c)) for c in cases]


@pytest.mark.parametrize("case", list(FORWARD_CASES), ids=_ids(FORWARD_CASES))
def test_forward_exact(case):
    n, h, w, cin, cout, cap = case
    C = ops.ext()
    assert tuple(C.conv3x3_s2_plan(n, h, w, cin, cout, cap)) \
        == FORWARD_CASES[case]
    g = ex.case_generator("conv3x3_s2", *case)
    x = ex.int_operand((n, cin, h, w), 16, "cpu", g)
    wt = ex.int_operand((cout, cin, 3, 3), 16, "cpu", g)
    ex.check_exact_bound(16, 16, 9 * cin)
    want = ex.to_bf16(_conv(x.double(), wt.double())) \
        .permute(0, 2, 3, 1).contiguous()
    xg, wg = _nhwc(x), _nhwc(wt)
    got = C.conv3x3_s2(xg, wg, cap)
    ex.assert_equal(got.cpu(), want, "y %s" % (case,))
    assert torch.equal(C.conv3x3_s2(xg, wg, cap), got)


@pytest.mark.parametrize("case", list(DGRAD_CASES), ids=_ids(DGRAD_CASES))
def test_dgrad_exact(case):
    n, h, w, cin, cout, cap = case
    C = ops.ext()
    assert tuple(C.conv3x3_s2_dgrad_plan(n, h, w, cin, cout, cap)) \
        == DGRAD_CASES[case]
    g = ex.case_generator("conv3x3_s2 dgrad", *case)
    dy = ex.int_operand((n, cout, _out(h), _out(w)), 16, "cpu", g)
    wt = ex.int_operand((cout, cin, 3, 3), 16, "cpu", g)
    ex.check_exact_bound(16, 16, 4 * cout)
    xr = torch.zeros(n, cin, h, w, dtype=torch.float64, requires_grad=True)
    _conv(xr, wt.double()).backward(dy.double())
    want = ex.to_bf16(xr.grad).permute(0, 2, 3, 1).contiguous()
    dyg = _nhwc(dy)
    wd = wt.permute(1, 2, 3, 0).contiguous().cuda()  # [Cin,3,3,Cout]
    got = C.conv3x3_s2_dgrad(dyg, wd, h, w, cap)
    ex.assert_equal(got.cpu(), want, "dx %s" % (case,))
    assert torch.equal(C.conv3x3_s2_dgrad(dyg, wd, h, w, cap), got)


@pytest.mark.parametrize("n,h,w,cin,cout",
                         [(2, 16, 14, 64, 128), (3, 9, 13, 128, 64)])
def test_autograd_exact(monkeypatch, n, h, w, cin, cout):
    ho, wo = _out(h), _out(w)
    g = ex.case_generator("conv3x3_s2 autograd", n, h, w, cin, cout)
    x = ex.int_operand((n, cin, h, w), 1, "cpu", g)
    wt = ex.int_operand((cout, cin, 3, 3), 1, "cpu", g)
    dy = ex.int_operand((n, cout, ho, wo), 1, "cpu", g)
    assert n * ho * wo <= 256
    xr = x.double().requires_grad_()
    wr = wt.double().requires_grad_()
    yr = _conv(xr, wr)
    yr.backward(dy.double())

    cl = torch.channels_last
    mod = ops.Conv3x3(cin, cout, 2).cuda().to(memory_format=cl)
    with torch.no_grad():
        mod.weight.copy_(wt)
    mod = mod.bfloat16()

    def via_function(xg):
        wg = wt.cuda().to(memory_format=cl).requires_grad_()
        return ops.conv3x3(xg, wg, stride=2), wg

    def via_module(xg):
        mod.weight.grad = None
        return mod(xg), mod.weight

    monkeypatch.setenv("SPARKDL_CONV3X3_S2", "1")
    for run in (via_function, via_module):
        xg = x.cuda().to(memory_format=cl).requires_grad_()
        y, wg = run(xg)
        assert "Conv3x3S2" in type(y.grad_fn).__name__
        y.backward(dy.cuda().to(memory_format=cl))
        ex.assert_equal(y.detach().cpu(), ex.to_bf16(yr.detach()), "y")
        ex.assert_equal(xg.grad.cpu(), ex.to_bf16(xr.grad), "dx")
        assert wg.grad.shape == wt.shape
        assert torch.equal(wg.grad.cpu().double(), wr.grad), "dw"

    xg = x.cuda().to(memory_format=cl)
    with pytest.raises(ValueError):
        ops.conv3x3(xg, mod.weight, wgrad=True, stride=2)
    # switch unset: the module is the library's convolution
    monkeypatch.delenv("SPARKDL_CONV3X3_S2")
    assert "ConvolutionBackward" in type(mod(xg).grad_fn).__name__


def test_bad_arguments_raise():
    C = ops.ext()

    def z(*shape):
        return torch.zeros(*shape, device="cuda", dtype=torch.bfloat16)

    with pytest.raises(RuntimeError):   # Cin = 96
        C.conv3x3_s2(z(1, 4, 4, 96), z(64, 3, 3, 96))
    with pytest.raises(RuntimeError):   # Cin of x and wt differ
        C.conv3x3_s2(z(1, 4, 4, 64), z(64, 3, 3, 128))
    with pytest.raises(RuntimeError):   # 5x5 taps
        C.conv3x3_s2(z(1, 4, 4, 64), z(64, 5, 5, 64))
    with pytest.raises(RuntimeError):   # non-contiguous x
        C.conv3x3_s2(z(1, 4, 4, 128)[..., :64], z(64, 3, 3, 64))
    with pytest.raises(RuntimeError):   # dy 2x2 is not the output of 5x5
        C.conv3x3_s2_dgrad(z(1, 2, 2, 64), z(64, 3, 3, 64), 5, 5)
    with pytest.raises(RuntimeError):   # Cout of dy and wd differ
        C.conv3x3_s2_dgrad(z(1, 2, 2, 64), z(64, 3, 3, 128), 4, 4)
