"""GPU tests for the fused BatchNorm + ReLU + MaxPool2d(3, 2, 1) chain
(the ResNet stem): `batch_norm_relu_maxpool` against the composed path
of the same build, `batch_norm_act(relu=True)` followed by torch's
`max_pool2d`, selected with SPARKDL_FUSED_STEM=0.

Both paths compute the same rounded values in the same order, so every
comparison is exact (`torch.equal`), over all elements."""

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
    (1, 8, 1, 1),        # a single window, 8 of 9 taps clipped
    (1, 8, 2, 2),        # a single window, clipped on two sides
    (1, 8, 5, 5),        # odd size, clipped on all four borders
    (2, 24, 8, 6),       # even size: last row/column in one window only;
                         # 3 threads per row
    (3, 64, 7, 9),       # the stem's channel count, H != W
    (2, 2048, 4, 4),     # widest C, one row per block
    # 2116 output-row blocks and 8464 input-row blocks against grid
    # limits of 2048; reduce grid 512: 16 rows per thread in the
    # unrolled loop and a tail
    (64, 8, 184, 184),
]
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


def _pooled_shape(shape):
    N, C, H, W = shape
    return (N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)


def _nhwc_bf16(t):
    return t.bfloat16().to(memory_format=torch.channels_last)


def _inputs(shape, kind):
    """x, pooled grad, gamma, beta, running_mean, running_var."""
    C = shape[1]
    g = torch.Generator(device="cuda").manual_seed(1234)
    pshape = _pooled_shape(shape)
    if kind == "normal":
        x = torch.randn(shape, device="cuda", generator=g)
        dy = torch.randn(pshape, device="cuda", generator=g)
    else:
        # 9 values per channel: ties in most windows, and the ReLU
        # zeroes whole windows
        x = torch.randint(-4, 5, shape, device="cuda", generator=g).float()
        dy = torch.randint(-4, 5, pshape, device="cuda",
                           generator=g).float()
    c = torch.arange(C, device="cuda")
    gamma = 0.5 + 0.25 * (c % 5).float()
    beta = ((c % 3).float() - 1.0) * 0.5
    rm = ((c % 7).float() - 3.0) * 0.25
    rv = 0.5 + 0.125 * (c % 4).float()
    return _nhwc_bf16(x), _nhwc_bf16(dy), gamma, beta, rm, rv


def _run(monkeypatch, fused, inputs, training=True, backward=True):
    monkeypatch.setenv("SPARKDL_FUSED_STEM", "1" if fused else "0")
    x0, dy, gamma0, beta0, rm0, rv0 = inputs
    x = x0.clone(memory_format=torch.preserve_format).requires_grad_(True)
    gamma = gamma0.clone().requires_grad_(True)
    beta = beta0.clone().requires_grad_(True)
    rm, rv = rm0.clone(), rv0.clone()
    y = ops.batch_norm_relu_maxpool(x, gamma, beta, rm, rv, momentum=0.1,
                                    eps=1e-5, training=training)
    # the comparison must be between the two paths
    assert (type(y.grad_fn).__name__ == "_BNReLUPoolFnBackward") == fused, \
        y.grad_fn
    out = {"pooled": y.detach(), "running_mean": rm, "running_var": rv}
    if backward:
        y.backward(dy)
        out.update({"dx": x.grad, "dgamma": gamma.grad,
                    "dbeta": beta.grad})
    return out


def _assert_same(a, b):
    assert a.keys() == b.keys()
    bad = []
    for k in a:
        assert a[k].shape == b[k].shape, k
        n = (a[k] != b[k]).sum().item()
        print("%s: %d of %d elements differ" % (k, n, a[k].numel()))
        if not torch.equal(a[k], b[k]):
            bad.append(k)
    assert not bad, bad


@pytest.mark.parametrize("kind", ["normal", "integer"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_fused_equals_composed(monkeypatch, shape, kind):
    inputs = _inputs(shape, kind)
    fused = _run(monkeypatch, True, inputs)
    composed = _run(monkeypatch, False, inputs)
    assert fused["pooled"].shape == _pooled_shape(shape)
    _assert_same(fused, composed)


@pytest.mark.parametrize("kind", ["normal", "integer"])
@pytest.mark.parametrize("shape", SHAPES[:-1], ids=_ids)
def test_eval_mode_equals_composed(monkeypatch, shape, kind):
    """training=False normalises with the running statistics and leaves
    them untouched."""
    inputs = _inputs(shape, kind)
    fused = _run(monkeypatch, True, inputs, training=False)
    composed = _run(monkeypatch, False, inputs, training=False)
    _assert_same(fused, composed)
    assert torch.equal(fused["running_mean"], inputs[4])
    assert torch.equal(fused["running_var"], inputs[5])


def test_fused_bitwise_reproducible(monkeypatch):
    inputs = _inputs((8, 64, 56, 56), "normal")
    a = _run(monkeypatch, True, inputs)
    b = _run(monkeypatch, True, inputs)
    _assert_same(a, b)


def test_ineligible_inputs_compose():
    """fp32 and ragged channel counts take the composed path."""
    x = torch.randn(2, 12, 6, 6, device="cuda", requires_grad=True)
    C = x.shape[1]
    args = (torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"),
            torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"))
    y = ops.batch_norm_relu_maxpool(x, *args)
    assert y.shape == (2, 12, 3, 3)
    assert type(y.grad_fn).__name__ != "_BNReLUPoolFnBackward"


# state_dict() of ResNet50 before the stem fusion: checkpoints and
# bench.py --dump-outputs go by these names and this order.
def _bn(prefix):
    return [prefix + s for s in (".weight", ".bias", ".running_mean",
                                 ".running_var")]


def _block(prefix, down):
    keys = []
    for i in (1, 2, 3):
        keys += ["%s.conv%d.weight" % (prefix, i)]
        keys += _bn("%s.bn%d" % (prefix, i))
    if down:
        keys += [prefix + ".down_conv.weight"] + _bn(prefix + ".down_bn")
    return keys


PARENT_STATE_DICT_KEYS = (
    ["stem_conv.weight"] + _bn("stem_bn")
    + _block("stages.0.0", True) + _block("stages.0.1", False)
    + _block("stages.0.2", False)
    + _block("stages.1.0", True) + _block("stages.1.1", False)
    + _block("stages.1.2", False) + _block("stages.1.3", False)
    + _block("stages.2.0", True) + _block("stages.2.1", False)
    + _block("stages.2.2", False) + _block("stages.2.3", False)
    + _block("stages.2.4", False) + _block("stages.2.5", False)
    + _block("stages.3.0", True) + _block("stages.3.1", False)
    + _block("stages.3.2", False)
    + ["fc.weight", "fc.bias"])


def test_resnet50_fused_stem_equals_composed(monkeypatch):
    from sparkdl.models.resnet import ResNet50

    def run(fused):
        monkeypatch.setenv("SPARKDL_FUSED_STEM", "1" if fused else "0")
        torch.manual_seed(0)
        model = ResNet50(num_classes=10).cuda() \
            .to(memory_format=torch.channels_last).train()
        x = torch.randn(2, 3, 64, 64, device="cuda") \
            .to(memory_format=torch.channels_last)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = model(x)
        logits.float().square().mean().backward()
        return model, logits.detach()

    mf, lf = run(True)
    mc, lc = run(False)
    assert list(mf.state_dict().keys()) == PARENT_STATE_DICT_KEYS
    assert [n for n, _ in mf.named_parameters()] \
        == [n for n, _ in mc.named_parameters()]
    assert isinstance(mf.stem_pool, torch.nn.MaxPool2d)
    print("logits max abs diff", (lf.float() - lc.float()).abs().max().item())
    assert torch.equal(lf, lc)
    assert torch.equal(mf.stem_bn.running_mean, mc.stem_bn.running_mean)
    assert torch.equal(mf.stem_bn.running_var, mc.stem_bn.running_var)
    # MIOpen's weight-gradient kernels are not bitwise run to run, so
    # the gradients are only required to exist and be finite
    for name, p in mf.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
