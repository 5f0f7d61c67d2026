"""The plumbing of the forked BatchNorm output without a GPU: on the
CPU `batch_norm_act(..., fork=True)` takes the reference path and
returns `(y, y)`, so ResNet-50 must compute exactly what it computed
with a single tensor passed from block to block, whatever
SPARKDL_FUSED_RESGRAD says."""

import pytest
import torch

from sparkdl.models.resnet import Bottleneck, ResNet50
from sparkdl.ops import BatchNormAct2d
from tests.ops.test_bn_pool_gpu import PARENT_STATE_DICT_KEYS


def _resnet_run(monkeypatch, switch, bn3_gamma):
    monkeypatch.setenv("SPARKDL_FUSED_RESGRAD", switch)
    torch.manual_seed(0)
    model = ResNet50(num_classes=10).train()
    if bn3_gamma is not None:
        for m in model.modules():
            if isinstance(m, Bottleneck):
                torch.nn.init.constant_(m.bn3.weight, bn3_gamma)
    x = torch.randn(2, 3, 32, 32)
    logits = model(x)
    logits.square().mean().backward()
    return model, logits.detach()


# gamma of every bn3: None keeps the model's zero init, under which no
# gradient comes back through the convolutions of a block; 0.5 makes
# both partial gradients of every fork nonzero
@pytest.mark.parametrize("bn3_gamma", [None, 0.5], ids=["zero_init", "g0.5"])
def test_resnet50_cpu_switch_on_equals_off(monkeypatch, bn3_gamma):
    m1, l1 = _resnet_run(monkeypatch, "1", bn3_gamma)
    m0, l0 = _resnet_run(monkeypatch, "0", bn3_gamma)
    assert list(m1.state_dict().keys()) == PARENT_STATE_DICT_KEYS
    names = [n for n, _ in m1.named_parameters()]
    assert names == [n for n, _ in m0.named_parameters()]
    assert names == [k for k in PARENT_STATE_DICT_KEYS
                     if not k.endswith(("running_mean", "running_var"))]
    assert torch.equal(l1, l0)
    g0 = dict((n, p.grad) for n, p in m0.named_parameters())
    for n, p in m1.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        assert torch.equal(p.grad, g0[n]), n


def test_bottleneck_takes_tensor_or_pair():
    for cin, width, stride in ((16, 4, 1), (8, 4, 2)):
        torch.manual_seed(1)
        blk = Bottleneck(cin, width, stride).train()
        torch.nn.init.constant_(blk.bn3.weight, 0.5)
        t = torch.randn(2, cin, 6, 6, requires_grad=True)
        g = torch.randn(2, 4 * width, 6 // stride, 6 // stride)
        params = list(blk.parameters())
        results = []
        for arg in (t, (t, t)):
            out = blk(arg)
            assert isinstance(out, tuple) and len(out) == 2
            # each member once, as the next block consumes them
            grads = torch.autograd.grad(
                [out[0], out[1]], [t] + params, [g, 0.5 * g])
            results.append((out[0].detach(), out[1].detach()) + grads)
        for a, b in zip(*results):
            assert torch.equal(a, b)


def test_forked_module_equals_unforked_used_twice():
    torch.manual_seed(2)
    x0 = torch.randn(3, 8, 5, 4)
    r0 = torch.randn(3, 8, 5, 4)
    ga, gb = torch.randn(3, 8, 5, 4), torch.randn(3, 8, 5, 4)
    results = []
    for fork in (True, False):
        bn = BatchNormAct2d(8, relu=True).train()
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, 8))
            bn.bias.copy_(torch.linspace(-0.5, 0.5, 8))
        x = x0.clone().requires_grad_(True)
        r = r0.clone().requires_grad_(True)
        if fork:
            y, y2 = bn(x, residual=r, fork=True)
        else:
            y = y2 = bn(x, residual=r)
        torch.autograd.backward([y, y2], [ga, gb])
        results.append((y.detach(), y2.detach(), x.grad, r.grad,
                        bn.weight.grad, bn.bias.grad, bn.running_mean,
                        bn.running_var))
    for a, b in zip(*results):
        assert torch.equal(a, b)
