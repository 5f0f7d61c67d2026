"""Conv3x3 off the GPU: the SPARKDL_CONV3X3 routing table, and that the
module and the ResNet bottleneck built on it are nn.Conv2d in everything
but the opt-in kernel route."""

import pytest
import torch
import torch.nn as nn

import sparkdl.ops as ops
from sparkdl.models import resnet


@pytest.mark.parametrize("env,cin,cout,stride,want", [
    (None, 64, 64, 1, False),     # unset is off
    ("0", 64, 64, 1, False),
    ("1", 64, 64, 1, True),
    ("1", 512, 512, 1, True),
    ("1", 128, 128, 2, False),    # stride 2 is off
    ("1", 96, 64, 1, False),      # Cin = 96 is off
    ("1", 64, 96, 1, False),
])
def test_route(monkeypatch, env, cin, cout, stride, want):
    if env is None:
        monkeypatch.delenv("SPARKDL_CONV3X3", raising=False)
    else:
        monkeypatch.setenv("SPARKDL_CONV3X3", env)
    assert ops.conv3x3_route(cin, cout, stride) is want
    assert ops.conv3x3_route(cin, cout, stride, mode="0") is False


@pytest.mark.parametrize("env", [None, "1"])
def test_module_is_conv2d_on_cpu(monkeypatch, env):
    if env is None:
        monkeypatch.delenv("SPARKDL_CONV3X3", raising=False)
    else:
        monkeypatch.setenv("SPARKDL_CONV3X3", env)
    torch.manual_seed(3)
    m = ops.Conv3x3(64, 64)
    x = torch.randn(2, 64, 6, 5)
    assert torch.equal(m(x), nn.Conv2d.forward(m, x))
    assert torch.equal(ops.conv3x3(x, m.weight),
                       torch.nn.functional.conv2d(x, m.weight, padding=1))


def test_bottleneck_state_dict_unchanged(monkeypatch):
    torch.manual_seed(11)
    new = resnet.Bottleneck(256, 64, stride=2).state_dict()
    # the bottleneck as it was: conv2 a plain nn.Conv2d
    monkeypatch.setattr(
        resnet, "Conv3x3",
        lambda cin, cout, stride: nn.Conv2d(cin, cout, 3, stride=stride,
                                            padding=1, bias=False))
    torch.manual_seed(11)
    old = resnet.Bottleneck(256, 64, stride=2).state_dict()
    assert list(new) == list(old)
    for k in old:
        assert torch.equal(new[k], old[k]), k
