"""Stride-2 Conv3x3 off the GPU: the SPARKDL_CONV3X3_S2 routing table,
and that module and function are the library's convolution on the CPU."""

import pytest
import torch
import torch.nn as nn

import sparkdl.ops as ops


@pytest.mark.parametrize("env,cin,cout,want", [
    (None, 64, 64, False),     # unset is off
    ("0", 64, 64, False),
    ("1", 64, 64, True),
    ("1", 512, 512, True),
    ("1", 96, 64, False),      # Cin = 96 is off
    ("1", 64, 96, False),
])
def test_route(monkeypatch, env, cin, cout, want):
    monkeypatch.setenv("SPARKDL_CONV3X3", "1")  # has no say at stride 2
    if env is None:
        monkeypatch.delenv("SPARKDL_CONV3X3_S2", raising=False)
    else:
        monkeypatch.setenv("SPARKDL_CONV3X3_S2", env)
    assert ops.conv3x3_s2_route(cin, cout) is want
    assert ops.conv3x3_s2_route(cin, cout, mode="0") is False
    assert ops.conv3x3_route(cin, cout, 2) is False


def test_module_is_conv2d_on_cpu(monkeypatch):
    monkeypatch.setenv("SPARKDL_CONV3X3_S2", "1")
    torch.manual_seed(3)
    m = ops.Conv3x3(64, 64, 2)
    x = torch.randn(2, 64, 7, 6)
    assert torch.equal(m(x), nn.Conv2d.forward(m, x))
    assert m(x).shape == (2, 64, 4, 3)
    assert torch.equal(
        ops.conv3x3(x, m.weight, stride=2),
        torch.nn.functional.conv2d(x, m.weight, stride=2, padding=1))
    with pytest.raises(ValueError):
        ops.conv3x3(x, m.weight, stride=3)
    with pytest.raises(ValueError):
        ops.conv3x3(x, m.weight, wgrad=True, stride=2)
