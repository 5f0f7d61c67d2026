"""conv3x3's weight-gradient route off the GPU: only SPARKDL_CONV3X3=all
turns it on, and on CPU tensors the wgrad argument changes nothing."""

import pytest
import torch

import sparkdl.ops as ops


@pytest.mark.parametrize("env,want", [(None, False), ("0", False),
                                      ("1", False), ("all", True)])
def test_wgrad_route(monkeypatch, env, want):
    if env is None:
        monkeypatch.delenv("SPARKDL_CONV3X3", raising=False)
    else:
        monkeypatch.setenv("SPARKDL_CONV3X3", env)
    assert ops.conv3x3_wgrad_route() is want
    assert ops.conv3x3_wgrad_route(mode="all") is True


def test_forward_route_with_all(monkeypatch):
    monkeypatch.setenv("SPARKDL_CONV3X3", "all")
    assert ops.conv3x3_route(64, 64, 1) is True


def test_cpu_is_conv2d():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 64, 6, 5, generator=g)
    w = torch.randn(64, 64, 3, 3, generator=g)
    dy = torch.randn(2, 64, 6, 5, generator=g)
    grads = []
    for fn in (lambda a, b: ops.conv3x3(a, b, wgrad=True),
               lambda a, b: torch.nn.functional.conv2d(a, b, padding=1)):
        a, b = x.clone().requires_grad_(), w.clone().requires_grad_()
        y = fn(a, b)
        y.backward(dy)
        grads.append((y.detach(), a.grad, b.grad))
    for got, ref in zip(*grads):
        assert torch.equal(got, ref)
