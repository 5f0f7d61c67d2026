"""ResNet-50 with the fused 1x1-convolution + BatchNorm-statistics
forward (conv1x1_bn_act) against the unfused route.

ResNet50(num_classes=10) on 8 x 3 x 64 x 64, forward and backward, with
torch.backends.cudnn.deterministic = True (without it a step is not
reproducible run to run, see profiles/README.md, round 6). The BatchNorm
weights are drawn in [0.5, 1.5]: with the recipe's zero bn3 weights the
residual branches would not reach the logits at all.

The fused route swaps the convolution implementation and the order in
which the statistics are summed, so its logits are not bitwise those of
SPARKDL_CONV1X1_STATS=0. The yardstick for "what swapping a bf16 1x1
implementation costs" exists on the parent: default route against
SPARKDL_CONV1X1=all. The new difference has to stay within twice that
(twice, because the summation order of the statistics changes too).

Measured on MI355X, relative L2 of the logits against the unfused
route: fused 1.743e-01 and 1.752e-01 in two sessions,
SPARKDL_CONV1X1=all (the yardstick) 1.328e-01 in both.
Both are large, supposedly because the last stage normalises over
8 x 2 x 2 = 32 rows with randomly scaled BatchNorms, which amplifies any
bf16-level difference; the test compares the two, not either with zero.
"""

import pytest
import torch

from tests.ops.test_bn_pool_gpu import PARENT_STATE_DICT_KEYS

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")


def _run(monkeypatch, stats, conv1x1="0"):
    from sparkdl.models.resnet import ResNet50
    from sparkdl.ops import BatchNormAct2d
    monkeypatch.setenv("SPARKDL_CONV1X1_STATS", stats)
    monkeypatch.setenv("SPARKDL_CONV1X1", conv1x1)
    torch.manual_seed(0)
    model = ResNet50(num_classes=10).cuda() \
        .to(memory_format=torch.channels_last).train()
    g = torch.Generator(device="cpu")
    g.manual_seed(1)
    for m in model.modules():
        if isinstance(m, BatchNormAct2d):
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
    x = torch.randn(8, 3, 64, 64, device="cuda") \
        .to(memory_format=torch.channels_last)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = model(x)
    logits.float().square().mean().backward()
    return model, logits.detach().float()


def _rel_l2(a, b):
    return ((a - b).norm() / b.norm()).item()


def test_resnet50_fused_conv_bn(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    m_new, l_new = _run(monkeypatch, "1")
    m_new2, l_new2 = _run(monkeypatch, "1")
    m_old, l_old = _run(monkeypatch, "0")
    _, l_all = _run(monkeypatch, "0", conv1x1="all")

    assert list(m_new.state_dict().keys()) == PARENT_STATE_DICT_KEYS
    assert [n for n, _ in m_new.named_parameters()] \
        == [n for n, _ in m_old.named_parameters()]
    grads = [(n, p.grad) for n, p in m_new.named_parameters()]
    assert len(grads) == 161
    for name, gr in grads:
        assert gr is not None and torch.isfinite(gr).all(), name

    # the new default is reproducible bit for bit
    assert torch.equal(l_new, l_new2)
    for (n, b), (_, b2) in zip(m_new.named_buffers(), m_new2.named_buffers()):
        assert torch.equal(b, b2), n

    d_new = _rel_l2(l_new, l_old)
    d_yard = _rel_l2(l_all, l_old)
    print("relative L2 of the logits against the unfused route: "
          "fused %.3e, SPARKDL_CONV1X1=all %.3e" % (d_new, d_yard))
    assert torch.isfinite(l_new).all()
    assert d_new <= 2 * d_yard
