"""ops.linear_cross_entropy off the GPU is the composed expression bit
for bit, and the BERT plumbing around it (BertConfig.fused_mlm_loss,
BertBase.mlm_loss, bert_pretrain_step)."""

import pytest
import torch
import torch.nn.functional as F

import sparkdl.ops as ops
from sparkdl.models.bert import BertBase, BertConfig, bert_pretrain_step

IGNORE = -100


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_is_the_composed_expression(reduction, dtype):
    g = torch.Generator().manual_seed(5)
    leaves = [torch.randn(9, 24, generator=g).to(dtype),
              torch.randn(37, 24, generator=g).to(dtype),
              torch.randn(37, generator=g)]
    labels = torch.randint(0, 37, (9,), generator=g)
    labels[0] = labels[8] = IGNORE
    grad = torch.randn(9, generator=g) if reduction == "none" \
        else torch.tensor(0.75)
    assert not ops.linear_cross_entropy_ok(*leaves, labels)

    def run(fn):
        h, W, bias = (t.clone().requires_grad_(True) for t in leaves)
        loss = fn(h, W, bias)
        loss.backward(grad)
        return loss.detach(), h.grad, W.grad, bias.grad

    got = run(lambda h, W, bias: ops.linear_cross_entropy(
        h, W, bias, labels, IGNORE, reduction))
    want = run(lambda h, W, bias: F.cross_entropy(
        (F.linear(h, W) + bias.to(dtype)).float(), labels,
        ignore_index=IGNORE, reduction=reduction))
    assert got[0].dtype == torch.float32
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError):
        ops.linear_cross_entropy(*leaves, labels, reduction="batchmean")


def _small_bert(fused):
    torch.manual_seed(3)
    return BertBase(BertConfig(vocab_size=100, hidden=64, layers=2, heads=2,
                               ffn=128, max_seq=16, dropout=0.0,
                               fused_mlm_loss=fused))


def test_bert_switch(monkeypatch):
    monkeypatch.delenv("SPARKDL_FUSED_MLM_LOSS", raising=False)
    assert BertConfig().fused_mlm_loss is False         # the default: off
    monkeypatch.setenv("SPARKDL_FUSED_MLM_LOSS", "1")
    assert BertConfig().fused_mlm_loss is True
    assert BertConfig(fused_mlm_loss=False).fused_mlm_loss is False
    monkeypatch.setenv("SPARKDL_FUSED_MLM_LOSS", "0")
    assert BertConfig().fused_mlm_loss is False
    assert BertConfig(fused_mlm_loss=True).fused_mlm_loss is True
    on, off = _small_bert(True), _small_bert(False)
    assert list(on.state_dict()) == list(off.state_dict())


def test_mlm_loss_is_cross_entropy_of_forward_mlm():
    model = _small_bert(True)
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, 100, (2, 16), generator=g)
    positions = torch.tensor([0, 5, 17, 31])
    labels = torch.tensor([7, IGNORE, 99, 0])
    want = F.cross_entropy(model.forward_mlm(ids, positions).float(), labels)
    params = [p for n, p in model.named_parameters() if "token_type" not in n]
    grads = torch.autograd.grad(want, params)
    got = model.mlm_loss(ids, positions, labels)
    assert torch.equal(got, want)
    assert all(torch.equal(a, b)
               for a, b in zip(torch.autograd.grad(got, params), grads))


def test_pretrain_step_follows_the_switch():
    losses = []
    for fused in (False, True):
        model = _small_bert(fused)
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        step = bert_pretrain_step(model, opt, 2, 16, "cpu", False)
        losses.append([step().item() for _ in range(2)])
    assert losses[0] == losses[1]
