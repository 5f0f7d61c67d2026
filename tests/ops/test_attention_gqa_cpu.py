"""BertConfig(kv_heads=...) on the composed path, without a GPU."""

import pytest
import torch

from sparkdl.models.bert import BertBase, BertConfig

CFG = dict(vocab_size=100, hidden=64, layers=2, heads=4, ffn=64, max_seq=16,
           dropout=0.0)


def test_gqa_model_equals_multi_head_model_with_repeated_kv_rows():
    """A kv_heads=1 model and the multi-head model whose K and V
    projection rows are its rows repeated for every head of the group
    compute the same function."""
    torch.manual_seed(0)
    gqa = BertBase(BertConfig(kv_heads=1, **CFG)).eval()
    mha = BertBase(BertConfig(**CFG)).eval()
    sd = gqa.state_dict()
    for name, t in list(sd.items()):
        if ".attn.qkv." in name:  # [64 Q | 16 K | 16 V] rows
            q, k, v = t.split([64, 16, 16])
            rep = (4,) + (1,) * (t.dim() - 1)
            sd[name] = torch.cat([q, k.repeat(rep), v.repeat(rep)])
    mha.load_state_dict(sd)
    ids = torch.randint(0, 100, (3, 16))
    lens = torch.tensor([16, 9, 1], dtype=torch.int32)
    with torch.no_grad():
        for kw in ({}, {"seq_lens": lens}):
            a, b = gqa.encode(ids, **kw), mha.encode(ids, **kw)
            assert torch.allclose(a, b, atol=1e-5, rtol=0), kw


@pytest.mark.parametrize("kv_heads", [None, 4])
def test_kv_heads_equal_to_heads_changes_no_parameter(kv_heads):
    shapes = {k: tuple(v.shape) for k, v in
              BertBase(BertConfig(kv_heads=kv_heads, **CFG))
              .state_dict().items()}
    assert shapes["encoder.0.attn.qkv.weight"] == (192, 64)
    assert shapes == {k: tuple(v.shape) for k, v in
                      BertBase(BertConfig(**CFG)).state_dict().items()}


def test_kv_heads_must_divide_heads():
    with pytest.raises(ValueError):
        BertConfig(heads=4, kv_heads=3)
