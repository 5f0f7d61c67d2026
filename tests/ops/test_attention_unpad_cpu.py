"""The unpadded (cu_seqlens) interface on the CPU: the reference against
masked_attention_ref on the same sequences right-padded, the gather /
scatter pair, and an fp32 BertBase packed against padded."""

import pytest
import torch

from sparkdl.ops import functional as F_

LENS = [5, 0, 9, 1, 12]
S = 12


@pytest.mark.parametrize("causal", [False, True])
def test_ref_equals_padded_ref(causal):
    torch.manual_seed(0)
    B, H, D = len(LENS), 2, 8
    padded = torch.randn(B, S, 3, H, D)
    packed, cu, index, max_seqlen = F_.unpad_batch(padded, LENS)
    assert max_seqlen == S and cu.tolist() == [0, 5, 5, 14, 15, 27]
    spare = torch.randn(3, 3, H, D)  # T = 30: three spare tokens
    o = F_.unpadded_attention_ref(torch.cat([packed, spare]), cu,
                                  causal=causal)
    q, k, v = padded.permute(2, 0, 3, 1, 4).unbind(0)
    want = F_.masked_attention_ref(q, k, v, torch.tensor(LENS),
                                   causal=causal)
    want = want.transpose(1, 2).reshape(B * S, H * D)[index]
    assert o.shape == (30, H * D) and (o[27:] == 0).all()
    assert torch.allclose(o[:27], want, atol=1e-6, rtol=1e-6)


def test_unpad_pad_round_trip():
    torch.manual_seed(1)
    x = torch.randn(len(LENS), S, 3)
    packed, cu, index, _ = F_.unpad_batch(x, torch.tensor(LENS))
    assert packed.shape == (sum(LENS), 3) and cu.dtype == torch.int32
    back = F_.pad_batch(packed, index, len(LENS), S)
    valid = torch.arange(S) < torch.tensor(LENS).unsqueeze(1)
    assert torch.equal(back[valid], x[valid]) and (back[~valid] == 0).all()
    assert torch.equal(F_.unpad_batch(back, LENS)[0], packed)


@pytest.mark.parametrize("with_types", [False, True])
def test_bert_packed_equals_padded(with_types):
    from sparkdl.models.bert import BertBase, BertConfig
    torch.manual_seed(2)
    m = BertBase(BertConfig(vocab_size=50, hidden=32, layers=2, heads=2,
                            ffn=64, max_seq=16)).eval()
    B = len(LENS)
    ids = torch.randint(0, 50, (B, S))
    types = torch.randint(0, 2, (B, S)) if with_types else None
    ids_p, cu, index, _ = F_.unpad_batch(ids, LENS)
    types_p = types.flatten()[index] if with_types else None
    with torch.no_grad():
        want = m.encode(ids, types, seq_lens=torch.tensor(LENS))
        got = m.encode(ids_p, types_p, cu_seqlens=cu)
    assert got.shape == (sum(LENS), 32)
    assert torch.allclose(got, want.reshape(B * S, 32)[index], atol=1e-5,
                          rtol=1e-5)
    with pytest.raises(ValueError):
        m.encode(ids_p, cu_seqlens=cu, seq_lens=torch.tensor(LENS))
