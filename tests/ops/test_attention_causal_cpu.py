"""Causal attention on the CPU: the fp32 reference against an explicit
fp64 tril-masked softmax, and causality of BertBase through the fallback
path. No GPU needed."""

import pytest
import torch

from sparkdl.ops import functional as F_

S, D = 8, 4


def _fp64(q, k, v, lens):
    """Row n alone: softmax over keys k <= q, k < len; padded rows 0."""
    outs = []
    for n, L in enumerate(lens):
        s = q[n, :L] @ k[n, :L].T / D ** 0.5
        s = s.masked_fill(~torch.ones(L, L, dtype=torch.bool).tril(),
                          float("-inf"))
        o = torch.softmax(s, dim=-1) @ v[n, :L]
        outs.append(torch.cat([o, o.new_zeros(S - L, D)]))
    return torch.stack(outs)


@pytest.mark.parametrize("lens", [None, [8, 5, 1, 0]])
def test_masked_attention_ref_causal_matches_fp64(lens):
    torch.manual_seed(0)
    N = 4
    x32 = [torch.randn(N, S, D, requires_grad=True) for _ in range(3)]
    x64 = [t.detach().double().requires_grad_(True) for t in x32]
    do = torch.randn(N, S, D)
    lt = None if lens is None else torch.tensor(lens, dtype=torch.int32)
    o = F_.masked_attention_ref(*x32, lt, causal=True)
    o.backward(do)
    o64 = _fp64(*x64, lens or [S] * N)
    o64.backward(do.double())
    assert torch.allclose(o.double(), o64, atol=1e-6, rtol=0)
    for a, b in zip(x32, x64):
        assert torch.isfinite(a.grad).all()
        assert torch.allclose(a.grad.double(), b.grad, atol=1e-6, rtol=0)
    if lens is not None:  # causal=False: what it returned before
        dense = F_.masked_attention_ref(*x32, lt, causal=False)
        assert torch.equal(dense, F_.masked_attention_ref(*x32, lt))
        assert not torch.equal(dense, o)


def test_bert_causal_fallback_path():
    from sparkdl.models.bert import BertBase, BertConfig
    torch.manual_seed(0)
    t = 9
    ids = torch.randint(0, 120, (3, 16))
    ids2 = ids.clone()
    ids2[:, t + 1:] = (ids[:, t + 1:] + 1) % 120
    lens = torch.tensor([16, 12, 4], dtype=torch.int32)
    for causal in (True, False):
        m = BertBase(BertConfig(vocab_size=120, hidden=32, layers=2,
                                heads=2, ffn=64, max_seq=16, dropout=0.0,
                                causal=causal)).eval()
        for kw in ({}, {"seq_lens": lens}):  # SDPA, masked_attention_ref
            with torch.no_grad():
                a, b = m.encode(ids, **kw), m.encode(ids2, **kw)
            assert torch.isfinite(a).all()
            assert torch.equal(a[:, :t + 1], b[:, :t + 1]) == causal
