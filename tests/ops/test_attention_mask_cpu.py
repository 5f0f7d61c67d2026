"""Variable-length (right-padded) attention on the CPU: the fp32
reference semantics, mask -> length conversion, and padding invariance
of BertBase through the fallback path. No GPU needed."""

import pytest
import torch

from sparkdl.ops import functional as F_


LENS = [128, 65, 1, 0]
S = 128


def _unpadded(q, k, v):
    s = q @ k.transpose(-1, -2) / q.shape[-1] ** 0.5
    return torch.softmax(s, dim=-1) @ v


def test_masked_attention_ref_semantics():
    torch.manual_seed(0)
    N = len(LENS)
    q = torch.randn(N, S, 64, requires_grad=True)
    k = torch.randn(N, S, 64, requires_grad=True)
    v = torch.randn(N, S, 64, requires_grad=True)
    lens = torch.tensor(LENS, dtype=torch.int32)
    o = F_.masked_attention_ref(q, k, v, lens)
    do = torch.randn_like(o)
    o.backward(do)
    grads = (q.grad, k.grad, v.grad)
    assert torch.isfinite(o).all()
    for g in grads:
        assert torch.isfinite(g).all()

    for n, L in enumerate(LENS):
        # padded rows: exactly zero, output and every gradient
        assert (o[n, L:] == 0).all()
        for g in grads:
            assert (g[n, L:] == 0).all()
        if L == 0:
            continue
        # valid rows: the sequence alone, unpadded — whatever dO holds
        # on the padded rows
        qs = q[n, :L].detach().clone().requires_grad_(True)
        ks = k[n, :L].detach().clone().requires_grad_(True)
        vs = v[n, :L].detach().clone().requires_grad_(True)
        os_ = _unpadded(qs, ks, vs)
        os_.backward(do[n, :L])
        assert torch.allclose(o[n, :L], os_, atol=1e-6, rtol=0)
        for g, gs in zip(grads, (qs.grad, ks.grad, vs.grad)):
            assert torch.allclose(g[n, :L], gs, atol=1e-6, rtol=0)


def test_masked_attention_ref_4d_matches_sdpa_mask():
    """[B,h,S,d] layout with [B] lengths, against SDPA's boolean key
    mask on the valid rows."""
    torch.manual_seed(1)
    B, h = 3, 2
    lens = torch.tensor([128, 65, 1])
    q, k, v = (torch.randn(B, h, S, 64) for _ in range(3))
    o = F_.masked_attention_ref(q, k, v, lens)
    keymask = (torch.arange(S)[None] < lens[:, None])[:, None, None, :]
    ref = torch.nn.functional.scaled_dot_product_attention(
        q, k, v, attn_mask=keymask)
    for b, L in enumerate(lens.tolist()):
        assert torch.allclose(o[b, :, :L], ref[b, :, :L], atol=2e-6)
        assert (o[b, :, L:] == 0).all()


def test_seqlens_from_mask():
    lens = [16, 9, 1, 0]
    mask = (torch.arange(16)[None] < torch.tensor(lens)[:, None])
    for m in (mask, mask.long(), mask.int()):
        got = F_.seqlens_from_mask(m)
        assert got.dtype == torch.int32 and got.shape == (4,)
        assert got.tolist() == lens
    hole = mask.clone()
    hole[0, 5] = False
    with pytest.raises(ValueError):
        F_.seqlens_from_mask(hole)
    left = mask.flip(1)
    with pytest.raises(ValueError):
        F_.seqlens_from_mask(left)
    # validation off: just the sums
    assert F_.seqlens_from_mask(left, validate=False).tolist() == lens


def test_bert_padding_invariance_cpu():
    from sparkdl.models.bert import BertBase, BertConfig
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size=120, hidden=32, layers=2, heads=2,
                     ffn=64, max_seq=16, dropout=0.0)
    m = BertBase(cfg)
    ids = torch.randint(0, 120, (3, 16))
    lens = [16, 9, 1]
    seq_lens = torch.tensor(lens, dtype=torch.int32)
    mask = (torch.arange(16)[None] < seq_lens[:, None]).long()

    by_lens = m(ids, seq_lens=seq_lens)
    by_mask = m(ids, attention_mask=mask)
    assert torch.equal(by_lens, by_mask)
    assert torch.isfinite(by_lens).all()
    for b, L in enumerate(lens):
        alone = m(ids[b:b + 1, :L])
        assert torch.allclose(by_lens[b, :L], alone[0], atol=1e-5), \
            (b, (by_lens[b, :L] - alone[0]).abs().max())

    # masked-position head agrees with the full head at valid positions
    positions = torch.tensor([0, 5, 16 + 3, 16 + 8, 32])
    mlm = m.forward_mlm(ids, positions, attention_mask=mask)
    full = by_mask.reshape(-1, 120)[positions]
    assert torch.allclose(mlm, full, atol=1e-5)

    with pytest.raises(ValueError):
        m(ids, attention_mask=mask, seq_lens=seq_lens)
    with pytest.raises(ValueError):
        m.forward_mlm(ids, positions, attention_mask=mask,
                      seq_lens=seq_lens)

    mlm.sum().backward()
    for name, p in m.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all(), name
    assert m.embeddings.word.weight.grad is not None
    assert m.encoder[0].attn.qkv.weight.grad is not None


def test_pretrain_step_draws_valid_positions_only():
    from sparkdl.models.bert import (BertBase, BertConfig,
                                     bert_pretrain_step)
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size=120, hidden=32, layers=1, heads=2,
                     ffn=64, max_seq=16, dropout=0.0)
    m = BertBase(cfg)
    seen = {}
    orig = m.forward_mlm

    def spy(ids, positions, **kw):
        seen["positions"], seen["kw"] = positions, kw
        return orig(ids, positions, **kw)

    m.forward_mlm = spy
    opt = torch.optim.SGD(m.parameters(), lr=0.01)
    lens = [16, 9, 4, 0]
    step = bert_pretrain_step(m, opt, 4, 16, "cpu", False, mask_frac=0.5,
                              seq_lens=lens)
    loss = step()
    assert torch.isfinite(loss)
    pos = seen["positions"]
    assert pos.numel() > 0
    row, col = pos // 16, pos % 16
    assert (col < torch.tensor(lens)[row]).all()
    assert seen["kw"]["seq_lens"].tolist() == lens
