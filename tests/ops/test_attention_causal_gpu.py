"""Causal flash attention (k <= q, and k < len with seq_lens) against
functional.masked_attention_ref(causal=True) in fp32 on the same bf16
inputs; tolerances of test_attention_mask_gpu.py (3e-2 O, 8e-2 dq/dk/dv,
1e-1 packed dqkv; inputs / 2). H=2: bh / H indexes lengths."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sparkdl.ops as ops
    from sparkdl.ops import functional as F_


@pytest.fixture(autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")


# full | one key into a tile | tile edge | across a wave edge | one | empty
LENS = [10 ** 6, 129, 128, 65, 17, 1, 0]


def _inputs(seed, B, S, H=2):
    torch.manual_seed(seed)
    qkv = (torch.randn(B, S, 3, H, 64, device="cuda") / 2).bfloat16()
    do = torch.randn(B, S, H * 64, device="cuda").bfloat16()
    return qkv, do


def _close(got, want, tol, name):
    err = (got.float() - want).abs().max().item()
    print("%s max abs err %.4g (tol %g)" % (name, err, tol))
    assert torch.isfinite(got.float()).all(), name
    assert torch.allclose(got.float(), want, atol=tol, rtol=tol), (name, err)


# S=64: the diagonal tile alone; 128: a skipped tile and two trips; 192:
# both buffer parities, dK/dV loops starting at tiles 1 and 2
@pytest.mark.parametrize("S", [64, 128, 192])
@pytest.mark.parametrize("with_lens", [False, True])
def test_packed_fwd_bwd_matches_oracle(S, with_lens):
    lens = [min(L, S) for L in LENS] if with_lens else [S] * 2
    B, H = len(lens), 2
    qkv, do = _inputs(60 + S, B, S)
    lt = torch.tensor(lens, dtype=torch.int32, device="cuda") \
        if with_lens else None
    g = qkv.clone().requires_grad_(True)
    o = F_.flash_attention_packed(g, 0.0, seq_lens=lt, causal=True)
    o.backward(do)

    r = qkv.float().requires_grad_(True)
    q, k, v = r.permute(2, 0, 3, 1, 4).unbind(0)  # [B,H,S,64]
    o_r = F_.masked_attention_ref(q, k, v, lt, causal=True) \
        .transpose(1, 2).reshape(B, S, H * 64)
    o_r.backward(do.float())

    _close(o, o_r.detach(), 3e-2, "O")
    _close(g.grad, r.grad, 1e-1, "dqkv")
    for b, L in enumerate(lens):
        assert (o[b, L:] == 0).all() and (g.grad[b, L:] == 0).all(), b


def test_unpacked_fwd_bwd_matches_oracle():
    torch.manual_seed(71)
    B, h, S = 3, 2, 128
    lt = torch.tensor([128, 65, 17], dtype=torch.int32, device="cuda")
    q, k, v = ((torch.randn(B, h, S, 64, device="cuda") / 2).bfloat16()
               for _ in range(3))
    gs = [t.clone().requires_grad_(True) for t in (q, k, v)]
    o = F_.flash_attention(*gs, 0.0, seq_lens=lt, causal=True)
    do = torch.randn_like(o)
    o.backward(do)
    rs = [t.float().requires_grad_(True) for t in (q, k, v)]
    o_r = F_.masked_attention_ref(*rs, lt, causal=True)
    o_r.backward(do.float())
    _close(o, o_r.detach(), 3e-2, "O")
    for got, want, name in zip(gs, rs, ("dq", "dk", "dv")):
        _close(got.grad, want.grad, 8e-2, name)


@pytest.mark.parametrize("t", [0, 63, 64, 130])
def test_future_independence_bitwise(t):
    """Positions > t hold other, large values: O[:, :t+1] keeps its bits,
    without dropout and with it (fixed seed: same bits on every run)."""
    C = ops.ext()
    S, p = 192, 0.25
    qkv, do = _inputs(73, 2, S)
    torch.manual_seed(74)
    other = qkv.clone()
    other[:, t + 1:] = (torch.randn_like(qkv[:, t + 1:].float()) * 50) \
        .bfloat16()
    seed = torch.tensor([4242], dtype=torch.int64, device="cuda")

    def run(x, p, seed):
        o, lse = C.attn_fwd_packed(x, p, seed, None, True)
        drow = (do.float() * o.float()).view(2, S, 2, 64).sum(-1) \
            .transpose(1, 2).reshape(4, S).contiguous()
        return o, C.attn_bwd_packed(x, do, lse, drow, p, seed, None, True)

    o0, g0 = run(qkv, 0.0, None)
    assert torch.equal(run(other, 0.0, None)[0][:, :t + 1], o0[:, :t + 1])
    o1, g1 = run(qkv, p, seed)
    assert torch.equal(run(other, p, seed)[0][:, :t + 1], o1[:, :t + 1])
    o2, g2 = run(qkv, p, seed)
    assert torch.equal(o1, o2) and torch.equal(g1, g2)
    assert not torch.equal(o1, o0) and not torch.equal(g1, g0)


def test_dense_path_is_neutral():
    """causal=False passed explicitly is, bitwise, the call without it."""
    C = ops.ext()
    qkv, do = _inputs(75, 2, 128)
    B, S, _, H, _ = qkv.shape
    q, k, v = (qkv[:, :, i].transpose(1, 2).reshape(B * H, S, 64)
               .contiguous() for i in range(3))
    dou = do.view(B, S, H, 64).transpose(1, 2).reshape(B * H, S, 64) \
        .contiguous()
    for fwd, bwd, fn, x, d in (
            (C.attn_fwd_packed, C.attn_bwd_packed, F_._FlashAttnPackedFn,
             (qkv,), do),
            (C.attn_fwd, C.attn_bwd, F_._FlashAttnFn, (q, k, v), dou)):
        o0, lse0 = fwd(*x, 0.0, None)
        ou = o0 if fwd is C.attn_fwd else o0.view(B, S, H, 64) \
            .transpose(1, 2).reshape(B * H, S, 64)
        drow = (dou.float() * ou.float()).sum(-1)
        g0 = bwd(*x, d, lse0, drow, 0.0, None)
        o1, lse1 = fwd(*x, 0.0, None, None, False)
        g1 = bwd(*x, d, lse0, drow, 0.0, None, None, False)
        assert torch.equal(o1, o0) and torch.equal(lse1, lse0)
        g0, g1 = ((g,) if torch.is_tensor(g) else g for g in (g0, g1))
        assert all(torch.equal(a, b) for a, b in zip(g1, g0))
        for extra in ((), (None, False)):
            xs = [t.clone().requires_grad_(True) for t in x]
            o2 = fn.apply(*xs, 0.0, *extra)
            o2.backward(d)
            assert torch.equal(o2, o0)
            assert all(torch.equal(t.grad, b) for t, b in zip(xs, g0))


def test_bert_causal_model():
    from sparkdl.models.bert import BertBase, BertConfig
    S, t = 128, 70
    ids = torch.randint(0, 200, (2, S), device="cuda",
                        generator=torch.Generator("cuda").manual_seed(5))
    ids2 = ids.clone()
    ids2[:, t + 1:] = (ids[:, t + 1:] + 1) % 200
    models = {}
    for causal in (True, False):
        torch.manual_seed(3)
        m = BertBase(BertConfig(vocab_size=200, hidden=128, layers=1,
                                heads=2, ffn=256, max_seq=128,
                                causal=causal)).cuda()
        ops.convert_bf16_training(m)
        models[causal] = m.eval()
        with torch.no_grad():
            a, b = m.encode(ids), m.encode(ids2)
        assert torch.isfinite(a.float()).all()
        assert torch.equal(a[:, :t + 1], b[:, :t + 1]) == causal

    m = models[True].train()  # next-token LM through forward_mlm
    positions = (torch.arange(2, device="cuda")[:, None] * S +
                 torch.arange(S - 1, device="cuda")[None]).flatten()
    logits = m.forward_mlm(ids, positions)
    loss = torch.nn.functional.cross_entropy(
        logits.float(), ids[:, 1:].flatten())
    loss.backward()
    assert torch.isfinite(loss)
    assert m.encoder[0].attn.qkv.weight.grad is not None
    assert all(torch.isfinite(prm.grad.float()).all()
               for prm in m.parameters() if prm.grad is not None)
