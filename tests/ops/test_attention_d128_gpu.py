"""Flash attention for 128-wide heads (attention_d128.hip) against
functional.masked_attention_ref in fp32 on the same bf16 inputs, at the
tolerances of the 64-wide tests for this input scale (inputs / 2: 3e-2 O,
8e-2 dq/dk/dv, 1e-1 packed dqkv; the score variance does not depend on
the head width at this scaling). H=2: bh / H indexes the lengths and
h * 128 is the column offset into the packed buffer."""

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
    qkv = (torch.randn(B, S, 3, H, 128, device="cuda") / 2).bfloat16()
    do = torch.randn(B, S, H * 128, device="cuda").bfloat16()
    return qkv, do


def _close(got, want, tol, name):
    err = (got.float() - want).abs().max().item()
    print("%s max abs err %.4g (tol %g)" % (name, err, tol))
    assert torch.isfinite(got.float()).all(), name
    assert torch.allclose(got.float(), want, atol=tol, rtol=tol), (name, err)


# S=64: one tile; 128: two trips and a skipped causal tile; 192: both
# buffer parities, dK/dV loops starting at tiles 1 and 2
@pytest.mark.parametrize("S", [64, 128, 192])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("with_lens", [False, True])
def test_packed_fwd_bwd_matches_oracle(S, causal, with_lens):
    lens = [min(L, S) for L in LENS] if with_lens else [S] * 2
    B, H = len(lens), 2
    qkv, do = _inputs(160 + S, B, S)
    lt = torch.tensor(lens, dtype=torch.int32, device="cuda") \
        if with_lens else None
    g = qkv.clone().requires_grad_(True)
    o = F_.flash_attention_packed(g, 0.0, seq_lens=lt, causal=causal)
    o.backward(do)

    r = qkv.float().requires_grad_(True)
    q, k, v = r.permute(2, 0, 3, 1, 4).unbind(0)  # [B,H,S,128]
    o_r = F_.masked_attention_ref(q, k, v, lt, causal=causal) \
        .transpose(1, 2).reshape(B, S, H * 128)
    o_r.backward(do.float())

    _close(o, o_r.detach(), 3e-2, "O")
    _close(g.grad, r.grad, 1e-1, "dqkv")
    for b, L in enumerate(lens):
        assert (o[b, L:] == 0).all() and (g.grad[b, L:] == 0).all(), b


def test_unpacked_fwd_bwd_matches_oracle():
    torch.manual_seed(171)
    B, h, S = 3, 2, 128
    lt = torch.tensor([128, 65, 17], dtype=torch.int32, device="cuda")
    q, k, v = ((torch.randn(B, h, S, 128, device="cuda") / 2).bfloat16()
               for _ in range(3))
    assert F_.flash_attention_ok(q)
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


@pytest.mark.parametrize("causal", [False, True])
def test_dropout_with_the_true_mask(causal):
    """V = I_128 (exact in bf16) makes the forward return the dropped,
    scaled P itself, so O != 0 is the keep mask of (seed, bh, q, k): every
    undropped p is positive at this input scale. The same seed with a
    random V must then match an fp32 autograd reference that applies that
    mask times 1/(1-p)."""
    C = ops.ext()
    BH, S, p = 4, 128, 0.25
    torch.manual_seed(172)
    q, k, v, do = ((torch.randn(BH, S, 128, device="cuda") / 2).bfloat16()
                   for _ in range(4))
    seed = torch.tensor([4242], dtype=torch.int64, device="cuda")
    eye = torch.eye(128, device="cuda").bfloat16().expand(BH, S, 128) \
        .contiguous()
    keep = C.attn_fwd(q, k, eye, p, seed, None, causal)[0] != 0
    allowed = torch.ones(S, S, dtype=torch.bool, device="cuda")
    if causal:
        allowed = allowed.tril()
    frac = keep[:, allowed].float().mean().item()
    assert not keep[:, ~allowed].any() and abs(frac - (1 - p)) < 0.02, frac

    def run():
        o, lse = C.attn_fwd(q, k, v, p, seed, None, causal)
        drow = (do.float() * o.float()).sum(-1)
        return (o,) + tuple(C.attn_bwd(q, k, v, do, lse, drow, p, seed,
                                       None, causal))

    got = run()
    assert all(torch.equal(a, b) for a, b in zip(got, run()))

    rs = [t.float().requires_grad_(True) for t in (q, k, v)]
    s = rs[0] @ rs[1].transpose(1, 2) / 128 ** 0.5
    s = s.masked_fill(~allowed, float("-inf"))
    o_r = (torch.softmax(s, -1) * keep / (1 - p)) @ rs[2]
    o_r.backward(do.float())
    _close(got[0], o_r.detach(), 3e-2, "O")
    for g, want, name in zip(got[1:], rs, ("dq", "dk", "dv")):
        _close(g, want.grad, 8e-2, name)


@pytest.mark.parametrize("t", [63, 130])
def test_causal_future_independence_bitwise(t):
    """Positions > t hold other, large values: O[:, :t+1] keeps its bits."""
    C = ops.ext()
    qkv, _ = _inputs(173, 2, 192)
    torch.manual_seed(174)
    other = qkv.clone()
    other[:, t + 1:] = (torch.randn_like(qkv[:, t + 1:].float()) * 50) \
        .bfloat16()
    o0 = C.attn_fwd_packed(qkv, 0.0, None, None, True)[0]
    o1 = C.attn_fwd_packed(other, 0.0, None, None, True)[0]
    assert torch.equal(o1[:, :t + 1], o0[:, :t + 1])
    assert not torch.equal(o1[:, t + 1:], o0[:, t + 1:])


def test_bert_model_path():
    """hidden 256 / 2 heads = 128-wide heads with seq_lens: the kernels
    against the same model sent through the composed fp32 reference. The
    outputs are bf16 LayerNorm outputs, |x| < 8, whose spacing is up to
    2^-5 = 3.1e-2: a difference in the attention output (itself within
    3e-2, then shrunk by the 0.02-std output projection) can move a value
    by one such step, and test_attention_mask_gpu.py's model test asks
    bitwise agreement only between runs of one path. So: 3.2e-2 absolute
    plus 3e-2 relative."""
    from sparkdl.models.bert import BertBase, BertConfig
    torch.manual_seed(3)
    m = BertBase(BertConfig(vocab_size=200, hidden=256, layers=1, heads=2,
                            ffn=256, max_seq=128)).cuda()
    ops.convert_bf16_training(m)
    m.eval()
    attn = m.encoder[0].attn
    assert attn.head_dim == 128
    lens = torch.tensor([128, 70, 5], dtype=torch.int32, device="cuda")
    ids = torch.randint(0, 200, (3, 128), device="cuda")
    with torch.no_grad():
        a = m.encode(ids, seq_lens=lens)
        attn.use_flash = False
        b = m.encode(ids, seq_lens=lens)
        attn.use_flash = True
    assert torch.isfinite(a.float()).all()
    assert torch.allclose(a.float(), b.float(), atol=3.2e-2, rtol=3e-2), \
        (a.float() - b.float()).abs().max().item()

    m.train()
    calls = []
    real = F_.flash_attention_packed
    F_.flash_attention_packed = lambda *x, **kw: (calls.append(1),
                                                  real(*x, **kw))[1]
    try:
        m.encode(ids, seq_lens=lens).float().square().mean().backward()
    finally:
        F_.flash_attention_packed = real
    assert calls, "the 128-wide model path did not take the kernels"
    assert torch.isfinite(attn.qkv.weight.grad.float()).all()
