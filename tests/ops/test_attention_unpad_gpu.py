"""Unpadded flash attention (attention_unpad.hip) against
functional.unpadded_attention_ref in fp32 on the same bf16 inputs, at the
tolerances of the 64- and 128-wide tests for this input scale (inputs / 2:
3e-2 O, 1e-1 packed dqkv). H=2: b*H + h enters the dropout hash and h * D
is the column offset into the packed buffer."""

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


# start no multiple of 8 | empty | exact tile | one token | one key into
# a third tile | one key past a tile edge | three tiles (both buffer
# parities, dK/dV loops from tiles 1 and 2) | short last sequence
LENS = [17, 0, 64, 1, 129, 65, 192, 3]
H = 2


def _cu():
    cu = torch.tensor([0] + LENS).cumsum(0)
    assert cu[-1] == 471
    return cu.to("cuda", torch.int32)


def _inputs(seed, T, D, scale=0.5):
    torch.manual_seed(seed)
    qkv = (torch.randn(T, 3, H, D, device="cuda") * scale).bfloat16()
    do = (torch.randn(T, H * D, device="cuda") * 2 * scale).bfloat16()
    return qkv, do


def _close(got, want, tol, name):
    err = (got.float() - want).abs().max().item()
    print("%s max abs err %.4g (tol %g)" % (name, err, tol))
    assert torch.isfinite(got.float()).all(), name
    assert torch.allclose(got.float(), want, atol=tol, rtol=tol), (name, err)


def _run(qkv, do, cu, causal, max_seqlen=192, p=0.0):
    g = qkv.clone().requires_grad_(True)
    o = F_.flash_attention_unpadded(g, cu, max_seqlen, p, causal)
    o.backward(do)
    return o.detach(), g.grad


# T=471: the last tile's staged rows run past the buffer; 512: spare
@pytest.mark.parametrize("T", [471, 512])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_fwd_bwd_matches_oracle(D, causal, T):
    cu = _cu()
    qkv, do = _inputs(200 + D, T, D)
    assert F_.flash_attention_unpadded_ok(qkv)
    o, dqkv = _run(qkv, do, cu, causal)
    r = qkv.float().requires_grad_(True)
    o_r = F_.unpadded_attention_ref(r, cu, causal=causal)
    o_r.backward(do.float())
    _close(o, o_r.detach(), 3e-2, "O")
    _close(dqkv, r.grad, 1e-1, "dqkv")
    assert (o[471:] == 0).all() and (dqkv[471:] == 0).all()


@pytest.mark.parametrize("target", [4, 3])  # the 129-long, the 1-long
@pytest.mark.parametrize("causal", [False, True])
def test_neighbour_independence_bitwise(causal, target):
    """Every token outside the target sequence, spare capacity included,
    holds other, large (finite) values: the target's rows keep their bits."""
    cu = _cu()
    s, e = cu[target].item(), cu[target + 1].item()
    qkv, do = _inputs(210, 512, 64)
    qkv1, do1 = _inputs(211, 512, 64, scale=25.0)
    qkv1[s:e], do1[s:e] = qkv[s:e], do[s:e]
    o0, g0 = _run(qkv, do, cu, causal)
    o1, g1 = _run(qkv1, do1, cu, causal)
    assert torch.isfinite(o1.float()).all() and torch.isfinite(g1.float()).all()
    assert torch.equal(o1[s:e], o0[s:e]) and torch.equal(g1[s:e], g0[s:e])
    assert not torch.equal(o1[:s], o0[:s]) and not torch.equal(g1[:s], g0[:s])


@pytest.mark.parametrize("D", [64, 128])
def test_dropout_draws_the_padded_mask(D):
    """One seed: bitwise repeatable, and the mask of the same sequences
    right-padded to S = max_seqlen = 192 through flash_attention_packed."""
    cu, p, B, S = _cu(), 0.25, len(LENS), 192
    qkv, do = _inputs(220 + D, 471, D)
    lens = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    padded, _, index, _ = F_.unpad_batch(
        torch.zeros(B, S, 3, H, D, device="cuda").bfloat16(), lens)
    seed = F_._attn_seed_tensor(qkv.device)
    start = seed.clone()
    o, g = _run(qkv, do, cu, False, S, p)
    seed.copy_(start)
    o2, g2 = _run(qkv, do, cu, False, S, p)
    assert torch.equal(o, o2) and torch.equal(g, g2)

    seed.copy_(start)
    gp = F_.pad_batch(qkv, index, B, S).requires_grad_(True)
    op = F_.flash_attention_packed(gp, p, seq_lens=lens)
    op.backward(F_.pad_batch(do, index, B, S))
    _close(o, op.detach().float().view(B * S, -1)[index], 3e-2, "O")
    _close(g, gp.grad.float().view(B * S, 3, H, D)[index], 1e-1, "dqkv")


@pytest.mark.parametrize("hidden", [128, 256])  # 2 heads of 64, of 128
def test_bert_model_path(hidden):
    """The kernels against the same model through the composed reference,
    at the tolerance test_attention_d128_gpu.py::test_bert_model_path
    derives for bf16 LayerNorm outputs (one 2^-5 step plus 3e-2 relative)."""
    from sparkdl.models.bert import BertBase, BertConfig
    torch.manual_seed(3)
    m = BertBase(BertConfig(vocab_size=200, hidden=hidden, layers=1, heads=2,
                            ffn=256, max_seq=192)).cuda()
    ops.convert_bf16_training(m)
    m.eval()
    attn = m.encoder[0].attn
    cu = _cu()
    ids = torch.randint(0, 200, (471,), device="cuda")
    with torch.no_grad():
        a = m.encode(ids, cu_seqlens=cu)
        attn.use_flash = False
        b = m.encode(ids, cu_seqlens=cu)
        attn.use_flash = True
    assert torch.isfinite(a.float()).all()
    assert torch.allclose(a.float(), b.float(), atol=3.2e-2, rtol=3e-2), \
        (a.float() - b.float()).abs().max().item()

    m.train()
    calls = []
    real = F_.flash_attention_unpadded
    F_.flash_attention_unpadded = lambda *x, **kw: (calls.append(1),
                                                    real(*x, **kw))[1]
    try:
        m.encode(ids, cu_seqlens=cu).float().square().mean().backward()
    finally:
        F_.flash_attention_unpadded = real
    assert calls, "the unpadded model path did not take the kernels"
    assert torch.isfinite(attn.qkv.weight.grad.float()).all()
