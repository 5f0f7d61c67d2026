"""Grouped-query flash attention (attention_gqa.hip) against
functional.masked_attention_ref in fp32 autograd on K/V expanded with
repeat_interleave(G), so autograd performs the group sum. Inputs / 2 as
in test_attention_d128_gpu.py; O 3e-2 and dQ 8e-2 as there (the per-head
arithmetic is the same).

dK/dV sum G heads, so their bound is measured, not fixed: each case runs
the composed path a user had before (the 128-wide kernels on expanded
K/V, autograd summing the G bf16 per-head gradients) on the same inputs
and allows the new kernels 1.5x its max abs error, and never more than
G * 8e-2: they round once where it rounds G + 1 times. Measured on an
MI355X (profiles/attn_gqa.log), largest max abs error over the 12 packed
cases of each group size, composed / new: G=1 1.30e-2 / 1.30e-2 (equal in
every case), G=2 2.68e-2 / 1.78e-2, G=3 3.07e-2 / 3.18e-2; per case the
new kernels' error is 0.61x to 1.04x the composed path's."""

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


def _err(got, want):
    assert torch.isfinite(got.float()).all()
    return (got.float() - want).abs().max().item()


def _close(got, want, tol, name):
    err = _err(got, want)
    print("%s max abs err %.4g (tol %g)" % (name, err, tol))
    assert torch.allclose(got.float(), want, atol=tol, rtol=tol), (name, err)


def _heads(t, G):
    """packed [B,S,Hq+2Hkv,128] -> q, k, v [B,Hq,S,128], K/V expanded"""
    hkv = t.shape[2] // (G + 2)
    q, k, v = t.transpose(1, 2).split([G * hkv, hkv, hkv], dim=1)
    return q, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)


# (4,2): two groups (group offsets; lengths by b, not by head); (3,1): an
# odd group, multi-query; (2,2): G = 1. S as in test_attention_d128_gpu.py
@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (3, 1), (2, 2)])
@pytest.mark.parametrize("S", [64, 128, 192])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("with_lens", [False, True])
def test_packed_fwd_bwd_matches_oracle(Hq, Hkv, S, causal, with_lens):
    lens = [min(L, S) for L in LENS] if with_lens else [S] * 2
    B, G = len(lens), Hq // Hkv
    torch.manual_seed(180 + S)
    qkv = (torch.randn(B, S, Hq + 2 * Hkv, 128, device="cuda") / 2).bfloat16()
    do = torch.randn(B, S, Hq * 128, device="cuda").bfloat16()
    lt = torch.tensor(lens, dtype=torch.int32, device="cuda") \
        if with_lens else None

    def run(attend):
        g = qkv.clone().requires_grad_(True)
        o = attend(g)
        o.backward(do)
        return o.detach(), g.grad

    o, dqkv = run(lambda g: F_.flash_attention_gqa_packed(
        g, Hkv, 0.0, seq_lens=lt, causal=causal))
    again = run(lambda g: F_.flash_attention_gqa_packed(
        g, Hkv, 0.0, seq_lens=lt, causal=causal))
    assert torch.equal(o, again[0]) and torch.equal(dqkv, again[1])
    # the composed path: the 128-wide kernels on [B,S,3,Hq,128]
    _, d_comp = run(lambda g: F_.flash_attention_packed(
        torch.stack([t.transpose(1, 2) for t in _heads(g, G)], 2), 0.0,
        seq_lens=lt, causal=causal))

    r = qkv.float().requires_grad_(True)
    o_r = F_.masked_attention_ref(*_heads(r, G), lt, causal=causal) \
        .transpose(1, 2).reshape(B, S, Hq * 128)
    o_r.backward(do.float())

    _close(o, o_r.detach(), 3e-2, "O")
    _close(dqkv[:, :, :Hq], r.grad[:, :, :Hq], 8e-2, "dQ")
    _kv_bound(dqkv[:, :, Hq:], d_comp[:, :, Hq:], r.grad[:, :, Hq:], G)
    for b, L in enumerate(lens):
        assert (o[b, L:] == 0).all() and (dqkv[b, L:] == 0).all(), b


def _kv_bound(new, comp, want, G):
    """The dK/dV bound of the module docstring."""
    e_new, e_comp = _err(new, want), _err(comp, want)
    print("dK/dV max abs err: new %.4g composed %.4g" % (e_new, e_comp))
    assert e_new <= min(1.5 * e_comp, G * 8e-2), (e_new, e_comp)


def test_unpacked_fwd_bwd_matches_oracle():
    torch.manual_seed(181)
    B, S = 3, 128
    lt = torch.tensor([128, 65, 17], dtype=torch.int32, device="cuda")
    q, k, v = ((torch.randn(B, h, S, 128, device="cuda") / 2).bfloat16()
               for h in (4, 2, 2))
    do = torch.randn_like(q)

    def run(dtype, attend):
        ts = [t.clone().to(dtype).requires_grad_(True) for t in (q, k, v)]
        o = attend(*ts)
        o.backward(do.to(dtype))
        return [o.detach()] + [t.grad for t in ts]

    def expanded(fn):
        return lambda q, k, v: fn(q, k.repeat_interleave(2, 1),
                                  v.repeat_interleave(2, 1), lt, causal=True)

    got = run(torch.bfloat16, lambda *t: F_.flash_attention(
        *t, 0.0, seq_lens=lt, causal=True))  # k, v keep their two heads
    comp = run(torch.bfloat16, expanded(
        lambda q, k, v, lt, causal: F_.flash_attention(
            q, k, v, 0.0, seq_lens=lt, causal=causal)))
    want = run(torch.float32, expanded(F_.masked_attention_ref))
    _close(got[0], want[0], 3e-2, "O")
    _close(got[1], want[1], 8e-2, "dq")
    for i in (2, 3):
        _kv_bound(got[i], comp[i], want[i], 2)


@pytest.mark.parametrize("causal", [False, True])
def test_dropout_with_the_true_mask(causal):
    """As test_attention_d128_gpu.py's test of this name: V = I_128 makes
    the forward return the dropped, scaled P, so O != 0 is the keep mask
    of (seed, b*Hq + hq, q, k); the same seed with a random V must match
    an fp32 reference that applies that mask times 1/(1-p)."""
    C = ops.ext()
    B, Hq, Hkv, S, p = 2, 4, 2, 128, 0.25
    torch.manual_seed(182)
    q, do = ((torch.randn(B * Hq, S, 128, device="cuda") / 2).bfloat16()
             for _ in range(2))
    k, v = ((torch.randn(B * Hkv, S, 128, device="cuda") / 2).bfloat16()
            for _ in range(2))
    seed = torch.tensor([4242], dtype=torch.int64, device="cuda")
    eye = torch.eye(128, device="cuda").bfloat16().expand(B * Hkv, S, 128) \
        .contiguous()
    keep = C.attn_gqa_fwd(q, k, eye, p, seed, None, causal, Hq, Hkv)[0] != 0
    allowed = torch.ones(S, S, dtype=torch.bool, device="cuda")
    if causal:
        allowed = allowed.tril()
    frac = keep[:, allowed].float().mean().item()
    assert not keep[:, ~allowed].any() and abs(frac - (1 - p)) < 0.02, frac

    o, lse = C.attn_gqa_fwd(q, k, v, p, seed, None, causal, Hq, Hkv)
    drow = (do.float() * o.float()).sum(-1)
    got = (o,) + tuple(C.attn_gqa_bwd(q, k, v, do, lse, drow, p, seed, None,
                                      causal, Hq, Hkv))
    # composed: the same seed draws the same mask on expanded K/V
    # ([B*Hkv,S,128] -> [B*Hq,S,128]: neighbouring heads share a K/V head)
    G = Hq // Hkv
    ke, ve = (t.repeat_interleave(G, 0) for t in (k, v))
    o_c, lse_c = C.attn_fwd(q, ke, ve, p, seed, None, causal)
    comp = [g.view(B * Hkv, G, S, 128).sum(1) for g in C.attn_bwd(
        q, ke, ve, do, lse_c, (do.float() * o_c.float()).sum(-1), p, seed,
        None, causal)[1:]]

    rs = [t.float().requires_grad_(True) for t in (q, k, v)]
    ke, ve = (t.repeat_interleave(G, 0) for t in rs[1:])
    s = rs[0] @ ke.transpose(1, 2) / 128 ** 0.5
    s = s.masked_fill(~allowed, float("-inf"))
    o_r = (torch.softmax(s, -1) * keep / (1 - p)) @ ve
    o_r.backward(do.float())
    _close(got[0], o_r.detach(), 3e-2, "O")
    _close(got[1], rs[0].grad, 8e-2, "dq")
    for g, c, want in zip(got[2:], comp, rs[1:]):
        _kv_bound(g, c, want.grad, G)


def test_bert_model_path():
    """hidden 256 / 2 heads = 128-wide heads, one shared K/V head, with
    seq_lens: the kernels against the same model on the composed fp32
    reference, at the tolerance of test_attention_d128_gpu.py's
    test_bert_model_path and for its reason (a bf16 LayerNorm output,
    |x| < 8, moves by steps of up to 2^-5)."""
    from sparkdl.models.bert import BertBase, BertConfig
    torch.manual_seed(3)
    m = BertBase(BertConfig(vocab_size=200, hidden=256, layers=1, heads=2,
                            kv_heads=1, ffn=256, max_seq=128)).cuda()
    ops.convert_bf16_training(m)
    m.eval()
    attn = m.encoder[0].attn
    assert attn.qkv.weight.shape == (512, 256)
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
    real = F_.flash_attention_gqa_packed
    F_.flash_attention_gqa_packed = lambda *x, **kw: (calls.append(1),
                                                      real(*x, **kw))[1]
    try:
        m.encode(ids, seq_lens=lens).float().square().mean().backward()
    finally:
        F_.flash_attention_gqa_packed = real
    assert calls, "the kv_heads model path did not take the kernels"
    assert torch.isfinite(attn.qkv.weight.grad.float()).all()
