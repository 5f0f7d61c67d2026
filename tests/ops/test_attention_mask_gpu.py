"""GPU numerics for variable-length (right-padded) batches through the
hand-written flash attention: key-padding by per-row length, zero
padded rows, tile skipping, neutrality of the fixed-length path, graph
capture, the BERT model surface and argument validation.

Oracle: functional.masked_attention_ref in fp32 on the same bf16-rounded
inputs; tolerances are the ones of test_attention_gpu.py (3e-2 forward,
8e-2 dq/dk/dv, 1e-1 packed dqkv; gradient inputs scaled /2).

S=128 is the smallest shape with both a skipped and a partial 64-wide
tile; H=2 the smallest that exercises the bh / H length lookup."""

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


# full row | one key in the tail tile | exact tile boundary (second tile
# skipped) | crosses the 16-row wave boundary | single key | empty row
LENS = [128, 65, 64, 17, 1, 0]


def _lens(vals):
    return torch.tensor(vals, dtype=torch.int32, device="cuda")


def _packed_oracle(qkv, lens, do):
    """fp32 reference O [B,S,H*64] and dqkv for packed [B,S,3,H,64]."""
    B, S, _, H, _ = qkv.shape
    qkv_r = qkv.float().requires_grad_(True)
    q, k, v = qkv_r.permute(2, 0, 3, 1, 4).unbind(0)  # [B,H,S,64]
    o = F_.masked_attention_ref(q, k, v, lens)
    o = o.transpose(1, 2).reshape(B, S, H * 64)
    o.backward(do.float())
    return o.detach(), qkv_r.grad


def _packed_inputs(seed, B=6, H=2, S=128, scale=0.5):
    torch.manual_seed(seed)
    qkv = (torch.randn(B, S, 3, H, 64, device="cuda") * scale).bfloat16()
    do = torch.randn(B, S, H * 64, device="cuda").bfloat16()
    return qkv, do


def _close(got, want, tol, name):
    err = (got.float() - want).abs().max().item()
    print("%s max abs err %.4g (tol %g)" % (name, err, tol))
    assert torch.allclose(got.float(), want, atol=tol, rtol=tol), \
        (name, err)


def test_packed_fwd_bwd_matches_oracle():
    qkv, do = _packed_inputs(41)
    lens = _lens(LENS)
    qkv_g = qkv.clone().requires_grad_(True)
    o = F_.flash_attention_packed(qkv_g, 0.0, seq_lens=lens)
    o.backward(do)
    o_r, dqkv_r = _packed_oracle(qkv, lens, do)
    _close(o, o_r, 3e-2, "O")
    _close(qkv_g.grad, dqkv_r, 1e-1, "dqkv")
    assert torch.isfinite(o.float()).all()
    assert torch.isfinite(qkv_g.grad.float()).all()
    for b, L in enumerate(LENS):
        assert (o[b, L:] == 0).all(), b
        # dQ rows, and the dK / dV parts, of every padded position
        assert (qkv_g.grad[b, L:] == 0).all(), b


@pytest.mark.parametrize("S,lens", [(128, LENS), (256, [256, 129, 3])])
def test_unpacked_fwd_bwd_matches_oracle(S, lens):
    torch.manual_seed(50 + S)
    BH = len(lens)
    q, k, v = ((torch.randn(BH, S, 64, device="cuda") / 2).bfloat16()
               for _ in range(3))
    lt = _lens(lens)
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = F_._FlashAttnFn.apply(qg, kg, vg, 0.0, lt)
    do = torch.randn_like(o)
    o.backward(do)

    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    o_r = F_.masked_attention_ref(qr, kr, vr, lt)
    o_r.backward(do.float())

    _close(o, o_r.detach(), 3e-2, "O")
    for got, want, name in ((qg.grad, qr.grad, "dq"),
                            (kg.grad, kr.grad, "dk"),
                            (vg.grad, vr.grad, "dv")):
        _close(got, want, 8e-2, name)
        for b, L in enumerate(lens):
            assert (got[b, L:] == 0).all(), (name, b)
    for b, L in enumerate(lens):
        assert (o[b, L:] == 0).all(), b


def test_bh_h_wrapper_expands_lengths():
    """[B,h,S,d] wrapper: [B] lengths reach every head of the row."""
    torch.manual_seed(57)
    B, h, S = 3, 2, 128
    lens = [128, 65, 0]
    q, k, v = ((torch.randn(B, h, S, 64, device="cuda") / 2).bfloat16()
               for _ in range(3))
    o = F_.flash_attention(q, k, v, 0.0, seq_lens=_lens(lens))
    o_r = F_.masked_attention_ref(q.float(), k.float(), v.float(),
                                  _lens(lens))
    _close(o, o_r, 3e-2, "O")
    for b, L in enumerate(lens):
        assert (o[b, :, L:] == 0).all()


def test_fixed_length_path_is_neutral():
    """seq_lens=None and seq_lens=full(S) both reproduce, bitwise, the
    calls made without the argument."""
    C = ops.ext()
    qkv, do = _packed_inputs(43, B=3)
    B, S, _, H, _ = qkv.shape
    full_b = _lens([S] * B)

    o0, lse0 = C.attn_fwd_packed(qkv, 0.0, None)
    drow = (do.float() * o0.float()).view(B, S, H, 64).sum(-1) \
        .transpose(1, 2).reshape(B * H, S).contiguous()
    g0 = C.attn_bwd_packed(qkv, do, lse0, drow, 0.0, None)
    for sl in (None, full_b):
        o1, lse1 = C.attn_fwd_packed(qkv, 0.0, None, sl)
        g1 = C.attn_bwd_packed(qkv, do, lse0, drow, 0.0, None, sl)
        assert torch.equal(o1, o0) and torch.equal(lse1, lse0)
        assert torch.equal(g1, g0)
        qkv_g = qkv.clone().requires_grad_(True)
        o2 = F_.flash_attention_packed(qkv_g, 0.0, seq_lens=sl)
        o2.backward(do)
        assert torch.equal(o2, o0) and torch.equal(qkv_g.grad, g0)

    # plain [BH,S,64] entry points, five- and eight-argument calls
    q, k, v = (qkv[:, :, i].transpose(1, 2).reshape(B * H, S, 64)
               .contiguous() for i in range(3))
    dou = torch.randn_like(q)
    full_bh = _lens([S] * (B * H))
    ou, lseu = C.attn_fwd(q, k, v, 0.0, None)
    drow_u = (dou.float() * ou.float()).sum(-1)
    gu = C.attn_bwd(q, k, v, dou, lseu, drow_u, 0.0, None)
    for sl in (None, full_bh):
        o1, lse1 = C.attn_fwd(q, k, v, 0.0, None, sl)
        g1 = C.attn_bwd(q, k, v, dou, lseu, drow_u, 0.0, None, sl)
        assert torch.equal(o1, ou) and torch.equal(lse1, lseu)
        for a, b_ in zip(g1, gu):
            assert torch.equal(a, b_)
        qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
        o2 = F_._FlashAttnFn.apply(qg, kg, vg, 0.0, sl)
        o2.backward(dou)
        assert torch.equal(o2, ou)
        for a, b_ in zip((qg.grad, kg.grad, vg.grad), gu):
            assert torch.equal(a, b_)


def test_results_independent_of_padding_content():
    lens = _lens(LENS)
    qkv_a, do_a = _packed_inputs(45)
    B, S = qkv_a.shape[:2]
    torch.manual_seed(46)
    pad = (torch.arange(S, device="cuda")[None] >= lens[:, None])  # [B,S]
    qkv_b = torch.where(pad[:, :, None, None, None],
                        (torch.randn_like(qkv_a.float()) * 50).bfloat16(),
                        qkv_a)
    do_b = torch.where(pad[:, :, None],
                       (torch.randn_like(do_a.float()) * 50).bfloat16(),
                       do_a)
    outs = []
    for qkv, do in ((qkv_a, do_a), (qkv_b, do_b)):
        g = qkv.clone().requires_grad_(True)
        o = F_.flash_attention_packed(g, 0.0, seq_lens=lens)
        o.backward(do)
        outs.append((o.detach(), g.grad))
    (oa, ga), (ob, gb) = outs
    assert not torch.equal(qkv_a, qkv_b)
    # padded O rows are zero in both, so all of O is equal as well
    assert torch.equal(oa, ob)
    assert torch.equal(ga, gb)


def test_dropout_with_mask():
    C = ops.ext()
    p = 0.25
    qkv, do = _packed_inputs(47)
    B, S, _, H, _ = qkv.shape
    lens = _lens(LENS)
    seed = torch.tensor([4242], dtype=torch.int64, device="cuda")

    def run(sl):
        o, lse = C.attn_fwd_packed(qkv, p, seed, sl)
        drow = (do.float() * o.float()).view(B, S, H, 64).sum(-1) \
            .transpose(1, 2).reshape(B * H, S).contiguous()
        return o, C.attn_bwd_packed(qkv, do, lse, drow, p, seed, sl)

    o1, g1 = run(lens)
    o2, g2 = run(lens)
    assert torch.equal(o1, o2) and torch.equal(g1, g2)
    assert torch.isfinite(o1.float()).all()
    assert torch.isfinite(g1.float()).all()
    for b, L in enumerate(LENS):
        assert (o1[b, L:] == 0).all() and (g1[b, L:] == 0).all(), b
    # dropout really is on
    o_nodrop, _ = C.attn_fwd_packed(qkv, 0.0, None, lens)
    assert not torch.equal(o1, o_nodrop)
    # same keep decisions as the unmasked call: rows of full length are
    # bitwise what the fixed-length kernels give with this seed
    o_un, g_un = run(None)
    for b, L in enumerate(LENS):
        if L == S:
            assert torch.equal(o1[b], o_un[b])
            assert torch.equal(g1[b], g_un[b])


def test_graph_capture_reads_lengths_on_device():
    qkv, do = _packed_inputs(49)
    lens = _lens(LENS)
    new_lens = [3, 128, 0, 64, 100, 65]
    qkv_g = qkv.clone().requires_grad_(True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):  # warm up outside the capture
            qkv_g.grad = None
            F_.flash_attention_packed(qkv_g, 0.0, seq_lens=lens) \
                .backward(do)
    torch.cuda.current_stream().wait_stream(side)
    qkv_g.grad = None

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_static = F_.flash_attention_packed(qkv_g, 0.0, seq_lens=lens)
        o_static.backward(do)
    g_static = qkv_g.grad

    lens.copy_(_lens(new_lens))
    graph.replay()
    torch.cuda.synchronize()

    qkv_e = qkv.clone().requires_grad_(True)
    o_e = F_.flash_attention_packed(qkv_e, 0.0, seq_lens=_lens(new_lens))
    o_e.backward(do)
    assert torch.equal(o_static, o_e)
    assert torch.equal(g_static, qkv_e.grad)
    for b, L in enumerate(new_lens):
        assert (o_static[b, L:] == 0).all()


def test_bert_padding_invariance_and_training():
    from sparkdl.models.bert import BertBase, BertConfig
    torch.manual_seed(3)
    cfg = BertConfig(vocab_size=200, hidden=128, layers=1, heads=2,
                     ffn=256, max_seq=128)
    m = BertBase(cfg).cuda()
    ops.convert_bf16_training(m)
    m.eval()
    lens = [128, 70, 5]
    S = 128
    seq_lens = _lens(lens)
    valid = torch.arange(S, device="cuda")[None] < seq_lens[:, None]
    ids = torch.randint(0, 200, (3, S), device="cuda")
    other = torch.randint(0, 200, (3, S), device="cuda")
    ids2 = torch.where(valid, ids, other)
    assert not torch.equal(ids, ids2)
    with torch.no_grad():
        a = m(ids, seq_lens=seq_lens)
        b = m(ids2, seq_lens=seq_lens)
        c = m(ids, attention_mask=valid)
    assert torch.isfinite(a.float()).all()
    assert torch.equal(a[valid], b[valid])
    assert torch.equal(a, c)
    with pytest.raises(ValueError):
        m(ids, attention_mask=valid, seq_lens=seq_lens)

    m.train()
    positions = valid.flatten().nonzero().flatten()[::3]
    labels = ids.flatten()[positions]
    logits = m.forward_mlm(ids, positions, attention_mask=valid.long())
    loss = torch.nn.functional.cross_entropy(logits.float(), labels)
    loss.backward()
    assert torch.isfinite(loss)
    assert m.encoder[0].attn.qkv.weight.grad is not None
    for name, prm in m.named_parameters():
        if prm.grad is not None:
            assert torch.isfinite(prm.grad.float()).all(), name


def test_malformed_calls_raise_before_launch():
    """Every call passes seqlens explicitly (a build without the
    argument rejects them at argument matching)."""
    C = ops.ext()
    BH, S = 2, 128
    q, k, v, do = (torch.randn(BH, S, 64, device="cuda").bfloat16()
                   for _ in range(4))
    lse = torch.zeros(BH, S, device="cuda")
    drow = torch.zeros(BH, S, device="cuda")
    ok = _lens([S, 65])
    qkv = torch.randn(BH, S, 3, 2, 64, device="cuda").bfloat16()

    with pytest.raises(RuntimeError):  # int64 lengths
        C.attn_fwd(q, k, v, 0.0, None, ok.long())
    with pytest.raises(RuntimeError):  # wrong numel (unpacked: BH)
        C.attn_fwd(q, k, v, 0.0, None, _lens([S]))
    with pytest.raises(RuntimeError):  # wrong numel (packed: B, not B*H)
        C.attn_fwd_packed(qkv, 0.0, None, _lens([S] * 4))
    with pytest.raises(RuntimeError):  # lengths on the host
        C.attn_fwd(q, k, v, 0.0, None, ok.cpu())
    with pytest.raises(RuntimeError):
        C.attn_bwd(q, k, v, do, lse, drow, 0.0, None, ok.cpu())
    with pytest.raises(RuntimeError):
        C.attn_bwd_packed(qkv, torch.zeros(BH, S, 128, device="cuda")
                          .bfloat16(), torch.zeros(4, S, device="cuda"),
                          torch.zeros(4, S, device="cuda"), 0.0, None,
                          ok.long())

    # attn_bwd mirrors the forward's shape checks
    q96, k96, v96, do96 = (t[:, :96].contiguous() for t in (q, k, v, do))
    with pytest.raises(RuntimeError):  # S % 64 != 0
        C.attn_bwd(q96, k96, v96, do96, lse[:, :96].contiguous(),
                   drow[:, :96].contiguous(), 0.0, None, ok)
    with pytest.raises(RuntimeError):  # K shorter than Q
        C.attn_bwd(q, k[:, :64].contiguous(), v, do, lse, drow, 0.0,
                   None, ok)
    do_nc = torch.randn(BH, S, 128, device="cuda").bfloat16()[:, :, ::2]
    assert do_nc.shape == do.shape and not do_nc.is_contiguous()
    with pytest.raises(RuntimeError):  # non-contiguous dO
        C.attn_bwd(q, k, v, do_nc, lse, drow, 0.0, None, ok)
    with pytest.raises(RuntimeError):  # LSE of the wrong shape
        C.attn_bwd(q, k, v, do, lse[:, :64].contiguous(), drow, 0.0,
                   None, ok)
