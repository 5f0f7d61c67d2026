"""The dropout + residual add + LayerNorm kernels (dropout_add_ln_fwd /
_bwd in csrc/layernorm.hip) and everything above them, on the GPU.

The definition is bitwise, so every comparison is torch.equal. The mask
comes from this suite's own hash (test_dropout_ln_cpu.keep_mask, numpy),
not from the repository's; the reference is built from it with torch
ops on the device:

    scale = 1 / (1 - p)                      in fp32
    d     = where(keep, bf16(sub * scale), +0)
    h_ref = bf16(res + d)

and y, mean, rstd, d_res, dgamma, dbeta are those of the plain LayerNorm
kernels on h_ref. Shapes: _rowwise.LN_FWD_SHAPES / LN_BWD_SHAPES, where
each kernel changes its path (see test_rowwise_exact_gpu.py).
"""

import pytest
import torch

from . import _exact as ex
from . import _rowwise as rw
from .test_dropout_ln_cpu import keep_mask

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sparkdl.ops as ops
    from sparkdl.ops import functional as F_

DEV = "cuda"
FWD_SEEDS = [12345, 2 ** 32 + 5]


@pytest.fixture(autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")


def _scale(p):
    """1 / (1 - p) evaluated in fp32, as a Python float."""
    one = torch.tensor(1.0, dtype=torch.float32)
    return (one / (one - torch.tensor(p, dtype=torch.float32))).item()


def _seed_tensor(seed):
    return torch.tensor([seed], dtype=torch.int64, device=DEV)


def _h_ref(sub, res, keep, p):
    d = torch.where(keep, (sub.float() * _scale(p)).bfloat16(),
                    torch.zeros((), dtype=torch.bfloat16, device=sub.device))
    return (res.float() + d.float()).bfloat16()


def _d_sub_ref(d_res, keep, p):
    return torch.where(keep, (d_res.float() * _scale(p)).bfloat16(),
                       torch.zeros((), dtype=torch.bfloat16,
                                   device=d_res.device))


def _same(got, want, what):
    """torch.equal, and the same bit patterns (a dropped element is +0)."""
    ex.assert_equal(got, want, what)
    if got.dtype == torch.bfloat16:
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
            what + ": differs in the sign of a zero"


def _counter():
    """The per-device seed counter: after a training call with p > 0 it
    is the seed that call used."""
    device = torch.empty(0, device=DEV).device
    return int(F_._attn_seed_tensor(device).item())


# ---------------------------------------------------------------------------
# 1: forward binding
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols", rw.LN_FWD_SHAPES)
def test_fwd_binding(rows, cols):
    C = ops.ext()
    res, gamma, beta, _ = rw.ln_fwd_operands(rows, cols, DEV)
    g = ex.case_generator("dropout_ln_fwd", rows, cols)
    sub = torch.randn(rows, cols, generator=g).bfloat16().to(DEV)
    for p in (0.0, 0.1, 0.5):
        for seed in FWD_SEEDS:
            what = "dropout_add_ln_fwd %dx%d p=%g seed=%d " % (rows, cols, p,
                                                               seed)
            keep = keep_mask(seed, rows, cols, p, DEV)
            h_ref = _h_ref(sub, res, keep, p)
            y_ref, mean_ref, rstd_ref = C.layernorm_fwd(h_ref, gamma, beta,
                                                        rw.LN_EPS)
            y, h, mean, rstd = C.dropout_add_ln_fwd(
                sub, res, gamma, beta, rw.LN_EPS, p, _seed_tensor(seed))
            assert mean.shape == rstd.shape == (rows,)
            _same(h, h_ref, what + "h")
            _same(mean, mean_ref, what + "mean")
            _same(rstd, rstd_ref, what + "rstd")
            _same(y, y_ref, what + "y")
    # p = 0 needs no seed, and the truncated seed is seed 5
    y0, h0, _, _ = C.dropout_add_ln_fwd(sub, res, gamma, beta, rw.LN_EPS,
                                        0.0, None)
    _same(h0, (res.float() + sub.float()).bfloat16(), "p=0 h")
    _same(C.dropout_add_ln_fwd(sub, res, gamma, beta, rw.LN_EPS, 0.5,
                               _seed_tensor(5))[1], h, "seed 2^32+5 vs 5")


# ---------------------------------------------------------------------------
# 2: backward binding
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols", list(rw.LN_BWD_SHAPES))
def test_bwd_binding(rows, cols):
    C = ops.ext()
    cpu = rw.ln_bwd_exact_operands(rows, cols)
    _, dg64, db64, _ = rw.ln_bwd_ref(*cpu)
    h, dy, gamma, mean, rstd = [t.to(DEV) for t in cpu]
    dx_plain = C.layernorm_bwd(h, dy, gamma, mean, rstd)[0]
    for p, seed in ((0.1, 12345), (0.5, 2 ** 32 + 5), (0.1, 2 ** 31 - 1)):
        what = "dropout_add_ln_bwd %dx%d p=%g seed=%d " % (rows, cols, p,
                                                           seed)
        d_sub, d_res, dgamma, dbeta = C.dropout_add_ln_bwd(
            h, dy, gamma, mean, rstd, p, _seed_tensor(seed))
        ex.assert_equal(dbeta.cpu(), db64.float(), what + "dbeta")
        ex.assert_equal(dgamma.cpu(), dg64.float(), what + "dgamma")
        _same(d_res, dx_plain, what + "d_res")
        keep = keep_mask(seed, rows, cols, p, DEV)
        _same(d_sub, _d_sub_ref(d_res, keep, p), what + "d_sub")
        assert d_sub.data_ptr() != d_res.data_ptr()
    # p = 0: one tensor for both gradients
    d_sub, d_res, dgamma, dbeta = C.dropout_add_ln_bwd(
        h, dy, gamma, mean, rstd, 0.0, None)
    assert d_sub.data_ptr() == d_res.data_ptr()
    assert d_sub.untyped_storage().data_ptr() \
        == d_res.untyped_storage().data_ptr()
    _same(d_res, dx_plain, "p=0 d_res")
    ex.assert_equal(dbeta.cpu(), db64.float(), "p=0 dbeta")
    ex.assert_equal(dgamma.cpu(), dg64.float(), "p=0 dgamma")


# ---------------------------------------------------------------------------
# 3: autograd
# ---------------------------------------------------------------------------

def _random_case(rows, cols, tag):
    g = ex.case_generator("dropout_ln_" + tag, rows, cols)
    x = torch.randn(rows, cols, generator=g).bfloat16().to(DEV)
    res = torch.randn(rows, cols, generator=g).bfloat16().to(DEV)
    gamma = (torch.rand(cols, generator=g) + 0.5).to(DEV)
    beta = torch.randn(cols, generator=g).to(DEV)
    dy = torch.randn(rows, cols, generator=g).bfloat16().to(DEV)
    return x, res, gamma, beta, dy


# two rows: at most two non-zero partial rows meet in the atomics of
# ln_reduce_parts_k, and a + b == b + a, so dgamma and dbeta have the
# same bits in any arrival order
@pytest.mark.parametrize("rows,cols", [(2, 769), (2, 2049)])
def test_autograd(rows, cols):
    p = 0.1
    case = _random_case(rows, cols, "autograd")
    x, res, gamma, beta = [t.clone().requires_grad_(True) for t in case[:4]]
    dy = case[4]
    before = _counter()
    y = F_.dropout_add_layer_norm(x, res, gamma, beta, p=p, training=True)
    seed = _counter()
    assert seed == before + 1
    y.backward(dy)

    keep = keep_mask(seed, rows, cols, p, DEV)
    x2, res2, gamma2, beta2 = [t.clone().requires_grad_(True)
                               for t in case[:4]]
    y_ref = ops.layer_norm(_h_ref(x2, res2, keep, p), gamma2, beta2)
    y_ref.backward(dy)
    assert int((~keep).sum()) > 0
    _same(y, y_ref, "y")
    _same(x.grad, x2.grad, "grad x")
    _same(res.grad, res2.grad, "grad residual")
    _same(gamma.grad, gamma2.grad, "grad gamma")
    _same(beta.grad, beta2.grad, "grad beta")

    # eval mode and p = 0: no dropout, no seed drawn
    for kw in (dict(p=p, training=False), dict(p=0.0, training=True)):
        y0 = F_.dropout_add_layer_norm(x, res, gamma, beta, **kw)
        _same(y0, ops.layer_norm((res.float() + x.float()).bfloat16(),
                                 gamma, beta), "no dropout %s" % kw)
    assert _counter() == seed
    # a 3-d input is a batch of rows
    y3 = F_.dropout_add_layer_norm(x.view(1, rows, cols),
                                   res.view(1, rows, cols), gamma, beta,
                                   p=p)
    k3 = keep_mask(_counter(), rows, cols, p, DEV)
    assert y3.shape == (1, rows, cols)
    _same(y3.view(rows, cols),
          ops.layer_norm(_h_ref(x, res, k3, p), gamma, beta), "3-d y")


# ---------------------------------------------------------------------------
# 4: seeds
# ---------------------------------------------------------------------------

def test_each_call_draws_its_own_mask():
    C = ops.ext()
    rows, cols, p = 6, 769, 0.1
    case = _random_case(rows, cols, "seeds")
    x, res, gamma, beta = [t.clone().requires_grad_(True) for t in case[:4]]
    dy = case[4]
    y1 = F_.dropout_add_layer_norm(x, res, gamma, beta, p=p)
    s1 = _counter()
    y2 = F_.dropout_add_layer_norm(x, res, gamma, beta, p=p)
    s2 = _counter()
    assert s2 == s1 + 1
    f1 = C.dropout_add_ln_fwd(x.detach(), res.detach(), gamma.detach(),
                              beta.detach(), 1e-5, p, _seed_tensor(s1))
    f2 = C.dropout_add_ln_fwd(x.detach(), res.detach(), gamma.detach(),
                              beta.detach(), 1e-5, p, _seed_tensor(s2))
    assert not torch.equal(f1[1], f2[1])            # h
    _same(y1, f1[0], "first call y")
    _same(y2, f2[0], "second call y")
    assert not torch.equal(y1, y2)
    # the first call's backward, after the second's forward, replays
    # the first seed
    y1.backward(dy)
    d_sub, d_res, dgamma, dbeta = C.dropout_add_ln_bwd(
        f1[1], dy, gamma.detach(), f1[2], f1[3], p, _seed_tensor(s1))
    _same(x.grad, d_sub, "grad x")
    _same(res.grad, d_res, "grad residual")
    wrong = C.dropout_add_ln_bwd(f1[1], dy, gamma.detach(), f1[2], f1[3], p,
                                 _seed_tensor(s2))[0]
    assert not torch.equal(x.grad, wrong)


# ---------------------------------------------------------------------------
# 5: graph capture
# ---------------------------------------------------------------------------

def test_graph_capture_advances_the_seed():
    C = ops.ext()
    rows, cols, p = 5, 512, 0.1
    case = _random_case(rows, cols, "graph")
    x, res, gamma, beta = [t.clone().requires_grad_(True) for t in case[:4]]
    dy = case[4]
    params = (x, res, gamma, beta)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):  # warm up outside the capture
            for t in params:
                t.grad = None
            F_.dropout_add_layer_norm(x, res, gamma, beta, p=p) \
                .backward(dy)
    torch.cuda.current_stream().wait_stream(side)
    for t in params:
        t.grad = None

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_static = F_.dropout_add_layer_norm(x, res, gamma, beta, p=p)
        y_static.backward(dy)
    gx_static = x.grad

    start = _counter()
    seen = []
    for i in range(2):
        graph.replay()
        torch.cuda.synchronize()
        seed = _counter()
        assert seed == start + i + 1
        y_ref, h, mean, rstd = C.dropout_add_ln_fwd(
            x.detach(), res.detach(), gamma.detach(), beta.detach(), 1e-5,
            p, _seed_tensor(seed))
        _same(y_static, y_ref, "replay %d y" % i)
        _same(gx_static, C.dropout_add_ln_bwd(
            h, dy, gamma.detach(), mean, rstd, p, _seed_tensor(seed))[0],
            "replay %d grad x" % i)
        seen.append(y_static.clone())
    assert not torch.equal(seen[0], seen[1])


# ---------------------------------------------------------------------------
# 6: fallbacks and errors
# ---------------------------------------------------------------------------

def test_fallbacks():
    # 8200 columns: past the backward kernels' LDS partials, so the
    # composed path (whose LayerNorm backward has the same limit: only
    # the forward is run here)
    x, res, gamma, beta, _ = _random_case(3, 8200, "wide")
    before = _counter()
    torch.manual_seed(4)
    y = F_.dropout_add_layer_norm(x, res, gamma, beta, p=0.1)
    assert _counter() == before          # torch's dropout, not the kernels'
    torch.manual_seed(4)
    _same(y, ops.layer_norm(res + torch.nn.functional.dropout(x, 0.1, True),
                            gamma, beta), "8200 columns, training")
    _same(F_.dropout_add_layer_norm(x, res, gamma, beta, p=0.1,
                                    training=False),
          ops.layer_norm(res + x, gamma, beta), "8200 columns, eval")
    # p = 1: everything dropped
    x, res, gamma, beta, _ = _random_case(4, 64, "p1")
    y = F_.dropout_add_layer_norm(x, res, gamma, beta, p=1.0)
    _same(y, ops.layer_norm(res + torch.zeros_like(x), gamma, beta), "p=1")
    assert _counter() == before


def test_binding_errors():
    C = ops.ext()
    x, res, gamma, beta, dy = _random_case(4, 64, "errors")
    seed = _seed_tensor(1)
    y, h, mean, rstd = C.dropout_add_ln_fwd(x, res, gamma, beta, 1e-5, 0.1,
                                            seed)

    def fwd(sub=x, res=res, gamma=gamma, beta=beta, p=0.1, seed=seed):
        return C.dropout_add_ln_fwd(sub, res, gamma, beta, 1e-5, p, seed)

    def bwd(h=h, dy=dy, gamma=gamma, mean=mean, rstd=rstd, p=0.1,
            seed=seed):
        return C.dropout_add_ln_bwd(h, dy, gamma, mean, rstd, p, seed)

    bad = [
        lambda: fwd(res=res[:3]),                       # shapes differ
        lambda: fwd(res=res.view(64, 4)),
        lambda: fwd(sub=x.float()),                     # not bf16
        lambda: fwd(res=res.float()),
        lambda: fwd(sub=x.cpu()),
        lambda: fwd(sub=x.t()),                         # not contiguous
        lambda: fwd(gamma=gamma[:63].contiguous()),     # wrong length
        lambda: fwd(beta=torch.cat([beta, beta])),
        lambda: fwd(gamma=gamma.bfloat16()),
        lambda: fwd(p=1.0),
        lambda: fwd(p=-0.1),
        lambda: fwd(seed=None),                         # p > 0, no seed
        lambda: fwd(seed=seed.cpu()),
        lambda: fwd(seed=seed.int()),
        lambda: bwd(dy=dy[:3]),
        lambda: bwd(h=h.float()),
        lambda: bwd(dy=dy.float()),
        lambda: bwd(gamma=gamma[:63].contiguous()),
        lambda: bwd(mean=mean[:3]),
        lambda: bwd(rstd=torch.cat([rstd, rstd])),
        lambda: bwd(p=1.0),
        lambda: bwd(seed=None),
    ]
    for i, call in enumerate(bad):
        try:
            call()
        except RuntimeError:
            continue
        pytest.fail("bad call %d did not raise" % i)
    # the backward holds its partials in LDS: 8192 columns at most
    wide = torch.zeros(2, 8200, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        C.dropout_add_ln_bwd(wide, wide, torch.ones(8200, device=DEV),
                             mean[:2].contiguous(), rstd[:2].contiguous(),
                             0.1, seed)
    # and the good calls still work
    fwd()
    bwd()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 7: BertBase
# ---------------------------------------------------------------------------

def _bert(fused):
    from sparkdl.models.bert import BertBase, BertConfig
    cfg = BertConfig(vocab_size=200, hidden=128, layers=1, heads=2, ffn=256,
                     max_seq=64, fused_dropout_ln=fused)
    m = BertBase(cfg).cuda()
    return ops.convert_bf16_training(m)


def test_bert_fused_tails():
    from sparkdl.models.bert import bert_pretrain_step
    torch.manual_seed(3)
    on, off = _bert(True), _bert(False)
    off.load_state_dict(on.state_dict())
    ids = torch.randint(0, 200, (2, 64), device=DEV)
    on.eval()
    off.eval()
    with torch.no_grad():
        a, b = on(ids), off(ids)
    assert bool(torch.isfinite(a.float()).all())
    _same(a, b, "eval logits")

    on.train()
    opt = ops.FusedAdamW(on.parameters(), lr=1e-4)
    step = bert_pretrain_step(on, opt, 2, 64, DEV, True)
    before = _counter()
    loss = step()
    assert bool(torch.isfinite(loss))
    # attention-probability dropout and the two fused tails of the layer
    assert _counter() == before + 3
    unused = {"embeddings.token_type.weight"}    # no token types passed
    for name, prm in on.named_parameters():
        if name in unused:
            continue
        assert prm.grad is not None, name
        assert bool(torch.isfinite(prm.grad.float()).all()), name
        assert bool(prm.grad.float().abs().sum() > 0), name
