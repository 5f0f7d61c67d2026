"""dropout_add_layer_norm without a GPU: the keep-mask specification
(functional.dropout_keep_mask) against this file's own scalar and vector
implementations of the counter hash, its keep rate, the composed CPU
path of the functional and of DropoutAddLayerNorm, and the BertBase
switch. The kernels themselves: test_dropout_ln_gpu.py, which imports
the hash from here.
"""

import math

import numpy as np
import pytest
import torch

import sparkdl.ops as ops
from sparkdl.ops import functional as F_

SEEDS = [1, 2, 12345, 2 ** 31 - 1, 2 ** 32 + 5]
M32 = 0xffffffff


# ---------------------------------------------------------------------------
# the tests' own hash: a scalar one in Python integers and a vector one
# in numpy uint64 (every product stays below 2^64), checked against each
# other below
# ---------------------------------------------------------------------------

def p24_of(p):
    """(unsigned)(p * 2^24) with p an fp32 number: the product is exact."""
    return int(float(np.float32(p)) * 16777216.0)


def hash_scalar(seed, idx):
    x = (seed & M32) ^ ((idx * 2654435761) & M32)
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def keep_scalar(seed, rows, cols, p):
    p24 = p24_of(p)
    return [[(hash_scalar(seed, r * cols + c) & 0xffffff) >= p24
             for c in range(cols)] for r in range(rows)]


def keep_mask(seed, rows, cols, p, device="cpu"):
    """bool [rows, cols] tensor on ``device``, computed with numpy."""
    m = np.uint64(M32)
    i = np.arange(rows * cols, dtype=np.uint64)
    x = np.uint64(seed & M32) ^ ((i * np.uint64(2654435761)) & m)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & m
    x ^= x >> np.uint64(16)
    keep = (x & np.uint64(0xffffff)) >= np.uint64(p24_of(p))
    return torch.from_numpy(keep.reshape(rows, cols)).to(device)


def test_own_hashes_agree():
    for seed in SEEDS:
        want = torch.tensor(keep_scalar(seed, 7, 509, 0.1))
        assert torch.equal(keep_mask(seed, 7, 509, 0.1), want)
    assert p24_of(0.5) == 2 ** 23 and p24_of(0.0) == 0
    assert p24_of(0.1) == 1677721        # float32(0.1) * 2^24 = 1677721.625


# ---------------------------------------------------------------------------
# 1, 2: dropout_keep_mask
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols,p", [(4, 16, 0.3), (7, 509, 0.1),
                                         (3, 8, 0.5)])
def test_keep_mask_matches_own_hash(rows, cols, p):
    for seed in SEEDS:
        got = F_.dropout_keep_mask(seed, rows, cols, p)
        assert got.dtype == torch.bool and got.shape == (rows, cols)
        assert torch.equal(got, torch.tensor(keep_scalar(seed, rows, cols,
                                                         p))), seed
        assert torch.equal(got, keep_mask(seed, rows, cols, p)), seed
    # only the low 32 bits of the seed count
    assert torch.equal(F_.dropout_keep_mask(2 ** 32 + 5, rows, cols, p),
                       F_.dropout_keep_mask(5, rows, cols, p))
    assert not torch.equal(F_.dropout_keep_mask(5, rows, cols, p),
                           F_.dropout_keep_mask(6, rows, cols, p))
    # a one-element tensor is a seed too; p = 0 keeps everything
    assert torch.equal(
        F_.dropout_keep_mask(torch.tensor([12345]), rows, cols, p),
        F_.dropout_keep_mask(12345, rows, cols, p))
    assert bool(F_.dropout_keep_mask(12345, rows, cols, 0.0).all())


@pytest.mark.parametrize("rows,cols,p", [(7, 509, 0.1), (64, 768, 0.1),
                                         (6, 1024, 0.5), (2051, 64, 0.1)])
def test_keep_rate(rows, cols, p):
    n = rows * cols
    q = 1.0 - p24_of(p) / 2.0 ** 24
    sd = math.sqrt(n * q * (1 - q))
    for seed in SEEDS[:4]:
        kept = int(F_.dropout_keep_mask(seed, rows, cols, p).sum())
        z = (kept - n * q) / sd
        print("keep rate %dx%d p=%g seed=%d: %d of %d, %.2f sd"
              % (rows, cols, p, seed, kept, n, z))
        assert abs(z) <= 4.0, (seed, kept, n * q, z)


# ---------------------------------------------------------------------------
# 3: the functional's composed path
# ---------------------------------------------------------------------------

def _operands(dtype, rows=6, cols=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g).to(dtype)
    res = torch.randn(rows, cols, generator=g).to(dtype)
    gamma = torch.rand(cols, generator=g) + 0.5
    beta = torch.randn(cols, generator=g)
    return x, res, gamma, beta


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_path_is_the_composed_one(dtype):
    x, res, gamma, beta = _operands(dtype)
    torch.manual_seed(11)
    got = F_.dropout_add_layer_norm(x, res, gamma, beta, p=0.3,
                                    training=True, eps=1e-5)
    torch.manual_seed(11)
    want = F_.layer_norm(res + torch.nn.functional.dropout(x, 0.3, True),
                         gamma, beta, 1e-5)
    assert got.dtype == dtype
    assert torch.equal(got, want)
    # the dropout did something
    plain = F_.layer_norm(res + x, gamma, beta, 1e-5)
    assert not torch.equal(got, plain)
    assert torch.equal(F_.dropout_add_layer_norm(
        x, res, gamma, beta, p=0.3, training=False), plain)
    assert torch.equal(F_.dropout_add_layer_norm(
        x, res, gamma, beta, p=0.0, training=True), plain)
    assert torch.equal(F_.dropout_add_layer_norm(x, res, gamma, beta),
                       plain)
    # p = 1 drops the sublayer altogether
    assert torch.equal(
        F_.dropout_add_layer_norm(x, res, gamma, beta, p=1.0),
        F_.layer_norm(res + torch.zeros_like(x), gamma, beta, 1e-5))


def test_cpu_path_gradients():
    x, res, gamma, beta = [t.requires_grad_(True)
                           for t in _operands(torch.float32)]
    torch.manual_seed(5)
    y = F_.dropout_add_layer_norm(x, res, gamma, beta, p=0.25)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(1))
    y.backward(dy)
    got = [t.grad.clone() for t in (x, res, gamma, beta)]
    for t in (x, res, gamma, beta):
        assert t.grad is not None and bool(t.grad.abs().sum() > 0)
        t.grad = None
    torch.manual_seed(5)
    F_.layer_norm(res + torch.nn.functional.dropout(x, 0.25, True),
                  gamma, beta, 1e-5).backward(dy)
    for g, t in zip(got, (x, res, gamma, beta)):
        assert torch.equal(g, t.grad)
    # dropped elements get no gradient, kept ones the residual's, scaled
    dropped = got[0] == 0
    assert 0 < int(dropped.sum()) < dropped.numel()
    assert torch.allclose(got[0][~dropped], got[1][~dropped] / 0.75)


# ---------------------------------------------------------------------------
# 4: the module
# ---------------------------------------------------------------------------

def test_module():
    m = ops.DropoutAddLayerNorm(40, p=0.5, eps=1e-6)
    assert m.weight.dtype == m.bias.dtype == torch.float32
    assert m.weight.shape == m.bias.shape == (40,)
    assert sorted(m.state_dict()) == ["bias", "weight"]
    assert ops.DropoutAddLayerNorm(8).p == 0.1
    with torch.no_grad():
        m.weight.uniform_(0.5, 1.5)
        m.bias.normal_()
    x, res, _, _ = _operands(torch.bfloat16)
    plain = F_.layer_norm(res + x, m.weight, m.bias, 1e-6)
    m.eval()
    assert torch.equal(m(x, res), plain)
    m.train()
    torch.manual_seed(2)
    got = m(x, res)
    torch.manual_seed(2)
    assert torch.equal(got, F_.dropout_add_layer_norm(
        x, res, m.weight, m.bias, 0.5, True, 1e-6))
    assert not torch.equal(got, plain)


# ---------------------------------------------------------------------------
# 5: BertBase
# ---------------------------------------------------------------------------

def _small_bert(fused):
    from sparkdl.models.bert import BertBase, BertConfig
    torch.manual_seed(3)
    return BertBase(BertConfig(vocab_size=100, hidden=32, layers=2, heads=2,
                               ffn=64, max_seq=16,
                               fused_dropout_ln=fused))


def test_bert_switch_cpu(monkeypatch):
    from sparkdl.models.bert import BertConfig
    on, off = _small_bert(True), _small_bert(False)
    assert on.cfg.fused_dropout_ln is True
    assert off.cfg.fused_dropout_ln is False
    assert list(on.state_dict()) == list(off.state_dict())
    assert [n for n, _ in on.named_modules()] \
        == [n for n, _ in off.named_modules()]
    for a, b in zip(on.state_dict().values(), off.state_dict().values()):
        assert torch.equal(a, b)

    ids = torch.randint(0, 100, (2, 16),
                        generator=torch.Generator().manual_seed(0))
    on.train()
    off.train()
    torch.manual_seed(9)
    a = on(ids)
    torch.manual_seed(9)
    b = off(ids)
    assert torch.equal(a, b)
    torch.manual_seed(10)
    assert not torch.equal(a, off(ids))      # dropout is active

    monkeypatch.delenv("SPARKDL_FUSED_DROPOUT_LN", raising=False)
    assert BertConfig().fused_dropout_ln is False      # the default: off
    monkeypatch.setenv("SPARKDL_FUSED_DROPOUT_LN", "1")
    assert BertConfig().fused_dropout_ln is True
    assert BertConfig(fused_dropout_ln=False).fused_dropout_ln is False
    monkeypatch.setenv("SPARKDL_FUSED_DROPOUT_LN", "0")
    assert BertConfig().fused_dropout_ln is False
    assert BertConfig(fused_dropout_ln=True).fused_dropout_ln is True
